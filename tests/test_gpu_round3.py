"""GPU tests added in round 3 (-m gpu): the weight-ring forward, the tightened split-bf16 gradient bounds (ReLU kink
flips separated from arithmetic error), bf16-vs-fp32 operand storage on every golden configuration, chunked rendering
with injected random draws, and the autograd-node hygiene fixes (no reference cycle, stale-parameter guard,
GradientSync stream ordering)."""
import gc
import weakref

import numpy as np
import pytest
import torch

import nerf_oracle as orc
from test_gpu_parity import GOLD, _golden_randoms, dev, maxdiff, nets, npa  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- weight-ring kernels
# (rounds 3-4 compared them bit for bit with the double-buffered kernels they replaced, kept in a test-only library; that library is
# gone -- tests/test_gpu_digests.py holds digests of every buffer recorded while those comparisons were green)
def test_the_split_forward_is_the_ring_kernel(npa, dev, nets):
    """hip_backend routes the split forwards (inference and saving, either 16-bit type) through the weight-ring kernel.  Checked
    through the per-kernel timer labels bench.py reports."""
    nc, nf, Pc, Pf = nets
    hb = npa.hip_backend
    rays = orc.synthetic_rays(16, seed=1).to(dev)
    z = torch.sort(torch.rand(16, 8, device=dev) * 4 + 2, -1)[0]
    hb.TIMER = hb.KernelTimer()
    try:
        for prec in ("bf16x3", "fp16x3"):
            hb.field_fwd(nf.packed_params(prec), rays, z, save_act=False, precision=prec)
            _, act = hb.field_fwd(nf.packed_params(prec), rays, z, save_act=True, precision=prec)
            hb.WORKSPACE.give(act)
        names = set(hb.TIMER.summary())
    finally:
        hb.TIMER = None
    assert names == {"field_fwd16r_kernel", "field_fwd16r_kernel<save bf16>", "field_fwd16r_kernel<fp16>", "field_fwd16r_kernel<fp16, save>"}, names


# ---------------------------------------------------------------- split-bf16 backward: arithmetic error vs kink flips
def _decode_masks(npa, act, P, n_rays, precision="bf16x3"):
    """ReLU patterns of a split datapath's save buffer as 9 boolean tensors [P, width] on the CPU (hip_backend.relu_patterns decodes
    the kernels' bitmask order)"""
    return [m.cpu() for m in npa.hip_backend.relu_patterns(act, n_rays, P // n_rays, precision)]


def _field_with_forced_relu(P64, feats, masks):
    """The reference MLP in fp64 with every ReLU replaced by a multiplication with a GIVEN 0/1 pattern (oracle.field_mlp_forced_relu)"""
    return orc.field_mlp_forced_relu(P64, feats, masks)


@pytest.mark.parametrize("n_rays,S", [(48, 64), (11, 192), (70, 20)])
def test_field_backward_bf16x3_arithmetic_and_flips(npa, dev, nets, n_rays, S):
    """The split-bf16 backward held to fp32-class ARITHMETIC bounds.  A ReLU unit whose pre-activation lies within the
    forward's error of zero legitimately takes either side of its kink (test_field_backward separates these points with a
    mask for the fp32 datapath; here a few units per point are affected, so masking points would leave nothing).  The
    two effects are separated exactly instead: the kernel SAVES the ReLU pattern it used (the bitmasks dgrad reads), so
      (1) the gradient is compared with fp64 autograd of the reference network evaluated with THAT pattern: what remains
          is arithmetic error: the three-term products and the bf16 rounding (2^-9, zero-mean) of the stored weight-gradient
          operands, held to 8e-3 of max|g| per tensor (measured 5.4e-3 on rgb_linear.weight, 384 entries): the upstream gradient
          here is RANDOM, the worst case for that rounding (incoherent sums: it does not average down relative to the result; under
          a training loss's upstream gradient it is 1.6e-4 of the gradient, test_gpu_fp16x3.py, and the fp16 split's 11-bit
          operands bring both numbers down 8x);
      (2) the pattern itself is compared with fp64's: every unit that differs must have |fp64 pre-activation| within the
          forward's error bound of zero, and such units must be rare."""
    nc, nf, Pc, Pf = nets
    hb = npa.hip_backend
    g = torch.Generator().manual_seed(7 * n_rays + S)
    rays = orc.synthetic_rays(n_rays, seed=S + 1)
    z = torch.sort(torch.rand(n_rays, S, generator=g) * 4.0 + 2.0, -1)[0]
    d_raw = torch.randn(n_rays, S, 4, generator=g)
    P = n_rays * S
    packed3 = nf.packed_params("bf16x3")
    raw, act = hb.field_fwd(packed3, rays.to(dev), z.to(dev), save_act=True, precision="bf16x3")
    masks = _decode_masks(npa, act, P, n_rays)
    grad = torch.full((595844,), float("nan"), device=dev)
    hb.field_bwd(packed3, act, d_raw.to(dev), grad, accumulate=False, precision="bf16x3", params=nf.flat_params())
    hb.WORKSPACE.give(act)
    grad = grad.cpu().double()
    assert not torch.isnan(grad).any()
    P64 = {k: v.double().requires_grad_(True) for k, v in Pf.items()}
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3).double()
    dirs = rays[:, None, 8:11].expand(n_rays, S, 3).reshape(-1, 3).double()
    feats = torch.cat([orc.posenc(pts, 10), orc.posenc(dirs, 4)], -1)
    out, pres = _field_with_forced_relu(P64, feats, masks)
    (out * d_raw.reshape(-1, 4).double()).sum().backward()
    # (1) arithmetic
    worst = {}
    for nm, off, shape in hb.param_table():
        gg = grad[off:off + int(np.prod(shape))].view(shape)
        r = P64[nm].grad
        worst[nm] = maxdiff(gg, r) / max(float(r.abs().max()), 1e-30)
    bound = 8e-3
    # (2) flips
    n_units = flips = 0
    worst_pre = 0.0
    for layer, (pre, m) in enumerate(zip(pres, masks)):
        ref_pattern = pre.detach() > 0
        diff = ref_pattern != m
        n_units += diff.numel()
        flips += int(diff.sum())
        if diff.any():
            scale = max(1.0, float(pre.detach().abs().max()))
            worst_pre = max(worst_pre, float(pre.detach().abs()[diff].max()) / scale)
    print(f"bf16x3 backward vs fp64 with the kernel's own ReLU pattern: max|err|/max|g| "
          f"{max(worst.values()):.1e} ({max(worst, key=worst.get)}); ReLU units on the other side of their kink: {flips} of {n_units} "
          f"({flips / P:.2f} per point), largest |pre-activation| among them {worst_pre:.1e} of the layer's max")
    assert max(worst.values()) <= bound, worst
    assert worst_pre <= 3e-4, worst_pre                       # flips only within the forward's error of zero
    assert flips <= 2e-3 * n_units, (flips, n_units)


# ---------------------------------------------------------------- operand storage on every golden configuration
# the six golden configurations of test_gpu_parity.py (same arguments, same generator seeds)
GOLDEN_CASES = [
    ("lego_det", dict(), None, None),
    ("lego_train", dict(perturb=1.0), 123, None),
    ("fern_train", dict(perturb=1.0, raw_noise_std=1.0, white_bkgd=False, N_importance=64, lindisp=True), 321, None),
    ("lego_coarse_only", dict(perturb=1.0, N_importance=0, network_fine=None), 11, None),
    ("fern_ndc_train", dict(perturb=1.0, raw_noise_std=1.0, white_bkgd=False, N_importance=128), 77, "fern"),
    ("lego_render_train", dict(perturb=1.0), 123, "lego"),
]


def _golden_grads(npa, dev, nets, kw, seed, render=None, precision="bf16x3"):
    nc, nf, Pc, Pf = nets
    target = torch.tensor(np.random.RandomState(99).rand(256, 3), dtype=torch.float32).to(dev)
    args = dict(N_samples=64, retraw=True, N_importance=128, network_fine=nf, perturb=0., white_bkgd=True, raw_noise_std=0., lindisp=False)
    args.update(kw)
    randoms = _golden_randoms(seed, 256, args)
    for m in (nc, nf):
        m.zero_grad()
    npa.set_precision(precision)
    try:
        if render is None:
            out = npa.render_rays(orc.synthetic_rays(256, seed=7).to(dev), nc, None, randoms=randoms, **args)
        else:
            cfg, batch = render
            rgb, disp, acc, extras = npa.render(cfg["H"], cfg["W"], orc.intrinsics(cfg), chunk=1024 * 32, rays=batch.to(dev), ndc=cfg["ndc"],
                                                near=cfg["near"], far=cfg["far"], use_viewdirs=True, network_fn=nc, network_query_fn=None,
                                                randoms=randoms, **args)
            out = dict(extras, rgb_map=rgb)
        loss = npa.img2mse(out["rgb_map"], target)
        if "rgb0" in out:
            loss = loss + npa.img2mse(out["rgb0"], target)
        loss.backward()
    finally:
        npa.set_precision("fp32")
    gs = [nc.last_flat_grad.double().cpu()]
    if args["N_importance"] > 0:
        gs.append(nf.last_flat_grad.double().cpu())
    return torch.cat(gs)


# ---------------------------------------------------------------- chunked rendering with injected draws
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_chunked_render_consumes_injected_randoms_per_chunk(npa, dev, nets, precision):
    """render(chunk < N, randoms=...) (run_nerf.py:54-66 slices the rays; the draws of a chunk are those of ITS rays): equal
    to the unchunked call bit for bit, and to the oracle's chunked trace."""
    nc, nf, Pc, Pf = nets
    import workloads as wl
    cfg = wl.LEGO
    n = 300
    batch = wl.lego_batch(n, seed=9).to(dev)
    rnd = {k: v.to(dev) for k, v in wl.synthetic_randoms(n, 64, 128, seed=3).items()}
    kw = dict(ndc=False, near=cfg["near"], far=cfg["far"], use_viewdirs=True, network_fn=nc, network_query_fn=None, N_samples=64,
              N_importance=128, network_fine=nf, perturb=1.0, white_bkgd=True, raw_noise_std=1.0, retraw=True, randoms=rnd)
    npa.set_precision(precision)
    try:
        with torch.no_grad():
            a = npa.render(cfg["H"], cfg["W"], wl.intrinsics(cfg), chunk=1 << 15, rays=batch, **kw)
            b = npa.render(cfg["H"], cfg["W"], wl.intrinsics(cfg), chunk=77, rays=batch, **kw)
    finally:
        npa.set_precision("fp32")
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))
    for k in a[3]:
        assert torch.equal(torch.nan_to_num(a[3][k]), torch.nan_to_num(b[3][k])), k
    if precision == "fp32":
        flat = orc.assemble_render_rays(cfg["H"], cfg["W"], wl.intrinsics(cfg), batch[0].cpu(), batch[1].cpu(), False, cfg["near"], cfg["far"])
        cpu = {k: v.cpu() for k, v in rnd.items()}
        ref = orc.trace_in_chunks(flat, 77, P_coarse=Pc, P_fine=Pf, n_coarse=64, n_fine=128, perturb=1.0, white_bkgd=True,
                                  raw_noise_std=1.0, **cpu)
        assert maxdiff(b[3]["rgb0"], ref["rgb0"]) <= 1e-5


# ---------------------------------------------------------------- autograd-node hygiene
def test_render_graph_dropped_without_backward_is_collected(npa, dev, nets):
    """A grad-enabled render whose graph is dropped without backward (validation loss outside no_grad, an exception between
    forward and backward) must free its saved activations: the node may not keep its own outputs alive."""
    nc, nf, Pc, Pf = nets
    rays = orc.synthetic_rays(64, seed=2).to(dev)
    out = npa.render_rays(rays, nc, None, N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, retraw=True)
    node = weakref.ref(out["rgb_map"].grad_fn)
    raw_ref = weakref.ref(out["raw"])
    assert node() is not None
    del out
    gc.collect()
    assert node() is None and raw_ref() is None, "the _RenderRays node survived: reference cycle through ctx"


def test_backward_after_parameter_update_is_refused_on_the_folded_datapath(npa, dev, nets):
    """The split-bf16 backward combines activations saved at forward time with the live feature_linear / views_linears
    weights (folded feature layer): an optimizer step between forward and backward must be an error, not a silently mixed
    gradient.  The exact-fp32 datapath has no such dependence and still works."""
    kw = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    nc, nf = npa.NeRF(**kw).to(dev), npa.NeRF(**kw).to(dev)
    nc.load_state_dict(nets[2])
    nf.load_state_dict(nets[3])
    rays = orc.synthetic_rays(32, seed=4).to(dev)
    args = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True)
    for precision, refused in (("bf16x3", True), ("fp32", False)):
        npa.set_precision(precision)
        try:
            out = npa.render_rays(rays, nc, None, **args)
            with torch.no_grad():
                nf.feature_linear.weight.mul_(1.0001)
            if refused:
                with pytest.raises(RuntimeError, match="parameters changed between"):
                    out["rgb_map"].sum().backward()
            else:
                out["rgb_map"].sum().backward()
        finally:
            npa.set_precision("fp32")


def test_gradient_sync_orders_the_exchange_on_a_side_stream(npa, dev, nets, monkeypatch):
    """GradientSync with an ASYNC work object on another stream (what RCCL gives): the early-started exchange writes the
    bucket on a side stream; finish() must wait for it before the scale, and the hand-over branch (autograd copied instead
    of adopting the views) must copy the averaged values.  A fake work object stands in for the nccl one (one GPU here):
    all_reduce(x) := x *= 2 on a side stream after a delay."""
    import torch.distributed as dist
    from nerf_pytorch_amd import parallel
    import sys
    render = sys.modules["nerf_pytorch_amd.render"]
    side = torch.cuda.Stream()

    class FakeWork:
        def __init__(self, t):
            self.t = t
            self.ev = torch.cuda.Event()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                torch.cuda._sleep(20_000_000)           # the exchange is still running when finish() is called
                t.mul_(2.0)                             # "sum over two ranks holding the same values"
                self.ev.record(side)
            self.waited = False

        def wait(self):
            torch.cuda.current_stream().wait_event(self.ev)
            self.waited = True

    works = []

    def fake_all_reduce(t, op=None, group=None, async_op=False):
        w = FakeWork(t)
        works.append(w)
        if not async_op:
            w.wait()
            return None
        return w
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "all_reduce", fake_all_reduce)
    kw = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    a, b = npa.NeRF(**kw).to(dev), npa.NeRF(**kw).to(dev)
    table = npa.hip_backend.param_table()
    with parallel.GradientSync([a, b]) as sync:
        fa = torch.full((npa.hip_backend.N_PARAMS,), 3.0, device=dev)
        fb = torch.full((npa.hip_backend.N_PARAMS,), 5.0, device=dev)
        render._grad_ready(a, fa)            # started early (async, side stream)
        render._grad_ready(b, fb)
        assert sync.started == 2 and len(works) == 2
        for nm, off, shape in table:         # a: autograd adopted the views; b: autograd copied
            n_el = int(np.prod(shape))
            dict(a.named_parameters())[nm].grad = fa[off:off + n_el].view(shape)
            dict(b.named_parameters())[nm].grad = fb[off:off + n_el].view(shape).clone()
        sync.finish()
        torch.cuda.synchronize()
    assert all(w.waited for w in works)
    assert all(bool((p.grad == 3.0).all()) for p in a.parameters())      # (3 * 2) / 2
    assert all(bool((p.grad == 5.0).all()) for p in b.parameters())
    assert render.GRAD_READY_HOOKS == []


# ---------------------------------------------------------------- render_rays in one call (C ABI)
def _one_call_step(npa, dev, flat_c, flat_f, rays, rnd, target, precision, lr_step=None, state=None):
    """forward + backward of one ray batch through nerf_render_rays_fwd / nerf_render_rays_bwd ONLY (plus the parameter
    repack and, with lr_step, nerf_adam_step): what a foreign host would write.  Returns (outputs, grad_c, grad_f)."""
    import ctypes
    hb = npa.hip_backend
    L = hb.lib()
    n = rays.shape[0]
    s = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: None if t is None else t.data_ptr()
    prec = hb.DATAPATHS[precision].cfg
    cfg = hb.NerfRenderCfg(64, 128, 0, 1, 1.0 if "noise_c" in rnd else 0.0, prec, 0)
    packed = []
    for flat in (flat_c, flat_f):
        p = torch.empty(L.nerf_packed3_floats() if prec else L.nerf_packed_floats(), device=dev)
        if prec:
            assert L.nerf_pack_params_split(flat.data_ptr(), p.data_ptr(), 5, int(prec in (3, 5)), s) == 0
        else:
            assert L.nerf_pack_params(flat.data_ptr(), p.data_ptr(), s) == 0
        packed.append(p)
    ws = torch.empty(L.nerf_render_workspace_floats(ctypes.byref(cfg), n, 1), device=dev)
    o = dict(rgb=torch.empty(n, 3, device=dev), disp=torch.empty(n, device=dev), acc=torch.empty(n, device=dev),
             raw=torch.empty(n, 192, 4, device=dev), rgb0=torch.empty(n, 3, device=dev), disp0=torch.empty(n, device=dev),
             acc0=torch.empty(n, device=dev), z_std=torch.empty(n, device=dev))
    rc = L.nerf_render_rays_fwd(ctypes.byref(cfg), ptr(packed[0]), ptr(packed[1]), ptr(rays), 11, n, ptr(rnd.get("t_rand")), ptr(rnd.get("noise_c")),
                                ptr(rnd.get("u")), ptr(rnd.get("noise_f")), ptr(o["rgb"]), ptr(o["disp"]), ptr(o["acc"]), ptr(o["raw"]),
                                ptr(o["rgb0"]), ptr(o["disp0"]), ptr(o["acc0"]), ptr(o["z_std"]), ptr(ws), 1, s)
    assert rc == 0, L.nerf_last_error()
    # the loss of train() (run_nerf.py:765-771) on the outputs; its gradient w.r.t. the outputs is all the backward needs
    rgb_l, rgb0_l = o["rgb"].clone().requires_grad_(True), o["rgb0"].clone().requires_grad_(True)
    (npa.img2mse(rgb_l, target) + npa.img2mse(rgb0_l, target)).backward()
    gc, gf = torch.empty(hb.N_PARAMS, device=dev), torch.empty(hb.N_PARAMS, device=dev)
    rc = L.nerf_render_rays_bwd(ctypes.byref(cfg), ptr(packed[0]), ptr(packed[1]), ptr(flat_c), ptr(flat_f), ptr(rays), 11, n,
                                ptr(rnd.get("noise_c")), ptr(rnd.get("noise_f")), ptr(o["raw"]), ptr(rgb_l.grad), None, None, None,
                                ptr(rgb0_l.grad), None, None, ptr(ws), ptr(gc), ptr(gf), 0, s)
    assert rc == 0, L.nerf_last_error()
    if lr_step is not None:
        for flat, g, (m, v) in ((flat_c, gc, state[0]), (flat_f, gf, state[1])):
            assert L.nerf_adam_step(flat.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), hb.N_PARAMS, 5e-4, 0.9, 0.999, 1e-8, lr_step, s) == 0
    return o, gc, gf


@pytest.mark.parametrize("precision,noise", [("fp32", False), ("bf16x3", True), ("fp16x3", True), ("fp16x3w", True)])
def test_one_call_abi_matches_the_binding(npa, dev, nets, precision, noise):
    """nerf_render_rays_fwd / _bwd (one C call per direction, caller-owned workspace) against the in-repo binding's
    render_rays + autograd on the same rays, draws and weights: the same launches in the same order, so outputs and both
    networks' gradients are bit-identical (the linspace tables are built in the library: torch.linspace bit for bit)."""
    nc, nf, Pc, Pf = nets
    import workloads as wl
    n = 200
    rays = orc.synthetic_rays(n, seed=12).to(dev)
    rnd = {k: v.to(dev) for k, v in wl.synthetic_randoms(n, 64, 128, seed=8).items() if noise or k in ("t_rand", "u")}
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(2)).to(dev)
    npa.set_precision(precision)
    try:
        for m in (nc, nf):
            m.zero_grad()
        ref = npa.render_rays(rays, nc, None, N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, retraw=True,
                              perturb=1.0, raw_noise_std=1.0 if noise else 0.0, randoms=rnd)
        (npa.img2mse(ref["rgb_map"], target) + npa.img2mse(ref["rgb0"], target)).backward()
        o, gc, gf = _one_call_step(npa, dev, nc.flat_params(), nf.flat_params(), rays, rnd, target, precision)
    finally:
        npa.set_precision("fp32")
    for a, b in (("rgb", "rgb_map"), ("disp", "disp_map"), ("acc", "acc_map"), ("raw", "raw"), ("rgb0", "rgb0"), ("disp0", "disp0"),
                 ("acc0", "acc0"), ("z_std", "z_std")):
        assert torch.equal(torch.nan_to_num(o[a]), torch.nan_to_num(ref[b].detach())), a
    assert torch.equal(gc, nc.last_flat_grad) and torch.equal(gf, nf.last_flat_grad)


def test_one_call_backward_writes_every_gradient_it_is_given(npa, dev, nets):
    """nerf_render_rays_bwd(accumulate = 0) with upstream gradients for ONE of the two passes only: the other network's gradient
    vector is WRITTEN (zeros), not left as it was; d_disp / d_acc without d_rgb is accepted (a zero d_rgb is
    synthesised) instead of surfacing a raw HIP error code."""
    import ctypes
    import workloads as wl
    nc, nf, Pc, Pf = nets
    hb = npa.hip_backend
    L = hb.lib()
    n = 96
    s = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: None if t is None else t.data_ptr()
    rays = orc.synthetic_rays(n, seed=4).to(dev)
    rnd = {k: v.to(dev) for k, v in wl.synthetic_randoms(n, 64, 128, seed=2).items() if k in ("t_rand", "u")}
    for precision, prec in (("fp16x3", 3), ("fp32", 0)):
        cfg = hb.NerfRenderCfg(64, 128, 0, 1, 0.0, prec, 1)
        packed = [m.packed_params(precision) for m in (nc, nf)]
        ws = torch.empty(L.nerf_render_workspace_floats(ctypes.byref(cfg), n, 1), device=dev)
        o = dict(rgb=torch.empty(n, 3, device=dev), disp=torch.empty(n, device=dev), acc=torch.empty(n, device=dev),
                 raw=torch.empty(n, 192, 4, device=dev), rgb0=torch.empty(n, 3, device=dev), disp0=torch.empty(n, device=dev),
                 acc0=torch.empty(n, device=dev), z_std=torch.empty(n, device=dev))
        assert L.nerf_render_rays_fwd(ctypes.byref(cfg), ptr(packed[0]), ptr(packed[1]), ptr(rays), 11, n, ptr(rnd["t_rand"]), None, ptr(rnd["u"]), None,
                                      ptr(o["rgb"]), ptr(o["disp"]), ptr(o["acc"]), ptr(o["raw"]), ptr(o["rgb0"]), ptr(o["disp0"]), ptr(o["acc0"]),
                                      ptr(o["z_std"]), ptr(ws), 1, s) == 0, L.nerf_last_error()
        g = torch.randn(n, 3, device=dev) * 1e-4
        ga = torch.randn(n, device=dev) * 1e-4

        def bwd(d_rgb, d_acc, d_rgb0, d_acc0):
            gc, gf = torch.full((hb.N_PARAMS,), float("nan"), device=dev), torch.full((hb.N_PARAMS,), float("nan"), device=dev)
            rc = L.nerf_render_rays_bwd(ctypes.byref(cfg), ptr(packed[0]), ptr(packed[1]), ptr(nc.flat_params()), ptr(nf.flat_params()), ptr(rays), 11, n,
                                        None, None, ptr(o["raw"]), ptr(d_rgb), None, ptr(d_acc), None, ptr(d_rgb0), None, ptr(d_acc0),
                                        ptr(ws), ptr(gc), ptr(gf), 0, s)
            assert rc == 0, (rc, L.nerf_last_error())
            return gc, gf
        gc, gf = bwd(g, None, None, None)                   # fine pass only: the coarse network's gradient is zeros
        assert bool((gc == 0).all()) and bool(torch.isfinite(gf).all()) and float(gf.abs().max()) > 0
        gc2, gf2 = bwd(None, None, g, None)                 # coarse pass only
        assert bool((gf2 == 0).all()) and bool(torch.isfinite(gc2).all()) and float(gc2.abs().max()) > 0
        gc3, gf3 = bwd(None, ga, None, ga)                  # d_acc without d_rgb, both passes
        assert bool(torch.isfinite(gc3).all()) and bool(torch.isfinite(gf3).all()) and float(gc3.abs().max()) > 0 and float(gf3.abs().max()) > 0
        # ... and equals the same call with an explicit zero d_rgb
        z3 = torch.zeros(n, 3, device=dev)
        gc4, gf4 = bwd(z3, ga, z3, ga)
        assert torch.equal(gc3, gc4) and torch.equal(gf3, gf4)
    rc = L.nerf_render_rays_bwd(ctypes.byref(cfg), ptr(packed[0]), ptr(packed[1]), ptr(nc.flat_params()), ptr(nf.flat_params()), ptr(rays), 11, n,
                                None, None, ptr(o["raw"]), None, None, None, None, None, None, None, ptr(ws), ptr(gc), ptr(gf), 0, s)
    assert rc == -1 and b"no upstream gradient" in L.nerf_last_error()


def test_one_call_abi_trains_two_steps(npa, dev, nets):
    """Two optimizer steps driven ONLY through the C entry points a foreign host would bind (pack -> render_rays_fwd ->
    render_rays_bwd -> adam_step), against the same two steps through the binding (render_rays + autograd + FlatAdam):
    identical parameters afterwards."""
    import workloads as wl
    hb = npa.hip_backend
    kw = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    nc, nf = npa.NeRF(**kw).to(dev), npa.NeRF(**kw).to(dev)
    nc.load_state_dict(nets[2])
    nf.load_state_dict(nets[3])
    flat_c, flat_f = nc.flat_params().clone(), nf.flat_params().clone()
    state = [(torch.zeros_like(flat_c), torch.zeros_like(flat_c)), (torch.zeros_like(flat_f), torch.zeros_like(flat_f))]
    opt = npa.FlatAdam(list(nc.parameters()) + list(nf.parameters()), lr=5e-4, betas=(0.9, 0.999))
    n = 256
    npa.set_precision("bf16x3")
    try:
        for step in (1, 2):
            rays = orc.synthetic_rays(n, seed=40 + step).to(dev)
            rnd = {k: v.to(dev) for k, v in wl.synthetic_randoms(n, 64, 128, seed=step).items() if k in ("t_rand", "u")}
            target = torch.rand(n, 3, generator=torch.Generator().manual_seed(step)).to(dev)
            out = npa.render_rays(rays, nc, None, N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, retraw=True,
                                  perturb=1.0, randoms=rnd)
            opt.zero_grad()
            (npa.img2mse(out["rgb_map"], target) + npa.img2mse(out["rgb0"], target)).backward()
            opt.step()
            _one_call_step(npa, dev, flat_c, flat_f, rays, rnd, target, "bf16x3", lr_step=step, state=state)
    finally:
        npa.set_precision("fp32")
    assert torch.equal(flat_c, nc.flat_params()) and torch.equal(flat_f, nf.flat_params())
    assert not torch.equal(flat_c, torch.cat([nets[2][k].reshape(-1) for k, _ in orc.param_shapes()]).to(dev))     # it did train


def test_weight_gradient_refuses_mismatched_buffers_on_the_gpu(npa, dev, nets):
    """The pairing checks of the C ABI with real buffers: bf16 rows + fp16 deltas, a save buffer of another sample count."""
    nc, nf, Pc, Pf = nets
    hb = npa.hip_backend
    L = hb.lib()
    s = torch.cuda.current_stream().cuda_stream
    n, S = 32, 16
    rays = orc.synthetic_rays(n, seed=1).to(dev)
    z = torch.sort(torch.rand(n, S, device=dev) * 4 + 2, -1)[0]
    p3 = nf.packed_params("bf16x3")
    raw = torch.empty(n, S, 4, device=dev)
    act = torch.empty(hb.act_floats(n, S), device=dev)
    d_raw = torch.randn(n, S, 4, device=dev)
    delta = torch.empty(L.nerf_delta_floats(n, S), device=dev)
    partial = torch.empty(L.nerf_wgrad_partial_floats(n, S), device=dev)
    grad = torch.empty(hb.N_PARAMS, device=dev)
    assert L.nerf_field_fwd_split(p3.data_ptr(), rays.data_ptr(), 11, z.data_ptr(), n, S, raw.data_ptr(), act.data_ptr(), 0, s) == 0
    assert hb.buffer_layout(act) == (4, False, n, S)
    assert L.nerf_field_dgrad_split(p3.data_ptr(), act.data_ptr(), d_raw.data_ptr(), n, S, delta.data_ptr(), 1, s) == 0      # fp16 deltas
    args = (act.data_ptr(), delta.data_ptr(), d_raw.data_ptr(), n, S, partial.data_ptr(), grad.data_ptr(), 0)
    assert L.nerf_field_wgrad_phase(*args, -1, 7, nf.flat_params().data_ptr(), s) == -1 and b"different datapaths" in L.nerf_last_error()
    assert L.nerf_field_dgrad_split(p3.data_ptr(), act.data_ptr(), d_raw.data_ptr(), n, S // 2, delta.data_ptr(), 0, s) == -1
    assert L.nerf_field_dgrad_split(p3.data_ptr(), act.data_ptr(), d_raw.data_ptr(), n, S, delta.data_ptr(), 0, s) == 0
    assert L.nerf_field_wgrad_phase(*args, -1, 7, nf.flat_params().data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad).all())


# ---------------------------------------------------------------- render_rays without gradients in one launch
@pytest.mark.parametrize("n_rays", [1, 17, 129, 1000])
@pytest.mark.parametrize("case", ["det", "random_white_noise", "lindisp", "coarse_only", "small", "same_net", "fp16x3_det", "fp16x3_random_white_noise"])
def test_one_launch_inference_is_bit_identical_to_the_chain_of_launches(npa, dev, nets, n_rays, case, monkeypatch):
    """render_infer_kernel (csrc/render_fused.hip): a workgroup takes 16 rays from the coarse depths through both networks,
    raw2outputs and sample_pdf + sort to the colours, calling the SAME device code as the separate launches -- so every
    output of render_rays (incl. extras: raw, z_std, rgb0 / disp0 / acc0) is bit-identical to the chain sample_coarse ->
    field forward -> composite -> sample_fine -> field forward -> composite; ragged ray counts (last workgroup partly empty,
    a single ray), injected random draws, density noise, white background, lindisp, no fine pass, one shared network."""
    nc, nf, Pc, Pf = nets
    hb = npa.hip_backend
    n_c, n_f = {"coarse_only": (64, 0), "small": (8, 16)}.get(case, (64, 128))
    kw = dict(N_samples=n_c, N_importance=n_f, network_fine=nf, retraw=True)
    rnd = None
    prec = "fp16x3" if case.startswith("fp16x3") else "bf16x3"
    case = case.replace("fp16x3_", "")
    if case == "random_white_noise":
        kw.update(white_bkgd=True, perturb=1.0, raw_noise_std=0.7)
        rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n_rays, n_c, n_f, seed=11).items()}
    elif case == "lindisp":
        kw.update(lindisp=True, white_bkgd=True)
    elif case == "same_net":
        kw.update(network_fine=None, white_bkgd=True)
    rays = orc.synthetic_rays(n_rays, seed=91).to(dev)
    npa.set_precision(prec)
    try:
        assert hb.render_infer_supported(n_c, n_f, npa.get_precision())
        outs = {}
        for one in (False, True):
            monkeypatch.setattr(hb, "INFER_ONE_LAUNCH", one)
            launches = []
            real = hb.render_rays_infer
            monkeypatch.setattr(hb, "render_rays_infer", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
            with torch.no_grad():
                outs[one] = npa.render_rays(rays, nc, None, randoms=rnd, **kw)
            monkeypatch.setattr(hb, "render_rays_infer", real)
            assert len(launches) == int(one)
    finally:
        npa.set_precision("fp32")
    assert set(outs[False]) == set(outs[True])
    for k in outs[False]:
        a, b = outs[False][k], outs[True][k]
        assert a.shape == b.shape, k
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)), (k, maxdiff(a, b))


def test_one_launch_inference_refuses_what_it_cannot_tile(npa, dev, nets):
    """16 rays must fill whole 128-point tiles in both passes and the datapath must be a three-term split: anything else is
    NERF_E_BADARG from the C entry point (and the host code keeps the chain of launches)."""
    import ctypes
    nc, nf, Pc, Pf = nets
    hb = npa.hip_backend
    L = hb.lib()
    assert not hb.render_infer_supported(63, 128, "bf16x3") and not hb.render_infer_supported(64, 127, "bf16x3")
    assert not hb.render_infer_supported(64, 128, "fp32") and hb.render_infer_supported(64, 128, "fp16x3")
    assert not hb.render_infer_supported(512, 1024, "bf16x3")      # per-ray scratch beyond one wavefront's share of the LDS
    cfg = hb.render_cfg(63, 128, False, True, 0.0, "bf16x3")
    n = 16
    rays = orc.synthetic_rays(n, seed=1).to(dev)
    e = lambda *s: torch.empty(s, device=dev)
    ws = e(L.nerf_render_workspace_floats(ctypes.byref(cfg), n, 0))
    p3 = nf.packed_params("bf16x3")
    rc = L.nerf_render_rays_infer(ctypes.byref(cfg), p3.data_ptr(), p3.data_ptr(), rays.data_ptr(), 11, n, None, None, None, None,
                                  e(n, 3).data_ptr(), e(n).data_ptr(), e(n).data_ptr(), e(n, 191, 4).data_ptr(), e(n, 3).data_ptr(),
                                  e(n).data_ptr(), e(n).data_ptr(), e(n).data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and b"one-launch inference" in L.nerf_last_error()


def test_one_launch_inference_is_what_render_runs_without_gradients(npa, dev, nets):
    """render() under no_grad on the split-bf16 datapath is ONE kernel per ray chunk (timer labels of bench.py); with gradients
    enabled, and on the exact-fp32 datapath, it stays the chain of launches."""
    nc, nf, Pc, Pf = nets
    hb = npa.hip_backend
    assert hb.INFER_ONE_LAUNCH
    H, W, focal = 16, 16, 20.0
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    rays = orc.synthetic_rays(H * W, seed=4).to(dev)
    kw = dict(network_fn=nc, network_fine=nf, network_query_fn=None, N_samples=64, N_importance=128, perturb=0., white_bkgd=True,
              raw_noise_std=0., use_viewdirs=True, near=2., far=6.)
    seen = {}
    for prec, grad in (("bf16x3", False), ("bf16x3", True), ("fp32", False)):
        npa.set_precision(prec)
        hb.TIMER = hb.KernelTimer()
        try:
            with torch.set_grad_enabled(grad):
                npa.render(H, W, K, chunk=100, rays=(rays[:, 0:3], rays[:, 3:6]), **kw)
            seen[(prec, grad)] = set(hb.TIMER.summary())
        finally:
            hb.TIMER = None
            npa.set_precision("fp32")
    assert seen[("bf16x3", False)] == {"render_infer_kernel"}, seen
    assert "render_infer_kernel" not in seen[("bf16x3", True)] and "render_infer_kernel" not in seen[("fp32", False)], seen


# ---------------------------------------------------------------- img2mse in one launch
@pytest.mark.parametrize("shape", [(1, 3), (4096, 3), (333, 7), (800 * 100, 3)])
def test_img2mse_kernel_matches_the_reference_expression(npa, dev, shape):
    """npa.img2mse on GPU tensors is one launch (+ one for the gradient): value and gradient against torch.mean((x - y) ** 2) in
    fp64; deterministic from run to run; CPU tensors and broadcasting keep the reference's expression."""
    g = torch.Generator().manual_seed(shape[0])
    x = torch.rand(shape, generator=g).to(dev).requires_grad_(True)
    y = torch.rand(shape, generator=g).to(dev)
    up = 0.7
    loss = npa.img2mse(x, y)
    (loss * up).backward()
    x64 = x.detach().double().requires_grad_(True)
    ref = torch.mean((x64 - y.double()) ** 2)
    (ref * up).backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 2e-6 * float(ref.detach())
    assert maxdiff(x.grad, x64.grad) <= 1e-6 * float(x64.grad.abs().max())
    again = npa.img2mse(x.detach(), y)
    assert torch.equal(again, loss.detach())
    yb = y[:1]                                     # broadcasting: the reference's expression
    assert torch.allclose(npa.img2mse(x.detach(), yb), torch.mean((x.detach() - yb) ** 2))
    assert torch.allclose(npa.img2mse(x.detach().cpu(), y.cpu()), torch.mean((x.detach().cpu() - y.cpu()) ** 2))
