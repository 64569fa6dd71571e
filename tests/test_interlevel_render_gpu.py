"""GPU tests (-m gpu) of render_rays(interlevel=True) on every render path it is supported on.

Off means off is the existing suite's business.  Here: the key changes no other key and no gradient of a loss that ignores it; the key
is interlevel_loss on the weights and depths of the chain of public pieces; the dense fused node against the hooked path
(interlevel_loss on _Composite's weights) by the comparison of test_fused_node_against_the_hooked_path; the three backward plans; the
two-pass grid node against the compacting hook, with early_stop_eps and clip_to_occupancy, bit for bit; DenseNeRF networks, one
network for both passes, the empty batch, render() across chunks, both loss options together, the no-grad call.

THE HINGE.  On the fixture networks a refining interval is shorter than the coarse one it lies in, so with similar densities a w_j
stays below its bound and a gradient test would pass on zeros.  Every test here renders with `thin`, a copy of the coarse fixture
network whose alpha_linear.bias is lowered by SHIFT = 2.0.  Chosen with the oracle on the CPU (trace_rays on synthetic_rays(48, seed=12)
with synthetic_randoms(seed=5), perturb 1, noise 1, white background; interlevel_loss_reference in float64 on its weights): the mean
loss per ray rises from 0.13 (SHIFT 0) to 0.31 and 48 of 48 rays have a positive loss (share 1.0; the two passes' noise draws differ,
which alone opens the hinge somewhere on every ray).  test_fused_node_against_the_hooked_path asserts the share (>= 0.5) on the chain of
public pieces."""
import sys

import numpy as np
import pytest
import torch

import nerf_oracle as orc
from test_gpu_dense import ARCHS, _net
from test_gpu_distortion_render import LAM, none_or_equal
from test_gpu_early_stop import Chain, eps_for
from test_gpu_occupancy import bits_equal
from test_gpu_occupancy_train import (NET_KW, _small_scene, ball_dgrid, compacting_hook, datapath_fp16x3, flat_of, grads_of,  # noqa: F401
                                      zero_grads)
from test_gpu_parity import datapath, dev, maxdiff, nets, npa  # noqa: F401  (fixtures)
from test_gpu_ray_grad import rel_l2

pytestmark = pytest.mark.gpu

SHIFT = 2.0


@pytest.fixture(scope="module")
def thin(npa, dev, nets):
    """the coarse fixture network with alpha_linear.bias lowered by SHIFT (module docstring)"""
    net = npa.NeRF(**NET_KW).to(dev)
    state = {k: v.clone() for k, v in nets[2].items()}
    state["alpha_linear.bias"] = state["alpha_linear.bias"] - SHIFT
    net.load_state_dict(state)
    return net


def image(npa, out, target):
    return npa.img2mse(out["rgb_map"], target) + (npa.img2mse(out["rgb0"], target) if "rgb0" in out else 0.0)


def total(npa, out, target, kind="both"):
    """the training loss with the proposal term: img loss + the coarse image's + LAM * mean interlevel; "alone": that term only"""
    reg = LAM * out["interlevel"].mean()
    return reg if kind == "alone" else image(npa, out, target) + reg


def public_chain(npa, rays, rnd, net_c, net_f, n_c, n_f, std, precision):
    """render_rays' dense chain from public pieces of hip_backend with the injected randoms: (rgb_map, w_c, z_c, w_f, z_f)"""
    hb = npa.hip_backend
    dev = rays.device
    with torch.no_grad():
        z_c = hb.sample_coarse(rays, torch.linspace(0.0, 1.0, n_c, device=dev), False, rnd["t_rand"])
        raw_c, _ = hb.field_fwd(net_c.packed_params(precision), rays, z_c, save_act=False, precision=precision)
        w_c = hb.raw2outputs(raw_c, z_c, rays, rays.shape[1], rnd["noise_c"], std, True, rays_d_offset=3)[3]
        z_f = hb.sample_fine(z_c, w_c, n_f, rnd["u"], None)[0]
        raw_f, _ = hb.field_fwd(net_f.packed_params(precision), rays, z_f, save_act=False, precision=precision)
        rgb, _, _, w_f, _ = hb.raw2outputs(raw_f, z_f, rays, rays.shape[1], rnd["noise_f"], std, True, rays_d_offset=3)
    return rgb, w_c, z_c, w_f, z_f


# ------------------------------------------------------------------------------------------------ 1. the dense fused node
@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
def test_fused_node_against_the_hooked_path(npa, dev, nets, thin, datapath):
    _, nf, _, _ = nets
    nc = thin
    n = 48
    rays = orc.synthetic_rays(n, seed=12).to(dev)
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, 64, 128, seed=5).items()}
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd)
    hook = lambda pts, viewdirs, net: npa.run_network(pts, viewdirs, net, None, None)

    def run(query_fn, loss_fn, **extra):
        zero_grads(nc, nf)
        r = rays.clone().requires_grad_(True)
        out = npa.render_rays(r, nc, query_fn, **kw, **extra)
        loss_fn(out).backward()
        return {k: v.detach() for k, v in out.items()}, (grads_of(nc), grads_of(nf)), r.grad.clone()
    off, g_off, r_off = run(None, lambda out: image(npa, out, target))
    on, g_on, r_on = run(None, lambda out: image(npa, out, target), interlevel=True)
    # the option adds one key, last, and changes nothing else: not a bit of another key, not a bit of a gradient that ignores it
    assert list(on) == list(off) + ["interlevel"] and on["interlevel"].shape == (n,) and on["interlevel"].dtype == torch.float32
    for k in off:
        assert bits_equal(on[k], off[k]), k
    assert all(none_or_equal(a, b) for ga, gb in zip(g_on, g_off) for a, b in zip(ga, gb)) and bits_equal(r_on, r_off)
    assert float(on["interlevel"].min()) >= 0.0
    # the key is interlevel_loss on the chain of public pieces, bit for bit; on that chain the hinge is open on at least half of the rays
    rgb, w_c, z_c, w_f, z_f = public_chain(npa, rays, rnd, nc, nf, 64, 128, 1.0, datapath)
    assert bits_equal(rgb, on["rgb_map"]) and bits_equal(npa.interlevel_loss(w_c, z_c, w_f, z_f), on["interlevel"])
    share = float((npa.interlevel_loss_reference(w_c.double(), z_c, w_f.double(), z_f) > 0).double().mean())
    print(f"\n{datapath}: rays with a positive interlevel loss on the public chain: {share:.3f}, mean loss {float(on['interlevel'].mean()):.3e}")
    assert share >= 0.5
    for kind in ("both", "alone"):
        fused, (gc_f, gf_f), r_fused = run(None, lambda out: total(npa, out, target, kind), interlevel=True)
        hooked, (gc_h, gf_h), r_hook = run(hook, lambda out: total(npa, out, target, kind), interlevel=True)
        assert set(hooked) == set(fused) and list(hooked)[-1] == "interlevel"
        for k in fused:
            assert maxdiff(hooked[k], fused[k]) <= 1e-6 * max(1.0, float(fused[k].abs().nan_to_num().max())), (kind, k)
        assert bits_equal(fused["interlevel"], on["interlevel"])
        if kind == "alone":     # the target is a constant of the graph: nothing reaches network_fine, on either path
            assert all(g is None for g in gf_f) and all(g is None for g in gf_h)
        assert all(g is not None for g in gc_f) and float(flat_of(gc_f).abs().max()) > 0
        for a, b in list(zip(gc_h, gc_f)) + ([] if kind == "alone" else list(zip(gf_h, gf_f))):
            assert maxdiff(a, b) <= 1e-4 * float(b.abs().max()) + 1e-12, (kind, maxdiff(a, b), float(b.abs().max()))
        print(f"{datapath} {kind}: d rays fused vs hooked max diff {maxdiff(r_hook, r_fused):.3e} of {float(r_fused.abs().max()):.3e}")
        assert maxdiff(r_hook, r_fused) <= 1e-4 * float(r_fused.abs().max()) + 1e-12 and not bool(r_fused[:, 6:8].any())
        assert float(r_fused.abs().max()) > 0
    # the gradient of the key is not the image's: the term does something
    assert not bits_equal(flat_of(gc_f), flat_of(g_off[0]))
    zero_grads(nc, nf)


def test_no_grad_call_both_options_and_one_network(npa, dev, nets, thin, datapath_fp16x3, monkeypatch):
    """the no-grad call takes the staged passes and keeps every other key's bits; distortion and interlevel together, in that order,
    each with the bits it has alone; one network for both passes: the key alone reaches it through the coarse pass only, which the
    hooked path confirms"""
    hb = npa.hip_backend
    _, nf, _, _ = nets
    nc = thin
    n = 48
    rays = orc.synthetic_rays(n, seed=12).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, 64, 128, seed=5).items()}
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, randoms=rnd)
    with torch.no_grad():
        got = npa.render_rays(rays, nc, None, interlevel=True, **kw)
        both = npa.render_rays(rays, nc, None, interlevel=True, distortion=True, **kw)
        dist = npa.render_rays(rays, nc, None, distortion=True, **kw)
        monkeypatch.setattr(hb, "INFER_ONE_LAUNCH", False)
        staged = npa.render_rays(rays, nc, None, **kw)
        monkeypatch.undo()
    assert list(got) == list(staged) + ["interlevel"] and list(both) == list(staged) + ["distortion", "interlevel"]
    for k in staged:
        assert bits_equal(got[k], staged[k]) and bits_equal(both[k], staged[k]), k
    assert bits_equal(both["interlevel"], got["interlevel"]) and bits_equal(both["distortion"], dist["distortion"])
    assert not got["interlevel"].requires_grad and float(got["interlevel"].max()) > 0
    # both keys with gradients: the sum of the two terms' gradients, per network, as the hooked path has it
    res = {}
    hook = lambda pts, viewdirs, net: npa.run_network(pts, viewdirs, net, None, None)
    for name, q in (("fused", None), ("hooked", hook)):
        zero_grads(nc, nf)
        out = npa.render_rays(rays, nc, q, interlevel=True, distortion=True, **kw)
        assert list(out)[-2:] == ["distortion", "interlevel"]
        (LAM * (out["distortion"].mean() + out["interlevel"].mean())).backward()
        res[name] = (out["interlevel"].detach(), grads_of(nc), grads_of(nf))
    assert bits_equal(res["fused"][0], got["interlevel"])
    for i in (1, 2):
        for a, b in zip(res["hooked"][i], res["fused"][i]):
            assert maxdiff(a, b) <= 1e-4 * float(b.abs().max()) + 1e-12
    # one network for both passes
    one = dict(kw, network_fine=None)
    for name, q in (("fused", None), ("hooked", hook)):
        zero_grads(nc)
        out = npa.render_rays(rays, nc, q, interlevel=True, **one)
        (LAM * out["interlevel"].mean()).backward()
        res[name] = (out["interlevel"].detach(), grads_of(nc))
    zero_grads(nc, nf)
    assert maxdiff(res["hooked"][0], res["fused"][0]) <= 1e-6 * max(1.0, float(res["fused"][0].max()))
    assert float(flat_of(res["fused"][1]).abs().max()) > 0
    for a, b in zip(res["hooked"][1], res["fused"][1]):
        assert maxdiff(a, b) <= 1e-4 * float(b.abs().max()) + 1e-12


def test_the_three_backward_plans(npa, dev, nets, thin, datapath_fp16x3, monkeypatch):
    """2500 rays: one launch, resident sub-chunks (a budget of a little over 1024 rays) and recompute give the same outputs bit for
    bit, bit-identical ray gradients, and parameter gradients whose relative L2 distance from the one-launch plan's is at most twice
    what the same plans show WITHOUT the option in this test (the sub-chunks' sums are added in another order), or the fp32 noise
    floor of one more addition per entry, 2^-23 -- as for distortion"""
    hb = npa.hip_backend
    render_mod = sys.modules["nerf_pytorch_amd.render"]
    _, nf, _, _ = nets
    nc = thin
    n = 2500
    rays = orc.synthetic_rays(n, seed=8).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, 64, 128, seed=6).items()}
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    kw = dict(randoms=rnd, N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=0.5)

    def run(option):
        zero_grads(nc, nf)
        r = rays.clone().requires_grad_(True)
        out = npa.render_rays(r, nc, None, interlevel=option, **kw)
        (total(npa, out, target) if option else image(npa, out, target)).backward()
        return (render_mod.LAST_BACKWARD_PLAN[0], {k: v.detach() for k, v in out.items()}, torch.cat([m.last_flat_grad for m in (nc, nf)]).clone(),
                r.grad.clone())
    with_opt, without = [run(True)], [run(False)]
    monkeypatch.setattr(hb, "SAVE_BUDGET_BYTES", 4 * hb.workspace_floats(1024, 64, 128, True, "fp16x3") + 1)
    with_opt.append(run(True))
    without.append(run(False))
    monkeypatch.setattr(hb, "SAVE_TOTAL_BYTES", 0)
    with_opt.append(run(True))
    without.append(run(False))
    zero_grads(nc, nf)
    assert [p[0] for p in with_opt] == ["one launch", "resident sub-chunks", "recompute"] == [p[0] for p in without]
    assert float(with_opt[0][1]["interlevel"].max()) > 0 and not bits_equal(with_opt[0][2], without[0][2])
    for (plan, out, g, r), (_, _, g0, _) in zip(with_opt[1:], without[1:]):
        for k in out:
            assert bits_equal(out[k], with_opt[0][1][k]), (plan, k)
        assert bits_equal(r, with_opt[0][3]), plan
        diff, yard = rel_l2(g, with_opt[0][2]), rel_l2(g0, without[0][2])
        print(f"\n{plan}: parameter gradients vs one launch, relative L2 {diff:.3e} with the option, {yard:.3e} without")
        assert diff <= max(2.0 * yard, 2.0 ** -23), (plan, diff, yard)
    assert bits_equal(with_opt[1][2], with_opt[2][2])        # recompute re-runs the sub-chunks: the same sums in the same order


# ------------------------------------------------------------------------------------------------ 2. the grid node
def test_two_grid_passes_against_the_compacting_hook(npa, dev, nets, thin, datapath_fp16x3):
    """DensityGrid, two networks, loss = image + coarse image + LAM * interlevel, and the key alone: outputs, the key included, and
    every parameter gradient of both networks equal the hooked path's with the compacting hook, bit for bit; the option changes no
    other key; alone, nothing reaches network_fine"""
    _, nf, _, _ = nets
    nc = thin
    rays, rnd, target = _small_scene(dev)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd)
    with torch.no_grad():
        plain = npa.render_rays(rays, nc, None, occupancy=grid, **kw)
        no_grad = npa.render_rays(rays, nc, None, occupancy=grid, interlevel=True, **kw)
    res = {}
    for name, fn in (("grid", lambda: npa.render_rays(rays, nc, None, occupancy=grid, interlevel=True, **kw)),
                     ("hook", lambda: npa.render_rays(rays, nc, compacting_hook(npa, grid), interlevel=True, **kw))):
        for kind in ("both", "alone"):
            zero_grads(nc, nf)
            out = fn()
            total(npa, out, target, kind).backward()
            res[name, kind] = ({k: v.detach() for k, v in out.items()}, grads_of(nc), grads_of(nf))
    zero_grads(nc, nf)
    out_g = res["grid", "both"][0]
    assert list(out_g)[-1] == "interlevel" and list(no_grad) == list(plain) + ["interlevel"]
    for k in plain:
        assert bits_equal(no_grad[k], plain[k]) and bits_equal(out_g[k], plain[k]), k
    assert bits_equal(no_grad["interlevel"], out_g["interlevel"]) and float((out_g["interlevel"] > 0).float().mean()) >= 0.5
    for kind in ("both", "alone"):
        (og, gc, gf), (oh, hc, hf) = res["grid", kind], res["hook", kind]
        for k in og:
            assert bits_equal(og[k], oh[k]), (kind, k)
        for name, a, b in (("coarse", gc, hc), ("fine", gf, hf)):
            if kind == "alone" and name == "fine":
                assert all(x is None for x in a) and all(x is None for x in b)
                continue
            assert all(x is not None for x in a) and float(flat_of(a).abs().max()) > 0
            for i, (x, y) in enumerate(zip(a, b)):
                assert bits_equal(x, y), (kind, name, i, maxdiff(x, y), rel_l2(flat_of(a), flat_of(b)))
    assert not bits_equal(flat_of(res["grid", "both"][1]), flat_of(res["grid", "alone"][1]))


def test_early_stop_and_clipping(npa, dev, nets, thin, datapath_fp16x3):
    """early_stop_eps against the chain of tests/test_gpu_early_stop.py (the hooked path with the stopping hook), bit for bit -- a
    stopped sample has weight 0 and contributes nothing; and clip_to_occupancy=True == the call on grid.clip_rays(rays)[0], for the key
    and the gradients too"""
    _, nf, _, _ = nets
    nc = thin
    rays, rnd, target = _small_scene(dev)
    grid = ball_dgrid(npa, dev, outside="skip")
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, randoms=rnd, interlevel=True)
    eps = eps_for(npa, grid, rays, nc, **{k: v for k, v in kw.items() if k != "interlevel"})
    res = []
    chain = Chain(npa, grid, eps)
    for fn in (lambda: npa.render_rays(rays, nc, None, occupancy=grid, early_stop_eps=eps, **kw),
               lambda: chain.run(npa.render_rays, rays, nc, chain.hook, **kw)):
        zero_grads(nc, nf)
        out = fn()
        total(npa, out, target).backward()
        res.append(({k: v.detach() for k, v in out.items()}, grads_of(nc) + grads_of(nf)))
    assert grid.last_stats["rays_stopped"] > 0 and list(res[0][0])[-1] == "interlevel" and float(res[0][0]["interlevel"].max()) > 0
    for k in res[0][0]:
        assert bits_equal(res[0][0][k], res[1][0][k]), k
    for i, (x, y) in enumerate(zip(res[0][1], res[1][1])):
        assert bits_equal(x, y), (i, maxdiff(x, y))
    clipped, hit = grid.clip_rays(rays)
    assert 0 < int(hit.sum())
    res = []
    for r, extra in ((rays, dict(clip_to_occupancy=True)), (clipped, {})):
        zero_grads(nc, nf)
        out = npa.render_rays(r, nc, None, occupancy=grid, **kw, **extra)
        total(npa, out, target, "alone").backward()
        res.append((out["interlevel"].detach(), flat_of(grads_of(nc))))
        assert all(p.grad is None for p in nf.parameters())
    zero_grads(nc, nf)
    assert bits_equal(res[0][0], res[1][0]) and bits_equal(res[0][1], res[1][1]) and float(res[0][1].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 3. the other paths
def test_dense_networks(npa, dev, monkeypatch):
    """DenseNeRF networks (the layer-by-layer path): the option changes no other key; the key and the gradients of the interlevel term
    against the same call with interlevel_loss replaced by interlevel_loss_reference in float64; nothing reaches the fine network"""
    render_mod = sys.modules["nerf_pytorch_amd.render"]
    arch = ARCHS["narrow_shallow"]
    net_c, _ = _net(npa, dev, arch, 31)
    net_f, _ = _net(npa, dev, arch, 32)
    n, n_c, n_f = 96, 24, 40
    rays = orc.synthetic_rays(n, seed=3).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, n_c, n_f, seed=21).items()}
    kw = dict(N_samples=n_c, N_importance=n_f, network_fine=net_f, perturb=1.0, white_bkgd=True, raw_noise_std=0.5, retraw=True, randoms=rnd)

    def run(**extra):
        zero_grads(net_c, net_f)
        out = npa.render_rays(rays, net_c, None, **kw, **extra)
        if "interlevel" in out:
            (LAM * out["interlevel"].mean()).backward()
        assert all(p.grad is None for p in net_f.parameters())
        return {k: v.detach() for k, v in out.items()}, [p.grad.clone() for p in net_c.parameters() if p.grad is not None]
    off, _ = run()
    on, g_on = run(interlevel=True)
    assert list(on) == list(off) + ["interlevel"] and on["interlevel"].shape == (n,)
    for k in off:
        assert bits_equal(on[k], off[k]), k
    monkeypatch.setattr(render_mod, "interlevel_loss",
                        lambda wp, zp, w, z: npa.interlevel_loss_reference(wp.double(), zp, w.double(), z).float())
    ref, g_ref = run(interlevel=True)
    assert maxdiff(on["interlevel"], ref["interlevel"]) <= 1e-6 * max(1.0, float(ref["interlevel"].abs().max()))
    assert len(g_on) == len(g_ref) > 0 and float((on["interlevel"] > 0).float().mean()) >= 0.5
    for a, b in zip(g_on, g_ref):
        assert maxdiff(a, b) <= 1e-4 * float(b.abs().max()) + 1e-12
    assert max(float(b.abs().max()) for b in g_ref) > 0


def test_empty_batch_and_render_in_chunks(npa, dev, nets, thin, datapath_fp16x3):
    _, nf, _, _ = nets
    nc = thin
    kw = dict(N_samples=16, N_importance=24, network_fine=nf, white_bkgd=True)
    ret = npa.render_rays(torch.zeros(0, 11, device=dev), nc, None, interlevel=True, **kw)
    assert list(ret)[-1] == "interlevel" and ret["interlevel"].shape == (0,) and ret["interlevel"].device.type == "cuda"
    ret = npa.render_rays(torch.zeros(0, 11, device=dev), nc, None, interlevel=True, distortion=True, occupancy=ball_dgrid(npa, dev), **kw)
    assert list(ret)[-2:] == ["distortion", "interlevel"] and ret["interlevel"].shape == (0,)
    # render(): extras["interlevel"] with the rays' leading shape, the same bits whatever the chunking; differentiable
    rays = orc.synthetic_rays(12 * 20, seed=4).to(dev)
    K = np.array([[20.0, 0, 10.0], [0, 20.0, 6.0], [0, 0, 1]])
    geo = dict(rays=(rays[:, 0:3].reshape(12, 20, 3), rays[:, 3:6].reshape(12, 20, 3)), ndc=False, near=2.0, far=6.0, use_viewdirs=True,
               network_fn=nc, network_query_fn=None, interlevel=True, **kw)
    with torch.no_grad():
        one = npa.render(12, 20, K, chunk=1 << 20, **geo)
        many = npa.render(12, 20, K, chunk=96, **geo)
    assert one[3]["interlevel"].shape == (12, 20) and list(one[3])[-1] == "interlevel"
    assert bits_equal(one[3]["interlevel"], many[3]["interlevel"]) and bits_equal(one[0], many[0])
    zero_grads(nc, nf)
    rgb, _, _, extras = npa.render(12, 20, K, chunk=96, **geo)
    (LAM * extras["interlevel"].mean()).backward()
    assert bits_equal(extras["interlevel"].detach(), one[3]["interlevel"])
    assert float(flat_of(grads_of(nc)).abs().max()) > 0 and all(p.grad is None for p in nf.parameters())
    zero_grads(nc, nf)
