"""GPU tests (-m gpu) of render_rays(distortion=True) on every render path.

Off means off is the existing suite's business (kernel digests, the grid call trace, every bit-for-bit test).  Here: the key changes no
other key and no gradient of a loss that ignores it; the dense fused node against the hooked path (distortion_loss on _Composite's
weights) by the comparison of test_user_network_query_fn_is_called_for_every_pass; the grid node against the chains the grid paths'
own tests build from public pieces, with distortion_loss on the chain's weights, bit for bit where those tests have bit equality; the
backward plans; DenseNeRF networks; the empty batch; render() across chunks; the no-grad call."""
import sys

import numpy as np
import pytest
import torch

import nerf_oracle as orc
import test_gpu_grid_proposal as gp
import test_gpu_march_step as ms
from test_gpu_dense import ARCHS, _net
from test_gpu_early_stop import Chain, eps_for
from test_gpu_grid_proposal import filled  # noqa: F401  (fixture)
from test_gpu_occupancy import bits_equal
from test_gpu_occupancy_train import (_small_scene, ball_dgrid, compacting_hook, datapath_fp16x3, flat_of, grads_of,  # noqa: F401
                                      zero_grads)
from test_gpu_parity import datapath, dev, maxdiff, nets, npa  # noqa: F401  (fixtures)
from test_gpu_ray_grad import rel_l2

pytestmark = pytest.mark.gpu

LAM = 0.1
NOISE_SEED = gp.NOISE_SEED


def total(npa, out, target, kind="both"):
    """the training loss with the regulariser: img loss (+ the coarse image's) + LAM * mean distortion; "alone": the distortion term only"""
    reg = LAM * out["distortion"].mean()
    if kind == "alone":
        return reg
    return npa.img2mse(out["rgb_map"], target) + (npa.img2mse(out["rgb0"], target) if "rgb0" in out else 0.0) + reg


def none_or_equal(a, b):
    return (a is None and b is None) or (a is not None and b is not None and bits_equal(a, b))


# ------------------------------------------------------------------------------------------------ 1. the dense fused node
@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
@pytest.mark.parametrize("n_f", [0, 128])
def test_fused_node_against_the_hooked_path(npa, dev, nets, datapath, n_f):
    nc, nf, _, _ = nets
    n = 48
    rays = orc.synthetic_rays(n, seed=12).to(dev)
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, 64, 128, seed=5).items()}
    kw = dict(N_samples=64, N_importance=n_f, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd)
    hook = lambda pts, viewdirs, net: npa.run_network(pts, viewdirs, net, None, None)
    models = (nc, nf) if n_f > 0 else (nc,)

    def run(query_fn, loss_fn, **extra):
        zero_grads(nc, nf)
        r = rays.clone().requires_grad_(True)
        out = npa.render_rays(r, nc, query_fn, **kw, **extra)
        loss_fn(out).backward()
        return {k: v.detach() for k, v in out.items()}, [g for m in models for g in grads_of(m)], r.grad.clone()
    image = lambda out: npa.img2mse(out["rgb_map"], target) + (npa.img2mse(out["rgb0"], target) if "rgb0" in out else 0.0)
    off, g_off, r_off = run(None, image)
    on, g_on, r_on = run(None, image, distortion=True)
    # the option adds one key, last, and changes nothing else: not a bit of another key, not a bit of a gradient that ignores it
    assert list(on) == list(off) + ["distortion"] and on["distortion"].shape == (n,) and on["distortion"].dtype == torch.float32
    for k in off:
        assert bits_equal(on[k], off[k]), k
    assert all(none_or_equal(a, b) for a, b in zip(g_on, g_off)) and bits_equal(r_on, r_off)
    assert float(on["distortion"].min()) >= 0.0 and float(on["distortion"].max()) > 1e-4
    for kind in ("both", "alone"):
        fused, g_fused, r_fused = run(None, lambda out: total(npa, out, target, kind), distortion=True)
        hooked, g_hook, r_hook = run(hook, lambda out: total(npa, out, target, kind), distortion=True)
        assert set(hooked) == set(fused) and list(hooked)[-1] == "distortion"
        for k in fused:
            assert maxdiff(hooked[k], fused[k]) <= 1e-6 * max(1.0, float(fused[k].abs().nan_to_num().max())), (kind, k)
        assert bits_equal(fused["distortion"], on["distortion"])
        live = 0
        for a, b in zip(g_hook, g_fused):
            assert (a is None) == (b is None), kind          # "alone" with a refining pass: the coarse network gets no gradient
            if b is not None:
                assert maxdiff(a, b) <= 1e-4 * float(b.abs().max()) + 1e-12, (kind, maxdiff(a, b), float(b.abs().max()))
                live += int(bool(b.any()))
        assert live > 0
        print(f"\n{datapath} n_f={n_f} {kind}: d rays fused vs hooked max diff {maxdiff(r_hook, r_fused):.3e} of {float(r_fused.abs().max()):.3e}")
        assert maxdiff(r_hook, r_fused) <= 1e-4 * float(r_fused.abs().max()) + 1e-12 and not bool(r_fused[:, 6:8].any())
    zero_grads(nc, nf)


def test_the_key_is_the_definition_on_the_last_pass_weights(npa, dev, nets, datapath_fp16x3, monkeypatch):
    """the fused node's key against distortion_loss_reference in float64 on the weights and depths the last compositing launch used (a
    spy on hip_backend.raw2outputs), at the kernel tolerance of tests/test_gpu_distortion.py measured on these inputs; and the no-grad
    call with the option: the staged passes, the same rgb_map bits as the staged no-grad path without it"""
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    n = 48
    rays = orc.synthetic_rays(n, seed=12).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, 64, 128, seed=5).items()}
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, randoms=rnd)
    seen = []
    real = hb.raw2outputs
    monkeypatch.setattr(hb, "raw2outputs", lambda raw, z, *a, **k: (lambda r: (seen.append((z, r[3])), r)[1])(real(raw, z, *a, **k)))
    with torch.no_grad():
        got = npa.render_rays(rays, nc, None, distortion=True, **kw)
    assert len(seen) == 2 and seen[1][1] is not None        # two staged compositing launches, the last one hands out its weights
    z, w = seen[1]
    ref64 = npa.distortion_loss_reference(w.double(), z.double(), rays[:, 6].double(), rays[:, 7].double())
    ref32 = npa.distortion_loss_reference(w, z, rays[:, 6], rays[:, 7])
    assert maxdiff(got["distortion"], ref64) <= max(4.0 * maxdiff(ref32, ref64), 2.0 ** -22)
    monkeypatch.setattr(hb, "INFER_ONE_LAUNCH", False)
    del seen[:]
    with torch.no_grad():
        staged = npa.render_rays(rays, nc, None, **kw)
    assert len(seen) == 2 and seen[1][1] is None
    assert list(got) == list(staged) + ["distortion"]
    for k in staged:
        assert bits_equal(got[k], staged[k]), k


@pytest.mark.parametrize("n_f", [0, 128])
def test_the_three_backward_plans(npa, dev, nets, datapath_fp16x3, monkeypatch, n_f):
    """2500 rays: one launch, resident sub-chunks (a budget of a little over 1024 rays) and recompute give the same outputs bit for
    bit, bit-identical ray gradients, and parameter gradients whose relative L2 distance from the one-launch plan's is at most twice
    what the same plans show WITHOUT the option in this test (the sub-chunks' sums are added in another order), or the fp32 noise
    floor of one more addition per entry, 2^-23"""
    hb = npa.hip_backend
    render_mod = sys.modules["nerf_pytorch_amd.render"]
    nc, nf, _, _ = nets
    n = 2500
    rays = orc.synthetic_rays(n, seed=8).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, 64, 128, seed=6).items()}
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    kw = dict(randoms=rnd, N_samples=64, N_importance=n_f, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=0.5)
    models = (nc, nf) if n_f > 0 else (nc,)

    def run(option):
        zero_grads(nc, nf)
        r = rays.clone().requires_grad_(True)
        out = npa.render_rays(r, nc, None, distortion=option, **kw)
        if option:
            total(npa, out, target).backward()
        else:
            (npa.img2mse(out["rgb_map"], target) + (npa.img2mse(out["rgb0"], target) if "rgb0" in out else 0.0)).backward()
        return (render_mod.LAST_BACKWARD_PLAN[0], {k: v.detach() for k, v in out.items()}, torch.cat([m.last_flat_grad for m in models]).clone(),
                r.grad.clone())
    with_opt, without = [run(True)], [run(False)]
    monkeypatch.setattr(hb, "SAVE_BUDGET_BYTES", 4 * hb.workspace_floats(1024, 64, n_f, True, "fp16x3") + 1)
    with_opt.append(run(True))
    without.append(run(False))
    monkeypatch.setattr(hb, "SAVE_TOTAL_BYTES", 0)
    with_opt.append(run(True))
    without.append(run(False))
    zero_grads(nc, nf)
    assert [p[0] for p in with_opt] == ["one launch", "resident sub-chunks", "recompute"] == [p[0] for p in without]
    for (plan, out, g, r), (_, _, g0, _) in zip(with_opt[1:], without[1:]):
        for k in out:
            assert bits_equal(out[k], with_opt[0][1][k]), (plan, k)
        assert bits_equal(r, with_opt[0][3]), plan
        diff, yard = rel_l2(g, with_opt[0][2]), rel_l2(g0, without[0][2])
        print(f"\nn_f={n_f} {plan}: parameter gradients vs one launch, relative L2 {diff:.3e} with the option, {yard:.3e} without")
        assert diff <= max(2.0 * yard, 2.0 ** -23), (plan, diff, yard)
    assert bits_equal(with_opt[1][2], with_opt[2][2])        # recompute re-runs the sub-chunks: the same sums in the same order


# ------------------------------------------------------------------------------------------------ 2. the grid node
def test_two_grid_passes_against_the_compacting_hook(npa, dev, nets, datapath_fp16x3):
    """DensityGrid, two networks, loss = image + coarse image + LAM * distortion: outputs, the key included, and every parameter
    gradient of both networks equal the hooked path's with the compacting hook, bit for bit; the option changes no other key"""
    nc, nf, _, _ = nets
    rays, rnd, target = _small_scene(dev)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd)
    with torch.no_grad():
        plain = npa.render_rays(rays, nc, None, occupancy=grid, **kw)
        no_grad = npa.render_rays(rays, nc, None, occupancy=grid, distortion=True, **kw)
    res = {}
    for name, fn in (("grid", lambda: npa.render_rays(rays, nc, None, occupancy=grid, distortion=True, **kw)),
                     ("hook", lambda: npa.render_rays(rays, nc, compacting_hook(npa, grid), distortion=True, **kw))):
        for kind in ("both", "alone"):
            zero_grads(nc, nf)
            out = fn()
            total(npa, out, target, kind).backward()
            res[name, kind] = ({k: v.detach() for k, v in out.items()}, grads_of(nc), grads_of(nf))
    zero_grads(nc, nf)
    out_g = res["grid", "both"][0]
    assert list(out_g)[-1] == "distortion" and list(no_grad) == list(plain) + ["distortion"]
    for k in plain:
        assert bits_equal(no_grad[k], plain[k]) and bits_equal(out_g[k], plain[k]), k
    assert bits_equal(no_grad["distortion"], out_g["distortion"]) and float(out_g["distortion"].max()) > 1e-4
    for kind in ("both", "alone"):
        (og, gc, gf), (oh, hc, hf) = res["grid", kind], res["hook", kind]
        for k in og:
            assert bits_equal(og[k], oh[k]), (kind, k)
        for name, a, b in (("coarse", gc, hc), ("fine", gf, hf)):
            if kind == "alone" and name == "coarse":        # no loss on the coarse pass: nothing reaches the coarse network
                assert all(x is None or not bool(x.any()) for x in a) and all(x is None or not bool(x.any()) for x in b)
                continue
            assert all(x is not None for x in a) and float(flat_of(a).abs().max()) > 0
            for i, (x, y) in enumerate(zip(a, b)):
                assert bits_equal(x, y), (kind, name, i, maxdiff(x, y), rel_l2(flat_of(a), flat_of(b)))


def composited(npa, raw, z, rays, noise, target, kind):
    """the tail of a chain of public pieces: ONE raw2outputs node for image and weights, distortion_loss on its weights"""
    if noise > 0:
        torch.manual_seed(NOISE_SEED)
    rgb, disp, acc, w, _ = npa.raw2outputs(raw, z, rays[:, 3:6], noise, True)
    out = dict(rgb_map=rgb, disp_map=disp, acc_map=acc, raw=raw, distortion=npa.distortion_loss(w, z, rays[:, 6], rays[:, 7]))
    return out, total(npa, out, target, kind)


def against_chain(npa, nets, grid, rays, target, kw, chain_raw_z, net, kind="both"):
    """render_rays(distortion=True, **kw) against a chain: outputs bit for bit, .grad of the evaluated network bit for bit"""
    nc, nf, _, _ = nets
    zero_grads(nc, nf)
    out = npa.render_rays(rays, nc, None, distortion=True, **kw)
    stats = dict(grid.last_stats)
    total(npa, out, target, kind).backward()
    got = grads_of(net)
    zero_grads(nc, nf)
    raw, z = chain_raw_z()
    want_out, loss = composited(npa, raw, z, rays, kw["raw_noise_std"], target, kind)
    loss.backward()
    want = grads_of(net)
    zero_grads(nc, nf)
    assert list(out)[-1] == "distortion"
    for k in ("rgb_map", "disp_map", "acc_map", "raw", "distortion"):
        assert bits_equal(out[k].detach(), want_out[k].detach()), k
    assert all(x is not None for x in got) and float(flat_of(got).abs().max()) > 0
    for i, (x, y) in enumerate(zip(got, want)):
        assert bits_equal(x, y), (i, maxdiff(x, y), rel_l2(flat_of(got), flat_of(want)))
    return out, stats


@pytest.mark.parametrize("kind", ["both", "alone"])
def test_grid_proposal_against_its_chain(npa, dev, nets, filled, datapath_fp16x3, kind):
    nc, nf, _, _ = nets
    rays, rnd, target = gp.scene(dev)
    grid = filled()
    kw = dict(N_samples=gp.N_C, N_importance=gp.N_F, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True,
              randoms=rnd, occupancy=grid, proposal="grid")

    def chain():
        out, z_f = gp.chain(npa, grid, rays, rnd, nf, 1.0, 0.0)      # (its own compositing is not used: no noise drawn)
        return out["raw"], z_f
    out, _ = against_chain(npa, nets, grid, rays, target, kw, chain, nf, kind)
    assert "rgb0" not in out and all(p.grad is None for p in nc.parameters())


@pytest.mark.parametrize("eps", [None, ms.STOP_EPS])
def test_the_march_in_world_steps_against_its_chain(npa, dev, nets, datapath_fp16x3, eps):
    """proposal="march" with march_step_size / march_fit, and with march_stop_eps on top: the padding slots repeat z_stop with w = 0"""
    nc, nf, _, _ = nets
    rays, rnd, target = ms.scene(dev)
    grid = ms.grid_of(npa, dev, "density" if eps is None else "stop", "evaluate")
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd,
              occupancy=grid, **ms.STEP_KW)
    if eps is not None:
        kw["march_stop_eps"] = eps

    def chain():
        out, z, *_ = ms.chain(npa, grid, rays, rnd["u_march"], nf, 0.0, eps)
        return out["raw"], z
    out, stats = against_chain(npa, nets, grid, rays, target, kw, chain, nf)
    assert stats["evaluated"] < stats["total"] and set(out) == {"rgb_map", "disp_map", "acc_map", "raw", "distortion"}
    if eps is not None:
        assert stats["rays_stopped"] > 0


def test_early_stop_and_clipping(npa, dev, nets, datapath_fp16x3):
    """early_stop_eps against the chain of tests/test_gpu_early_stop.py (the hooked path with the stopping hook), bit for bit; and
    clip_to_occupancy=True == the call on grid.clip_rays(rays)[0], for the key and the gradients too -- the loss's scale follows the
    clipped span, so the key differs from the unclipped call's"""
    nc, nf, _, _ = nets
    rays, rnd, target = _small_scene(dev)
    grid = ball_dgrid(npa, dev, outside="skip")
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, randoms=rnd, distortion=True)
    eps = eps_for(npa, grid, rays, nc, **{k: v for k, v in kw.items() if k != "distortion"})
    res = []
    chain = Chain(npa, grid, eps)
    for fn in (lambda: npa.render_rays(rays, nc, None, occupancy=grid, early_stop_eps=eps, **kw),
               lambda: chain.run(npa.render_rays, rays, nc, chain.hook, **kw)):
        zero_grads(nc, nf)
        out = fn()
        total(npa, out, target).backward()
        res.append(({k: v.detach() for k, v in out.items()}, grads_of(nc) + grads_of(nf)))
    assert grid.last_stats["rays_stopped"] > 0 and list(res[0][0])[-1] == "distortion"
    for k in res[0][0]:
        assert bits_equal(res[0][0][k], res[1][0][k]), k
    for i, (x, y) in enumerate(zip(res[0][1], res[1][1])):
        assert bits_equal(x, y), (i, maxdiff(x, y))
    clipped, hit = grid.clip_rays(rays)
    assert 0 < int(hit.sum())
    res = []
    for r, extra in ((rays, dict(clip_to_occupancy=True)), (clipped, {}), (rays, {})):
        zero_grads(nc, nf)
        out = npa.render_rays(r, nc, None, occupancy=grid, **kw, **extra)
        total(npa, out, target).backward()
        res.append((out["distortion"].detach(), flat_of(grads_of(nc) + grads_of(nf))))
    zero_grads(nc, nf)
    assert bits_equal(res[0][0], res[1][0]) and bits_equal(res[0][1], res[1][1]) and float(res[0][1].abs().max()) > 0
    assert not bits_equal(res[0][0], res[2][0])


def test_grid_sub_chunks_equal_one_piece(npa, dev, nets, monkeypatch, datapath_fp16x3):
    """2500 rays through the two-pass grid node under a budget forced to 1024 rays per sub-chunk: outputs bit for bit those of one
    piece, ray gradients finite, parameter gradients within twice the relative L2 distance the same two plans show without the
    option (or the fp32 noise floor 2^-23)"""
    hb = npa.hip_backend
    render_mod = sys.modules["nerf_pytorch_amd.render"]
    nc, nf, _, _ = nets
    n = 2500
    rays = orc.synthetic_rays(n, seed=8).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, 16, 48, seed=6).items()}
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    grid = ball_dgrid(npa, dev)
    kw = dict(randoms=rnd, N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=0.5, occupancy=grid)

    def run(option):
        zero_grads(nc, nf)
        r = rays.clone().requires_grad_(True)
        out = npa.render_rays(r, nc, None, distortion=option, **kw)
        if option:
            total(npa, out, target).backward()
        else:
            (npa.img2mse(out["rgb_map"], target) + npa.img2mse(out["rgb0"], target)).backward()
        return (render_mod.LAST_BACKWARD_PLAN[0], {k: v.detach() for k, v in out.items()},
                torch.cat([nc.last_flat_grad, nf.last_flat_grad]).clone(), r.grad.clone())
    one, one_off = run(True), run(False)
    monkeypatch.setattr(hb, "SAVE_BUDGET_BYTES", 1)
    sub, sub_off = run(True), run(False)
    zero_grads(nc, nf)
    assert one[0] == "one launch" and sub[0] == "resident sub-chunks"
    for k in one[1]:
        assert bits_equal(one[1][k], sub[1][k]), k
    diff, yard = rel_l2(sub[2], one[2]), rel_l2(sub_off[2], one_off[2])
    print(f"\ngrid sub-chunks vs one piece: parameter gradients relative L2 {diff:.3e} with the option, {yard:.3e} without; ray gradients "
          f"relative L2 {rel_l2(sub[3], one[3]):.1e}")
    assert diff <= max(2.0 * yard, 2.0 ** -23), (diff, yard)
    assert bool(torch.isfinite(sub[3]).all()) and float(sub[3].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 3. the other paths
def test_dense_networks(npa, dev, monkeypatch):
    """DenseNeRF networks (the layer-by-layer path): the option changes no other key; the key and the gradients of the distortion term
    against the same call with distortion_loss replaced by distortion_loss_reference in float64, by the hooked-path comparison"""
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
        if "distortion" in out:
            (LAM * out["distortion"].mean()).backward()
        return {k: v.detach() for k, v in out.items()}, [p.grad.clone() for p in net_f.parameters() if p.grad is not None]
    off, _ = run()
    on, g_on = run(distortion=True)
    assert list(on) == list(off) + ["distortion"] and on["distortion"].shape == (n,)
    for k in off:
        assert bits_equal(on[k], off[k]), k
    monkeypatch.setattr(render_mod, "distortion_loss",
                        lambda w, z, near, far: npa.distortion_loss_reference(w.double(), z.double(), near.double(), far.double()).float())
    ref, g_ref = run(distortion=True)
    assert maxdiff(on["distortion"], ref["distortion"]) <= 1e-6 * max(1.0, float(ref["distortion"].abs().max()))
    assert len(g_on) == len(g_ref) > 0 and float(on["distortion"].max()) > 1e-4
    for a, b in zip(g_on, g_ref):
        assert maxdiff(a, b) <= 1e-4 * float(b.abs().max()) + 1e-12


def test_empty_batch_and_render_in_chunks(npa, dev, nets, datapath_fp16x3):
    nc, nf, _, _ = nets
    kw = dict(N_samples=16, N_importance=24, network_fine=nf, white_bkgd=True)
    ret = npa.render_rays(torch.zeros(0, 11, device=dev), nc, None, distortion=True, **kw)
    assert list(ret)[-1] == "distortion" and ret["distortion"].shape == (0,) and ret["distortion"].device.type == "cuda"
    ret = npa.render_rays(torch.zeros(0, 11, device=dev), nc, None, distortion=True, occupancy=ball_dgrid(npa, dev), **kw)
    assert list(ret)[-1] == "distortion" and ret["distortion"].shape == (0,)
    # render(): extras["distortion"] with the rays' leading shape, the same bits whatever the chunking; differentiable
    rays = orc.synthetic_rays(12 * 20, seed=4).to(dev)
    K = np.array([[20.0, 0, 10.0], [0, 20.0, 6.0], [0, 0, 1]])
    geo = dict(rays=(rays[:, 0:3].reshape(12, 20, 3), rays[:, 3:6].reshape(12, 20, 3)), ndc=False, near=2.0, far=6.0, use_viewdirs=True,
               network_fn=nc, network_query_fn=None, distortion=True, **kw)
    with torch.no_grad():
        one = npa.render(12, 20, K, chunk=1 << 20, **geo)
        many = npa.render(12, 20, K, chunk=96, **geo)
    assert one[3]["distortion"].shape == (12, 20) and list(one[3])[-1] == "distortion"
    assert bits_equal(one[3]["distortion"], many[3]["distortion"]) and bits_equal(one[0], many[0])
    zero_grads(nc, nf)
    rgb, _, _, extras = npa.render(12, 20, K, chunk=96, **geo)
    (rgb.mean() + LAM * extras["distortion"].mean()).backward()
    assert bits_equal(extras["distortion"].detach(), one[3]["distortion"])
    assert float(flat_of(grads_of(nf)).abs().max()) > 0
    zero_grads(nc, nf)
