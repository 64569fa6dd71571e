"""GPU tests (-m gpu) of render_rays(proposal="grid"): nerf_occ_proposal_weights alone against DensityGrid.proposal_sigma and against
nerf_raw2outputs on raw = (0, 0, 0, sigma), then the render -- forward and backward -- against THE CHAIN, the same computation put
together from public pieces: hb.sample_coarse -> grid.proposal_sigma -> hb.raw2outputs' weights -> hb.sample_fine -> the compacting
hook (tests/test_gpu_occupancy_train.py) on o + d z_f with the evaluated network -> npa.raw2outputs.  The chain sends the same M
records through the same field launches, so the checks are bit for bit on the datapaths where the existing grid tests are."""
import sys

import numpy as np
import pytest
import torch

import nerf_oracle as orc
from test_gpu_occupancy import BOX_LO, BOX_HI, BOX_R, bits_equal
from test_gpu_occupancy_train import (U, _small_scene, ball_dgrid, compacting_hook, datapath_fp16x3, flat_of, fresh_nets,  # noqa: F401
                                      grads_of, positive_median_density, same_floats, scene_target, zero_grads)
from test_gpu_parity import datapath, dev, maxdiff, nets, npa  # noqa: F401  (fixtures)
from test_gpu_ray_grad import rel_l2

pytestmark = pytest.mark.gpu

N_C, N_F = 64, 128
NOISE_SEED = 4242


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def kernel_scene(npa, dev, outside, S):
    """a non-cubic grid with a random mask at share 0.35 and random densities (negatives and zeros among them); 301 rays: 0..99
    through the box, 100..199 with every sample ON a cell face (d = 0: the point is the origin; 100..119 the box's own corners), 200..279
    wholly outside the box, 280..284 with a NaN origin, 285..289 with a NaN direction, 290..300 through the box again"""
    g = torch.Generator().manual_seed(100 + S)
    res = (37, 21, 64)
    lo, hi = (-1.25, 0.5, -3.0), (1.75, 2.0, 0.2)
    grid = npa.DensityGrid.from_mask(torch.rand(res, generator=g) < 0.35, lo, hi, outside=outside, device=dev)
    grid.sigma_threshold = 0.7
    density = torch.randn(grid.n_cells, generator=g) * 3.0
    density[::7], density[3::11] = 0.0, -0.0
    grid.density = density.to(dev)
    n = 301
    lo_t, hi_t = torch.tensor(lo), torch.tensor(hi)
    o = lo_t + (hi_t - lo_t) * (torch.rand(n, 3, generator=g) * 1.2 - 0.1)
    d = torch.randn(n, 3, generator=g) * 0.6
    width = (hi_t - lo_t) / torch.tensor(res, dtype=torch.float32)
    k = torch.stack([torch.randint(0, r + 1, (100,), generator=g) for r in res], -1).float()
    o[100:200] = lo_t + k * width
    o[100:110], o[110:120] = lo_t, hi_t
    d[100:200] = 0.0
    o[200:280] = hi_t + 1.0 + torch.rand(80, 3, generator=g)
    d[200:280] = d[200:280].abs()               # (pointing away from the box)
    o[280:285, 0] = float("nan")
    d[285:290, 2] = float("nan")
    z = torch.sort(torch.rand(n, S, generator=g) * 2.0, -1).values
    rays = torch.cat([o, d, torch.zeros(n, 2), torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)], -1)
    return grid, rays.to(dev).contiguous(), z.to(dev).contiguous()


def weights_by_raw2outputs(hb, sigma, z, rays):
    raw = torch.cat([torch.zeros(sigma.shape + (3,), device=sigma.device), sigma[..., None]], -1).contiguous()
    return hb.raw2outputs(raw, z, rays, rays.shape[1], None, 0.0, False, want_weights=True, want_depth=False, rays_d_offset=3)[3]


@pytest.mark.parametrize("outside", ["evaluate", "skip"])
@pytest.mark.parametrize("S", [5, 64, 65, 192])
def test_kernel_equals_the_definition_and_raw2outputs_bit_for_bit(npa, dev, outside, S):
    """sigma == proposal_sigma(o + d z) and weights == nerf_raw2outputs' weights for raw = (0, 0, 0, sigma), no noise, bit for bit (a NaN
    ray gives NaNs in the same places); S = 64 / 65 straddle one and two samples per lane; two runs give the same bits; without the
    sigma buffer the weights are the same"""
    hb = npa.hip_backend
    grid, rays, z = kernel_scene(npa, dev, outside, S)
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]
    want_sigma = grid.proposal_sigma(pts)
    assert bits_equal(want_sigma.cpu(), grid.proposal_sigma(pts.cpu())), "proposal_sigma itself must not depend on the device"
    w, sigma = grid.proposal_weights(rays, z, want_sigma=True)
    torch.cuda.synchronize()
    assert bits_equal(sigma, want_sigma), int((sigma != want_sigma).sum())
    want_w = weights_by_raw2outputs(hb, sigma, z, rays)
    # (a NaN origin only puts the points outside the box: finite weights of the outside value; a NaN direction makes |d| a NaN)
    finite = ~torch.isnan(rays[:, 3:6]).any(-1)
    assert int(finite.sum()) == 296 and bool(torch.isnan(want_w[~finite]).all()) and not bool(torch.isnan(want_w[finite]).any())
    assert bits_equal(w[finite], want_w[finite]), maxdiff(w[finite], want_w[finite])
    assert same_floats(w, want_w)
    # the cases are there: looked-up densities of either sign and zero, cleared cells, the outside value, nonzero weights
    inside_set = grid.occupied(pts) & (want_sigma != (0.7 if outside == "evaluate" else 0.0))
    assert bool((sigma[inside_set] < 0).any()) and bool((sigma[inside_set] > 0).any()) and bool((sigma == 0).any())
    out_val = float(torch.tensor(0.7, dtype=torch.float32)) if outside == "evaluate" else 0.0
    assert bool((sigma[200:280] == out_val).all()) and bool((sigma[280:290] == out_val).all())
    assert bool((w[100:200] == 0).all())            # d = 0: every dist is 0
    assert float(w[finite].max()) > 0.01 and bool((w[finite] >= 0).all())
    if outside == "skip":
        assert bool((w[200:280] == 0).all())
    w2, sigma2 = grid.proposal_weights(rays, z, want_sigma=True)
    assert same_floats(w, w2) and bits_equal(sigma, sigma2)
    assert same_floats(w, grid.proposal_weights(rays, z))
    # a wider ray record (11 columns is the renderer's; 6 is the entry point's minimum)
    assert same_floats(w, grid.proposal_weights(rays[:, :6].contiguous(), z))


@pytest.mark.parametrize("outside", ["evaluate", "skip"])
def test_a_fresh_grid_gives_weights_that_are_exactly_zero(npa, dev, outside):
    """density = 0 and all bits set: alpha = 1 - exp(-0) = 0 for every sample inside the box, so its weight is exactly 0 whatever lies
    in front of it -- with outside="skip" that is every sample; with outside="evaluate" a sample outside the box carries sigma_threshold
    and a positive weight"""
    _, rays, z = kernel_scene(npa, dev, outside, 64)
    fresh = npa.DensityGrid((-1.25, 0.5, -3.0), (1.75, 2.0, 0.2), (37, 21, 64), outside=outside, device=dev, sigma_threshold=0.7)
    w, sigma = fresh.proposal_weights(rays, z, want_sigma=True)
    finite = ~torch.isnan(rays[:, 3:6]).any(-1)         # (a NaN direction makes |d|, and with it every weight of the ray, a NaN)
    if outside == "skip":
        assert bool((sigma == 0).all()) and bool((w[finite] == 0).all())
    else:
        inside = fresh.occupied(rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]) & (sigma == 0)
        assert bits_equal(sigma, torch.where(inside, 0.0, 0.7).to(torch.float32))
        assert int(inside[finite].sum()) > 1000 and bool((w[finite][inside[finite]] == 0).all())
        assert float(w[200:280].max()) > 0
    # the renderer's scene: every sample of the ball scene's rays that lies in the box has weight 0, and sample_fine makes of all-zero
    # weights the depths of a uniform pdf
    ball = npa.DensityGrid(BOX_LO, BOX_HI, BOX_R, outside="skip", device=dev)
    rays_b, _, _ = _small_scene(dev)
    hb = npa.hip_backend
    z_c = hb.sample_coarse(rays_b, torch.linspace(0.0, 1.0, N_C, device=dev), False, None)
    w_b = ball.proposal_weights(rays_b, z_c)
    assert bool((w_b == 0).all())
    lin = torch.linspace(0.0, 1.0, N_F, device=dev)
    z_f, _, z_s = hb.sample_fine(z_c, w_b, N_F, None, lin, want_samples=True)
    mid = 0.5 * (z_c[:, 1:] + z_c[:, :-1])
    uniform = mid[:, :1] + (mid[:, -1:] - mid[:, :1]) * lin
    # (an evenly spaced 62-step cdf inverted at an even u: the cdf's fp32 cumulative sum is within 62 * 2^-24 of exact, the depths span
    # less than 4, and the bound is doubled for the inversion's own roundings)
    assert float((z_s - uniform).abs().max()) <= 2.0 * 62 * U * 4.0


# ------------------------------------------------------------------------------------------------ 2. the render against the chain
@pytest.fixture(scope="module")
def filled(npa, dev, nets):
    """the 32^3 ball scene's DensityGrid (the ball's bits) with the densities of one update on the fixture's fine network, and the
    threshold that update used; never modified by a test"""
    nf = nets[1]
    thr = positive_median_density(npa, nf, dev, BOX_R)
    with torch.no_grad():
        probe = npa.DensityGrid(BOX_LO, BOX_HI, BOX_R, device=dev, sigma_threshold=thr).update(nf)

    def make(outside="evaluate"):
        g = ball_dgrid(npa, dev, sigma_threshold=thr, outside=outside)
        g.density = probe.density.clone()
        return g
    assert float(probe.density.max()) > thr
    return make


def chain(npa, grid, rays, rnd, net, perturb, noise, white=True, seen=None, taps=None):
    """THE YARDSTICK: render_rays(proposal="grid") from public pieces.  `noise` > 0: npa.raw2outputs draws its own noise from the
    device's global generator -- seeded here so that it draws rnd["noise_f"] (noise_f_of)."""
    hb = npa.hip_backend
    dev, n = rays.device, rays.shape[0]
    r0 = rays.detach()
    z_c = hb.sample_coarse(r0, torch.linspace(0.0, 1.0, N_C, device=dev), False, rnd["t_rand"] if perturb > 0 else None)
    sigma = grid.proposal_sigma(r0[:, None, 0:3] + r0[:, None, 3:6] * z_c[:, :, None])
    w = weights_by_raw2outputs(hb, sigma, z_c, r0)
    u = rnd["u"] if perturb > 0 else None
    z_f, z_std, _ = hb.sample_fine(z_c, w, N_F, u, None if u is not None else torch.linspace(0.0, 1.0, N_F, device=dev))
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z_f[:, :, None]
    raw = compacting_hook(npa, grid, seen, taps)(pts, rays[:, 8:11], net)
    if noise > 0:
        torch.manual_seed(NOISE_SEED)
    rgb, disp, acc, _, _ = npa.raw2outputs(raw, z_f, rays[:, 3:6], noise, white)
    return dict(z_std=z_std, rgb_map=rgb, disp_map=disp, acc_map=acc, raw=raw), z_f


def noise_f_of(dev, n):
    """the draws npa.raw2outputs makes after torch.manual_seed(NOISE_SEED)"""
    torch.manual_seed(NOISE_SEED)
    return torch.randn((n, N_C + N_F), device=dev)


def scene(dev, n=256):
    rays, rnd, target = _small_scene(dev, n)
    rnd = dict(rnd, noise_f=noise_f_of(dev, n))
    return rays, rnd, target


@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
@pytest.mark.parametrize("perturb,noise", [(1.0, 1.0), (0.0, 0.0)])
@pytest.mark.parametrize("outside", ["evaluate", "skip"])
def test_no_grad_render_equals_the_chain_bit_for_bit(npa, dev, nets, datapath, filled, perturb, noise, outside):
    """256 rays, 64 + 128 samples, perturbed with noise and deterministic: rgb_map, disp_map, acc_map, z_std and raw equal the chain's
    bit for bit (fp32 and fp16x3: the datapaths of test_gpu_occupancy's bit-for-bit render tests), the keys are the mode's (no rgb0),
    last_stats counts the one pass, the coarse network is never launched, and noise_c in `randoms` is ignored"""
    nc, nf, _, _ = nets
    rays, rnd, _ = scene(dev)
    grid = filled(outside)
    kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=perturb, raw_noise_std=noise, retraw=True)
    seen = []
    calls = []
    packed = nc.packed_params
    nc.packed_params = lambda *a, **k: (calls.append(a), packed(*a, **k))[1]
    try:
        with torch.no_grad():
            want, _ = chain(npa, grid, rays, rnd, nf, perturb, noise, seen=seen)
            got = npa.render_rays(rays, nc, None, occupancy=grid, proposal="grid", randoms=rnd, **kw)
            stats = dict(grid.last_stats)
            poisoned = dict(rnd, noise_c=torch.full((rays.shape[0], N_C), float("nan"), device=dev))
            again = npa.render_rays(rays, nc, None, occupancy=grid, proposal="grid", randoms=poisoned, **kw)
    finally:
        del nc.packed_params
    assert calls == []
    assert list(got) == ["z_std", "rgb_map", "disp_map", "acc_map", "raw"]
    for k in got:
        assert bits_equal(got[k], want[k]), (k, maxdiff(got[k], want[k]))
        assert bits_equal(got[k], again[k]), k
    assert stats == {"evaluated": seen[0][0], "total": rays.shape[0] * (N_C + N_F)} and 0 < stats["evaluated"] < stats["total"]
    assert float(got["acc_map"].max()) > 0.5 and got["raw"].shape == (rays.shape[0], N_C + N_F, 4)


def test_shared_network_and_the_reduced_inference_class(npa, dev, nets, filled):
    """network_fine=None: the one pass runs on network_fn.  "fp16_fp8c" maps to fp16x3 on the grid path, here as without the option."""
    nc, _, _, _ = nets
    rays, rnd, _ = scene(dev)
    grid = filled()
    kw = dict(N_samples=N_C, N_importance=N_F, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd, occupancy=grid,
              proposal="grid")
    prev = npa.get_precision()
    try:
        npa.set_precision("fp16x3")
        with torch.no_grad():
            want, _ = chain(npa, grid, rays, rnd, nc, 1.0, 1.0)
            got = npa.render_rays(rays, nc, None, **kw)
            npa.set_precision("fp16_fp8c")
            reduced = npa.render_rays(rays, nc, None, **kw)
    finally:
        npa.set_precision(prev)
    for k in got:
        assert bits_equal(got[k], want[k]) and bits_equal(got[k], reduced[k]), k


@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
def test_clipping_first_equals_the_call_on_clipped_rays(npa, dev, nets, datapath, filled):
    """clip_to_occupancy=True + proposal="grid" == the same call on grid.clip_rays(rays)[0], bit for bit, with and without gradients;
    last_stats keeps rays_hit / rays"""
    nc, nf, _, _ = nets
    rays, rnd, target = scene(dev)
    grid = filled("skip")
    kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd,
              occupancy=grid, proposal="grid")
    clipped, hit = grid.clip_rays(rays)
    assert 0 < int(hit.sum()) and not bits_equal(clipped, rays)
    with torch.no_grad():
        got = npa.render_rays(rays, nc, None, clip_to_occupancy=True, **kw)
        stats = dict(grid.last_stats)
        want = npa.render_rays(clipped, nc, None, **kw)
    assert stats == dict(grid.last_stats, rays_hit=int(hit.sum()), rays=rays.shape[0]) and stats["total"] == rays.shape[0] * (N_C + N_F)
    for k in want:
        assert bits_equal(got[k], want[k]), k
    grads = []
    for r, extra in ((rays, dict(clip_to_occupancy=True)), (clipped, {})):
        zero_grads(nc, nf)
        npa.img2mse(npa.render_rays(r, nc, None, **kw, **extra)["rgb_map"], target).backward()
        grads.append(flat_of(grads_of(nf)))
    zero_grads(nc, nf)
    assert bits_equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0


@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
@pytest.mark.parametrize("perturb,noise", [(1.0, 1.0), (0.0, 0.0)])
def test_forward_with_grad_equals_the_no_grad_render(npa, dev, nets, datapath, filled, perturb, noise):
    nc, nf, _, _ = nets
    rays, rnd, _ = scene(dev)
    grid = filled()
    kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=perturb, raw_noise_std=noise, retraw=True, randoms=rnd,
              occupancy=grid, proposal="grid")
    with torch.no_grad():
        want = npa.render_rays(rays, nc, None, **kw)
    stats = dict(grid.last_stats)
    grid.last_stats = None
    got = npa.render_rays(rays, nc, None, **kw)
    assert list(got) == list(want)
    for k in want:
        assert bits_equal(got[k], want[k]), (k, maxdiff(got[k], want[k]))
    assert grid.last_stats == stats
    assert got["rgb_map"].grad_fn is not None and got["raw"].grad_fn is not None and not got["z_std"].requires_grad
    del got          # (a graph dropped without backward)


# ------------------------------------------------------------------------------------------------ 3. backward
@pytest.mark.parametrize("datapath", ["fp32", "fp16x3", "fp16x3w", "bf16x3"], indirect=True)
def test_parameter_gradients_equal_the_chains_bit_for_bit(npa, dev, nets, datapath, filled):
    """loss = img2mse(rgb_map, t): .grad of every parameter of the evaluated (fine) network equals autograd's through the chain, bit for
    bit, on the datapaths of test_parameter_gradients_two_networks_bit_for_bit; the coarse network's .grad stays None; with
    network_fine=None the one network is network_fn"""
    nc, nf, _, _ = nets
    rays, rnd, target = scene(dev)
    grid = filled()
    kw = dict(N_samples=N_C, N_importance=N_F, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, randoms=rnd, occupancy=grid, proposal="grid")
    for net, fine in ((nf, nf), (nc, None)):
        zero_grads(nc, nf)
        out = npa.render_rays(rays, nc, None, network_fine=fine, **kw)
        assert "rgb0" not in out
        loss_g = npa.img2mse(out["rgb_map"], target)
        loss_g.backward()
        other = nc if net is nf else nf
        assert all(p.grad is None for p in other.parameters())
        got = grads_of(net)
        zero_grads(nc, nf)
        ref, _ = chain(npa, grid, rays, rnd, net, 1.0, 1.0)
        loss_h = npa.img2mse(ref["rgb_map"], target)
        loss_h.backward()
        want = grads_of(net)
        zero_grads(nc, nf)
        assert bits_equal(loss_g.detach(), loss_h.detach())
        assert all(x is not None for x in got) and float(flat_of(got).abs().max()) > 0
        for i, (x, y) in enumerate(zip(got, want)):
            assert bits_equal(x, y), (i, maxdiff(x, y), rel_l2(flat_of(got), flat_of(want)))


@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
def test_ray_gradients_against_the_float64_fold_of_the_chain(npa, dev, nets, datapath, filled, monkeypatch):
    """rays.requires_grad_(): the chain yields the per-point gradients d_pts / d_viewdirs of the M evaluated points (tensor hooks) and
    the compositing's d_rays_d; their float64 fold -- [0:3] sum d_pts, [3:6] sum z d_pts + the |d| term, [8:11] sum d_viewdirs -- is what
    rays.grad must equal within (S + 1) * 2^-24 * sum|terms| * 1.01 per element, S = 192: the bound
    test_ray_gradients_against_the_float64_fold_of_the_hooks derives (S fp32 terms in any order with one product rounding each, one more
    rounding for the added |d| term), for the one pass there is.  Columns 6:8 are exactly 0."""
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    rays0, rnd, target = scene(dev)
    grid = filled()
    kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=0.5, randoms=rnd, occupancy=grid,
              proposal="grid")
    rg = rays0.clone().requires_grad_(True)
    npa.img2mse(npa.render_rays(rg, nc, None, **kw)["rgb_map"], target).backward()
    got = rg.grad.clone()
    dns, taps = [], []
    bwd = hb.raw2outputs_bwd
    monkeypatch.setattr(hb, "raw2outputs_bwd", lambda *a, **k: (dns.append(k.get("d_rays_d")), bwd(*a, **k))[1])
    rh = rays0.clone().requires_grad_(True)
    ref, z_f = chain(npa, grid, rh, rnd, nf, 1.0, 0.5, taps=taps)
    npa.img2mse(ref["rgb_map"], target).backward()
    zero_grads(nc, nf)
    assert len(taps) == 1 and len(dns) == 1 and dns[0] is not None
    n, S, tap = rays0.shape[0], N_C + N_F, taps[0]
    want = torch.zeros(n, 11, dtype=torch.float64, device=dev)
    mag = torch.zeros_like(want)
    ray_of = tap["idx"] // S
    gp, gv, zz = tap["d_pts"].double(), tap["d_viewdirs"].double(), z_f.reshape(-1)[tap["idx"]].double()[:, None]
    for cols, terms in ((slice(0, 3), gp), (slice(3, 6), zz * gp), (slice(8, 11), gv)):
        want[:, cols] = want[:, cols].index_add(0, ray_of, terms)
        mag[:, cols] = mag[:, cols].index_add(0, ray_of, terms.abs())
    want[:, 3:6] += dns[0].double()
    mag[:, 3:6] += dns[0].double().abs()
    err = (got.double() - want).abs()
    bound = 1.01 * (S + 1) * U * mag
    geo = [0, 1, 2, 3, 4, 5, 8, 9, 10]
    print(f"\n[{datapath}] ray gradient: worst error / bound {float((err[:, geo] / bound[:, geo].clamp(min=1e-300)).max()):.3f}; "
          f"relative L2 vs the chain's own rays.grad {rel_l2(got, rh.grad):.2e}")
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    assert bool((got[:, 6:8] == 0).all())
    assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())


def test_grad_ready_fires_once_and_the_other_network_is_never_touched(npa, dev, nets, filled):
    render_mod = sys.modules["nerf_pytorch_amd.render"]
    nc, nf = fresh_nets(npa, dev, nets)
    rays, rnd, target = scene(dev)
    grid = filled()
    fired = []
    hook = lambda model, flat: fired.append((model, flat, flat.clone()))
    render_mod.GRAD_READY_HOOKS.append(hook)
    try:
        out = npa.render_rays(rays, nc, None, N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=1.0, randoms=rnd,
                              occupancy=grid, proposal="grid")
        npa.img2mse(out["rgb_map"], target).backward()
    finally:
        render_mod.GRAD_READY_HOOKS.remove(hook)
    assert len(fired) == 1 and fired[0][0] is nf
    _, flat, at_hook = fired[0]
    assert flat is nf.last_flat_grad and flat.shape == (npa.hip_backend.N_PARAMS,) and bits_equal(flat, at_hook)
    assert all(p.grad is not None and p.grad.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() for p in nf.parameters())
    assert all(p.grad is None for p in nc.parameters()) and getattr(nc, "last_flat_grad", None) is None
    assert float(flat.abs().max()) > 0


def test_frozen_network_second_backward_and_stale_parameters(npa, dev, nets, filled, datapath_fp16x3):
    render_mod = sys.modules["nerf_pytorch_amd.render"]
    hb = npa.hip_backend
    nc, nf = fresh_nets(npa, dev, nets)
    rays, rnd, target = scene(dev)
    grid = filled()
    kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=1.0, randoms=rnd, occupancy=grid, proposal="grid")
    # a frozen evaluated network under rays that need a gradient: the delta chain runs, no weight-gradient GEMM, no _grad_ready
    for p in nf.parameters():
        p.requires_grad_(False)
    fired, wgrad_calls = [], []
    hook = lambda model, flat: fired.append(model)
    render_mod.GRAD_READY_HOOKS.append(hook)
    real_bwd = hb.field_bwd
    r = rays.clone().requires_grad_(True)
    try:
        hb.field_bwd = lambda packed, act, d_raw, grad, *a, **k: (wgrad_calls.append(grad is not None), real_bwd(packed, act, d_raw, grad, *a, **k))[1]
        npa.img2mse(npa.render_rays(r, nc, None, **kw)["rgb_map"], target).backward()
    finally:
        hb.field_bwd = real_bwd
        render_mod.GRAD_READY_HOOKS.remove(hook)
    assert fired == [] and wgrad_calls == [False]
    assert all(p.grad is None for p in nf.parameters()) and all(p.grad is None for p in nc.parameters())
    assert r.grad is not None and float(r.grad.abs().max()) > 0
    # frozen and nothing else to differentiate: the render is the no_grad one, whatever the coarse network requires
    out = npa.render_rays(rays, nc, None, **kw)
    assert out["rgb_map"].grad_fn is None
    for p in nf.parameters():
        p.requires_grad_(True)
    # a second backward through the same graph
    loss = npa.img2mse(npa.render_rays(rays, nc, None, **kw)["rgb_map"], target)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="already consumed"):
        loss.backward()
    zero_grads(nc, nf)
    # an optimizer step between forward and backward
    opt = npa.FlatAdam(list(nf.parameters()), lr=5e-4)
    npa.img2mse(npa.render_rays(rays, nc, None, **kw)["rgb_map"], target).backward()
    loss = npa.img2mse(npa.render_rays(rays, nc, None, **kw)["rgb_map"], target)
    opt.step()
    with pytest.raises(RuntimeError, match="parameters changed between"):
        loss.backward()


def test_resident_sub_chunks_give_the_gradients_of_one_piece(npa, dev, nets, filled, monkeypatch, datapath_fp16x3):
    """As test_gpu_occupancy_train.test_resident_sub_chunks_give_the_gradients_of_one_piece, for the one-pass mode: 2500 rays under
    SAVE_BUDGET_BYTES forced down to 1024 rays per sub-chunk (hb.max_saved_rays never goes below 1024, so fewer rays cannot split): the
    plan says "resident sub-chunks" and the evaluated network's gradient matches the one-piece call within that test's bound -- twice the
    relative L2 difference between the dense _RenderRays path (sub-chunks accumulated in the weight-gradient kernel) and the stock hooked
    path (one piece) on the same rays under the same forced budget, taken over the same (fine) network's vector.  The ray gradients are
    bit-identical or reported.  A total budget of zero raises and names the budget."""
    hb = npa.hip_backend
    render_mod = sys.modules["nerf_pytorch_amd.render"]
    nc, nf, _, _ = nets
    n = 2500
    rays = orc.synthetic_rays(n, seed=8).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, N_C, N_F, seed=6).items()}
    target = scene_target(dev, n)
    grid = filled()
    kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=0.5, randoms=rnd)

    def run(**extra):
        zero_grads(nc, nf)
        r = rays.clone().requires_grad_(True)
        out = npa.render_rays(r, nc, extra.pop("hook", None), **kw, **extra)
        npa.img2mse(out["rgb_map"], target).backward()
        return render_mod.LAST_BACKWARD_PLAN, nf.last_flat_grad.clone(), r.grad.clone()
    plan1, g1, r1 = run(occupancy=grid, proposal="grid")
    stats1 = dict(grid.last_stats)
    _, stock, _ = run(hook=lambda p, v, m: npa.run_network(p, v, m, None, None))
    monkeypatch.setattr(hb, "SAVE_BUDGET_BYTES", 4 * hb.workspace_floats(1024, N_C, N_F, True, "fp16x3") + 1)
    plan2, g2, r2 = run(occupancy=grid, proposal="grid")
    plan_dense, dense, _ = run()
    zero_grads(nc, nf)
    assert plan1 == ("one launch", n, n) and plan2[0] == "resident sub-chunks" and plan2[1] == n and plan2[2] <= 1024
    assert plan_dense[0] == "resident sub-chunks"
    assert grid.last_stats == stats1 and stats1["total"] == n * (N_C + N_F)
    diff, yard = rel_l2(g2, g1), rel_l2(dense, stock)
    print(f"\nsub-chunks vs one piece: parameter gradients relative L2 {diff:.3e} (yardstick {yard:.3e}); ray gradients bit-identical "
          f"{torch.equal(r1, r2)}, relative L2 {rel_l2(r2, r1):.1e}")
    assert diff <= 2.0 * yard
    assert bool(torch.isfinite(r2).all())
    monkeypatch.setattr(hb, "SAVE_TOTAL_BYTES", 0)
    with pytest.raises(RuntimeError, match="SAVE_TOTAL_BYTES"):
        npa.render_rays(rays, nc, None, occupancy=grid, proposal="grid", **kw)


# ------------------------------------------------------------------------------------------------ 4. plumbing
def test_draw_order_and_the_layers_that_forward_the_keyword(npa, dev, nets, filled):
    """without `randoms` the draws are t_rand, u, noise_f in that order from the device's generator (no noise_c); render() and
    batchify_rays hand `proposal` on with `occupancy`, chunked calls sum last_stats; the empty batch has the mode's keys"""
    nc, nf, _, _ = nets
    rays, _, _ = scene(dev)
    n = rays.shape[0]
    grid = filled()
    kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, occupancy=grid,
              proposal="grid")
    with torch.no_grad():
        torch.manual_seed(99)
        drawn = npa.render_rays(rays, nc, None, **kw)
        torch.manual_seed(99)
        rnd = dict(t_rand=torch.rand((n, N_C), device=dev), u=torch.rand((n, N_F), device=dev), noise_f=torch.randn((n, N_C + N_F), device=dev))
        given = npa.render_rays(rays, nc, None, randoms=rnd, **kw)
        for k in given:
            assert bits_equal(drawn[k], given[k]), k
        total = dict(grid.last_stats)
        chunked = npa.batchify_rays(rays, 100, network_fn=nc, network_query_fn=None, randoms=rnd, **kw)
        assert grid.last_stats == total and list(chunked) == list(given)
        for k in given:
            assert bits_equal(chunked[k], given[k]), k
        K = np.array([[20.0, 0, 8.0], [0, 20.0, 8.0], [0, 0, 1]])
        rgb, disp, acc, extras = npa.render(16, 16, K, chunk=100, rays=(rays[:, 0:3], rays[:, 3:6]), ndc=False, near=2.0, far=6.0,
                                            use_viewdirs=True, network_fn=nc, network_query_fn=None, **dict(kw, perturb=0.0, raw_noise_std=0.0))
        assert set(extras) == {"z_std", "raw"} and rgb.shape == (n, 3) and grid.last_stats["total"] == n * (N_C + N_F)
        empty = npa.render_rays(rays[:0], nc, None, **kw)
    assert list(empty) == ["rgb_map", "disp_map", "acc_map", "raw", "z_std"] and empty["raw"].shape == (0, N_C + N_F, 4)
    assert grid.last_stats == {"evaluated": 0, "total": 0}
