"""GPU tests (-m gpu) of render_rays(proposal="march"): nerf_occ_march alone against its definition (OccupancyGrid.march_reference,
evaluated on the CPU) as raw bits, then the render -- forward and backward -- against THE CHAIN, the same computation put together
from public pieces: march_reference -> pts = o + d z -> the compacting hook of tests/test_gpu_occupancy_train.py with the extra
predicate z < z_stop -> npa.raw2outputs.  The chain sends the same M records through the same field launches, so the checks are bit
for bit on the datapaths where the existing grid tests are."""
import sys

import numpy as np
import pytest
import torch

import nerf_oracle as orc
from test_gpu_occupancy import BOX_HI, BOX_LO, ball_grid, bits_equal, masking_hook
from test_gpu_occupancy_train import (U, _small_scene, ball_dgrid, datapath_fp16x3, flat_of, fresh_nets, grads_of,  # noqa: F401
                                      scene_target, zero_grads)
from test_gpu_parity import datapath, dev, maxdiff, nets, npa  # noqa: F401  (fixtures)
from test_gpu_ray_grad import rel_l2

pytestmark = pytest.mark.gpu

M_STEPS, N_SLOTS = 256, 64
NOISE_SEED = 4242
INF = float("inf")


def reference_on_cpu(grid, rays, u, M, S):
    """the definition, evaluated on the CPU (its one division is IEEE there whatever the device's torch build does), on `rays`' device"""
    out = grid.march_reference(rays.detach().cpu(), None if u is None else u.cpu(), M, S)
    return tuple(t.to(rays.device) for t in out)


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
N_KERNEL = 301
INVALID = {"NaN origin": 17, "NaN direction": 80, "infinite direction": 129, "NaN near": 190, "infinite far": 191, "near == far": 255,
           "near > far": 256, "-inf origin": 300}


def kernel_scene(npa, dev, outside):
    """a non-cubic grid with a random mask at share 0.35 whose lower half in z is cleared; 301 rays (four rays per block: 76 blocks, the last one ragged) that start
    around the box and point anywhere, near 0 .. 0.5, far 0.5 .. 3.5 behind it; 40 of them with d = 0 (every candidate is the same
    point, on a cell face for 20 of them), 60 slow ones that start in the cleared half (under outside="evaluate" the rays that emit
    little); the invalid ones of INVALID planted in the first, in middle and in the last block"""
    g = torch.Generator().manual_seed(31)
    res = (37, 21, 64)
    lo, hi = (-1.25, 0.5, -3.0), (1.75, 2.0, 0.2)
    mask = torch.rand(res, generator=g) < 0.35
    mask[:, :, :32] = False
    grid = npa.OccupancyGrid.from_mask(mask, lo, hi, outside=outside, device=dev)
    n = N_KERNEL
    lo_t, hi_t = torch.tensor(lo), torch.tensor(hi)
    o = lo_t + (hi_t - lo_t) * (torch.rand(n, 3, generator=g) * 1.4 - 0.2)
    d = torch.randn(n, 3, generator=g) * 0.8
    near = 0.5 * torch.rand(n, 1, generator=g)
    far = near + 0.5 + 3.0 * torch.rand(n, 1, generator=g)
    d[200:240] = 0.0
    o[240:300] = lo_t + (hi_t - lo_t) * (torch.tensor([0.2, 0.2, 0.1]) + torch.tensor([0.6, 0.6, 0.3]) * torch.rand(60, 3, generator=g))
    d[240:300] = torch.randn(60, 3, generator=g) * 0.2
    width = (hi_t - lo_t) / torch.tensor(res, dtype=torch.float32)
    o[200:220] = lo_t + torch.stack([torch.randint(0, r + 1, (20,), generator=g) for r in res], -1).float() * width
    rays = torch.cat([o, d, near, far, torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)], -1)
    rays[INVALID["NaN origin"], 1] = float("nan")
    rays[INVALID["NaN direction"], 3] = float("nan")
    rays[INVALID["infinite direction"], 5] = INF
    rays[INVALID["NaN near"], 6] = float("nan")
    rays[INVALID["infinite far"], 7] = INF
    rays[INVALID["near == far"], 6] = rays[INVALID["near == far"], 7]
    rays[INVALID["near > far"], 6] = rays[INVALID["near > far"], 7] + 1.0
    rays[INVALID["-inf origin"], 0] = -INF
    u = torch.rand(n, generator=g)
    u[5], u[6] = 0.0, float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    return grid, rays, u


@pytest.mark.parametrize("outside", ["evaluate", "skip"])
@pytest.mark.parametrize("M,S", [(1, 1), (7, 2), (64, 5), (65, 64), (256, 64), (1024, 192)])
def test_kernel_equals_the_definition_bit_for_bit(npa, dev, outside, M, S):
    """z_vals, z_stop and truncated equal march_reference's as raw bits: M around the 64-candidate round (1, 7, 64, 65) and many rounds,
    S from 1 up, u random (0 and the largest fp32 below 1 among them) and None, ray records of 8 and of 11 columns, twice"""
    hb = npa.hip_backend
    grid, rays, u = kernel_scene(npa, dev, outside)
    invalid = torch.tensor(sorted(INVALID.values()))
    seen = {"truncated": 0, "fit": 0, "miss": 0}
    for uu in (u, None):
        want = grid.march_reference(rays, uu, M, S)
        for cols in (11, 8):
            r = rays[:, :cols].contiguous().to(dev)
            z, z_stop, tr = hb.occ_march(grid._desc(), r, None if uu is None else uu.to(dev), M, S)
            torch.cuda.synchronize()
            assert z.shape == (N_KERNEL, S) and z.dtype == torch.float32 and z_stop.shape == tr.shape == (N_KERNEL,) and tr.dtype == torch.int32
            assert bits_equal(z.cpu(), want[0]), int((z.cpu() != want[0]).sum())
            assert bits_equal(z_stop.cpu(), want[1]) and torch.equal(tr.cpu().bool(), want[2])
        again = grid.march(rays.to(dev), M, S, u=None if uu is None else uu.to(dev))
        assert bits_equal(again[0], z) and bits_equal(again[1], z_stop) and torch.equal(again[2], tr.bool()) and again[2].dtype == torch.bool
        # the invalid rays: their own far in every slot, -inf, not truncated
        assert bits_equal(z.cpu()[invalid], rays[invalid, 7:8].expand(-1, S).contiguous())
        assert bool((z_stop.cpu()[invalid] == -INF).all()) and not bool(tr.cpu()[invalid].any())
        valid = torch.ones(N_KERNEL, dtype=torch.bool)
        valid[invalid] = False
        assert bool((z.cpu()[valid][:, 1:] >= z.cpu()[valid][:, :-1]).all())
        miss = valid & ~want[2] & (want[0][:, 0] == rays[:, 7])
        seen["truncated"] += int(want[2].sum())
        seen["miss"] += int(miss.sum())
        seen["fit"] += int((valid & ~want[2] & ~miss).sum())
    if (M, S) == (256, 64):         # the cases are there
        assert min(seen.values()) >= 16, seen
    if S == 1:                      # no slot but the stop depth's: every valid ray that emits anything is truncated
        assert seen["fit"] == 0 and seen["truncated"] > 0


# ------------------------------------------------------------------------------------------------ 2. the render against the chain
def stopping_hook(npa, grid, z, z_stop, seen=None, taps=None):
    """compacting_hook (tests/test_gpu_occupancy_train.py) with one more predicate: a sample at or behind its ray's stop depth is not
    evaluated either -- nerf_occ_compact_stop's not (z >= z_stop)"""
    def hook(pts, viewdirs, net):
        N, S = pts.shape[:2]
        keep = grid.occupied(pts) & ~(z >= z_stop[:, None])
        idx = keep.reshape(-1).nonzero()[:, 0]
        if seen is not None:
            seen.append((int(idx.numel()), N * S))
        p_sel = pts.reshape(-1, 3)[idx]
        v_sel = viewdirs[:, None].expand_as(pts).reshape(-1, 3)[idx]
        if taps is not None:
            tap = {"idx": idx, "N": N, "S": S}
            taps.append(tap)
            if p_sel.requires_grad:
                p_sel.register_hook(lambda g, tap=tap: tap.__setitem__("d_pts", g.detach().clone()))
                v_sel.register_hook(lambda g, tap=tap: tap.__setitem__("d_viewdirs", g.detach().clone()))
        raw_c = npa.query_points(net, p_sel, v_sel) if idx.numel() else torch.zeros(0, 4, device=pts.device)
        return torch.zeros(N * S, 4, device=pts.device).index_put((idx,), raw_c).view(N, S, 4)
    return hook


def chain(npa, grid, rays, u, net, noise, M=M_STEPS, S=N_SLOTS, white=True, seen=None, taps=None):
    """THE YARDSTICK: render_rays(proposal="march") from public pieces.  `noise` > 0: npa.raw2outputs draws its own noise from the
    device's global generator -- seeded here so that it draws noise_of(dev, n, S)."""
    z, z_stop, tr = reference_on_cpu(grid, rays, u, M, S)
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]
    raw = stopping_hook(npa, grid, z, z_stop, seen, taps)(pts, rays[:, 8:11], net)
    if noise > 0:
        torch.manual_seed(NOISE_SEED)
    rgb, disp, acc, _, _ = npa.raw2outputs(raw, z, rays[:, 3:6], noise, white)
    return dict(rgb_map=rgb, disp_map=disp, acc_map=acc, raw=raw), z, z_stop, tr


def noise_of(dev, n, S=N_SLOTS):
    """the draws npa.raw2outputs makes after torch.manual_seed(NOISE_SEED)"""
    torch.manual_seed(NOISE_SEED)
    return torch.randn((n, S), device=dev)


def scene(dev, n=256, S=N_SLOTS):
    rays, _, target = _small_scene(dev, n)
    u = torch.rand(n, generator=torch.Generator().manual_seed(23)).to(dev)
    return rays, {"u_march": u, "noise_f": noise_of(dev, n, S)}, target


def grid_of(npa, dev, kind, outside):
    if kind == "plain":
        return ball_grid(npa, dev, outside)
    return ball_dgrid(npa, dev, outside=outside)


@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
@pytest.mark.parametrize("perturb,noise", [(1.0, 1.0), (0.0, 0.0)])
@pytest.mark.parametrize("outside", ["evaluate", "skip"])
@pytest.mark.parametrize("kind", ["plain", "density"])
def test_no_grad_render_equals_the_chain_bit_for_bit(npa, dev, nets, datapath, perturb, noise, outside, kind):
    """256 rays, M = 256, S = 64: rgb_map, disp_map, acc_map and raw equal the chain's bit for bit; the keys are the mode's; N_samples =
    64, N_importance = 0 gives the bits of 16 + 48; last_stats counts what the hook evaluated and the rays the definition truncates;
    the other network is never launched; t_rand, u and noise_c in `randoms` are not read"""
    nc, nf, _, _ = nets
    rays, rnd, _ = scene(dev)
    n = rays.shape[0]
    grid = grid_of(npa, dev, kind, outside)
    kw = dict(network_fine=nf, white_bkgd=True, perturb=perturb, raw_noise_std=noise, retraw=True, occupancy=grid, proposal="march",
              march_steps=M_STEPS)
    seen, calls = [], []
    packed = nc.packed_params
    nc.packed_params = lambda *a, **k: (calls.append(a), packed(*a, **k))[1]
    try:
        with torch.no_grad():
            want, z, z_stop, tr = chain(npa, grid, rays, rnd["u_march"] if perturb > 0 else None, nf, noise, seen=seen)
            got = npa.render_rays(rays, nc, None, N_samples=16, N_importance=48, randoms=rnd, **kw)
            stats = dict(grid.last_stats)
            nan = lambda *s: torch.full(s, float("nan"), device=dev)
            poisoned = dict(rnd, t_rand=nan(n, 64), u=nan(n, 0), noise_c=nan(n, 64))
            again = npa.render_rays(rays, nc, None, N_samples=64, N_importance=0, randoms=poisoned, **kw)
            assert grid.last_stats == stats
    finally:
        del nc.packed_params
    assert calls == []
    assert list(got) == list(again) == ["rgb_map", "disp_map", "acc_map", "raw"]
    for k in got:
        assert bits_equal(got[k], want[k]), (k, maxdiff(got[k], want[k]))
        assert bits_equal(got[k], again[k]), k
    assert got["raw"].shape == (n, N_SLOTS, 4)
    assert stats == {"evaluated": seen[0][0], "total": n * N_SLOTS, "rays_truncated": int(tr.sum())}
    assert 0 < stats["evaluated"] < stats["total"] and 0 < stats["rays_truncated"] < n
    assert float(got["acc_map"].max()) > 0.5
    # what is not evaluated is exactly zero: the closing samples, the padding and whatever lies at or behind the stop depth
    assert bool((got["raw"][z >= z_stop[:, None]] == 0).all())


def test_shared_network_and_the_reduced_inference_class(npa, dev, nets):
    """network_fine=None: the one pass runs on network_fn.  "fp16_fp8c" maps to fp16x3 on the grid path, here as without the option."""
    nc, _, _, _ = nets
    rays, rnd, _ = scene(dev)
    grid = ball_grid(npa, dev, "skip")
    kw = dict(N_samples=16, N_importance=48, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd, occupancy=grid,
              proposal="march", march_steps=M_STEPS)
    prev = npa.get_precision()
    try:
        npa.set_precision("fp16x3")
        with torch.no_grad():
            want = chain(npa, grid, rays, rnd["u_march"], nc, 1.0)[0]
            got = npa.render_rays(rays, nc, None, **kw)
            npa.set_precision("fp16_fp8c")
            reduced = npa.render_rays(rays, nc, None, **kw)
    finally:
        npa.set_precision(prev)
    for k in got:
        assert bits_equal(got[k], want[k]) and bits_equal(got[k], reduced[k]), k


def test_the_march_means_compositing_all_candidates(npa, dev, nets):
    """M = 256, S = 192, outside="skip", no noise, no ray truncated: the march render against compositing ALL 256 candidates through the
    masking hook (test_gpu_occupancy.masking_hook: every candidate evaluated, the rows of the empty ones zeroed).  Both sides evaluate
    the same points with the same dists -- behind an evaluated sample sits the next candidate on either side, and an empty candidate has
    alpha = 0 exactly --; only the LENGTH of the fp32 product (transmittance) and of the fp32 sum (the ray integrals) differs: 192 slots
    against 256.  Each factor 1 - alpha + 1e-10 <= 1 and each term <= 1, so with 3 roundings budgeted per transmittance factor and 1 per
    summed term |delta rgb_map| and |delta acc_map| stay within 4 M 2^-24 = 6.1e-5.  disp_map is left out: the reference's 0 / 0 on
    empty rays.

    The rays are the scene's 256 with far = 7.5 instead of 6, so that every ray has left the ball before its last candidate (asserted).
    "The same dists" holds for every candidate but an OCCUPIED LAST one: compositing all candidates gives it the reference's 1e10
    interval, the march by its definition the interval up to far (its run is closed at far; the last slot is always dropped).  With
    far = 6 seven of these rays end inside the ball and differ there by up to 0.29 in acc_map (measured on an MI355X) -- the
    definition's choice, not rounding, and no case for a rounding bound.
    MEASURED on an MI355X (fp32 datapath): max |delta rgb_map| 1.49e-7, max |delta acc_map| 1.79e-7."""
    nc, nf, _, _ = nets
    rays, _, _ = scene(dev)
    rays = rays.clone()
    rays[:, 7] = 7.5
    M, S = 256, 192
    grid = ball_grid(npa, dev, "skip")
    k = torch.arange(M, dtype=torch.float32)[None, :]
    r = rays.cpu()
    t = (k + 0.5) / torch.tensor(float(M))
    z_all = (r[:, 6:7] * (1.0 - t) + r[:, 7:8] * t).to(dev)
    with torch.no_grad():
        got = npa.render_rays(rays, nc, None, N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, retraw=True, occupancy=grid,
                              proposal="march", march_steps=M)
        stats = dict(grid.last_stats)
        seen = []
        pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z_all[:, :, None]
        assert not bool(grid.occupied(pts)[:, -1].any())
        raw = masking_hook(npa, grid, seen)(pts, rays[:, 8:11], nf)
        rgb, _, acc, _, _ = npa.raw2outputs(raw, z_all, rays[:, 3:6], 0.0, True)
    assert stats == {"evaluated": seen[0][0], "total": rays.shape[0] * S, "rays_truncated": 0} and stats["evaluated"] > 1000
    bound = 4 * M * U
    d_rgb, d_acc = float((got["rgb_map"] - rgb).abs().max()), float((got["acc_map"] - acc).abs().max())
    print(f"\nmarch vs all {M} candidates: max |delta rgb_map| {d_rgb:.3e}, max |delta acc_map| {d_acc:.3e} (bound {bound:.3e})")
    assert float(acc.max()) > 0.5
    assert d_rgb <= bound and d_acc <= bound


# ------------------------------------------------------------------------------------------------ 3. gradients
@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
@pytest.mark.parametrize("perturb,noise", [(1.0, 1.0), (0.0, 0.0)])
def test_forward_with_grad_equals_the_no_grad_render(npa, dev, nets, datapath, perturb, noise):
    nc, nf, _, _ = nets
    rays, rnd, _ = scene(dev)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=perturb, raw_noise_std=noise, retraw=True, randoms=rnd,
              occupancy=grid, proposal="march", march_steps=M_STEPS)
    with torch.no_grad():
        want = npa.render_rays(rays, nc, None, **kw)
    stats = dict(grid.last_stats)
    grid.last_stats = None
    got = npa.render_rays(rays, nc, None, **kw)
    assert list(got) == list(want) == ["rgb_map", "disp_map", "acc_map", "raw"]
    for k in want:
        assert bits_equal(got[k], want[k]), (k, maxdiff(got[k], want[k]))
    assert grid.last_stats == stats and 0 < stats["rays_truncated"] < rays.shape[0]
    assert got["rgb_map"].grad_fn is not None and got["raw"].grad_fn is not None
    del got          # (a graph dropped without backward)


@pytest.mark.parametrize("datapath", ["fp32", "fp16x3", "fp16x3w", "bf16x3"], indirect=True)
def test_parameter_gradients_equal_the_chains_bit_for_bit(npa, dev, nets, datapath):
    """loss = img2mse(rgb_map, t): .grad of every parameter of the evaluated network equals autograd's through the chain, bit for bit;
    the other network's .grad stays None; with network_fine=None the one network is network_fn"""
    nc, nf, _, _ = nets
    rays, rnd, target = scene(dev)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=16, N_importance=48, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, randoms=rnd, occupancy=grid, proposal="march",
              march_steps=M_STEPS)
    for net, fine in ((nf, nf), (nc, None)):
        zero_grads(nc, nf)
        out = npa.render_rays(rays, nc, None, network_fine=fine, **kw)
        assert "rgb0" not in out and "z_std" not in out
        loss_g = npa.img2mse(out["rgb_map"], target)
        loss_g.backward()
        other = nc if net is nf else nf
        assert all(p.grad is None for p in other.parameters())
        got = grads_of(net)
        zero_grads(nc, nf)
        loss_h = npa.img2mse(chain(npa, grid, rays, rnd["u_march"], net, 1.0)[0]["rgb_map"], target)
        loss_h.backward()
        want = grads_of(net)
        zero_grads(nc, nf)
        assert bits_equal(loss_g.detach(), loss_h.detach())
        assert all(x is not None for x in got) and float(flat_of(got).abs().max()) > 0
        for i, (x, y) in enumerate(zip(got, want)):
            assert bits_equal(x, y), (i, maxdiff(x, y), rel_l2(flat_of(got), flat_of(want)))


@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
def test_ray_gradients_against_the_float64_fold_of_the_chain(npa, dev, nets, datapath, monkeypatch):
    """rays.requires_grad_(): by the method and at the bound of test_gpu_grid_proposal's test of the same name -- the float64 fold of the
    chain's tapped per-point gradients plus the compositing's |d| term, within (S + 1) * 2^-24 * sum|terms| * 1.01 per element, S = 64.
    The depths are constants of the graph: columns 6:8 are exactly 0."""
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    rays0, rnd, target = scene(dev)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=0.5, randoms=rnd, occupancy=grid,
              proposal="march", march_steps=M_STEPS)
    rg = rays0.clone().requires_grad_(True)
    npa.img2mse(npa.render_rays(rg, nc, None, **kw)["rgb_map"], target).backward()
    got = rg.grad.clone()
    dns, taps = [], []
    bwd = hb.raw2outputs_bwd
    monkeypatch.setattr(hb, "raw2outputs_bwd", lambda *a, **k: (dns.append(k.get("d_rays_d")), bwd(*a, **k))[1])
    rh = rays0.clone().requires_grad_(True)
    ref, z, _, _ = chain(npa, grid, rh, rnd["u_march"], nf, 0.5, taps=taps)
    npa.img2mse(ref["rgb_map"], target).backward()
    zero_grads(nc, nf)
    assert len(taps) == 1 and len(dns) == 1 and dns[0] is not None
    n, S, tap = rays0.shape[0], N_SLOTS, taps[0]
    want = torch.zeros(n, 11, dtype=torch.float64, device=dev)
    mag = torch.zeros_like(want)
    ray_of = tap["idx"] // S
    gp, gv, zz = tap["d_pts"].double(), tap["d_viewdirs"].double(), z.reshape(-1)[tap["idx"]].double()[:, None]
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


def test_an_upstream_gradient_on_a_dropped_slot_reaches_no_parameter(npa, dev, nets, datapath_fp16x3, monkeypatch):
    """loss = sum(raw * G) through retraw: the network's gradient with a random G equals, bit for bit, the one with G zeroed on the slots
    the pass did not evaluate (slot < 0: closing samples, padding, truncated) -- and those slots did carry a nonzero G"""
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    rays, rnd, _ = scene(dev)
    n = rays.shape[0]
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, randoms=rnd, retraw=True, occupancy=grid,
              proposal="march", march_steps=M_STEPS)
    slots, stops = [], []
    real = hb.occ_compact
    monkeypatch.setattr(hb, "occ_compact", lambda *a, **k: (lambda r: (slots.append(r[0].clone()), stops.append(a[5] if len(a) > 5 else k.get("z_stop")), r)[2])(real(*a, **k)))
    G = torch.randn(n, N_SLOTS, 4, generator=torch.Generator().manual_seed(5)).to(dev)
    grads = []
    for mask_it in (False, True):
        zero_grads(nc, nf)
        del slots[:], stops[:]
        raw = npa.render_rays(rays, nc, None, **kw)["raw"]
        assert len(slots) == 1 and stops[0] is not None
        live = (slots[0] >= 0).view(n, N_SLOTS, 1)
        (raw * (G * live if mask_it else G)).sum().backward()
        grads.append(flat_of(grads_of(nf)))
        assert all(p.grad is None for p in nc.parameters())
    zero_grads(nc, nf)
    assert 0 < int(live.sum()) < n * N_SLOTS and float((G * ~live).abs().max()) > 0
    assert bits_equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0


def test_grad_ready_frozen_network_second_backward_and_stale_parameters(npa, dev, nets, datapath_fp16x3):
    render_mod = sys.modules["nerf_pytorch_amd.render"]
    hb = npa.hip_backend
    nc, nf = fresh_nets(npa, dev, nets)
    rays, rnd, target = scene(dev)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, randoms=rnd, occupancy=grid, proposal="march",
              march_steps=M_STEPS)
    fired = []
    hook = lambda model, flat: fired.append(model)
    render_mod.GRAD_READY_HOOKS.append(hook)
    wgrad_calls = []
    real_bwd = hb.field_bwd
    try:
        hb.field_bwd = lambda packed, act, d_raw, grad, *a, **k: (wgrad_calls.append(grad is not None), real_bwd(packed, act, d_raw, grad, *a, **k))[1]
        # the evaluated network fires once; the other one is never touched
        npa.img2mse(npa.render_rays(rays, nc, None, **kw)["rgb_map"], target).backward()
        assert fired == [nf] and wgrad_calls == [True] and all(p.grad is None for p in nc.parameters())
        assert all(p.grad is not None for p in nf.parameters())
        zero_grads(nc, nf)
        del fired[:], wgrad_calls[:]
        # the evaluated network frozen: nothing needs a gradient (the other network's parameters do not count) ...
        for p in nf.parameters():
            p.requires_grad_(False)
        out = npa.render_rays(rays, nc, None, **kw)
        assert not out["rgb_map"].requires_grad
        # ... unless the rays do: the delta chain runs for them, without a weight gradient and without _grad_ready
        rg = rays.clone().requires_grad_(True)
        npa.img2mse(npa.render_rays(rg, nc, None, **kw)["rgb_map"], target).backward()
        assert fired == [] and wgrad_calls == [False]
        assert all(p.grad is None for m in (nc, nf) for p in m.parameters())
        assert bool(torch.isfinite(rg.grad).all()) and float(rg.grad.abs().max()) > 0
    finally:
        hb.field_bwd = real_bwd
        render_mod.GRAD_READY_HOOKS.remove(hook)
    for p in nf.parameters():
        p.requires_grad_(True)
    # a second backward through the same graph
    loss = npa.img2mse(npa.render_rays(rays, nc, None, **kw)["rgb_map"], target)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="already consumed"):
        loss.backward()
    zero_grads(nc, nf)
    # an optimizer step between forward and backward (fp16x3: the backward reads live weights next to fragments packed at forward time)
    opt = npa.FlatAdam(list(nf.parameters()), lr=5e-4)
    npa.img2mse(npa.render_rays(rays, nc, None, **kw)["rgb_map"], target).backward()
    loss = npa.img2mse(npa.render_rays(rays, nc, None, **kw)["rgb_map"], target)
    opt.step()
    with pytest.raises(RuntimeError, match="parameters changed between"):
        loss.backward()


def test_resident_sub_chunks_equal_one_piece(npa, dev, nets, monkeypatch, datapath_fp16x3):
    """2500 rays under a budget forced to 1024 rays per sub-chunk: the march runs per sub-chunk, the outputs and the stats are those of
    one piece bit for bit, and the parameter gradients match the one-piece call within the bound of
    test_gpu_occupancy_train.test_resident_sub_chunks_give_the_gradients_of_one_piece: twice the relative L2 difference between the
    dense path and the stock hooked path on the same rays and sample counts, no grid, under the same forced budget (the same pair of
    summation orders).  The ray gradients' difference is reported."""
    hb = npa.hip_backend
    render_mod = sys.modules["nerf_pytorch_amd.render"]
    nc, nf, _, _ = nets
    n = 2500
    rays = orc.synthetic_rays(n, seed=8).to(dev)
    rnd = {"u_march": torch.rand(n, generator=torch.Generator().manual_seed(24)).to(dev), "noise_f": noise_of(dev, n)}
    dense_rnd = {"t_rand": torch.rand(n, N_SLOTS, generator=torch.Generator().manual_seed(25)).to(dev), "noise_c": rnd["noise_f"]}
    target = scene_target(dev, n)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=N_SLOTS, N_importance=0, white_bkgd=True, perturb=1.0, raw_noise_std=0.5)
    march_calls = []
    real = hb.occ_march
    monkeypatch.setattr(hb, "occ_march", lambda desc, r, *a: (march_calls.append(r.shape[0]), real(desc, r, *a))[1])

    def run(hook=None, **extra):
        zero_grads(nc, nf)
        r = rays.clone().requires_grad_(True)
        out = npa.render_rays(r, nf, hook, **kw, **extra)
        npa.img2mse(out["rgb_map"], target).backward()
        return render_mod.LAST_BACKWARD_PLAN, nf.last_flat_grad.clone(), r.grad.clone(), {k: v.detach() for k, v in out.items()}
    marching = dict(occupancy=grid, proposal="march", march_steps=M_STEPS, randoms=rnd)
    plan1, g1, r1, out1 = run(**marching)
    stats1 = dict(grid.last_stats)
    assert march_calls == [n]
    _, stock, _, _ = run(hook=lambda p, v, m: npa.run_network(p, v, m, None, None), randoms=dense_rnd)
    monkeypatch.setattr(hb, "SAVE_BUDGET_BYTES", 1)
    plan2, g2, r2, out2 = run(**marching)
    plan_dense, dense, _, _ = run(randoms=dense_rnd)
    zero_grads(nc, nf)
    assert plan1 == ("one launch", n, n) and plan2[0] == "resident sub-chunks" and plan2[1] == n and plan2[2] <= 1024
    assert plan_dense[0] == "resident sub-chunks"
    assert len(march_calls) >= 4 and sum(march_calls[1:]) == n and max(march_calls[1:]) <= 1024
    assert grid.last_stats == stats1 and 0 < stats1["rays_truncated"] < n and 0 < stats1["evaluated"] < stats1["total"] == n * N_SLOTS
    for k in out1:
        assert bits_equal(out1[k], out2[k]), k
    diff, yard = rel_l2(g2, g1), rel_l2(dense, stock)
    print(f"\nsub-chunks vs one piece: parameter gradients relative L2 {diff:.3e} (yardstick {yard:.3e}); ray gradients bit-identical "
          f"{torch.equal(r1, r2)}, relative L2 {rel_l2(r2, r1):.1e}")
    assert diff <= 2.0 * yard
    assert bool(torch.isfinite(r2).all()) and float(r2.abs().max()) > 0


def test_with_clipping_and_through_render_in_chunks(npa, dev, nets, datapath_fp16x3):
    """clip_to_occupancy=True + proposal="march" == the same call on grid.clip_rays(rays)[0] (the M steps then span the hull: fewer rays
    are truncated); render(chunk=96) == the unchunked call with last_stats summed over the chunks (batchify_rays slices u_march too)"""
    nc, nf, _, _ = nets
    rays, rnd, target = scene(dev)
    n = rays.shape[0]
    grid = ball_dgrid(npa, dev, outside="skip")
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd,
              occupancy=grid, proposal="march", march_steps=M_STEPS)
    clipped, hit = grid.clip_rays(rays)
    assert 0 < int(hit.sum()) and not bits_equal(clipped, rays)
    with torch.no_grad():
        got = npa.render_rays(rays, nc, None, clip_to_occupancy=True, **kw)
        stats = dict(grid.last_stats)
        want = npa.render_rays(clipped, nc, None, **kw)
        assert stats == dict(grid.last_stats, rays_hit=int(hit.sum()), rays=n) and stats["total"] == n * N_SLOTS
        for k in want:
            assert bits_equal(got[k], want[k]), k
        whole = npa.render_rays(rays, nc, None, **kw)
        total = dict(grid.last_stats)
        chunked = npa.batchify_rays(rays, 96, network_fn=nc, network_query_fn=None, **kw)
        assert grid.last_stats == total and 0 < total["rays_truncated"] < n
        for k in whole:
            assert bits_equal(chunked[k], whole[k]), k
        K = np.array([[20.0, 0, 8.0], [0, 20.0, 8.0], [0, 0, 1]])
        geo = dict(rays=(rays[:, 0:3], rays[:, 3:6]), ndc=False, near=2.0, far=6.0, use_viewdirs=True, network_fn=nc, network_query_fn=None)
        one = npa.render(16, 16, K, chunk=1 << 20, **geo, **kw)
        total = dict(grid.last_stats)
        many = npa.render(16, 16, K, chunk=96, **geo, **kw)
        assert grid.last_stats == total and 0 < total["rays_truncated"] < n and total["total"] == n * N_SLOTS
        assert 0 < total["evaluated"] < total["total"]
        for a, b in zip(one[:3], many[:3]):
            assert bits_equal(a, b)
        assert set(one[3]) == set(many[3]) == {"raw"} and bits_equal(one[3]["raw"], many[3]["raw"])
    # with gradients the clipped call is the call on the clipped rays as well
    grads = []
    for r, extra in ((rays, dict(clip_to_occupancy=True)), (clipped, {})):
        zero_grads(nc, nf)
        npa.img2mse(npa.render_rays(r, nc, None, **kw, **extra)["rgb_map"], target).backward()
        grads.append(flat_of(grads_of(nf)))
    zero_grads(nc, nf)
    assert bits_equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 4. draws, off means off
def test_the_draws_are_u_march_then_the_noise(npa, dev, nets):
    """without `randoms`: torch.rand(n) then torch.randn((n, S)) from the device's generator, nothing else; pytest=True: the reference's
    np.random.seed(0) draws"""
    nc, nf, _, _ = nets
    rays, _, _ = scene(dev)
    n = rays.shape[0]
    grid = ball_grid(npa, dev, "skip")
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, retraw=True, occupancy=grid, proposal="march", march_steps=M_STEPS)
    with torch.no_grad():
        torch.manual_seed(17)
        got = npa.render_rays(rays, nc, None, perturb=1.0, raw_noise_std=1.0, **kw)
        after = torch.rand(4, device=dev)
        torch.manual_seed(17)
        rnd = {"u_march": torch.rand(n, device=dev), "noise_f": torch.randn((n, N_SLOTS), device=dev)}
        assert torch.equal(after, torch.rand(4, device=dev))
        want = npa.render_rays(rays, nc, None, perturb=1.0, raw_noise_std=1.0, randoms=rnd, **kw)
        for k in got:
            assert bits_equal(got[k], want[k]), k
        # perturb alone draws u_march alone; noise alone draws the noise alone; neither: nothing
        for perturb, noise, draws in ((1.0, 0.0, [lambda: torch.rand(n, device=dev)]), (0.0, 1.0, [lambda: torch.randn((n, N_SLOTS), device=dev)]),
                                     (0.0, 0.0, [])):
            torch.manual_seed(3)
            npa.render_rays(rays, nc, None, perturb=perturb, raw_noise_std=noise, **kw)
            after = torch.rand(4, device=dev)
            torch.manual_seed(3)
            for d in draws:
                d()
            assert torch.equal(after, torch.rand(4, device=dev)), (perturb, noise)
        got = npa.render_rays(rays, nc, None, perturb=1.0, raw_noise_std=0.5, pytest=True, **kw)
        np.random.seed(0)
        u = torch.Tensor(np.random.rand(n)).to(dev)
        np.random.seed(0)
        nz = torch.Tensor(np.random.rand(n, N_SLOTS) * 0.5).to(dev)
        want = npa.render_rays(rays, nc, None, perturb=1.0, raw_noise_std=1.0, randoms={"u_march": u, "noise_f": nz}, **kw)
        for k in got:
            assert bits_equal(got[k], want[k]), k


@pytest.mark.parametrize("grad", [False, True])
def test_none_and_grid_are_the_calls_without_the_keyword(npa, dev, nets, datapath_fp16x3, monkeypatch, grad):
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    rays, rnd, _ = _small_scene(dev)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, occupancy=grid)
    calls = []
    real = hb.occ_march
    monkeypatch.setattr(hb, "occ_march", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.set_grad_enabled(grad):
        for proposal in (None, "grid"):
            a = npa.render_rays(rays, nc, None, randoms=rnd, proposal=proposal, **kw)
            stats_a = dict(grid.last_stats)
            b = npa.render_rays(rays, nc, None, randoms=rnd, proposal=proposal, march_steps=None, **kw)
            assert grid.last_stats == stats_a and "rays_truncated" not in grid.last_stats
            # the same random draws: without `randoms` a seeded call consumes the generator identically
            torch.manual_seed(17)
            c = npa.render_rays(rays, nc, None, proposal=proposal, **kw)
            after_c = torch.rand(4, device=dev)
            torch.manual_seed(17)
            d = npa.render_rays(rays, nc, None, proposal=proposal, march_steps=None, **kw)
            after_d = torch.rand(4, device=dev)
            # ... which is t_rand, (noise_c,) u, noise_f of the reference's order
            torch.manual_seed(17)
            n = rays.shape[0]
            torch.rand((n, 64), device=dev)
            if proposal is None:
                torch.randn((n, 64), device=dev)
            torch.rand((n, 128), device=dev)
            torch.randn((n, 192), device=dev)
            after_e = torch.rand(4, device=dev)
            assert list(a) == list(b) == list(c) == list(d)
            for k in a:
                assert bits_equal(a[k].detach(), b[k].detach()) and bits_equal(c[k].detach(), d[k].detach()), k
            assert torch.equal(after_c, after_d) and torch.equal(after_c, after_e)
        assert calls == []
        npa.render_rays(rays, nc, None, **dict(kw, N_samples=16, N_importance=48), proposal="march", march_steps=M_STEPS)
    assert calls == [1]         # (the wrapper does count)


def test_all_empty_grid_and_a_ray_that_misses(npa, dev, nets, monkeypatch):
    """an all-empty grid with outside="skip": every ray misses, m == 0, no field launch, white background, zero gradients, no ray
    truncated -- with gradients and without"""
    hb = npa.hip_backend
    nc, nf = fresh_nets(npa, dev, nets)
    rays, rnd, target = scene(dev)
    empty = npa.DensityGrid.from_mask(torch.zeros(2, 2, 2, dtype=torch.bool), BOX_LO, BOX_HI, outside="skip", device=dev)
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = hb.field_fwd, hb.field_bwd
    monkeypatch.setattr(hb, "field_fwd", lambda *a, **k: (calls.__setitem__("fwd", calls["fwd"] + 1), fwd(*a, **k))[1])
    monkeypatch.setattr(hb, "field_bwd", lambda *a, **k: (calls.__setitem__("bwd", calls["bwd"] + 1), bwd(*a, **k))[1])
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, randoms=rnd, occupancy=empty, retraw=True,
              proposal="march", march_steps=M_STEPS)
    r = rays.clone().requires_grad_(True)
    out = npa.render_rays(r, nc, None, **kw)
    assert empty.last_stats == {"evaluated": 0, "total": 256 * N_SLOTS, "rays_truncated": 0}
    assert bool((out["rgb_map"] == 1).all()) and bool((out["raw"] == 0).all()) and bool((out["acc_map"] == 0).all())
    npa.img2mse(out["rgb_map"], target).backward()
    assert calls == {"fwd": 0, "bwd": 0}
    assert all(p.grad is not None and bool((p.grad == 0).all()) for p in nf.parameters()) and all(p.grad is None for p in nc.parameters())
    assert r.grad is not None and bool(torch.isfinite(r.grad).all())
    with torch.no_grad():
        out = npa.render_rays(rays, nc, None, **kw)
    assert empty.last_stats == {"evaluated": 0, "total": 256 * N_SLOTS, "rays_truncated": 0} and calls == {"fwd": 0, "bwd": 0}
    assert bool((out["rgb_map"] == 1).all())
