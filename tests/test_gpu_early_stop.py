"""GPU tests (-m gpu) of render_rays(early_stop_eps=): nerf_occ_stop_depth alone against its definition, nerf_occ_compact_stop alone
against torch, then the render -- forward and backward -- against THE CHAIN: the same computation put together from public pieces.
The chain is the stock hooked path (hb.sample_coarse -> hook -> hb.raw2outputs -> hb.sample_fine -> hook -> raw2outputs) with
occupancy.stop_depth called on what hb.sample_fine is handed (the coarse depths and weights) and a hook that, in the refining pass,
evaluates only the points with occupied(pts) & ~(z_f >= z_stop) -- the compacting hook of tests/test_gpu_occupancy_train.py with one more
predicate.  It sends the same M records through the same field launches, so the checks are bit for bit."""
import sys

import numpy as np
import pytest
import torch

import nerf_oracle as orc
from test_early_stop_cpu import HAND_ROWS, hand_rows, loop_stop_depth
from test_gpu_grid_proposal import NOISE_SEED, filled, noise_f_of  # noqa: F401  (fixture)
from test_gpu_occupancy import BOX_LO, BOX_HI, ball_grid, bits_equal
from test_gpu_occupancy_train import (U, _small_scene, ball_dgrid, datapath_fp16x3, flat_of, fresh_nets, grads_of,  # noqa: F401
                                      loss_of, same_floats, scene_target, slots_of, zero_grads)
from test_gpu_parity import datapath, dev, maxdiff, nets, npa  # noqa: F401  (fixtures)
from test_gpu_ray_grad import rel_l2

pytestmark = pytest.mark.gpu

N_C, N_F = 64, 128
INF = float("inf")


# ------------------------------------------------------------------------------------------------ 1. the stop depth alone
@pytest.mark.parametrize("eps", [1e-4, 0.3])
@pytest.mark.parametrize("S", [1, 5, 64, 65, 192])
def test_stop_depth_kernel_equals_the_definition_bit_for_bit(npa, dev, S, eps):
    """301 rays (five blocks of 64, the last one ragged), S around the 64-sample tile: random non-negative weights whose totals are
    spread so that a third of the rays crosses in the first half, a third in the second half and a third never (asserted), the hand-made
    rows of the CPU test planted among them; z_stop equals stop_depth_reference and the Python loop as raw bits, twice"""
    g = torch.Generator().manual_seed(1000 + S)
    n = 301
    thr = float(np.float32(1.0 - eps))
    z = torch.sort(2.0 + 4.0 * torch.rand(n, S, generator=g), -1).values
    shape = torch.rand(n, S, generator=g) + 0.05
    shape = shape / shape.sum(-1, keepdim=True)
    # the total of a ray decides where its (near-uniform) running sum crosses: > 2 thr in the first half, thr .. 2 thr in the second, < thr never
    total = torch.cat([thr * (2.2 + torch.rand(100, generator=g)), thr * (1.05 + 0.8 * torch.rand(100, generator=g)), thr * 0.9 * torch.rand(101, generator=g)])
    w = shape * total[torch.randperm(n, generator=g)][:, None]
    zh, wh = hand_rows(S, eps)
    rows = torch.arange(len(HAND_ROWS)) * 29 + 3          # (spread over the blocks, the ragged last one included: 3 .. 264)
    rows[-1] = 300
    z[rows], w[rows] = zh, wh
    want = npa.occupancy.stop_depth_reference(z, w, eps)
    assert bits_equal(want, loop_stop_depth(z, w, eps))
    got = npa.occupancy.stop_depth(z.to(dev), w.to(dev), eps)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.shape == (n,) and got.is_cuda
    assert bits_equal(got.cpu(), want), int((got.cpu() != want).sum())
    assert bits_equal(got, npa.occupancy.stop_depth(z.to(dev), w.to(dev), eps))
    assert bits_equal(got[rows.to(dev)].cpu(), loop_stop_depth(zh, wh, eps))
    # the thirds are there (S = 1 has no "behind": everything is +inf)
    plain = torch.ones(n, dtype=torch.bool)
    plain[rows] = False
    if S >= 5:
        idx = (z == want[:, None]).float().argmax(-1) - 1           # i* of the rays that stop
        stopped = torch.isfinite(want) & plain
        early, late, never = (stopped & (idx < S // 2)).sum(), (stopped & (idx >= S // 2)).sum(), (~torch.isfinite(want) & plain).sum()
        assert min(int(early), int(late), int(never)) >= 60, (int(early), int(late), int(never))
    else:
        assert bool(torch.isinf(want).all())
    assert bool((want[torch.isinf(want)] > 0).all())
    # device reference == host reference: the definition does not depend on where the tensors live
    assert bits_equal(npa.occupancy.stop_depth_reference(z.to(dev), w.to(dev), eps).cpu(), want)


# ------------------------------------------------------------------------------------------------ 2. the compaction with a stop
def compaction_scene(npa, dev, outside):
    """the 1000 x 200 scene of test_gpu_occupancy.test_compact_agrees_with_occupied_on_200k_points (P is no multiple of 1024, points on
    cell faces, outside the box, NaN / inf components), with depths sorted per ray"""
    g = torch.Generator().manual_seed(11)
    res = (37, 21, 64)
    mask = torch.rand(res, generator=g) < 0.35
    lo, hi = (-1.25, 0.5, -3.0), (1.75, 2.0, 0.2)
    grid = npa.OccupancyGrid.from_mask(mask, lo, hi, outside=outside, device=dev)
    n, S = 1000, 200
    lo_t, hi_t = torch.tensor(lo), torch.tensor(hi)
    o = lo_t + (hi_t - lo_t) * (torch.rand(n, 3, generator=g) * 1.2 - 0.1)
    d = torch.randn(n, 3, generator=g) * 0.3
    z = torch.sort(torch.rand(n, S, generator=g) * 2.0, -1).values
    width = (hi_t - lo_t) / torch.tensor(res, dtype=torch.float32)
    k = torch.stack([torch.randint(0, r + 1, (300,), generator=g) for r in res], -1).float()
    o[300:600] = lo_t + k * width
    o[300:320], o[320:340] = lo_t, hi_t
    d[300:600] = 0.0
    o[600:800] = hi_t + 1.0 + torch.rand(200, 3, generator=g)
    o[800:810, 0] = float("nan")
    d[810:820, 2] = float("inf")
    z[820:830, 7] = float("nan")            # a NaN depth: never stopped (and, its point being a NaN, outside the box)
    vd = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    rays = torch.cat([o, d, torch.zeros(n, 2), vd], -1).to(dev).contiguous()
    # z_stop: +inf, -inf, NaN, inside the ray's range, and EQUAL to one of the ray's own depths (that sample is dropped: >=)
    kind = torch.arange(n) % 5
    own = z[torch.arange(n), torch.randint(0, S, (n,), generator=g)]
    z_stop = torch.where(kind == 0, torch.full((n,), INF), torch.where(kind == 1, torch.full((n,), -INF), torch.where(
        kind == 2, torch.full((n,), float("nan")), torch.where(kind == 3, 2.0 * torch.rand(n, generator=g), own))))
    return grid, rays, z.to(dev).contiguous(), z_stop.to(dev).contiguous(), kind.to(dev)


@pytest.mark.parametrize("outside", ["evaluate", "skip"])
def test_compact_with_a_stop_equals_the_torch_construction(npa, dev, outside):
    hb = npa.hip_backend
    grid, rays, z, z_stop, kind = compaction_scene(npa, dev, outside)
    n, S = z.shape
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]
    occ = grid.occupied(pts)
    keep = occ & ~(z >= z_stop[:, None])
    slot, records, count = hb.occ_compact(grid._desc(), rays, z, z_stop=z_stop)
    torch.cuda.synchronize()
    m = int(count.item())
    assert m == int(keep.sum()) and 0 < m < int(occ.sum())
    assert torch.equal(slot, slots_of(keep))
    flat = keep.reshape(-1)
    recs = records[:m]
    owner = torch.arange(n, device=dev).repeat_interleave(S)[flat]
    want = torch.cat([pts.reshape(-1, 3)[flat], torch.zeros(m, 5, device=dev), rays[owner, 8:11]], -1)
    assert bits_equal(recs, want)
    # every kind of stop did what it says: +inf and NaN stop nothing, -inf everything, an own depth drops that very sample
    per_ray, occ_ray = keep.sum(-1), occ.sum(-1)
    assert torch.equal(per_ray[(kind == 0) | (kind == 2)], occ_ray[(kind == 0) | (kind == 2)]) and int(occ_ray[kind == 2].sum()) > 0
    # (-inf stops every sample with a depth; the ten NaN depths are not stopped by anything)
    assert torch.equal(per_ray[kind == 1], (occ & torch.isnan(z)).sum(-1)[kind == 1]) and int(per_ray[kind == 1].sum()) <= 10
    assert int(occ_ray[kind == 1].sum()) > 1000
    assert int((occ & (z == z_stop[:, None]))[kind == 4].sum()) > 0 and not bool((keep & (z == z_stop[:, None])).any())
    assert 0 < int(per_ray[kind == 3].sum()) < int(occ_ray[kind == 3].sum())
    nan_z = torch.isnan(z)
    assert int(nan_z.sum()) == 10 and torch.equal(keep[nan_z], occ[nan_z])
    # deterministic
    slot2, records2, count2 = hb.occ_compact(grid._desc(), rays, z, z_stop=z_stop)
    assert torch.equal(slot, slot2) and bits_equal(records[:m], records2[:m]) and int(count2.item()) == m
    # z_stop all +inf: the entry point without a stop, bit for bit
    a = hb.occ_compact(grid._desc(), rays, z)
    b = hb.occ_compact(grid._desc(), rays, z, z_stop=torch.full((n,), INF, device=dev))
    ma = int(a[2].item())
    assert ma == int(b[2].item()) == int(occ.sum()) and torch.equal(a[0], b[0]) and bits_equal(a[1][:ma], b[1][:ma])
    with pytest.raises(hb.NerfHipError, match="one depth per ray"):
        hb.occ_compact(grid._desc(), rays, z, z_stop=z_stop[:-1])


# ------------------------------------------------------------------------------------------------ 3. the render against the chain
class Chain:
    """THE YARDSTICK: render_rays(early_stop_eps=eps) from public pieces (module docstring).  run(...) is render_rays / render with the
    hook; afterwards z_stop (a list, one per render_rays call), kept (evaluated points per hook call) and taps (as compacting_hook's)."""

    def __init__(self, npa, grid, eps, taps=False):
        self.npa, self.grid, self.eps = npa, grid, eps
        self.z_stop, self.z_c, self.w, self.z_f, self.kept, self.totals = [], [], [], [], [], []
        self.taps = [] if taps else None
        self._pending = None

    def _sample_fine(self, real):
        def sample_fine(z_c, weights, *a, **k):
            out = real(z_c, weights, *a, **k)
            z_stop = self.npa.occupancy.stop_depth(z_c, weights, self.eps)
            self.z_c.append(z_c)
            self.w.append(weights)
            self.z_stop.append(z_stop)
            self.z_f.append(out[0])
            self._pending = (out[0], z_stop)
            return out
        return sample_fine

    def hook(self, pts, viewdirs, net):
        npa = self.npa
        N, S = pts.shape[:2]
        keep = self.grid.occupied(pts)
        if self._pending is not None:       # the refining pass: the call that follows hb.sample_fine
            z_f, z_stop = self._pending
            self._pending = None
            keep = keep & ~(z_f >= z_stop[:, None])
        idx = keep.reshape(-1).nonzero()[:, 0]
        self.kept.append(int(idx.numel()))
        self.totals.append(N * S)
        p_sel = pts.reshape(-1, 3)[idx]
        v_sel = viewdirs[:, None].expand_as(pts).reshape(-1, 3)[idx]
        if self.taps is not None:
            tap = {"idx": idx, "N": N, "S": S}
            self.taps.append(tap)
            if p_sel.requires_grad:
                p_sel.register_hook(lambda g, tap=tap: tap.__setitem__("d_pts", g.detach().clone()))
                v_sel.register_hook(lambda g, tap=tap: tap.__setitem__("d_viewdirs", g.detach().clone()))
        raw_c = npa.query_points(net, p_sel, v_sel) if idx.numel() else torch.zeros(0, 4, device=pts.device)
        return torch.zeros(N * S, 4, device=pts.device).index_put((idx,), raw_c).view(N, S, 4)

    def run(self, fn, *a, **kw):
        hb = self.npa.hip_backend
        real = hb.sample_fine
        hb.sample_fine = self._sample_fine(real)
        try:
            return fn(*a, **kw)
        finally:
            hb.sample_fine = real


def coverage(npa, grid, rays, z_c, w, z_f, eps):
    """(share of rays with a finite z_stop, share of the refining-pass points the grid keeps that the stop drops, rays with occupied
    points that keep all of them) for one eps, from the unstopped call's depths and weights: plain torch and the stop-depth kernel"""
    z_stop = npa.occupancy.stop_depth(z_c, w, eps)
    occ = grid.occupied(rays[:, None, 0:3] + rays[:, None, 3:6] * z_f[:, :, None])
    keep = occ & ~(z_f >= z_stop[:, None])
    full = (keep.sum(-1) == occ.sum(-1)) & (occ.sum(-1) > 0)
    return float(torch.isfinite(z_stop).float().mean()), 1.0 - int(keep.sum()) / max(int(occ.sum()), 1), int(full.sum())


def covered(c):
    return 0.25 <= c[0] <= 0.75 and c[1] >= 0.05 and c[2] >= 1


def eps_for(npa, grid, rays, network_fn, **kw):
    """eps FROM THE DATA (the fixture networks' scene is part fog, and with raw_noise_std > 0 all fog: no fixed eps splits every
    configuration).  The unstopped render of the same call is run once with hb.sample_fine tapped for the coarse depths and weights and
    the refining pass's depths; 1 - eps is then a quantile of the rays' opacity IN FRONT OF THE LAST SAMPLE (the sum of the weights but
    the last: a ray can only stop behind a sample that has one behind it), the median first, and the first quantile whose coverage --
    computed here from those tensors -- is the one test_no_grad_render_equals_the_chain_bit_for_bit asserts is taken (the median if
    none is: that test then fails and says so)."""
    hb = npa.hip_backend
    seen = {}
    real = hb.sample_fine
    hb.sample_fine = lambda z_c, w, *a, **k: (lambda r: (seen.update(z_c=z_c, w=w, z_f=r[0]), r)[1])(real(z_c, w, *a, **k))
    try:
        with torch.no_grad():
            npa.render_rays(rays.detach(), network_fn, None, occupancy=grid, **kw)
    finally:
        hb.sample_fine = real
    front = seen["w"][:, :-1].sum(-1)
    pick = lambda q: min(max(1.0 - float(front.quantile(q)), 1e-6), 1.0 - 1e-6)
    for q in (0.5, 0.4, 0.6, 0.3, 0.7):
        if covered(coverage(npa, grid, rays.detach(), seen["z_c"], seen["w"], seen["z_f"], pick(q))):
            return pick(q)
    return pick(0.5)


def grid_of(npa, dev, kind):
    return ball_grid(npa, dev) if kind == "plain" else ball_dgrid(npa, dev)


@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
@pytest.mark.parametrize("perturb,noise", [(0.0, 0.0), (1.0, 1.0)])
@pytest.mark.parametrize("kind", ["plain", "density"])
def test_no_grad_render_equals_the_chain_bit_for_bit(npa, dev, nets, datapath, perturb, noise, kind):
    """256 rays, 64 + 128 samples: rgb_map, disp_map, acc_map, raw and z_std equal the chain's bit for bit; rgb0 / disp0 / acc0 (and
    z_std) equal those of the same call WITHOUT the option; last_stats counts what the chain evaluated and the rays with a finite
    z_stop.  The test asserts its own coverage: 25 .. 75 % of the rays stop, the stop drops at least 5 % of the refining-pass points the
    grid alone keeps, and at least one ray keeps all of its points."""
    nc, nf, _, _ = nets
    rays, rnd, _ = _small_scene(dev)
    n = rays.shape[0]
    grid = grid_of(npa, dev, kind)
    kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=perturb, raw_noise_std=noise, retraw=True, randoms=rnd)
    eps = eps_for(npa, grid, rays, nc, **kw)
    chain = Chain(npa, grid, eps)
    with torch.no_grad():
        want = chain.run(npa.render_rays, rays, nc, chain.hook, **kw)
        got = npa.render_rays(rays, nc, None, occupancy=grid, early_stop_eps=eps, **kw)
        stats = dict(grid.last_stats)
        off = npa.render_rays(rays, nc, None, occupancy=grid, **kw)
        stats_off = dict(grid.last_stats)
    assert list(got) == list(want) == list(off)
    for k in ("rgb_map", "disp_map", "acc_map", "raw", "z_std", "rgb0", "disp0", "acc0"):
        assert bits_equal(got[k], want[k]), (k, maxdiff(got[k], want[k]))
    for k in ("rgb0", "disp0", "acc0", "z_std"):
        assert bits_equal(got[k], off[k]), k
    z_stop, z_f = chain.z_stop[0], chain.z_f[0]
    stopped = torch.isfinite(z_stop)
    assert chain.totals == [n * N_C, n * (N_C + N_F)]
    assert stats == {"evaluated": sum(chain.kept), "total": n * (2 * N_C + N_F), "rays_stopped": int(stopped.sum())}
    assert "rays_stopped" not in stats_off
    # coverage
    share = float(stopped.float().mean())
    fine_grid_only = stats_off["evaluated"] - chain.kept[0]
    dropped = fine_grid_only - chain.kept[1]
    print(f"\n[{datapath} {kind} perturb={perturb}] eps {eps:.4g}: rays stopped {share:.3f}; refining-pass points: grid keeps {fine_grid_only}, "
          f"the stop drops {dropped} ({dropped / max(fine_grid_only, 1):.3f}); image difference to the unstopped render "
          f"{maxdiff(got['rgb_map'], off['rgb_map']):.2e}")
    assert 0.25 <= share <= 0.75
    assert dropped >= 0.05 * fine_grid_only
    assert covered(coverage(npa, grid, rays, chain.z_c[0], chain.w[0], z_f, eps))
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z_f[:, :, None]
    occ = grid.occupied(pts)
    full = (occ & ~(z_f >= z_stop[:, None])).sum(-1) == occ.sum(-1)
    assert bool((full & (occ.sum(-1) > 0)).any())
    assert bool((got["raw"][z_f >= z_stop[:, None]] == 0).all())


# ------------------------------------------------------------------------------------------------ 4. gradients
@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
def test_parameter_gradients_equal_the_chains_bit_for_bit(npa, dev, nets, datapath):
    """DensityGrid, two networks, loss = img2mse(rgb_map, t) + img2mse(rgb0, t): .grad of every parameter of both networks equals
    autograd's through the chain, bit for bit; with the loss on rgb0 alone the coarse network's gradient is that of the call without
    the option and the fine network gets none"""
    nc, nf, _, _ = nets
    rays, rnd, target = _small_scene(dev)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, randoms=rnd)
    eps = eps_for(npa, grid, rays, nc, **kw)
    zero_grads(nc, nf)
    out = npa.render_rays(rays, nc, None, occupancy=grid, early_stop_eps=eps, **kw)
    stats = dict(grid.last_stats)
    loss_g = loss_of(npa, out, target)
    loss_g.backward()
    gc, gf = grads_of(nc), grads_of(nf)
    zero_grads(nc, nf)
    chain = Chain(npa, grid, eps)
    loss_h = loss_of(npa, chain.run(npa.render_rays, rays, nc, chain.hook, **kw), target)
    loss_h.backward()
    hc, hf = grads_of(nc), grads_of(nf)
    zero_grads(nc, nf)
    assert stats["evaluated"] == sum(chain.kept) and 0 < stats["rays_stopped"] == int(torch.isfinite(chain.z_stop[0]).sum()) < rays.shape[0]
    assert bits_equal(loss_g.detach(), loss_h.detach())
    for name, a, b in (("coarse", gc, hc), ("fine", gf, hf)):
        assert all(x is not None for x in a) and float(flat_of(a).abs().max()) > 0
        for i, (x, y) in enumerate(zip(a, b)):
            assert bits_equal(x, y), (name, i, maxdiff(x, y), rel_l2(flat_of(a), flat_of(b)))
    # the rgb0 term alone: the stop reaches neither the coarse pass nor its gradient
    coarse_only = []
    for extra in (dict(early_stop_eps=eps), {}):
        zero_grads(nc, nf)
        npa.img2mse(npa.render_rays(rays, nc, None, occupancy=grid, **kw, **extra)["rgb0"], target).backward()
        assert all(p.grad is None or not bool(p.grad.any()) for p in nf.parameters())
        coarse_only.append(flat_of(grads_of(nc)))
    zero_grads(nc, nf)
    assert bits_equal(coarse_only[0], coarse_only[1]) and float(coarse_only[0].abs().max()) > 0


@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
def test_ray_gradients_against_the_float64_fold_of_the_hooks(npa, dev, nets, datapath, monkeypatch):
    """rays.requires_grad_(): by the method and at the bound of test_gpu_occupancy_train's test of the same name -- the float64 fold of
    the chain's tapped per-point gradients (the refining pass's taps hold only the points in front of z_stop) plus the two |d| terms,
    within (S_c + S_f + 2) * 2^-24 * sum|terms| * 1.01 per element.  Columns 6:8 are exactly 0."""
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    rays0, rnd, target = _small_scene(dev)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=0.5, randoms=rnd)
    eps = eps_for(npa, grid, rays0, nc, **kw)
    rg = rays0.clone().requires_grad_(True)
    loss_of(npa, npa.render_rays(rg, nc, None, occupancy=grid, early_stop_eps=eps, **kw), target).backward()
    got = rg.grad.clone()
    dns = []
    bwd = hb.raw2outputs_bwd
    monkeypatch.setattr(hb, "raw2outputs_bwd", lambda *a, **k: (dns.append(k.get("d_rays_d")), bwd(*a, **k))[1])
    chain = Chain(npa, grid, eps, taps=True)
    rh = rays0.clone().requires_grad_(True)
    loss_of(npa, chain.run(npa.render_rays, rh, nc, chain.hook, **kw), target).backward()
    zero_grads(nc, nf)
    assert len(chain.taps) == 2 and len(dns) == 2 and all(d is not None for d in dns)
    n = rays0.shape[0]
    want = torch.zeros(n, 11, dtype=torch.float64, device=dev)
    mag = torch.zeros_like(want)
    for z, tap in zip((chain.z_c[0], chain.z_f[0]), chain.taps):
        S = tap["S"]
        assert z.shape == (n, S)
        ray_of = tap["idx"] // S
        gp, gv, zz = tap["d_pts"].double(), tap["d_viewdirs"].double(), z.reshape(-1)[tap["idx"]].double()[:, None]
        for cols, terms in ((slice(0, 3), gp), (slice(3, 6), zz * gp), (slice(8, 11), gv)):
            want[:, cols] = want[:, cols].index_add(0, ray_of, terms)
            mag[:, cols] = mag[:, cols].index_add(0, ray_of, terms.abs())
    for d in dns:
        want[:, 3:6] += d.double()
        mag[:, 3:6] += d.double().abs()
    err = (got.double() - want).abs()
    bound = 1.01 * (N_C + N_C + N_F + 2) * U * mag
    geo = [0, 1, 2, 3, 4, 5, 8, 9, 10]
    print(f"\n[{datapath}] ray gradient: worst error / bound {float((err[:, geo] / bound[:, geo].clamp(min=1e-300)).max()):.3f}; "
          f"relative L2 vs the chain's own rays.grad {rel_l2(got, rh.grad):.2e}")
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    assert bool((got[:, 6:8] == 0).all())
    assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())


def test_an_upstream_gradient_on_a_stopped_sample_reaches_no_parameter(npa, dev, nets, datapath_fp16x3, monkeypatch):
    """loss = sum(raw * G) through retraw: the fine network's gradient with a random G equals, bit for bit, the one with G zeroed on the
    rows the pass did not evaluate (slot < 0: skipped by the grid or stopped) -- and stopped rows did carry a nonzero G"""
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    rays, rnd, _ = _small_scene(dev)
    n = rays.shape[0]
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=1.0, randoms=rnd, retraw=True)
    kw = dict(kw, occupancy=grid, early_stop_eps=eps_for(npa, grid, rays, nc, **kw))
    slots, stops = [], []
    real = hb.occ_compact
    monkeypatch.setattr(hb, "occ_compact", lambda *a, **k: (lambda r: (slots.append(r[0].clone()), stops.append(a[5] if len(a) > 5 else k.get("z_stop")), r)[2])(real(*a, **k)))
    G = torch.randn(n, N_C + N_F, 4, generator=torch.Generator().manual_seed(5)).to(dev)
    grads = []
    for mask_it in (False, True):
        zero_grads(nc, nf)
        del slots[:], stops[:]
        raw = npa.render_rays(rays, nc, None, **kw)["raw"]
        assert len(slots) == 2 and stops[0] is None and stops[1] is not None
        live = (slots[1] >= 0).view(n, N_C + N_F, 1)
        (raw * (G * live if mask_it else G)).sum().backward()
        grads.append(flat_of(grads_of(nf)))
    zero_grads(nc, nf)
    z_stop = stops[1]
    assert 0 < int(torch.isfinite(z_stop).sum()) and int((~live).sum()) > 0 and float((G * ~live).abs().max()) > 0
    assert bits_equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 5. combinations
def test_with_the_grid_proposal(npa, dev, nets, filled, datapath_fp16x3):
    """proposal="grid": the weights the stop is read from are grid.proposal_weights; the chain is test_gpu_grid_proposal's with the stop
    between the weights and the refining pass.  No rgb0, the coarse network gets no launch and no gradient."""
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    rays, rnd, target = _small_scene(dev)
    n = rays.shape[0]
    rnd = dict(rnd, noise_f=noise_f_of(dev, n))
    grid = filled("skip")
    with torch.no_grad():
        z_c = hb.sample_coarse(rays, torch.linspace(0.0, 1.0, N_C, device=dev), False, rnd["t_rand"])
        w = grid.proposal_weights(rays, z_c)
    eps = min(max(1.0 - float(w.sum(-1).median()), 1e-6), 1.0 - 1e-6)        # (from the data: the median opacity the grid proposes)
    z_stop = npa.occupancy.stop_depth(z_c, w, eps)
    assert 0.1 * n <= int(torch.isfinite(z_stop).sum()) <= 0.9 * n
    z_f, z_std, _ = hb.sample_fine(z_c, w, N_F, rnd["u"], None)
    kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd,
              occupancy=grid, proposal="grid")
    calls = []
    packed = nc.packed_params
    nc.packed_params = lambda *a, **k: (calls.append(a), packed(*a, **k))[1]
    try:
        zero_grads(nc, nf)
        got = npa.render_rays(rays, nc, None, early_stop_eps=eps, **kw)
        stats = dict(grid.last_stats)
        loss_g = npa.img2mse(got["rgb_map"], target)
        loss_g.backward()
    finally:
        del nc.packed_params
    g_got = grads_of(nf)
    assert calls == [] and all(p.grad is None for p in nc.parameters())
    assert list(got) == ["z_std", "rgb_map", "disp_map", "acc_map", "raw"]
    zero_grads(nc, nf)
    # the chain
    chain = Chain(npa, grid, eps)
    chain._pending = (z_f, z_stop)
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z_f[:, :, None]
    raw = chain.hook(pts, rays[:, 8:11], nf)
    torch.manual_seed(NOISE_SEED)
    rgb, disp, acc, _, _ = npa.raw2outputs(raw, z_f, rays[:, 3:6], 1.0, True)
    loss_h = npa.img2mse(rgb, target)
    loss_h.backward()
    g_want = grads_of(nf)
    zero_grads(nc, nf)
    for k, v in (("rgb_map", rgb), ("disp_map", disp), ("acc_map", acc), ("raw", raw), ("z_std", z_std)):
        assert bits_equal(got[k].detach(), v.detach()), (k, maxdiff(got[k], v))
    assert stats == {"evaluated": chain.kept[0], "total": n * (N_C + N_F), "rays_stopped": int(torch.isfinite(z_stop).sum())}
    with torch.no_grad():
        npa.render_rays(rays, nc, None, **kw)
    assert chain.kept[0] < grid.last_stats["evaluated"]
    assert bits_equal(loss_g.detach(), loss_h.detach()) and float(flat_of(g_got).abs().max()) > 0
    for i, (x, y) in enumerate(zip(g_got, g_want)):
        assert bits_equal(x, y), (i, maxdiff(x, y))


def test_with_clipping_and_through_render_in_chunks(npa, dev, nets, datapath_fp16x3):
    """clip_to_occupancy=True + early_stop_eps == the same call on grid.clip_rays(rays)[0]; render(chunk=96) == the unchunked call with
    last_stats summed over the chunks (batchify_rays)"""
    nc, nf, _, _ = nets
    rays, rnd, _ = _small_scene(dev)
    n = rays.shape[0]
    grid = npa.OccupancyGrid.from_mask(ball_grid(npa, dev).to_mask(), BOX_LO, BOX_HI, outside="skip", device=dev)
    kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd)
    kw = dict(kw, occupancy=grid, early_stop_eps=eps_for(npa, grid, rays, nc, **kw))
    clipped, hit = grid.clip_rays(rays)
    assert 0 < int(hit.sum()) and not bits_equal(clipped, rays)
    with torch.no_grad():
        got = npa.render_rays(rays, nc, None, clip_to_occupancy=True, **kw)
        stats = dict(grid.last_stats)
        want = npa.render_rays(clipped, nc, None, **kw)
        assert stats == dict(grid.last_stats, rays_hit=int(hit.sum()), rays=n) and 0 < stats["rays_stopped"] < n
        for k in want:
            assert bits_equal(got[k], want[k]), k
        # chunks: render() hands the keyword to batchify_rays, which slices the randoms and sums the stats
        whole = npa.render_rays(rays, nc, None, **kw)
        total = dict(grid.last_stats)
        chunked = npa.batchify_rays(rays, 96, network_fn=nc, network_query_fn=None, **kw)
        assert grid.last_stats == total and 0 < total["rays_stopped"] < n
        for k in whole:
            assert bits_equal(chunked[k], whole[k]), k
        K = np.array([[20.0, 0, 8.0], [0, 20.0, 8.0], [0, 0, 1]])
        geo = dict(rays=(rays[:, 0:3], rays[:, 3:6]), ndc=False, near=2.0, far=6.0, use_viewdirs=True, network_fn=nc, network_query_fn=None)
        one = npa.render(16, 16, K, chunk=1 << 20, **geo, **kw)
        total = dict(grid.last_stats)
        many = npa.render(16, 16, K, chunk=96, **geo, **kw)
        assert grid.last_stats == total and 0 < total["rays_stopped"] < n and total["total"] == n * (2 * N_C + N_F)
        for a, b in zip(one[:3], many[:3]):
            assert bits_equal(a, b)
        assert set(one[3]) == set(many[3]) == {"raw", "rgb0", "disp0", "acc0", "z_std"}
        for k in one[3]:
            assert bits_equal(one[3][k], many[3][k]), k


def test_resident_sub_chunks_give_the_gradients_of_one_piece(npa, dev, nets, monkeypatch, datapath_fp16x3):
    """As test_gpu_occupancy_train's test of the same name, with the option on: 2500 rays under a budget forced to 1024 rays per
    sub-chunk; z_stop is computed per sub-chunk, the stats are those of one piece, and the parameter gradients match the one-piece call
    within that test's bound (twice the dense-vs-stock-hook difference under the same forced budget); the ray gradients' difference is
    reported"""
    hb = npa.hip_backend
    render_mod = sys.modules["nerf_pytorch_amd.render"]
    nc, nf, _, _ = nets
    n = 2500
    rays = orc.synthetic_rays(n, seed=8).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, N_C, N_F, seed=6).items()}
    target = scene_target(dev, n)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=0.5, randoms=rnd)
    eps = eps_for(npa, grid, rays, nc, **kw)
    stop_calls = []
    real = hb.occ_stop_depth
    monkeypatch.setattr(hb, "occ_stop_depth", lambda z, w, e: (stop_calls.append(z.shape[0]), real(z, w, e))[1])

    def run(**extra):
        zero_grads(nc, nf)
        r = rays.clone().requires_grad_(True)
        loss_of(npa, npa.render_rays(r, nc, extra.pop("hook", None), **kw, **extra), target).backward()
        return render_mod.LAST_BACKWARD_PLAN, torch.cat([nc.last_flat_grad, nf.last_flat_grad]).clone(), r.grad.clone()
    plan1, g1, r1 = run(occupancy=grid, early_stop_eps=eps)
    stats1 = dict(grid.last_stats)
    assert stop_calls == [n]
    _, stock, _ = run(hook=lambda p, v, m: npa.run_network(p, v, m, None, None))
    monkeypatch.setattr(hb, "SAVE_BUDGET_BYTES", 4 * hb.workspace_floats(1024, N_C, N_F, True, "fp16x3") + 1)
    plan2, g2, r2 = run(occupancy=grid, early_stop_eps=eps)
    plan_dense, dense, _ = run()
    zero_grads(nc, nf)
    assert plan1 == ("one launch", n, n) and plan2[0] == "resident sub-chunks" and plan2[1] == n and plan2[2] <= 1024
    assert plan_dense[0] == "resident sub-chunks"
    assert len(stop_calls) >= 4 and sum(stop_calls[1:]) == n and max(stop_calls[1:]) <= 1024
    assert grid.last_stats == stats1 and 0 < stats1["rays_stopped"] < n
    diff, yard = rel_l2(g2, g1), rel_l2(dense, stock)
    print(f"\nsub-chunks vs one piece: parameter gradients relative L2 {diff:.3e} (yardstick {yard:.3e}); ray gradients bit-identical "
          f"{torch.equal(r1, r2)}, relative L2 {rel_l2(r2, r1):.1e}")
    assert diff <= 2.0 * yard
    assert bool(torch.isfinite(r2).all())


# ------------------------------------------------------------------------------------------------ 6. off means off
@pytest.mark.parametrize("grad", [False, True])
def test_none_is_the_call_without_the_keyword(npa, dev, nets, datapath_fp16x3, monkeypatch, grad):
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    rays, rnd, _ = _small_scene(dev)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, occupancy=grid)
    counts = {"stop": 0, "compact_stop": 0}
    real_stop, real_compact = hb.occ_stop_depth, hb.occ_compact
    monkeypatch.setattr(hb, "occ_stop_depth", lambda *a, **k: (counts.__setitem__("stop", counts["stop"] + 1), real_stop(*a, **k))[1])

    def compact(*a, **k):
        if (a[5] if len(a) > 5 else k.get("z_stop")) is not None:
            counts["compact_stop"] += 1
        return real_compact(*a, **k)
    monkeypatch.setattr(hb, "occ_compact", compact)
    with torch.set_grad_enabled(grad):
        a = npa.render_rays(rays, nc, None, randoms=rnd, **kw)
        stats_a = dict(grid.last_stats)
        b = npa.render_rays(rays, nc, None, randoms=rnd, early_stop_eps=None, **kw)
        assert grid.last_stats == stats_a and "rays_stopped" not in grid.last_stats
        # the same random draws: without `randoms` a seeded call consumes the generator identically
        torch.manual_seed(17)
        c = npa.render_rays(rays, nc, None, **kw)
        after_c = torch.rand(4, device=dev)
        torch.manual_seed(17)
        d = npa.render_rays(rays, nc, None, early_stop_eps=None, **kw)
        after_d = torch.rand(4, device=dev)
        assert counts == {"stop": 0, "compact_stop": 0}
        torch.manual_seed(17)
        e = npa.render_rays(rays, nc, None, early_stop_eps=0.5, **kw)
        after_e = torch.rand(4, device=dev)
    assert counts == {"stop": 1, "compact_stop": 1}         # (the wrappers do count)
    assert list(a) == list(b) == list(c) == list(d)
    for k in a:
        assert bits_equal(a[k].detach(), b[k].detach()) and bits_equal(c[k].detach(), d[k].detach()), k
    assert torch.equal(after_c, after_d) and torch.equal(after_c, after_e)
    assert bits_equal(c["rgb0"].detach(), e["rgb0"].detach()) and bits_equal(c["z_std"], e["z_std"])


# ------------------------------------------------------------------------------------------------ 7. degenerate
def test_every_ray_stops_behind_the_first_interval(npa, dev, nets, datapath_fp16x3, monkeypatch):
    """eps = 1 - 1e-6 on weights whose first entry is positive (an all-occupied grid over the whole ray range, so the first coarse sample
    is evaluated, and a constant on the coarse density head's bias, so its density is positive): every ray stops at z_c[1], the
    refining pass evaluates exactly the depths in front of it, and the outputs are finite"""
    hb = npa.hip_backend
    nc, nf = fresh_nets(npa, dev, nets)
    with torch.no_grad():
        nc.alpha_linear.bias += 200.0
    rays, rnd, _ = _small_scene(dev)
    n = rays.shape[0]
    grid = npa.OccupancyGrid((-8.0, -8.0, -8.0), (8.0, 8.0, 8.0), 4, device=dev)
    eps = 1.0 - 1e-6
    seen = {}
    real_stop, real_fine = hb.occ_stop_depth, hb.sample_fine
    monkeypatch.setattr(hb, "occ_stop_depth", lambda z, w, e: seen.update(z_c=z, w=w, z_stop=real_stop(z, w, e)) or seen["z_stop"])
    monkeypatch.setattr(hb, "sample_fine", lambda *a, **k: (lambda r: (seen.update(z_f=r[0]), r)[1])(real_fine(*a, **k)))
    kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=1.0, randoms=rnd, retraw=True, occupancy=grid)
    with torch.no_grad():
        out = npa.render_rays(rays, nc, None, early_stop_eps=eps, **kw)
        stats = dict(grid.last_stats)
        off = npa.render_rays(rays, nc, None, **kw)
    assert grid.last_stats == {"evaluated": n * (2 * N_C + N_F), "total": n * (2 * N_C + N_F)}
    assert bool((seen["w"][:, 0] > 0).all())
    assert bits_equal(seen["z_stop"], seen["z_c"][:, 1].contiguous())
    in_front = seen["z_f"] < seen["z_c"][:, 1:2]
    assert stats == {"evaluated": n * N_C + int(in_front.sum()), "total": n * (2 * N_C + N_F), "rays_stopped": n}
    assert bool((in_front.sum(-1) >= 1).all()) and int(in_front.sum()) < n * N_F        # z_c[0] itself, and far from everything
    assert bool((out["raw"][~in_front] == 0).all()) and bool((out["raw"][in_front] != 0).any(-1).all())
    for k in ("rgb_map", "acc_map", "raw", "rgb0", "z_std"):
        assert bool(torch.isfinite(out[k]).all()), k
    assert bits_equal(out["rgb0"], off["rgb0"]) and bits_equal(out["z_std"], off["z_std"])


def test_all_empty_grid_with_the_option(npa, dev, nets, monkeypatch):
    """as test_gpu_occupancy_train.test_all_empty_grid_gives_zero_gradients_and_no_field_launch, with early_stop_eps: m == 0 in both
    passes, no field launch, zero gradients, no ray stops (all weights are 0)"""
    hb = npa.hip_backend
    nc, nf = fresh_nets(npa, dev, nets)
    rays, rnd, target = _small_scene(dev)
    empty = npa.DensityGrid.from_mask(torch.zeros(2, 2, 2, dtype=torch.bool), BOX_LO, BOX_HI, outside="skip", device=dev)
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = hb.field_fwd, hb.field_bwd
    monkeypatch.setattr(hb, "field_fwd", lambda *a, **k: (calls.__setitem__("fwd", calls["fwd"] + 1), fwd(*a, **k))[1])
    monkeypatch.setattr(hb, "field_bwd", lambda *a, **k: (calls.__setitem__("bwd", calls["bwd"] + 1), bwd(*a, **k))[1])
    r = rays.clone().requires_grad_(True)
    out = npa.render_rays(r, nc, None, N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=1.0, randoms=rnd,
                          occupancy=empty, retraw=True, early_stop_eps=0.01)
    assert empty.last_stats == {"evaluated": 0, "total": 256 * 256, "rays_stopped": 0}
    assert bool((out["rgb_map"] == 1).all()) and bool((out["raw"] == 0).all())
    loss_of(npa, out, target).backward()
    assert calls == {"fwd": 0, "bwd": 0}
    for m in (nc, nf):
        assert all(p.grad is not None and bool((p.grad == 0).all()) for p in m.parameters())
    assert r.grad is not None and bool(torch.isfinite(r.grad).all()) and bool((r.grad[:, [0, 1, 2, 6, 7, 8, 9, 10]] == 0).all())
    with torch.no_grad():
        npa.render_rays(rays, nc, None, N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, occupancy=empty, early_stop_eps=0.01)
    assert empty.last_stats == {"evaluated": 0, "total": 256 * 256, "rays_stopped": 0} and calls == {"fwd": 0, "bwd": 0}
