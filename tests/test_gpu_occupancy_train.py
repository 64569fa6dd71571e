"""GPU tests (-m gpu) of training through an occupancy grid: the three kernels of the backward path alone, DensityGrid.update against its
plain-torch definition, and render_rays(occupancy=DensityGrid) with gradients against the COMPACTING HOOK -- a user network_query_fn,
built from public pieces, that evaluates only the occupied points and leaves exact zeros elsewhere.  The hook sends the same M records
through the same field launches as the grid path, so most checks are bit for bit."""
import sys

import numpy as np
import pytest
import torch

import nerf_oracle as orc
from test_gpu_occupancy import BOX_LO, BOX_HI, BOX_R, N_RAYS, _scene, ball_mask, bits_equal
from test_gpu_parity import datapath, dev, maxdiff, nets, npa  # noqa: F401  (fixtures)
from test_gpu_ray_grad import rel_l2

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32
NET_KW = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)


def ball_dgrid(npa, device, **kw):
    """the scene's grid (test_gpu_occupancy.ball_grid) as a DensityGrid: the ball's bits copied in"""
    g = npa.DensityGrid(BOX_LO, BOX_HI, BOX_R, device=device, **kw)
    g.bits = npa.OccupancyGrid.from_mask(ball_mask(), BOX_LO, BOX_HI, device=device).bits.clone()
    return g


def compacting_hook(npa, grid, seen=None, taps=None):
    """THE YARDSTICK: evaluate the occupied points only (ray-major, sample-minor: the compaction's order), exact zeros elsewhere.
    taps (a list): per call a dict with idx and, after the backward, the per-point gradients d_pts / d_viewdirs [M, 3]."""
    def hook(pts, viewdirs, net):
        N, S = pts.shape[:2]
        occ = grid.occupied(pts)
        idx = occ.reshape(-1).nonzero()[:, 0]
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
        raw_c = npa.query_points(net, p_sel, v_sel)
        return torch.zeros(N * S, 4, device=pts.device).index_put((idx,), raw_c).view(N, S, 4)
    return hook


def positive_median_density(npa, net, dev, res):
    """a threshold that splits the scene: the median of the POSITIVE densities of `net` at the cell centres (a running maximum that
    starts at 0 never falls below 0, so a threshold at or below 0 would keep every cell)"""
    with torch.no_grad():
        probe = npa.DensityGrid(BOX_LO, BOX_HI, res, device=dev)
        sigma = npa.query_points(net, probe.cell_points(0, probe.n_cells).reshape(-1, 3),
                                 torch.tensor([0.0, 0.0, 1.0], device=dev).expand(probe.n_cells, 3))[:, 3]
    assert int((sigma > 0).sum()) > 10
    return float(sigma[sigma > 0].median())


def fresh_nets(npa, dev, nets):
    nc, nf = npa.NeRF(**NET_KW).to(dev), npa.NeRF(**NET_KW).to(dev)
    nc.load_state_dict(nets[2])
    nf.load_state_dict(nets[3])
    return nc, nf


def zero_grads(*models):
    for m in models:
        for p in m.parameters():
            p.grad = None


def grads_of(model):
    return [None if p.grad is None else p.grad.detach().clone() for p in model.parameters()]


def flat_of(grads):
    return torch.cat([g.reshape(-1) for g in grads])


def loss_of(npa, out, target):
    return npa.img2mse(out["rgb_map"], target) + (npa.img2mse(out["rgb0"], target) if "rgb0" in out else 0.0)


def scene_target(dev, n=N_RAYS):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(77)).to(dev)


def slots_of(mask):
    flat = mask.reshape(-1)
    return torch.where(flat, torch.cumsum(flat.to(torch.int64), 0) - 1, torch.full_like(flat, -1, dtype=torch.int64)).to(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the kernels alone
def test_gather_equals_torch_indexing(npa, dev):
    """nerf_occ_gather == d_raw[mask], exactly; sizes that do not fill a block, M = 0 and M = P; rows beyond M are not touched"""
    hb = npa.hip_backend
    g = torch.Generator().manual_seed(2)
    for P in (1, 63, 255, 256, 257, 1000, 70001):
        for frac in (0.0, 0.4, 1.0):
            mask = (torch.rand(P, generator=g) < frac).to(dev)
            slot = slots_of(mask)
            m = int(mask.sum())
            d_raw = torch.randn(P, 4, generator=g).to(dev)
            out = torch.full((m + 3, 4), 7.0, device=dev)
            hb.occ_gather(slot, d_raw, out[:m])
            assert bits_equal(out[:m], d_raw[mask]), (P, frac)
            assert bool((out[m:] == 7.0).all()), (P, frac)
    # gather after expand gives back the compacted rows: the two kernels mirror each other
    mask = (torch.rand(5000, generator=g) < 0.3).to(dev)
    slot, m = slots_of(mask), int(mask.sum())
    a = torch.randn(m, 4, generator=g).to(dev)
    back = hb.occ_gather(slot, hb.occ_expand(slot, a, torch.empty(5000, 4, device=dev)), torch.empty(m, 4, device=dev))
    assert bits_equal(back, a)


def _fold64(slot, z, d_rec, n, S):
    """float64 fold of the same fp32 inputs, and the sum of the terms' magnitudes per element: [n, 11] each"""
    s = slot.view(n, S).long()
    on = (s >= 0).double()[..., None]
    rec = d_rec.double()[s.clamp(min=0)]                         # [n, S, 11]
    gp, gv, z64 = rec[..., 0:3] * on, rec[..., 8:11] * on, z.double()[..., None]
    zero = torch.zeros(n, 2, dtype=torch.float64, device=z.device)
    total = torch.cat([gp.sum(1), (z64 * gp).sum(1), zero, gv.sum(1)], -1)
    mag = torch.cat([gp.abs().sum(1), (z64 * gp).abs().sum(1), zero, gv.abs().sum(1)], -1)
    return total, mag


@pytest.mark.parametrize("S", [64, 192, 5])
def test_fold_rays_against_a_float64_fold(npa, dev, S):
    """nerf_occ_fold_rays on random slot patterns (rays 0..9 empty, 10..19 full, a ray count that does not fill the last block) against
    the float64 fold of the same inputs.  Bound per element: S * 2^-24 * sum|terms| * 1.01 -- DERIVED, not measured: a sum of S fp32
    terms in any order is within (S - 1) u sum|t| (first order in u = 2^-24), each z * g term carries one more rounding u |t|, and 1.01
    covers the higher orders (S u < 2e-5).  Columns 6:8 are exactly 0, columns 3:8 of d_rec are never read (NaN there), two runs give
    the same bits, and accumulate = 1 is one fp32 addition onto what was there (columns 6:8 untouched)."""
    hb = npa.hip_backend
    g = torch.Generator().manual_seed(40 + S)
    n = 301
    mask = torch.rand(n, S, generator=g) < 0.3
    mask[0:10], mask[10:20] = False, True
    mask = mask.to(dev)
    slot, m = slots_of(mask), int(mask.sum())
    d_rec = (torch.randn(m, 11, generator=g) * torch.logspace(-3, 3, m)[torch.randperm(m, generator=g)][:, None]).to(dev)
    d_rec[:, 3:8] = float("nan")
    z = (torch.rand(n, S, generator=g) * 4.0 + 2.0).to(dev)
    out = hb.occ_fold_rays(slot, z, d_rec, torch.full((n, 11), 9.0, device=dev))
    want, mag = _fold64(slot, z, d_rec, n, S)
    err = (out.double() - want).abs()
    bound = 1.01 * S * U * mag
    print(f"\nS={S}: worst error / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}, max error {float(err.max()):.3e}")
    assert bool((err <= bound).all())
    assert bool((out[:, 6:8] == 0).all()) and bool((out[0:10] == 0).all())
    again = hb.occ_fold_rays(slot, z, d_rec, torch.empty((n, 11), device=dev))
    assert bits_equal(out, again)
    prior = torch.randn(n, 11, generator=g).to(dev)
    acc = hb.occ_fold_rays(slot, z, d_rec, prior.clone(), accumulate=True)
    assert bits_equal(acc[:, 6:8], prior[:, 6:8])
    cols = [0, 1, 2, 3, 4, 5, 8, 9, 10]
    assert bits_equal(acc[:, cols], prior[:, cols] + out[:, cols])
    # M = 0: zeros (the entry point never reads d_rec)
    none = slots_of(torch.zeros(n, S, dtype=torch.bool, device=dev))
    assert bool((hb.occ_fold_rays(none, z, torch.empty(0, 11, device=dev), torch.full((n, 11), 3.0, device=dev)) == 0).all())


def same_floats(a, b):
    """bit for bit where neither is a NaN; NaNs in the same places (the payload of a propagated NaN is the hardware's)"""
    a, b = a.cpu(), b.cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


@pytest.mark.parametrize("K", [1, 4])
def test_density_update_equals_the_reference_bit_for_bit(npa, dev, K):
    """nerf_occ_density_update against DensityGrid._update_reference: NaN / negative / infinite samples, negative, zero, infinite and NaN
    densities, a cell count that does not fill a block, a run inside the grid (cells outside it untouched)"""
    hb = npa.hip_backend
    g = torch.Generator().manual_seed(7 + K)
    ref = npa.DensityGrid((0, 0, 0), (1, 1, 1), (10, 10, 11), device=torch.device("cpu"), decay=0.95)
    n = ref.n_cells
    density = torch.randn(n, generator=g) * 3.0
    density[::13], density[5::17], density[7::29], density[11::31] = 0.0, float("inf"), float("nan"), -0.0
    sigma = torch.randn(n, K, generator=g) * 3.0
    sigma[torch.rand(n, K, generator=g) < 0.2] = float("nan")
    sigma[3::19, 0], sigma[4::23, K - 1] = float("inf"), float("-inf")
    for first, last in ((0, n), (32, 777), (1056, n)):
        ref.density = density.clone()
        ref._update_reference(sigma[first:last].reshape(-1), first, last)
        got = density.clone().to(dev)
        hb.occ_density_update(sigma[first:last].reshape(-1).contiguous().to(dev), K, 0.95, got[first:last])
        assert same_floats(got, ref.density), (first, last)
        assert same_floats(got[:first], density[:first]) and same_floats(got[last:], density[last:])
    assert bool(torch.isnan(ref.density).any()) and bool((ref.density < 0).any())


def test_update_equals_the_plain_torch_definition(npa, dev, nets):
    """DensityGrid.update(model) on the device against a CPU twin stepped by _update_reference / _bits_reference from densities
    evaluated with query_points at cell_points: density and bits bit for bit over three updates (everything, then two partial runs that
    wrap), with dilation and a grid whose cell count is no multiple of 32; the slices of a large run give the same as one piece"""
    nc, nf, _, _ = nets
    res = (9, 11, 13)
    thr = positive_median_density(npa, nf, dev, res)
    kw = dict(decay=0.9, sigma_threshold=thr, dilate=1)
    g = npa.DensityGrid(BOX_LO, BOX_HI, res, device=dev, **kw)
    twin = npa.DensityGrid(BOX_LO, BOX_HI, res, device=torch.device("cpu"), **kw)
    gen_a, gen_b = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    for fraction, model in ((0.3, nf), (0.6, nc), (0.6, nf)):
        assert g.update(model, fraction=fraction, samples_per_cell=3, generator=gen_a) is g
        for first, last in twin._next_runs(fraction):
            pts = g.cell_points(first, last, 3, gen_b).reshape(-1, 3)
            with torch.no_grad():
                sigma = npa.query_points(model, pts, torch.tensor([0.0, 0.0, 1.0], device=dev).expand(pts.shape[0], 3))[:, 3]
            twin._update_reference(sigma.cpu(), first, last)
        twin.bits = twin._bits_reference()
        assert same_floats(g.density, twin.density) and torch.equal(g.bits.cpu(), twin.bits)
        assert (g.cursor, g.n_updates) == (twin.cursor, twin.n_updates)
    assert 0.0 < g.fraction_occupied() < 1.0
    # slices
    big = npa.DensityGrid(BOX_LO, BOX_HI, 32, device=dev, sigma_threshold=thr).update(nf)
    occ_mod = npa.occupancy
    keep, occ_mod._SLICE_CELLS = occ_mod._SLICE_CELLS, 1 << 12
    try:
        sliced = npa.DensityGrid(BOX_LO, BOX_HI, 32, device=dev, sigma_threshold=thr).update(nf)
    finally:
        occ_mod._SLICE_CELLS = keep
    assert same_floats(big.density, sliced.density) and torch.equal(big.bits, sliced.bits)
    # the bits are what from_network builds from the same network (decay plays no part in the first update)
    static = npa.OccupancyGrid.from_network(nf, BOX_LO, BOX_HI, 32, sigma_threshold=thr, dilate=0)
    assert torch.equal(static.bits, big.bits)


# ------------------------------------------------------------------------------------------------ 2. forward
@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
@pytest.mark.parametrize("perturb,noise", [(0.0, 0.0), (1.0, 1.0), (1.0, 0.0), (0.0, 1.0)])
def test_forward_with_grad_equals_the_no_grad_render(npa, dev, nets, datapath, perturb, noise):
    """grad mode on + DensityGrid: every returned tensor equals the no_grad render with the same bits, bit for bit; same keys in the
    same order, same last_stats; the maps carry a grad_fn, z_std does not"""
    nc, nf, _, _ = nets
    rays, rnd = _scene(dev)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=perturb, raw_noise_std=noise, retraw=True, randoms=rnd)
    for extra in ({}, dict(N_importance=0), dict(network_fine=None)):
        kw2 = dict(kw, **extra)
        with torch.no_grad():
            want = npa.render_rays(rays, nc, None, occupancy=grid, **kw2)
        stats = dict(grid.last_stats)
        grid.last_stats = None
        got = npa.render_rays(rays, nc, None, occupancy=grid, **kw2)
        assert list(got) == list(want), extra
        for k in want:
            assert bits_equal(got[k], want[k]), (extra, k, maxdiff(got[k], want[k]))
        assert grid.last_stats == stats and 0 < stats["evaluated"] < stats["total"]
        assert got["rgb_map"].grad_fn is not None and got["raw"].grad_fn is not None and want["rgb_map"].grad_fn is None
        if "z_std" in got:
            assert not got["z_std"].requires_grad
        del got          # (a graph dropped without backward)


# ------------------------------------------------------------------------------------------------ 3. / 4. parameter gradients
def _param_grads(npa, rays, rnd, target, nc, nf, grid, hook, **extra):
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, randoms=rnd)
    kw.update(extra)
    zero_grads(nc, *([nf] if nf is not None else []))
    if hook is None:
        out = npa.render_rays(rays, nc, None, occupancy=grid, **kw)
    else:
        out = npa.render_rays(rays, nc, hook, **kw)
    loss = loss_of(npa, out, target)
    loss.backward()
    return loss.detach(), grads_of(nc), (grads_of(nf) if nf is not None else None)


@pytest.mark.parametrize("datapath", ["fp32", "fp16x3", "fp16x3w", "bf16x3"], indirect=True)
def test_parameter_gradients_two_networks_bit_for_bit(npa, dev, nets, datapath):
    """loss = img2mse(rgb_map, t) + img2mse(rgb0, t): .grad of every parameter of both networks equals the compacting hook's, bit for
    bit -- both paths run the same field_fwd / delta chain / weight-gradient launches on the same M records"""
    nc, nf, _, _ = nets
    rays, rnd = _scene(dev)
    target = scene_target(dev)
    grid = ball_dgrid(npa, dev)
    seen = []
    l_g, gc, gf = _param_grads(npa, rays, rnd, target, nc, nf, grid, None)
    stats = dict(grid.last_stats)
    l_h, hc, hf = _param_grads(npa, rays, rnd, target, nc, nf, grid, compacting_hook(npa, grid, seen))
    zero_grads(nc, nf)
    assert stats == {"evaluated": seen[0][0] + seen[1][0], "total": N_RAYS * 256} and 0 < stats["evaluated"] < stats["total"]
    assert bits_equal(l_g, l_h)
    for name, a, b in (("coarse", gc, hc), ("fine", gf, hf)):
        assert all(x is not None for x in a) and float(flat_of(a).abs().max()) > 0
        for i, (x, y) in enumerate(zip(a, b)):
            assert bits_equal(x, y), (name, i, maxdiff(x, y), rel_l2(flat_of(a), flat_of(b)))


def test_parameter_gradients_shared_network(npa, dev, nets, datapath_fp16x3):
    """network_fine=None, N_importance=128: the grid path accumulates the fine pass into the coarse network's vector INSIDE the
    weight-gradient kernel (accumulate=True), autograd adds the hook's two vectors afterwards.  Bit equality is tried first; where the
    accumulation order forbids it, the relative L2 difference is bounded by twice the same difference between two paths the dense
    renderer already has -- _RenderRays (in-kernel accumulation) against the stock hooked path (network_query_fn = run_network; autograd's
    addition), same rays, no grid -- measured in this test.
    MEASURED on an MI355X (fp16x3, 1024 rays): bit-identical (relative L2 0); the yardstick is 0 as well -- the weight-gradient kernel's
    accumulate adds its finished sum to what the vector holds, one fp32 addition per element, as autograd does."""
    nc, _, _, _ = nets
    rays, rnd = _scene(dev)
    target = scene_target(dev)
    grid = ball_dgrid(npa, dev)
    _, g, _ = _param_grads(npa, rays, rnd, target, nc, None, grid, None, network_fine=None)
    _, h, _ = _param_grads(npa, rays, rnd, target, nc, None, grid, compacting_hook(npa, grid), network_fine=None)
    zero_grads(nc)
    kw = dict(N_samples=64, N_importance=128, network_fine=None, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, randoms=rnd)
    loss_of(npa, npa.render_rays(rays, nc, None, **kw), target).backward()
    dense = grads_of(nc)
    zero_grads(nc)
    loss_of(npa, npa.render_rays(rays, nc, lambda p, v, m: npa.run_network(p, v, m, None, None), **kw), target).backward()
    stock = grads_of(nc)
    zero_grads(nc)
    equal = all(bits_equal(x, y) for x, y in zip(g, h))
    diff, yard = rel_l2(flat_of(g), flat_of(h)), rel_l2(flat_of(dense), flat_of(stock))
    print(f"\nshared network: grid vs compacting hook bit-identical {equal}, relative L2 {diff:.3e}; yardstick (dense vs stock hook) {yard:.3e}")
    assert equal or diff <= 2.0 * yard, (diff, yard)


@pytest.fixture
def datapath_fp16x3(npa):
    prev = npa.get_precision()
    npa.set_precision("fp16x3")
    yield "fp16x3"
    npa.set_precision(prev)


# ------------------------------------------------------------------------------------------------ 5. ray gradients
@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
def test_ray_gradients_against_the_float64_fold_of_the_hooks(npa, dev, nets, datapath, monkeypatch):
    """rays.requires_grad_(): the hook side yields the per-point gradients d_pts / d_viewdirs (tensor hooks on the M selected points)
    and the compositing's d_rays_d of both passes; their float64 fold -- [0:3] sum d_pts, [3:6] sum z d_pts + the two |d| terms, [8:11]
    sum d_viewdirs -- is what the grid path's rays.grad must equal within (S_c + S_f + 2) * 2^-24 * sum|terms| * 1.01 per element: the
    bound of the fold kernel's test for the S_c + S_f sample terms of both passes (any order, one product rounding each), and one more
    rounding for each pass's added |d| term.  Columns 6:8 are exactly 0."""
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    rays0, rnd = _scene(dev)
    target = scene_target(dev)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=0.5, randoms=rnd)
    rg = rays0.clone().requires_grad_(True)
    loss_of(npa, npa.render_rays(rg, nc, None, occupancy=grid, **kw), target).backward()
    got = rg.grad.clone()
    # the hook side, with the depths and the compositing's direction gradients recorded on the way
    zs, dns = [], []
    sc, sf, bwd = hb.sample_coarse, hb.sample_fine, hb.raw2outputs_bwd
    monkeypatch.setattr(hb, "sample_coarse", lambda *a, **k: (zs.append(sc(*a, **k)), zs[-1])[1])
    monkeypatch.setattr(hb, "sample_fine", lambda *a, **k: (lambda r: (zs.append(r[0]), r)[1])(sf(*a, **k)))
    monkeypatch.setattr(hb, "raw2outputs_bwd", lambda *a, **k: (dns.append(k.get("d_rays_d")), bwd(*a, **k))[1])
    taps = []
    rh = rays0.clone().requires_grad_(True)
    loss_of(npa, npa.render_rays(rh, nc, compacting_hook(npa, grid, taps=taps), **kw), target).backward()
    zero_grads(nc, nf)
    assert len(zs) == 2 and len(taps) == 2 and len(dns) == 2 and all(d is not None for d in dns)
    n = N_RAYS
    want = torch.zeros(n, 11, dtype=torch.float64, device=dev)
    mag = torch.zeros_like(want)
    for z, tap in zip(zs, taps):
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
    bound = 1.01 * (64 + 192 + 2) * U * mag
    geo = [0, 1, 2, 3, 4, 5, 8, 9, 10]
    print(f"\n[{datapath}] ray gradient: worst error / bound {float((err[:, geo] / bound[:, geo].clamp(min=1e-300)).max()):.3f}; "
          f"relative L2 vs the hook path's own rays.grad {rel_l2(got, rh.grad):.2e}")
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    assert bool((got[:, 6:8] == 0).all())
    assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())


def test_pose_gradient_through_the_grid(npa, dev, nets):
    """render(c2w=pose.requires_grad_(), occupancy=DensityGrid): d loss / d c2w is finite and matches the compacting hook's through the
    same call (chunks of 150 rays) within 3e-3 relative L2, the bound test_gpu_ray_grad.test_pose_gradient_through_render holds pose
    gradients to"""
    nc, nf, _, _ = nets
    H, W, focal = 20, 20, 25.0
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    pose = torch.tensor([[1.0, 0, 0, 0.1], [0, 0.8, -0.6, 0.2], [0, 0.6, 0.8, 4.0]])
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(4)).to(dev)
    grid = ball_dgrid(npa, dev)
    kw = dict(network_fn=nc, N_samples=64, N_importance=128, network_fine=nf, perturb=0., white_bkgd=True, raw_noise_std=0.,
              chunk=150, ndc=False, near=2., far=6., use_viewdirs=True)
    grads = []
    for extra in (dict(network_query_fn=None, occupancy=grid), dict(network_query_fn=compacting_hook(npa, grid))):
        c2w = pose.to(dev).requires_grad_(True)
        rgb, _, _, ex = npa.render(H, W, K, c2w=c2w, **kw, **extra)
        (npa.img2mse(rgb, target) + npa.img2mse(ex["rgb0"], target)).backward()
        grads.append(c2w.grad.clone())
        zero_grads(nc, nf)
    assert grid.last_stats["total"] == 400 * 256 and 0 < grid.last_stats["evaluated"] < 400 * 256
    err = rel_l2(grads[0], grads[1])
    print(f"\npose gradient through the grid vs the compacting hook: relative L2 {err:.2e}")
    assert bool(torch.isfinite(grads[0]).all()) and float(grads[0].abs().max()) > 0 and err <= 3e-3


# ------------------------------------------------------------------------------------------------ 6. twenty optimizer steps
def test_twenty_optimizer_steps_stay_bit_identical(npa, dev, nets, datapath_fp16x3):
    """Two copies of the networks, FlatAdam on both sides, the same seeded ray batches and randoms; one side renders with
    occupancy=DensityGrid, the other through the compacting hook over a second DensityGrid; both grids follow their fine network with
    maybe_update (warmup_steps=4, update_every=4, two samples per cell from seeded generators, a threshold at the median density of the
    initial network).  After 20 steps the parameters of both networks, density and bits are bit-identical: update, forward and backward
    tied together without a tolerance."""
    n = 256
    LR = 1e-5       # (small: the targets are noise, and the densities should stay near the scene's, which the threshold was chosen for)
    thr = positive_median_density(npa, nets[1], dev, BOX_R)
    sides = []
    for _ in range(2):
        nc, nf = fresh_nets(npa, dev, nets)
        sides.append(dict(nc=nc, nf=nf, opt=npa.FlatAdam(list(nc.parameters()) + list(nf.parameters()), lr=LR),
                          grid=npa.DensityGrid(BOX_LO, BOX_HI, BOX_R, device=dev, warmup_steps=4, update_every=4, sigma_threshold=thr),
                          gen=torch.Generator().manual_seed(31), updates=0, shares=[], occupied=[]))
    for step in range(20):
        rays = orc.synthetic_rays(n, seed=100 + step).to(dev)
        rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, 64, 128, seed=200 + step).items()}
        target = torch.rand(n, 3, generator=torch.Generator().manual_seed(300 + step)).to(dev)
        kw = dict(N_samples=64, N_importance=128, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, randoms=rnd)
        for i, s in enumerate(sides):
            if s["grid"].maybe_update(s["nf"], step, fraction=0.5, samples_per_cell=2, generator=s["gen"]):
                s["updates"] += 1
                s["occupied"].append(round(s["grid"].fraction_occupied(), 4))
            if i == 0:
                out = npa.render_rays(rays, s["nc"], None, network_fine=s["nf"], occupancy=s["grid"], **kw)
                s["shares"].append(s["grid"].last_stats["evaluated"] / s["grid"].last_stats["total"])
            else:
                out = npa.render_rays(rays, s["nc"], compacting_hook(npa, s["grid"]), network_fine=s["nf"], **kw)
            s["opt"].zero_grad()
            loss_of(npa, out, target).backward()
            s["opt"].step()
    a, b = sides
    print(f"\nevaluated share per step: {[round(x, 3) for x in a['shares']]}; threshold {thr:.4g}, "
          f"occupied cells after each update {a['occupied']}")
    assert a["updates"] == b["updates"] == 4 and a["grid"].n_updates == 4
    assert a["shares"][0] == 1.0 and a["shares"][-1] < 1.0       # all-occupied through the warm-up, then the grid skips
    assert 0.0 < a["grid"].fraction_occupied() < 1.0
    assert torch.equal(a["grid"].bits, b["grid"].bits) and bits_equal(a["grid"].density, b["grid"].density)
    for net in ("nc", "nf"):
        assert bits_equal(a[net].flat_params(), b[net].flat_params()), net
        assert not bits_equal(a[net].flat_params(), nets[0 if net == "nc" else 1].flat_params())     # (they did train)


# ------------------------------------------------------------------------------------------------ 7. plumbing
def _small_scene(dev, n=256):
    rays = orc.synthetic_rays(n, seed=21).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, 64, 128, seed=22).items()}
    return rays, rnd, scene_target(dev, n)


@pytest.mark.parametrize("shared", [False, True])
def test_grad_ready_fires_once_per_network_and_the_flat_vector_backs_every_grad(npa, dev, nets, shared):
    render_mod = sys.modules["nerf_pytorch_amd.render"]
    nc, nf = fresh_nets(npa, dev, nets)
    models = [nc] if shared else [nc, nf]
    rays, rnd, target = _small_scene(dev)
    grid = ball_dgrid(npa, dev)
    fired = []
    hook = lambda model, flat: fired.append((model, flat, flat.clone()))
    render_mod.GRAD_READY_HOOKS.append(hook)
    try:
        out = npa.render_rays(rays, nc, None, N_samples=64, N_importance=128, network_fine=None if shared else nf, white_bkgd=True, perturb=1.0,
                              randoms=rnd, occupancy=grid)
        loss_of(npa, out, target).backward()
    finally:
        render_mod.GRAD_READY_HOOKS.remove(hook)
    assert sorted(id(m) for m, _, _ in fired) == sorted(id(m) for m in models)      # once per network
    for model, flat, at_hook in fired:
        assert flat is model.last_flat_grad and flat.shape == (npa.hip_backend.N_PARAMS,)
        assert bits_equal(flat, at_hook)        # final when the hook saw it (a shared network: after the fine pass's accumulation)
        lo, hi = flat.data_ptr(), flat.data_ptr() + 4 * flat.numel()
        off = 0
        for p in model.parameters():
            assert p.grad is not None and lo <= p.grad.data_ptr() < hi and p.grad.is_contiguous()
            assert p.grad.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
            off += p.numel()
        assert off == flat.numel() and float(flat.abs().max()) > 0
    if shared:
        assert all(p.grad is None for p in nf.parameters())


def test_frozen_fine_network_second_backward_and_stale_parameters(npa, dev, nets, datapath_fp16x3):
    render_mod = sys.modules["nerf_pytorch_amd.render"]
    hb = npa.hip_backend
    nc, nf = fresh_nets(npa, dev, nets)
    rays, rnd, target = _small_scene(dev)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, randoms=rnd, occupancy=grid)
    # a frozen fine network: no weight-gradient launch for it, .grad stays None, no _grad_ready
    for p in nf.parameters():
        p.requires_grad_(False)
    fired = []
    hook = lambda model, flat: fired.append(model)
    render_mod.GRAD_READY_HOOKS.append(hook)
    wgrad_calls = []
    real_bwd = hb.field_bwd
    try:
        hb.field_bwd = lambda packed, act, d_raw, grad, *a, **k: (wgrad_calls.append(grad is not None), real_bwd(packed, act, d_raw, grad, *a, **k))[1]
        loss_of(npa, npa.render_rays(rays, nc, None, **kw), target).backward()
    finally:
        hb.field_bwd = real_bwd
        render_mod.GRAD_READY_HOOKS.remove(hook)
    assert fired == [nc] and wgrad_calls == [True]      # the frozen network's pass has nothing to compute: not even a delta chain
    assert all(p.grad is None for p in nf.parameters()) and all(p.grad is not None for p in nc.parameters())
    for p in nf.parameters():
        p.requires_grad_(True)
    zero_grads(nc, nf)
    # a second backward through the same graph
    loss = loss_of(npa, npa.render_rays(rays, nc, None, **kw), target)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="already consumed"):
        loss.backward()
    zero_grads(nc, nf)
    # an optimizer step between forward and backward (fp16x3: the backward reads live weights next to fragments packed at forward time)
    opt = npa.FlatAdam(list(nc.parameters()) + list(nf.parameters()), lr=5e-4)
    loss_of(npa, npa.render_rays(rays, nc, None, **kw), target).backward()
    loss = loss_of(npa, npa.render_rays(rays, nc, None, **kw), target)
    opt.step()
    with pytest.raises(RuntimeError, match="parameters changed between"):
        loss.backward()


def test_all_empty_grid_gives_zero_gradients_and_no_field_launch(npa, dev, nets, monkeypatch):
    hb = npa.hip_backend
    nc, nf = fresh_nets(npa, dev, nets)
    rays, rnd, target = _small_scene(dev)
    empty = npa.DensityGrid.from_mask(torch.zeros(2, 2, 2, dtype=torch.bool), BOX_LO, BOX_HI, outside="skip", device=dev)
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = hb.field_fwd, hb.field_bwd
    monkeypatch.setattr(hb, "field_fwd", lambda *a, **k: (calls.__setitem__("fwd", calls["fwd"] + 1), fwd(*a, **k))[1])
    monkeypatch.setattr(hb, "field_bwd", lambda *a, **k: (calls.__setitem__("bwd", calls["bwd"] + 1), bwd(*a, **k))[1])
    r = rays.clone().requires_grad_(True)
    out = npa.render_rays(r, nc, None, N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, randoms=rnd,
                          occupancy=empty, retraw=True)
    assert empty.last_stats == {"evaluated": 0, "total": 256 * 256}
    assert bool((out["rgb_map"] == 1).all()) and bool((out["raw"] == 0).all())
    loss_of(npa, out, target).backward()
    assert calls == {"fwd": 0, "bwd": 0}
    for m in (nc, nf):
        assert all(p.grad is not None and bool((p.grad == 0).all()) for p in m.parameters())
    assert r.grad is not None and bool(torch.isfinite(r.grad).all()) and bool((r.grad[:, [0, 1, 2, 6, 7, 8, 9, 10]] == 0).all())
    # the counters do count: the ball grid launches one forward and one backward per pass
    grid = ball_dgrid(npa, dev)
    zero_grads(nc, nf)
    loss_of(npa, npa.render_rays(rays, nc, None, N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, randoms=rnd,
                                 occupancy=grid), target).backward()
    assert calls == {"fwd": 2, "bwd": 2}


def test_resident_sub_chunks_give_the_gradients_of_one_piece(npa, dev, nets, monkeypatch, datapath_fp16x3):
    """2500 rays under a budget forced to 1024 rays per sub-chunk: the plan says "resident sub-chunks", every sub-chunk keeps leases of
    its own M, and the parameter gradients match the one-piece call within the bound of the shared-network test: twice the relative
    L2 difference between the dense _RenderRays path and the stock hooked path (network_query_fn = run_network) on the same rays, no
    grid, measured here UNDER THE SAME FORCED BUDGET -- there the dense path accumulates its sub-chunks in the weight-gradient kernel
    while the hooked path sums one piece, which is the pair of summation orders this test compares on the grid path.  (With the
    default budget that yardstick is 0 on these rays: both dense paths are bit-identical in one piece, and so are the grid path and
    the compacting hook.)  The ray gradients' difference is reported.  A total budget of zero raises and names the budget.
    MEASURED on an MI355X: 1.17e-7 against a yardstick of 1.48e-7 (bound 2.96e-7); ray gradients bit-identical."""
    hb = npa.hip_backend
    render_mod = sys.modules["nerf_pytorch_amd.render"]
    nc, nf, _, _ = nets
    n = 2500
    rays = orc.synthetic_rays(n, seed=8).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, 64, 128, seed=6).items()}
    target = scene_target(dev, n)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=0.5, randoms=rnd)

    def run(**extra):
        zero_grads(nc, nf)
        r = rays.clone().requires_grad_(True)
        loss_of(npa, npa.render_rays(r, nc, extra.pop("hook", None), **kw, **extra), target).backward()
        return render_mod.LAST_BACKWARD_PLAN, torch.cat([nc.last_flat_grad, nf.last_flat_grad]).clone(), r.grad.clone()
    plan1, g1, r1 = run(occupancy=grid)
    stats1 = dict(grid.last_stats)
    _, stock, _ = run(hook=lambda p, v, m: npa.run_network(p, v, m, None, None))
    monkeypatch.setattr(hb, "SAVE_BUDGET_BYTES", 4 * hb.workspace_floats(1024, 64, 128, True, "fp16x3") + 1)
    plan2, g2, r2 = run(occupancy=grid)
    plan_dense, dense, _ = run()
    zero_grads(nc, nf)
    assert plan1 == ("one launch", n, n) and plan2[0] == "resident sub-chunks" and plan2[1] == n and plan2[2] <= 1024
    assert plan_dense[0] == "resident sub-chunks"
    assert grid.last_stats == stats1
    diff, yard = rel_l2(g2, g1), rel_l2(dense, stock)
    print(f"\nsub-chunks vs one piece: parameter gradients relative L2 {diff:.3e} (yardstick {yard:.3e}); ray gradients bit-identical "
          f"{torch.equal(r1, r2)}, relative L2 {rel_l2(r2, r1):.1e}")
    assert diff <= 2.0 * yard
    assert bool(torch.isfinite(r2).all())
    monkeypatch.setattr(hb, "SAVE_TOTAL_BYTES", 0)
    with pytest.raises(RuntimeError, match="SAVE_TOTAL_BYTES"):
        npa.render_rays(rays, nc, None, occupancy=grid, **kw)


def test_three_identical_steps_do_not_leak(npa, dev, nets, datapath_fp16x3):
    """same rays, same randoms, so the same M: torch.cuda.memory_allocated() after step 3 equals that after step 2 -- with a backward
    (the leases go back to the pool) and with graphs dropped without one (the leases die with the graph)"""
    nc, nf, _, _ = nets
    rays, rnd, target = _small_scene(dev, 512)
    grid = ball_dgrid(npa, dev)
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, randoms=rnd, occupancy=grid)
    for backward in (True, False):
        npa.hip_backend.WORKSPACE.clear()       # (idle leases of earlier tests would be taken and die with the dropped graphs)
        mem = []
        for _ in range(3):
            r = rays.clone().requires_grad_(True)
            loss = loss_of(npa, npa.render_rays(r, nc, None, **kw), target)
            if backward:
                loss.backward()
            del loss, r
            zero_grads(nc, nf)
            nc.last_flat_grad = nf.last_flat_grad = None
            torch.cuda.synchronize()
            mem.append(torch.cuda.memory_allocated())
        print(f"\nbackward={backward}: allocated after each step {mem}")
        assert mem[2] == mem[1], (backward, mem)


# ------------------------------------------------------------------------------------------------ 8. guards
def test_guards(npa, dev, nets):
    nc, nf, _, _ = nets
    rays = orc.synthetic_rays(64, seed=3).to(dev)
    kw = dict(N_samples=16, N_importance=16, network_fine=nf)
    plain = npa.OccupancyGrid.from_mask(ball_mask(), BOX_LO, BOX_HI, device=dev)
    with pytest.raises(NotImplementedError, match="gradient") as e:
        npa.render_rays(rays, nc, None, occupancy=plain, **kw)
    assert "DensityGrid" in str(e.value)
    with pytest.raises(NotImplementedError, match="gradient"):      # rays that require grad, frozen or not
        with torch.enable_grad():
            npa.render_rays(rays.clone().requires_grad_(True), nc, None, occupancy=plain, **kw)
    grid = ball_dgrid(npa, dev)
    with pytest.raises(NotImplementedError, match="network_query_fn"):
        npa.render_rays(rays, nc, lambda p, v, m: npa.run_network(p, v, m, None, None), occupancy=grid, **kw)
    arch = orc.arch_of(D=4, W=64, multires=-1, multires_views=-1, output_ch=4)
    ctor = ("D", "W", "input_ch", "input_ch_views", "output_ch", "skips", "use_viewdirs")
    dense = npa.NeRF(**{k: arch[k] for k in ctor}).to(dev)
    with pytest.raises(NotImplementedError, match="DenseNeRF"):
        npa.render_rays(rays, dense, None, N_samples=16, occupancy=grid)
    with pytest.raises(NotImplementedError):
        grid.update(dense)
    with pytest.raises(npa.hip_backend.NerfHipError, match="GPU"):
        npa.render_rays(rays, nc, None, occupancy=ball_dgrid(npa, torch.device("cpu")), **kw)
    # a DensityGrid under no_grad is the plain grid's render
    with torch.no_grad():
        a = npa.render_rays(rays, nc, None, occupancy=grid, **kw)
        b = npa.render_rays(rays, nc, None, occupancy=plain, **kw)
    assert all(bits_equal(a[k], b[k]) for k in a)
    # fp16_fp8c with a gradient falls to fp16x3, as everywhere
    prev = npa.get_precision()
    try:
        npa.set_precision("fp16_fp8c")
        x = npa.render_rays(rays, nc, None, occupancy=grid, **kw)
        npa.set_precision("fp16x3")
        y = npa.render_rays(rays, nc, None, occupancy=grid, **kw)
    finally:
        npa.set_precision(prev)
    assert x["rgb_map"].grad_fn is not None and all(bits_equal(x[k], y[k]) for k in x)
