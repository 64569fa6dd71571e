"""GPU tests (-m gpu) of occupancy-grid empty-space skipping: the classifier / compaction kernels against OccupancyGrid.occupied,
render_rays(occupancy=grid) bit for bit against the masking network_query_fn hook, against the masked oracle, the all-occupied and
all-empty grids, OccupancyGrid.from_network, and the guards."""
import numpy as np
import pytest
import torch

import nerf_oracle as orc
from test_gpu_parity import BOUNDARY_DATAPATHS, BOUNDARY_TOL, datapath, dev, maxdiff, nets, npa  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

# the scene of the render tests: scene_params' networks seen by synthetic_rays (origins near (0, 0, 4) looking at the origin, depths
# 2..6), a 32^3 grid over [-2, 2]^3 whose occupied cells are those with their centre inside a ball of radius BALL_R around the origin
BOX_LO, BOX_HI, BOX_R, BALL_R = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), 32, 1.0
N_RAYS, RAY_SEED, RND_SEED = 1024, 12, 5
_QUERY_FIELD = orc.query_field


def ball_mask(R=BOX_R, radius=BALL_R, lo=BOX_LO[0], hi=BOX_HI[0]):
    c = lo + (torch.arange(R, dtype=torch.float64) + 0.5) * (hi - lo) / R
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    return (x * x + y * y + z * z) <= radius * radius


def ball_grid(npa, device, outside="evaluate"):
    return npa.OccupancyGrid.from_mask(ball_mask(), BOX_LO, BOX_HI, outside=outside, device=device)


def bits_equal(a, b):
    """bit-for-bit equality of two fp32 tensors (NaNs -- disp of an empty ray is 0 / 0 as in the reference -- included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def masking_hook(npa, grid, seen=None):
    """the yardstick: a user network_query_fn that zeroes the rows of the samples the grid skips"""
    def hook(pts, viewdirs, net):
        occ = grid.occupied(pts)
        if seen is not None:
            seen.append((int(occ.sum()), occ.numel()))
        raw = npa.run_network(pts, viewdirs, net, None, None)
        return torch.where(occ[..., None], raw, torch.zeros_like(raw))
    return hook


def near_face_rays(grid, rays64, z_lists, eps=1e-4):
    """Rays with a sample point, in float64, within eps cell widths of a face between an occupied and an unoccupied cell (the box's own
    faces included: outside counts as occupied or not by the grid's mode): probes t +- eps on each axis and compares the classification
    with the point's own."""
    mask = grid.to_mask().cpu()
    R = torch.tensor(grid.resolution, dtype=torch.float64)
    lo, hi = torch.tensor(grid.lo.astype(np.float64)), torch.tensor(grid.hi.astype(np.float64))

    def occ(t):
        inside = ((t >= 0) & (t < R)).all(-1)
        i = torch.where(inside[..., None], t, torch.zeros_like(t)).floor().long()
        return torch.where(inside, mask[i[..., 0], i[..., 1], i[..., 2]], torch.full_like(inside, grid.outside == "evaluate"))
    bad = torch.zeros(rays64.shape[0], dtype=torch.bool)
    for z in z_lists:
        pts = rays64[:, None, 0:3] + rays64[:, None, 3:6] * z.double()[..., None]
        t = (pts - lo) * (R / (hi - lo))
        own = occ(t)
        for axis in range(3):
            for sign in (-eps, eps):
                d = torch.zeros(3, dtype=torch.float64)
                d[axis] = sign
                bad |= (occ(t + d) != own).any(-1)
    return bad


# ------------------------------------------------------------------------------------------------ 1. classifier / compaction
@pytest.mark.parametrize("outside", ["evaluate", "skip"])
def test_compact_agrees_with_occupied_on_200k_points(npa, dev, outside):
    """nerf_occ_compact on 1000 rays x 200 samples: random points, points snapped onto cell faces (d = 0: the point IS the origin),
    points outside the box, NaNs -- the classification equals grid.occupied(o + d z) exactly, slot is the stable enumeration,
    records[:, 0:3] == pts[mask], records[:, 8:11] the owning ray's view direction, columns 3:8 zero, M == mask.sum()."""
    hb = npa.hip_backend
    g = torch.Generator().manual_seed(11)
    res = (37, 21, 64)
    mask = torch.rand(res, generator=g) < 0.35
    lo, hi = (-1.25, 0.5, -3.0), (1.75, 2.0, 0.2)
    grid = npa.OccupancyGrid.from_mask(mask, lo, hi, outside=outside, device=dev)
    n, S = 1000, 200
    lo_t, hi_t = torch.tensor(lo), torch.tensor(hi)
    o = lo_t + (hi_t - lo_t) * (torch.rand(n, 3, generator=g) * 1.2 - 0.1)
    d = torch.randn(n, 3, generator=g) * 0.3
    z = torch.rand(n, S, generator=g) * 2.0
    # rays 300..599: every sample ON a cell face (per axis lo + k * width in fp32, k = 0..R: the box's own faces included), d = 0
    width = (hi_t - lo_t) / torch.tensor(res, dtype=torch.float32)
    k = torch.stack([torch.randint(0, r + 1, (300,), generator=g) for r in res], -1).float()
    o[300:600] = lo_t + k * width
    o[300:320] = lo_t                    # exactly lo
    o[320:340] = hi_t                    # exactly hi
    d[300:600] = 0.0
    # rays 600..799: far outside; 800..819: NaN / inf components
    o[600:800] = hi_t + 1.0 + torch.rand(200, 3, generator=g)
    o[800:810, 0] = float("nan")
    d[810:820, 2] = float("inf")
    vd = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    rays = torch.cat([o, d, torch.zeros(n, 2), vd], -1).to(dev).contiguous()
    z = z.to(dev).contiguous()
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]
    want = grid.occupied(pts).reshape(-1)
    assert torch.equal(want.cpu(), grid.occupied(pts.cpu()).reshape(-1)), "occupied() itself must not depend on the device"
    slot, records, count = hb.occ_compact(grid._desc(), rays, z)
    torch.cuda.synchronize()
    m = int(count.item())
    assert m == int(want.sum()) and 0 < m < n * S
    assert torch.equal(slot >= 0, want)
    enum = (torch.cumsum(want.to(torch.int64), 0) - 1).to(torch.int32)
    assert torch.equal(slot[want], enum[want]) and bool((slot[~want] == -1).all())
    recs = records[:m]
    assert bits_equal(recs[:, 0:3], pts.reshape(-1, 3)[want])
    assert bool((recs[:, 3:8] == 0).all())
    owner = torch.arange(n, device=dev).repeat_interleave(S)[want]
    assert bits_equal(recs[:, 8:11], rays[owner, 8:11])
    # deterministic: a second call gives the same list
    slot2, records2, count2 = hb.occ_compact(grid._desc(), rays, z)
    assert torch.equal(slot, slot2) and bits_equal(records[:m], records2[:m]) and int(count2.item()) == m
    # expand: rows by slot, exact zeros elsewhere
    raw_c = torch.randn(m, 4, device=dev)
    raw = hb.occ_expand(slot, raw_c, torch.full((n, S, 4), 7.0, device=dev))
    ref = torch.zeros(n * S, 4, device=dev)
    ref[want] = raw_c
    assert bits_equal(raw.reshape(-1, 4), ref)


def test_compact_sizes_that_do_not_fill_a_block(npa, dev):
    """point counts around the 1024-point blocks and the 64-lane waves, an all-empty and an all-full grid"""
    hb = npa.hip_backend
    g = torch.Generator().manual_seed(5)
    for n, S in ((1, 1), (1, 63), (3, 65), (16, 64), (5, 205), (1025, 1), (33, 1000), (6000, 200)):     # (the last: more blocks than one piece of the scan)
        for frac in (0.0, 0.5, 1.0):
            mask = torch.rand(8, 8, 8, generator=g) < frac
            grid = npa.OccupancyGrid.from_mask(mask, (-1, -1, -1), (1, 1, 1), outside="skip", device=dev)
            rays = torch.cat([torch.rand(n, 3, generator=g) * 2.4 - 1.2, torch.randn(n, 3, generator=g) * 0.1, torch.zeros(n, 2),
                              torch.randn(n, 3, generator=g)], -1).to(dev)
            z = torch.rand(n, S, generator=g).to(dev)
            want = grid.occupied(rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).reshape(-1)
            slot, records, count = hb.occ_compact(grid._desc(), rays, z)
            assert int(count.item()) == int(want.sum()), (n, S, frac)
            assert torch.equal(slot, torch.where(want, torch.cumsum(want.to(torch.int64), 0) - 1, -torch.ones_like(want, dtype=torch.int64)).to(torch.int32))


# ------------------------------------------------------------------------------------------------ 2. exactness
def _scene(dev):
    rays = orc.synthetic_rays(N_RAYS, seed=RAY_SEED).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(N_RAYS, 64, 128, seed=RND_SEED).items()}
    return rays, rnd


@pytest.mark.parametrize("datapath", BOUNDARY_DATAPATHS, indirect=True)
@pytest.mark.parametrize("perturb,noise,white", [(0.0, 0.0, False), (1.0, 1.0, True), (1.0, 0.0, True), (0.0, 1.0, False)])
def test_grid_render_equals_the_masking_hook_bit_for_bit(npa, dev, nets, datapath, perturb, noise, white):
    """render_rays(occupancy=grid) == render_rays with the masking network_query_fn, every returned tensor bit for bit (1024 rays,
    64 + 128 samples, retraw), and last_stats == the masks' sums."""
    nc, nf, _, _ = nets
    rays, rnd = _scene(dev)
    grid = ball_grid(npa, dev)
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=white, perturb=perturb, raw_noise_std=noise, retraw=True, randoms=rnd)
    seen = []
    with torch.no_grad():
        want = npa.render_rays(rays, nc, masking_hook(npa, grid, seen), **kw)
        got = npa.render_rays(rays, nc, None, occupancy=grid, **kw)
    assert list(got) == list(want) and set(got) == {"rgb_map", "disp_map", "acc_map", "raw", "rgb0", "disp0", "acc0", "z_std"}
    for k in want:
        assert bits_equal(got[k], want[k]), (k, maxdiff(got[k], want[k]))
    assert [s[1] for s in seen] == [N_RAYS * 64, N_RAYS * 192]
    assert grid.last_stats == {"evaluated": seen[0][0] + seen[1][0], "total": N_RAYS * 256}
    assert 0 < grid.last_stats["evaluated"] < grid.last_stats["total"]
    assert float(got["acc_map"].max()) > 0.5      # (the masked scene is not empty)
    # coarse only, coarse network for both passes
    with torch.no_grad():
        for extra in (dict(N_importance=0), dict(network_fine=None)):
            kw2 = dict(kw, **extra)
            want = npa.render_rays(rays, nc, masking_hook(npa, grid), **kw2)
            got = npa.render_rays(rays, nc, None, occupancy=grid, **kw2)
            assert list(got) == list(want)
            for k in want:
                assert bits_equal(got[k], want[k]), (extra, k)


@pytest.mark.parametrize("datapath", BOUNDARY_DATAPATHS, indirect=True)
def test_grid_render_through_render_with_chunks_and_a_ragged_tail(npa, dev, nets, datapath):
    """render(c2w=..., chunk=150) of a 20 x 20 frame (chunks of 150, 150, 100 rays) with render_kwargs["occupancy"] = grid: equal to the
    masking hook through the same call, last_stats summed over the chunks"""
    nc, nf, _, _ = nets
    H, W, focal = 20, 20, 25.0
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    c2w = torch.tensor([[1.0, 0, 0, 0.1], [0, 0.8, -0.6, 0.2], [0, 0.6, 0.8, 4.0]]).to(dev)
    grid = ball_grid(npa, dev)
    kw = dict(network_fn=nc, N_samples=64, N_importance=128, network_fine=nf, perturb=0., white_bkgd=True, raw_noise_std=0., retraw=True)
    geo = dict(chunk=150, c2w=c2w, ndc=False, near=2., far=6., use_viewdirs=True)
    seen = []
    with torch.no_grad():
        want = npa.render(H, W, K, network_query_fn=masking_hook(npa, grid, seen), **geo, **kw)
        got = npa.render(H, W, K, network_query_fn=None, occupancy=grid, **geo, **kw)
        one = npa.render(H, W, K, network_query_fn=None, occupancy=grid, **dict(geo, chunk=1 << 20), **kw)
    assert len(seen) == 6
    assert grid.last_stats["total"] == 400 * 256
    for a, b in zip(got[:3], want[:3]):
        assert bits_equal(a, b)
    assert set(got[3]) == set(want[3]) and got[0].shape == (H, W, 3) and got[3]["raw"].shape == (H, W, 192, 4)
    for k in want[3]:
        assert bits_equal(got[3][k], want[3][k]), k
    assert bits_equal(one[0], got[0])
    with torch.no_grad():
        npa.render(H, W, K, network_query_fn=None, occupancy=grid, **geo, **kw)
    assert grid.last_stats == {"evaluated": sum(s[0] for s in seen), "total": 400 * 256}
    # render_path: the grid in render_kwargs is all it takes
    rkw = dict(kw, network_query_fn=None, ndc=False, near=2., far=6., use_viewdirs=True, occupancy=grid)
    rkw.pop("retraw")
    poses = torch.stack([c2w, c2w + torch.tensor([[0, 0, 0, 0.05], [0, 0, 0, 0.0], [0, 0, 0, 0.0]], device=dev)])
    with torch.no_grad():
        rgbs, disps = npa.render_path(poses, (H, W, focal), K, 150, rkw)
    assert rgbs.shape == (2, H, W, 3) and np.array_equal(rgbs[0], got[0].cpu().numpy())
    assert np.array_equal(np.isnan(disps[0]), np.isnan(got[1].cpu().numpy())) and not np.array_equal(rgbs[0], rgbs[1])
    assert grid.last_stats["total"] == 400 * 256


# ------------------------------------------------------------------------------------------------ 3. against the reference semantics
CDF_ROUNDING = 62 * 2.0 ** -24      # worst-case rounding of the 62-term fp32 cumulative sum behind sample_pdf's cdf (values <= 1)


def cdf_sensitive_rays(grid, rays64, z0, w0, n_fine=128, delta=CDF_ROUNDING):
    """Rays on which, in the float64 oracle, the classification of a fine sample changes when sample_pdf's u (equivalently its cdf) is
    moved by +-delta: the fine depth is drawn in a bin the masked coarse pass left empty, where inverse_cdf divides by its 1e-5 guard
    (run_nerf_helpers.py:234-236) and a rounding of the cdf moves the depth by whole cells across an occupied / unoccupied face."""
    zmid = 0.5 * (z0[..., 1:] + z0[..., :-1])
    u0 = torch.linspace(0.0, 1.0, n_fine, dtype=torch.float64).expand(z0.shape[0], n_fine)

    def classify(u):
        z, _ = torch.sort(torch.cat([z0, orc.inverse_cdf(zmid, w0[..., 1:-1], n_fine, u.contiguous())], -1), -1)
        return grid.occupied((rays64[:, None, 0:3] + rays64[:, None, 3:6] * z[..., None]).float())
    base = classify(u0)
    bad = torch.zeros(z0.shape[0], dtype=torch.bool)
    for shift in (-delta, delta):
        bad |= (classify((u0 + shift).clamp(0.0, 1.0)) != base).any(-1)
    return bad


# maps whose bound is the no-grid yardstick instead of the bare tolerance (see the test's docstring): every other map holds BOUNDARY_TOL
YARDSTICK_MAPS = {"fp32": ("disp0", "disp_map", "acc_map"), "fp16x3": ("disp_map",)}


@pytest.mark.parametrize("datapath", BOUNDARY_DATAPATHS, indirect=True)
def test_grid_render_against_the_masked_oracle(npa, dev, nets, datapath, monkeypatch):
    """The same scene and mask against nerf_oracle.trace_rays with query_field zeroed where grid.occupied is false, worst component per
    ray, all six maps: rgb0 / disp0 / acc0 within BOUNDARY_TOL[datapath]["coarse"], rgb_map / disp_map / acc_map within ["fine"] -- the
    bare tolerances.  Only the maps in YARDSTICK_MAPS, which miss the bare tolerance, are held to the yardstick instead: the error of
    the NO-GRID render of the same kept rays against the UNMASKED oracle, measured in this test (bound = max(tolerance, yardstick)).
    Masking replaces values by exact zeros and must not make a map worse than that.  On those maps the oracle's own fp32 run misses
    or all but misses the bare tolerance against float64 (fp32-vs-float64: disp0 6.2e-6, disp_map 3.2e-5, acc_map 2.5e-5 against 1e-5),
    so no fp32 pipeline can be asked for it.

    Rays left out, both criteria computed on the CPU from the float64 oracle alone, together capped at 2 %:
      (a) a sample point (coarse or fine) within 1e-4 cell widths of a face between an occupied and an unoccupied cell, where an ulp of
          z flips the classification: 3 of 1024 rays for this mask (ball of radius 1 in a 32^3 grid over [-2, 2]^3) and these seeds;
      (b) cdf_sensitive_rays: a fine sample whose classification changes when sample_pdf's cdf moves by its own worst-case fp32
          rounding (62 terms x 2^-24 = 3.7e-6).  Such a depth sits in a bin the masked coarse pass left exactly empty; inverse_cdf
          divides by its 1e-5 guard there.  Ray 289 is the case that showed it: in the float64 oracle a cdf shift of ONE fp32 ulp moves
          one of its depths by 7e-4 and a shift of 3.7e-6 by 0.022 (a sixth of a cell); the device's sample_pdf (unchanged by the grid)
          puts that one sample on the other side of a face than torch's cumsum does -- one flipped sample of 192, 1.0e-4 in rgb_map on
          both datapaths, while no sample of the ray is within 1e-2 cell widths of a face.  9 of 1024 rays; (a) or (b): 11 = 1.07 %.

    MEASURED on an MI355X, worst kept ray, grid render vs masked oracle | yardstick (no grid vs unmasked oracle, kept rays); * = held to
    the yardstick, every other map to the bare tolerance (fp32 1e-5, fp16x3 3e-5):
      fp32    rgb0 1.5e-6 | 2.1e-6    disp0* 1.4e-5 | 2.3e-5    acc0 3.0e-6 | 3.7e-6
              rgb_map 6.2e-6 | 2.2e-5    disp_map* 2.6e-5 | 2.0e-3    acc_map* 1.1e-5 | 3.5e-5
      fp16x3  rgb0 5.3e-6 | 4.8e-6    disp0 8.7e-6 | 8.0e-5    acc0 1.0e-5 | 8.0e-6
              rgb_map 1.2e-5 | 5.8e-5    disp_map* 1.5e-4 | 1.0e-3    acc_map 1.8e-5 | 9.0e-5
    (disp = 1 / depth of mostly-empty rays: the unmasked scene's worst ray is far worse than any masked one.)"""
    nc, nf, Pc, Pf = nets
    tol = BOUNDARY_TOL[datapath]
    rays, rnd = _scene(dev)
    grid = ball_grid(npa, dev)
    cpu_grid = ball_grid(npa, torch.device("cpu"))
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=0.0, raw_noise_std=0.0)
    with torch.no_grad():
        got = npa.render_rays(rays, nc, None, occupancy=grid, **kw)
        dense = npa.render_rays(rays, nc, None, **kw)

    def masked(P, pts, viewdirs, *a, **k):
        raw = _QUERY_FIELD(P, pts, viewdirs, *a, **k)
        return torch.where(cpu_grid.occupied(pts)[..., None], raw, torch.zeros_like(raw))
    plain_ref = orc.trace_rays(rays.cpu(), Pc, Pf, 64, 128, perturb=0., white_bkgd=True)
    monkeypatch.setattr(orc, "query_field", masked)
    ref = orc.trace_rays(rays.cpu(), Pc, Pf, 64, 128, perturb=0., white_bkgd=True)
    d64 = lambda P: {k: v.double() for k, v in P.items()}
    rays64 = rays.cpu().double()
    ref64 = orc.trace_rays(rays64, d64(Pc), d64(Pf), 64, 128, perturb=0., white_bkgd=True)
    near = near_face_rays(cpu_grid, rays64, [ref64["_z_vals0"], ref64["_z_vals"]])
    sens = cdf_sensitive_rays(cpu_grid, rays64, ref64["_z_vals0"], ref64["_weights0"])
    left_out = near | sens
    share = float(left_out.float().mean())
    print(f"\n[{datapath}] rays left out: near a face {int(near.sum())}, cdf-sensitive {int(sens.sum())} (ray 289: {bool(sens[289])}), "
          f"together {int(left_out.sum())} of {N_RAYS} = {100 * share:.2f} %")
    keep = ~left_out
    fig = {}
    for k, cls in (("rgb0", "coarse"), ("disp0", "coarse"), ("acc0", "coarse"), ("rgb_map", "fine"), ("disp_map", "fine"), ("acc_map", "fine")):
        yard = maxdiff(dense[k][keep.to(dev)], plain_ref[k][keep])
        bound = max(tol[cls], yard) if k in YARDSTICK_MAPS[datapath] else tol[cls]
        fig[k] = (maxdiff(got[k][keep.to(dev)], ref[k][keep]), yard, bound)
        print(f"[{datapath}] {k:9s} grid vs masked oracle {fig[k][0]:.3e}   no grid vs plain oracle (yardstick, kept rays) {yard:.3e}   "
              f"bare {tol[cls]:.1e}   bound {bound:.3e}")
    assert share <= 0.02
    assert bool(sens[289]) and not bool(near[289])
    for k, (err, _, bound) in fig.items():
        assert err <= bound, (k, fig)


# ------------------------------------------------------------------------------------------------ 4. all-occupied / all-empty
@pytest.mark.parametrize("datapath", BOUNDARY_DATAPATHS, indirect=True)
def test_all_occupied_grid_matches_render_without_a_grid(npa, dev, nets, datapath):
    """an all-occupied grid evaluates every point: the outputs match render_rays without a grid within the 1e-6 (relative) that
    test_user_network_query_fn_is_called_for_every_pass holds between the hooked and the fused path; an all-empty grid with
    outside="skip" gives the background and launches no field kernel"""
    nc, nf, _, _ = nets
    rays, rnd = _scene(dev)
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd)
    full = npa.OccupancyGrid(BOX_LO, BOX_HI, BOX_R, device=dev)
    assert full.fraction_occupied() == 1.0
    with torch.no_grad():
        plain = npa.render_rays(rays, nc, None, **kw)
        got = npa.render_rays(rays, nc, None, occupancy=full, **kw)
    assert full.last_stats == {"evaluated": N_RAYS * 256, "total": N_RAYS * 256}
    assert set(got) == set(plain)
    for k in plain:
        assert maxdiff(got[k], plain[k]) <= 1e-6 * max(1.0, float(plain[k].abs().nan_to_num().max())), k
    # (without density noise from here on: the reference adds its noise to ANY sigma, a skipped sample's zero included)
    kw = dict(kw, raw_noise_std=0.0)
    empty = npa.OccupancyGrid.from_mask(torch.zeros(2, 2, 2, dtype=torch.bool), BOX_LO, BOX_HI, outside="skip", device=dev)
    timer, npa.hip_backend.TIMER = npa.hip_backend.TIMER, npa.hip_backend.KernelTimer()
    try:
        with torch.no_grad():
            out = npa.render_rays(rays, nc, None, occupancy=empty, **kw)
        launched = set(npa.hip_backend.TIMER.summary())
    finally:
        npa.hip_backend.TIMER = timer
    assert empty.last_stats == {"evaluated": 0, "total": N_RAYS * 256}
    assert not any(name.startswith("field_fwd") for name in launched), launched
    assert bool((out["acc_map"] == 0).all()) and bool((out["rgb_map"] == 1).all()) and bool((out["raw"] == 0).all()) and bool((out["rgb0"] == 1).all())
    # outside="evaluate" on the same empty grid: only what the box does not cover is evaluated
    part = npa.OccupancyGrid.from_mask(torch.zeros(2, 2, 2, dtype=torch.bool), BOX_LO, BOX_HI, device=dev)
    with torch.no_grad():
        npa.render_rays(rays, nc, None, occupancy=part, **kw)
    assert 0 < part.last_stats["evaluated"] < part.last_stats["total"]


# ------------------------------------------------------------------------------------------------ 5. from_network
@pytest.mark.parametrize("datapath", BOUNDARY_DATAPATHS, indirect=True)
def test_from_network_marks_dense_cells_and_their_neighbours(npa, dev, nets, datapath, monkeypatch):
    """resolution 64 on the scene_params scene: every cell whose centre density from query_points exceeds the threshold is set, with
    its 26 neighbours (one round of dilation), and no other cell; a threshold below every density gives the full grid"""
    nc, nf, _, _ = nets
    R = 64
    def centres_of(res):        # lo + (i + 0.5) * width, computed here (not by the method from_network uses)
        ax = [BOX_LO[a] + (torch.arange(res[a], dtype=torch.float64) + 0.5) * ((BOX_HI[a] - BOX_LO[a]) / res[a]) for a in range(3)]
        return torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3).float().to(dev)
    centres = centres_of((R, R, R))
    with torch.no_grad():
        sigma = npa.query_points(nf, centres, torch.tensor([0.0, 0.0, 1.0], device=dev).expand(R ** 3, 3))[:, 3]
    thr = float(sigma.median())
    core = (sigma > thr).view(R, R, R)
    assert 0.2 < float(core.float().mean()) < 0.8
    dil = lambda m: torch.nn.functional.max_pool3d(m[None, None].float(), 3, 1, 1)[0, 0] > 0
    g0 = npa.OccupancyGrid.from_network(nf, BOX_LO, BOX_HI, R, sigma_threshold=thr, dilate=0)
    assert g0.device == centres.device and torch.equal(g0.to_mask(), core)
    g1 = npa.OccupancyGrid.from_network(nf, BOX_LO, BOX_HI, R, sigma_threshold=thr)
    assert torch.equal(g1.to_mask(), dil(core))
    g2 = npa.OccupancyGrid.from_network(nf, BOX_LO, BOX_HI, R, sigma_threshold=thr, dilate=2)
    assert torch.equal(g2.to_mask(), dil(dil(core)))
    # slices that end inside the grid (word-aligned), a non-cubic grid whose cell count is no multiple of 32
    monkeypatch.setattr(npa.occupancy, "_SLICE_CELLS", 1 << 12)
    assert torch.equal(npa.OccupancyGrid.from_network(nf, BOX_LO, BOX_HI, R, sigma_threshold=thr, dilate=0).bits, g0.bits)
    res = (9, 11, 13)
    odd = npa.OccupancyGrid(BOX_LO, BOX_HI, res, device=dev)
    with torch.no_grad():
        s_odd = npa.query_points(nf, centres_of(res), torch.tensor([0.0, 0.0, 1.0], device=dev).expand(odd.n_cells, 3))[:, 3]
    core_odd = (s_odd > thr).view(res)
    assert torch.equal(npa.OccupancyGrid.from_network(nf, BOX_LO, BOX_HI, res, sigma_threshold=thr, dilate=0).to_mask(), core_odd)
    assert torch.equal(npa.OccupancyGrid.from_network(nf, BOX_LO, BOX_HI, res, sigma_threshold=thr, dilate=1).to_mask(), dil(core_odd))
    # more samples per cell only add cells; a threshold below every density: the full grid
    g4 = npa.OccupancyGrid.from_network(nf, BOX_LO, BOX_HI, res, sigma_threshold=thr, samples_per_cell=4, dilate=0,
                                        generator=torch.Generator().manual_seed(1))
    assert bool((g4.to_mask() | ~core_odd).all()) and int(g4.to_mask().sum()) > int(core_odd.sum())
    assert npa.OccupancyGrid.from_network(nf, BOX_LO, BOX_HI, R, sigma_threshold=float(sigma.min()) - 1.0).fraction_occupied() == 1.0
    assert npa.OccupancyGrid.from_network(nf, BOX_LO, BOX_HI, R, sigma_threshold=float(sigma.max()) + 1.0, dilate=3).fraction_occupied() == 0.0


# ------------------------------------------------------------------------------------------------ 6. guards
def test_unsupported_combinations_raise_and_none_changes_nothing(npa, dev, nets):
    nc, nf, _, _ = nets
    rays = orc.synthetic_rays(64, seed=3).to(dev)
    grid = ball_grid(npa, dev)
    kw = dict(N_samples=16, N_importance=16, network_fine=nf)
    with pytest.raises(NotImplementedError, match="gradient"):      # grad mode on, parameters require grad
        npa.render_rays(rays, nc, None, occupancy=grid, **kw)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="network_query_fn"):
            npa.render_rays(rays, nc, lambda p, v, m: npa.run_network(p, v, m, None, None), occupancy=grid, **kw)
        arch = orc.arch_of(D=4, W=64, multires=-1, multires_views=-1, output_ch=4)
        ctor = ("D", "W", "input_ch", "input_ch_views", "output_ch", "skips", "use_viewdirs")
        dense = npa.NeRF(**{k: arch[k] for k in ctor}).to(dev)
        assert type(dense).__name__ == "DenseNeRF"
        with pytest.raises(NotImplementedError, match="DenseNeRF"):
            npa.render_rays(rays, dense, None, N_samples=16, occupancy=grid)
        with pytest.raises(NotImplementedError):
            npa.OccupancyGrid.from_network(dense, BOX_LO, BOX_HI, 8)
        with pytest.raises(npa.hip_backend.NerfHipError, match="GPU"):
            npa.render_rays(rays, nc, None, occupancy=ball_grid(npa, torch.device("cpu")), **kw)
        a = npa.render_rays(rays, nc, None, occupancy=grid, **kw)
        # occupancy=None is the call without the keyword
        b, c = npa.render_rays(rays, nc, None, occupancy=None, **kw), npa.render_rays(rays, nc, None, **kw)
    assert set(a) == set(b) and all(bits_equal(b[k], c[k]) for k in b)
    # an empty batch with a grid: nothing evaluated, and last_stats says so instead of keeping the previous call's figures
    with torch.no_grad():
        e0 = npa.render_rays(rays[:0], nc, None, occupancy=grid, **kw)
    assert e0["rgb_map"].shape == (0, 3) and grid.last_stats == {"evaluated": 0, "total": 0}
    for p in list(nc.parameters()) + list(nf.parameters()):      # frozen networks under grad mode need no gradient: the grid path runs
        p.requires_grad_(False)
    try:
        e = npa.render_rays(rays, nc, None, occupancy=grid, **kw)
    finally:
        for p in list(nc.parameters()) + list(nf.parameters()):
            p.requires_grad_(True)
    assert all(bits_equal(a[k], e[k]) for k in a)
