"""CPU: the occupied span of a ray -- OccupancyGrid.ray_span_reference (the float64 definition the kernel nerf_occ_ray_span is held to)
against a brute-force classification of 4096 depths per ray and on hand-made rays with hulls known in closed form, the export and the
binding of the entry point, the guard of render_rays(clip_to_occupancy=True) and the autograd contract of clip_rays.  The masks, the
hand-made rays and check_span() are shared with tests/test_gpu_ray_clip.py."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import nerf_oracle as orc
import nerf_pytorch_amd as npa

CPU = torch.device("cpu")
BOX_LO, BOX_HI = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)
N_RAYS, RAY_SEED = 1024, 12
NAN, INF = float("nan"), float("inf")
CLEAR = 2.0 ** -8           # a depth counts when its float64 grid coordinate is at least this far (in cells) from every face
PAD_CELLS = 2.0 ** -10      # the kernel's pad, in cells on the ray's fastest axis


def ball_mask(R=32, radius=1.0, centre=(0.0, 0.0, 0.0)):
    c = BOX_LO[0] + (torch.arange(R, dtype=torch.float64) + 0.5) * (BOX_HI[0] - BOX_LO[0]) / R
    x, y, z = torch.meshgrid(c - centre[0], c - centre[1], c - centre[2], indexing="ij")
    return (x * x + y * y + z * z) <= radius * radius


def two_balls_mask():
    return ball_mask(32, 0.5, (0.0, 0.0, 0.9)) | ball_mask(32, 0.5, (0.3, 0.0, -0.9))


def one_cell_mask(res=(32, 20, 48), cell=(5, 17, 40)):
    m = torch.zeros(res, dtype=torch.bool)
    m[cell] = True
    return m


MASKS = {"ball": ball_mask, "two_balls": two_balls_mask}


def make_grid(mask, outside, device=CPU):
    return npa.OccupancyGrid.from_mask(mask, BOX_LO, BOX_HI, outside=outside, device=device)


def records(rows):
    """[(o3, d3, near, far)] -> ray records [n, 11] (view direction = d normalised, (0, 0, 1) for d = 0)"""
    o = torch.tensor([r[0] for r in rows], dtype=torch.float32)
    d = torch.tensor([r[1] for r in rows], dtype=torch.float32)
    nf = torch.tensor([[r[2], r[3]] for r in rows], dtype=torch.float32)
    vd = torch.where(d.norm(dim=-1, keepdim=True) > 0, d / d.norm(dim=-1, keepdim=True), torch.tensor([0.0, 0.0, 1.0]))
    return torch.cat([o, d, nf, vd.nan_to_num()], -1)


def hand_rays():
    """64 hand-made rays for the boxes over [-2, 2]^3: axis-aligned through cell centres (both senses, all axes), origins inside the
    box, rays pointing away, zero components, near behind the box, near == far, near > far, NaN and infinite components"""
    rows = []
    for a in range(3):
        for s in (1.0, -1.0):
            for off in (0.03, -0.91, 0.4):      # (no cell plane of a 32 / 20 / 48 / 128 grid at these offsets)
                o, d = [off, off * 0.5 + 0.01, -off + 0.02], [0.0, 0.0, 0.0]
                o[a], d[a] = -3.0 * s, s
                rows.append((o, d, 0.0, 6.0))                       # 18 through the box
            o, d = [0.03, 0.04, 0.05], [0.0, 0.0, 0.0]
            o[a], d[a] = -3.0 * s, -s
            rows.append((o, d, 0.0, 6.0))                           # 6 pointing away
            o, d = [0.03, 0.04, 0.05], [0.0, 0.0, 0.0]
            o[a], d[a] = -3.0 * s, 1.7 * s
            rows.append((o, d, 3.2, 4.0))                           # 6 with near behind the box (it is left at t = 5 / 1.7)
    for o in ((0.03, 0.04, 0.05), (0.9, -0.02, 0.3), (-1.9, 1.9, 0.01), (0.31, 0.02, -0.88)):
        for d in ((0.3, -0.5, 0.8), (-0.6, 0.1, -0.2), (0.0, 0.7, 0.7), (0.5, 0.0, 0.0)):
            rows.append((o, d, 0.0, 5.0))                           # 16 with the origin inside the box
    rows += [((0.03, 0.04, 3.0), (0.0, 0.0, 0.0), 0.0, 6.0), ((0.03, 0.04, 0.05), (0.0, 0.0, 0.0), 0.0, 6.0)]       # d = 0
    rows += [((0.1, 0.2, 4.0), (0.01, 0.02, -1.0), 3.0, 3.0), ((0.03, 0.04, 0.05), (0.0, 0.0, 1.0), 1.0, 1.0),       # near == far
             ((0.1, 0.2, 4.0), (0.01, 0.02, -1.0), 6.0, 2.0)]                                                        # near > far
    rows += [((NAN, 0.0, 4.0), (0.0, 0.0, -1.0), 2.0, 6.0), ((0.0, 0.0, 4.0), (0.0, NAN, -1.0), 2.0, 6.0),
             ((0.0, 0.0, 4.0), (0.0, 0.0, -1.0), NAN, 6.0), ((0.0, 0.0, 4.0), (0.0, 0.0, -1.0), 2.0, NAN),
             ((0.0, INF, 4.0), (0.0, 0.0, -1.0), 2.0, 6.0), ((0.0, 0.0, 4.0), (0.0, 0.0, -INF), 2.0, 6.0),
             ((0.0, 0.0, 4.0), (0.0, 0.0, -1.0), 2.0, INF), ((0.0, 0.0, 4.0), (0.0, 0.0, -1.0), -INF, 6.0)]
    # through the one occupied cell (5, 17, 40) of the (32, 20, 48) grid, along each axis, and grazing the ball
    rows += [((-1.3125, 1.5, -3.0), (0.0, 0.0, 1.0), 0.0, 6.0), ((-1.3125, -3.0, 1.375), (0.0, 2.0, 0.0), 0.0, 6.0),
             ((-3.0, 1.5, 1.375), (0.5, 0.0, 0.0), 0.0, 12.0), ((0.98, 0.03, 4.0), (0.0, 0.0, -1.0), 2.0, 6.0),
             ((1.3, 0.03, 4.0), (0.0, 0.001, -1.0), 2.0, 6.0)]
    assert len(rows) == 64
    return records(rows)


def all_rays():
    return torch.cat([orc.synthetic_rays(N_RAYS, seed=RAY_SEED), hand_rays()], 0)


def pad_t(grid, rays):
    """2^-10 cell on the ray's fastest axis, as a depth (float64; inf for d = 0)"""
    gd = rays[:, 3:6].double() * torch.tensor(grid.scale.astype(np.float64))
    return PAD_CELLS / gd.abs().amax(-1)


def check_span(grid, rays, span, hit):
    """the kernel's contract for EVERY ray of `rays` (cpu tensors; `grid` on the cpu): between the two float64 hulls of
    ray_span_reference, inside the ray's own interval, and the row untouched on a miss.  Returns (rays hit, rays on which the two
    hulls differ)."""
    h, near_all, far_all, near_thick, far_thick = grid.ray_span_reference(rays)
    hit_all, hit_thick = h[:, 0], h[:, 1]
    near, far = rays[:, 6], rays[:, 7]
    assert span.dtype == torch.float32 and span.shape == (rays.shape[0], 2) and hit.dtype == torch.bool and hit.shape == rays.shape[:1]
    assert bool((hit | ~hit_thick).all()), f"missed rays with a thick hull: {torch.nonzero(hit_thick & ~hit).reshape(-1).tolist()}"
    assert bool((hit_all | ~hit).all()), f"hit without any occupied segment: {torch.nonzero(hit & ~hit_all).reshape(-1).tolist()}"
    pad = pad_t(grid, rays)
    n1, f1 = span[:, 0].double(), span[:, 1].double()
    # (where the thick hull does not exist the all-hull bounds from both sides)
    upper_near = torch.where(hit_thick, near_thick, far_all)
    lower_far = torch.where(hit_thick, far_thick, near_all)
    bad = hit & ~((near_all - 2 * pad <= n1) & (n1 <= upper_near) & (lower_far <= f1) & (f1 <= far_all + 2 * pad))
    assert not bool(bad.any()), [(i, span[i].tolist(), near_all[i].item(), near_thick[i].item(), far_thick[i].item(), far_all[i].item())
                                 for i in torch.nonzero(bad).reshape(-1).tolist()[:5]]
    inside = (near <= span[:, 0]) & (span[:, 0] < span[:, 1]) & (span[:, 1] <= far)
    assert bool((inside | ~hit).all()), torch.nonzero(hit & ~inside).reshape(-1).tolist()
    miss = ~hit
    assert torch.equal(span[miss].view(torch.int32), rays[miss, 6:8].contiguous().view(torch.int32)), "a miss must copy (near, far) bit for bit"
    return int(hit.sum()), int(((near_all != near_thick) | (far_all != far_thick) | (hit_all != hit_thick)).sum())


# ------------------------------------------------------------------------------------------------ 1. the definition against brute force
@pytest.mark.parametrize("outside", ["evaluate", "skip"])
@pytest.mark.parametrize("mask", sorted(MASKS))
def test_reference_hull_contains_every_occupied_depth(mask, outside):
    """4096 uniform depths per ray of synthetic_rays(1024, 12), classified by the fp32 occupied(): every occupied depth whose float64
    grid coordinate is at least 2^-8 cell from every cell plane lies in [near_thick, far_thick], and its ray has a thick hull.  (Such a
    depth sits in a segment that reaches 2^-8 cell to either side on every axis, or ends at near / far on one side: longer than 2^-9
    cell on the fastest axis.)  The depths left out for being near a plane are at most 3 % of all: 3 axes x 2 x 2^-8 = 2.3 %."""
    grid = make_grid(MASKS[mask](), outside)
    rays = orc.synthetic_rays(N_RAYS, seed=RAY_SEED)
    S = 4096
    u = (torch.arange(S, dtype=torch.float32) + 0.5) / S
    z = rays[:, 6:7] + (rays[:, 7:8] - rays[:, 6:7]) * u
    occ = grid.occupied(rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None])
    r64, z64 = rays.double(), z.double()
    g = (r64[:, None, 0:3] + r64[:, None, 3:6] * z64[..., None] - torch.tensor(grid.lo.astype(np.float64))) * torch.tensor(grid.scale.astype(np.float64))
    clear = ((g - torch.round(g)).abs() >= CLEAR).all(-1)
    h, near_all, far_all, near_thick, far_thick = grid.ray_span_reference(rays)
    counted = occ & clear
    in_hull = (z64 >= near_thick[:, None]) & (z64 <= far_thick[:, None]) & h[:, 1:2]
    violating = (counted & ~in_hull).any(-1)
    excluded = 1.0 - float(clear.double().mean())
    differ = ((near_all != near_thick) | (far_all != far_thick) | (h[:, 0] != h[:, 1])).double().mean()
    print(f"\n[{mask}, {outside}] rays with an occupied depth {int(occ.any(-1).sum())}, thick hulls {int(h[:, 1].sum())}, excluded depths "
          f"{100 * excluded:.2f} %, violating rays {int(violating.sum())}, all != thick on {100 * float(differ):.2f} % of rays")
    assert excluded <= 0.03
    assert int(violating.sum()) == 0
    assert bool((h[:, 0] | ~h[:, 1]).all()) and bool((near_all <= near_thick)[h[:, 1]].all()) and bool((far_all >= far_thick)[h[:, 1]].all())
    # the hull is no wider than the ray's interval; with the outside skipped some rays have none
    assert bool((near_all >= r64[:, 6]).all()) and bool((far_all <= r64[:, 7]).all())
    if outside == "skip":
        assert 0 < int(h[:, 1].sum()) < N_RAYS


# ------------------------------------------------------------------------------------------------ 2. hand-made cases
def _one_cell_grid(outside):
    """8^3 cells of width 0.5 over [-2, 2]^3, occupied: cell (4, 4, 4) = [0, 0.5]^3"""
    return make_grid(one_cell_mask((8, 8, 8), (4, 4, 4)), outside)


def _expect(grid, row, hit, near, far, tol=1e-6):
    rays = records([row])
    h, na, fa, nt, ft = grid.ray_span_reference(rays)
    assert h.tolist() == [[hit, hit]], (row, h)
    same = lambda got, want: got == want or abs(got - want) <= tol or (want != want and got != got)
    for got in (na, nt):
        assert got.dtype == torch.float64 and same(float(got), near), (row, float(got), near)
    for got in (fa, ft):
        assert same(float(got), far), (row, float(got), far)


def test_reference_on_hand_made_rays():
    skip, ev = _one_cell_grid("skip"), _one_cell_grid("evaluate")
    # axis-aligned through the single occupied cell: inside it for t in [3, 3.5]; the box is [1, 5], what lies outside counts in "evaluate"
    row = ((-3.0, 0.25, 0.25), (1.0, 0.0, 0.0), 0.0, 6.0)
    _expect(skip, row, True, 3.0, 3.5)
    _expect(ev, row, True, 0.0, 6.0)
    _expect(ev, ((-3.0, 0.25, 0.25), (1.0, 0.0, 0.0), 1.5, 4.5), True, 3.0, 3.5)      # [near, far] inside the box: the cell alone
    _expect(ev, ((-3.0, 0.25, 0.25), (1.0, 0.0, 0.0), 0.5, 4.5), True, 0.5, 3.5)      # a stretch in front of the box fixes near
    _expect(ev, ((-3.0, 0.25, 0.25), (1.0, 0.0, 0.0), 1.5, 5.5), True, 3.0, 5.5)      # a stretch behind it fixes far
    _expect(ev, ((-3.0, 0.75, 0.25), (1.0, 0.0, 0.0), 1.5, 5.5), True, 5.0, 5.5)      # past the cell: only the stretch behind the box
    _expect(skip, ((-3.0, 0.75, 0.25), (1.0, 0.0, 0.0), 0.0, 6.0), False, 0.0, 6.0)
    _expect(skip, ((3.5, 0.25, 0.25), (-2.0, 0.0, 0.0), 0.0, 6.0), True, 1.5, 1.75)   # the other sense, |d| = 2
    # the origin inside the occupied cell
    _expect(skip, ((0.25, 0.25, 0.25), (0.0, 0.0, 1.0), 0.0, 3.0), True, 0.0, 0.25)
    _expect(ev, ((0.25, 0.25, 0.25), (0.0, 0.0, 1.0), 0.0, 3.0), True, 0.0, 3.0)
    _expect(ev, ((0.25, 0.25, 0.25), (0.0, 0.0, 1.0), 0.0, 1.5), True, 0.0, 0.25)
    _expect(skip, ((0.25, 0.25, 0.25), (0.0, 0.0, 1.0), 0.125, 0.2), True, 0.125, 0.2)     # [near, far] inside the cell
    # pointing away from the box; near behind the box
    _expect(skip, ((-3.0, 0.25, 0.25), (-1.0, 0.0, 0.0), 0.0, 6.0), False, 0.0, 6.0)
    _expect(ev, ((-3.0, 0.25, 0.25), (-1.0, 0.0, 0.0), 0.0, 6.0), True, 0.0, 6.0)
    _expect(skip, ((-3.0, 0.25, 0.25), (1.0, 0.0, 0.0), 5.5, 7.0), False, 5.5, 7.0)
    _expect(ev, ((-3.0, 0.25, 0.25), (1.0, 0.0, 0.0), 5.5, 7.0), True, 5.5, 7.0)
    # a zero direction component, not axis-aligned: x = -1.1 + t in [0, 0.5] and y = -0.9 + t in [0, 0.5]: t in [1.1, 1.4]
    _expect(skip, ((-1.1, -0.9, 0.25), (1.0, 1.0, 0.0), 0.0, 6.0), True, 1.1, 1.4)
    _expect(skip, ((-1.1, -0.9, 0.75), (1.0, 1.0, 0.0), 0.0, 6.0), False, 0.0, 6.0)         # the same in the layer above: empty
    # d = 0: one segment, of length 0 in cells: an all-hull where the point is occupied, never a thick one
    h, na, fa, nt, ft = skip.ray_span_reference(records([((0.25, 0.25, 0.25), (0.0, 0.0, 0.0), 1.0, 2.0), ((0.75, 0.25, 0.25), (0.0, 0.0, 0.0), 1.0, 2.0)]))
    assert h.tolist() == [[True, False], [False, False]] and na.tolist() == [1.0, 1.0] and fa.tolist() == [2.0, 2.0]
    # NaN / infinite components, near == far, near > far: no hull, the pair is the ray's own
    for row in (((NAN, 0.25, 0.25), (1.0, 0.0, 0.0), 0.0, 6.0), ((-3.0, 0.25, 0.25), (1.0, NAN, 0.0), 0.0, 6.0),
                ((-3.0, 0.25, 0.25), (1.0, 0.0, 0.0), NAN, 6.0), ((-3.0, 0.25, 0.25), (1.0, 0.0, 0.0), 0.0, INF),
                ((-3.0, 0.25, 0.25), (1.0, 0.0, 0.0), 3.25, 3.25), ((-3.0, 0.25, 0.25), (1.0, 0.0, 0.0), 3.4, 3.1)):
        for g in (skip, ev):
            _expect(g, row, False, row[2], row[3])
    # more than 8 columns, any leading count, an empty batch
    assert skip.ray_span_reference(torch.zeros(0, 11))[0].shape == (0, 2)
    assert skip.ray_span_reference(records([row] * 3)[:, :8])[0].shape == (3, 2)


def test_reference_on_a_non_cubic_grid():
    """(32, 20, 48) cells over [-2, 2]^3, occupied: cell (5, 17, 40) = [-1.375, -1.25] x [1.4, 1.6] x [4/3, 17/12] - wrong index order
    or a wrong axis' resolution misses it"""
    g = make_grid(one_cell_mask(), "skip")
    _expect(g, ((-1.3125, 1.5, -3.0), (0.0, 0.0, 1.0), 0.0, 6.0), True, 3.0 + 4.0 / 3.0, 3.0 + 17.0 / 12.0)
    _expect(g, ((-1.3125, -3.0, 1.375), (0.0, 2.0, 0.0), 0.0, 6.0), True, 2.2, 2.3)
    _expect(g, ((-3.0, 1.5, 1.375), (0.5, 0.0, 0.0), 0.0, 12.0), True, 3.25, 3.5)
    _expect(g, ((1.5, -1.3125, 1.375), (0.0, 0.0, 1.0), -6.0, 6.0), False, -6.0, 6.0)       # (x and y swapped)
    # a diagonal through the cell's centre (-1.3125, 1.5, 1.375): the cell is left through its x faces first
    c = np.array([-1.3125, 1.5, 1.375])
    d = np.array([0.5, 0.5, 0.25])
    _expect(g, (tuple(c - 4 * d), tuple(d), 0.0, 8.0), True, 4.0 - 0.125, 4.0 + 0.125)


# ------------------------------------------------------------------------------------------------ 3. the shared checker checks
def test_check_span_accepts_the_hulls_and_refuses_what_is_outside_them():
    grid = make_grid(ball_mask(), "skip")
    rays = all_rays()
    h, near_all, far_all, near_thick, far_thick = grid.ray_span_reference(rays)
    def rows(hit, near, far):
        return torch.where(hit[:, None], torch.stack([near, far], -1).float(), rays[:, 6:8])
    pad = pad_t(grid, rays)
    # (half a pad outside the thick hull: the fp32 rounding of a float64 end must not decide)
    mid = rows(h[:, 1], torch.maximum(near_thick - 0.5 * pad, rays[:, 6].double()), torch.minimum(far_thick + 0.5 * pad, rays[:, 7].double()))
    n_hit, n_differ = check_span(grid, rays, mid, h[:, 1])
    assert 0 < n_hit < rays.shape[0] and n_differ <= 0.01 * rays.shape[0]
    wide = rows(h[:, 0], torch.maximum(near_all - pad, rays[:, 6].double()), torch.minimum(far_all + pad, rays[:, 7].double()))
    check_span(grid, rays, wide, h[:, 0])
    with pytest.raises(AssertionError):         # a span cut short by a cell
        check_span(grid, rays, rows(h[:, 1], near_thick + 0.13, far_thick), h[:, 1])
    with pytest.raises(AssertionError):         # the unclipped interval called a hit
        check_span(grid, rays, rays[:, 6:8].contiguous(), h[:, 1])
    with pytest.raises(AssertionError):         # everything a miss
        check_span(grid, rays, rays[:, 6:8].contiguous(), torch.zeros_like(h[:, 1]))


# ------------------------------------------------------------------------------------------------ 4. exports and binding
def test_the_library_exports_and_binds_the_entry_point():
    hb = npa.hip_backend
    assert hasattr(ctypes.CDLL(npa.build.LIB_PATH), "nerf_occ_ray_span") and "nerf_occ_ray_span" in hb.EXPORTS
    assert callable(hb.occ_ray_span)
    L = hb.lib()
    assert L.nerf_abi_version() == 10
    assert L.nerf_occ_ray_span.argtypes is not None and len(L.nerf_occ_ray_span.argtypes) == 7
    assert L.nerf_occ_ray_span(None, None, 8, 1, None, None, None) != 0
    assert "null" in L.nerf_last_error().decode()
    fake = ctypes.c_void_p(256)             # never dereferenced: every check below fails before a launch
    desc = hb.NerfOccGrid((ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(2, 2, 2), (ctypes.c_int * 3)(4, 4, 4), 1, fake)
    d = ctypes.byref(desc)
    assert L.nerf_occ_ray_span(d, None, 8, 1, fake, fake, None) != 0 and "null" in L.nerf_last_error().decode()
    assert L.nerf_occ_ray_span(d, fake, 8, 1, None, fake, None) != 0
    assert L.nerf_occ_ray_span(d, fake, 8, 1, fake, None, None) != 0
    assert L.nerf_occ_ray_span(d, fake, 8, -1, fake, fake, None) != 0 and "size" in L.nerf_last_error().decode()
    assert L.nerf_occ_ray_span(d, fake, 7, 1, fake, fake, None) != 0            # a record holds (o, d, near, far)
    bad = hb.NerfOccGrid((ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(2, 2, 2), (ctypes.c_int * 3)(4, 0, 4), 1, fake)
    assert L.nerf_occ_ray_span(ctypes.byref(bad), fake, 8, 1, fake, fake, None) != 0
    assert L.nerf_occ_ray_span(d, fake, 8, 0, fake, fake, None) == 0            # no rays: nothing launched
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_hip.h")) as f:
        assert "int nerf_occ_ray_span(const NerfOccGrid* grid, const float* rays, int ray_stride, int n_rays, float* span, int* hit, void* stream);" in f.read()
    for cls in (npa.OccupancyGrid, npa.DensityGrid):
        assert all(callable(getattr(cls, name)) for name in ("ray_span_reference", "ray_span", "clip_rays"))


# ------------------------------------------------------------------------------------------------ 5. guards and autograd
def test_clip_to_occupancy_is_keyword_only_and_needs_a_grid():
    sig = inspect.signature(npa.render_rays)
    p = sig.parameters["clip_to_occupancy"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    net = npa.NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    rays = orc.synthetic_rays(8, seed=1)
    with pytest.raises(ValueError, match="clip_to_occupancy"):
        npa.render_rays(rays, net, None, N_samples=8, clip_to_occupancy=True)
    with pytest.raises(ValueError, match="clip_to_occupancy"):
        npa.render_rays(rays, net, None, N_samples=8, occupancy=None, clip_to_occupancy=True)
    with pytest.raises(npa.hip_backend.NerfHipError, match="GPU"):       # a grid that is not on the GPU is refused as it is without clipping
        make_grid(ball_mask(), "skip").ray_span(rays)


def test_clip_rays_keeps_the_history_of_every_column_but_near_and_far(monkeypatch):
    grid = make_grid(ball_mask(), "skip")
    rays = orc.synthetic_rays(16, seed=2).requires_grad_(True)
    span = torch.stack([torch.linspace(2.5, 3.0, 16), torch.linspace(4.0, 5.0, 16)], -1)
    hit = torch.arange(16) % 3 != 0
    seen = []

    def fake_span(r):
        seen.append((r.requires_grad, torch.is_grad_enabled()))
        return span, hit
    monkeypatch.setattr(grid, "ray_span", fake_span)
    out, h = grid.clip_rays(rays)
    assert seen and torch.equal(h, hit) and out.shape == rays.shape and out.dtype == rays.dtype
    assert torch.equal(out[:, 6:8], span) and torch.equal(out[:, :6], rays[:, :6]) and torch.equal(out[:, 8:], rays[:, 8:])
    w = torch.randn(16, 11, generator=torch.Generator().manual_seed(4))
    (out * w).sum().backward()
    assert torch.equal(rays.grad[:, :6], w[:, :6]) and torch.equal(rays.grad[:, 8:], w[:, 8:])
    assert bool((rays.grad[:, 6:8] == 0).all())
