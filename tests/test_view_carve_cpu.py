"""CPU: occupancy grids from training cameras and silhouettes without a GPU -- the export of nerf_occ_view_carve and its argument
checks, what the two definitions (OccupancyGrid.view_counts_reference, carved_reference) promise on a ring of cameras around a sphere
(no sampled point in an unseen cell, no foreground ray through a carved cell, no cell of the sphere lost, a hull well below the box), their
edge cases, and DensityGrid.restrict on CPU tensors.  The cameras are built here by a look-at construction in the convention of get_rays:
the columns of c2w are right, up, back, position, and pixel (i, j) looks along ((i - cx) / fx, -(j - cy) / fy, -1)."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import nerf_pytorch_amd as npa

CPU = torch.device("cpu")
NAN = float("nan")

H = W = 48
FOCAL = 24.0 / math.tan(0.3455556)
K = torch.tensor([[FOCAL, 0.0, 24.0], [0.0, FOCAL, 24.0], [0.0, 0.0, 1.0]])
NEAR, FAR = 2.0, 6.0
SPHERE = 0.8
N_DEPTHS = 256


def look_at(position, target=(0.0, 0.0, 0.0), world_up=(0.0, 0.0, 1.0)):
    """c2w [3, 4] of a camera at `position` that looks at `target`: back = the unit vector from the target to the camera, right = world_up x
    back, up = back x right (float64, rounded once)"""
    p, t, u = (np.asarray(v, dtype=np.float64) for v in (position, target, world_up))
    back = (p - t) / np.linalg.norm(p - t)
    right = np.cross(u, back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    return torch.tensor(np.stack([right, up, back, p], 1), dtype=torch.float32)


def ring(n, radius=4.0, elevation_deg=30.0):
    el = math.radians(elevation_deg)
    return torch.stack([look_at((radius * math.cos(el) * math.cos(2 * math.pi * k / n), radius * math.cos(el) * math.sin(2 * math.pi * k / n),
                                 radius * math.sin(el))) for k in range(n)])


def pixel_rays(c2w, K, H, W):
    """(o [3], d [H, W, 3]) of one camera, fp32: d = R ((i - cx) / fx, -(j - cy) / fy, -1) for the pixel in row j, column i"""
    i, j = torch.meshgrid(torch.arange(W, dtype=torch.float32), torch.arange(H, dtype=torch.float32), indexing="xy")
    dirs = torch.stack([(i - K[0, 2]) / K[0, 0], -(j - K[1, 2]) / K[1, 1], -torch.ones_like(i)], -1)
    return c2w[:, 3], (dirs[..., None, :] * c2w[:, :3]).sum(-1)


def sphere_silhouette(c2w, K, H, W, radius=SPHERE):
    """bool [H, W]: the pixel's ray passes within `radius` of the origin (float64)"""
    o, d = pixel_rays(c2w, K, H, W)
    o, d = o.double(), d.double()
    t = -(d * o).sum(-1) / (d * d).sum(-1)
    closest = o + d * t[..., None]
    return (closest.norm(dim=-1) <= radius) & (t > 0)


def samples(c2w, K, H, W, near=NEAR, far=FAR, n=N_DEPTHS):
    """the sample points render() would evaluate, fp32 [H, W, n, 3]: o + d z at n uniform depths in [near, far]"""
    o, d = pixel_rays(c2w, K, H, W)
    t = torch.linspace(0.0, 1.0, n)
    z = near * (1.0 - t) + far * t
    return o + d[..., None, :] * z[:, None]


def cells_of(grid, pts):
    """(inside bool [...], cell int64 [...]) by the grid's own classifier"""
    inside, c, _ = grid._classify(pts)
    return inside, c


@pytest.fixture(scope="module")
def hull_scene():
    c2w = ring(8)
    grid = npa.OccupancyGrid((-1.5,) * 3, (1.5,) * 3, 32, device=CPU)
    masks = torch.stack([sphere_silhouette(c, K, H, W) for c in c2w])
    count = grid.view_counts_reference(c2w, H, W, K, NEAR, FAR)
    carved = grid.carved_reference(c2w, H, W, K, NEAR, FAR, masks)
    keep = grid.views_keep_reference(c2w, H, W, K, NEAR, FAR, masks=masks)
    return c2w, grid, masks, count, carved, keep


# ------------------------------------------------------------------------------------------------ what the definitions promise
def test_the_hull_of_a_sphere_from_a_ring_of_cameras(hull_scene):
    """8 cameras on a circle (azimuth k 45 deg, 30 deg above the plane, radius 4), 48 x 48 pixels, a 32^3 grid over +-1.5, a sphere of
    radius 0.8 as analytic silhouettes, 256 uniform depths per pixel ray.  A prototype of the rules gave a kept share of 0.184 with 0.105
    of the cells touching the sphere; the bound 0.25 is the issue's: a rule that kept every seen cell would fail it."""
    c2w, grid, masks, count, carved, keep = hull_scene
    assert count.dtype == torch.int32 and carved.dtype == torch.bool and keep.dtype == torch.bool
    assert count.shape == carved.shape == keep.shape == (32, 32, 32)
    assert torch.equal(keep, (count >= 1) & ~carved)
    flat_count, flat_carved, flat_keep = count.reshape(-1), carved.reshape(-1), keep.reshape(-1)
    touched = torch.zeros(grid.n_cells, dtype=torch.bool)
    n_inside = 0
    for v in range(8):
        pts = samples(c2w[v], K, H, W)
        inside, c = cells_of(grid, pts)
        n_inside += int(inside.sum())
        # (a) no sample inside the box lies in a cell that no camera sees
        assert bool((flat_count[c[inside]] > 0).all()), v
        # (b) no sample of a foreground ray of camera v lies in a cell that camera v carves (other cameras do carve along it, in front
        # of the sphere and behind it: that is the hull)
        fg = inside & masks[v][..., None]
        own = grid.carved_reference(c2w[v:v + 1], H, W, K, NEAR, FAR, masks[v:v + 1]).reshape(-1)
        assert int(fg.sum()) > 1000 and int(own.sum()) > 1000 and not bool(own[c[fg]].any()), v
        assert bool((flat_carved | ~own).all())
        # (c) no cell that holds a sample inside the sphere is lost
        ball = inside & (pts.double().norm(dim=-1) < SPHERE)
        assert int(ball.sum()) > 1000 and bool(flat_keep[c[ball]].all()), v
        touched[c[ball]] = True
    share, ball_share = float(flat_keep.float().mean()), float(touched.float().mean())
    print(f"kept share {share:.4f}, carved {float(flat_carved.float().mean()):.4f}, cells holding a sample of the sphere {ball_share:.4f}, "
          f"{n_inside} samples inside the box")
    # (d)
    assert share < 0.25 and ball_share > 0.05 and n_inside > 100000
    assert bool((flat_keep | ~touched).all())


def test_two_cameras_leave_most_of_a_large_box_unseen():
    """(a) again with two cameras (azimuth 0 and 45 deg), the box +-3 and R = 24: the frustum test alone; the prototype left 0.31 seen"""
    c2w = ring(8)[:2]
    grid = npa.OccupancyGrid((-3.0,) * 3, (3.0,) * 3, 24, device=CPU)
    count = grid.view_counts_reference(c2w, H, W, K, NEAR, FAR).reshape(-1)
    keep = grid.views_keep_reference(c2w, H, W, K, NEAR, FAR)
    assert torch.equal(keep.reshape(-1), count >= 1) and int(count.max()) == 2
    n_inside = 0
    for v in range(2):
        inside, c = cells_of(grid, samples(c2w[v], K, H, W))
        n_inside += int(inside.sum())
        assert bool((count[c[inside]] > 0).all()), v
    share = float((count > 0).float().mean())
    print(f"seen share {share:.4f} ({n_inside} samples inside the box)")
    assert share < 0.5 and n_inside > 100000


# ------------------------------------------------------------------------------------------------ edge cases
def test_a_nan_camera_sees_nothing_and_carves_nothing(hull_scene):
    c2w, grid, masks, count, carved, _ = hull_scene
    background = torch.zeros(1, H, W, dtype=torch.bool)
    for r, col in ((0, 0), (1, 1), (2, 2), (0, 3)):
        bad = c2w[:1].clone()
        bad[0, r, col] = NAN
        assert int(grid.view_counts_reference(bad, H, W, K, NEAR, FAR).sum()) == 0, (r, col)
        assert not bool(grid.carved_reference(bad, H, W, K, NEAR, FAR, background).any()), (r, col)
    # next to good cameras it changes nothing
    both = torch.cat([c2w, bad])
    assert torch.equal(grid.view_counts_reference(both, H, W, K, NEAR, FAR), count)
    assert torch.equal(grid.carved_reference(both, H, W, K, NEAR, FAR, torch.cat([masks, background])), carved)
    # a NaN intrinsic, and a NaN depth range
    Kbad = K.clone()
    Kbad[0, 0] = NAN
    assert int(grid.view_counts_reference(c2w, H, W, Kbad, NEAR, FAR).sum()) == 0
    assert int(grid.view_counts_reference(c2w, H, W, K, NAN, FAR).sum()) == 0


def test_a_camera_inside_the_box_abstains_around_itself():
    """all-background silhouettes, near = 0.5: a cell with a corner in front of the near plane (every cell within 0.4 of the camera has
    one: s <= the distance) is never carved, though cells further along the view are"""
    grid = npa.OccupancyGrid((-1.5,) * 3, (1.5,) * 3, 32, device=CPU)
    eye = (0.3, -0.2, 0.1)
    c2w = look_at(eye, target=(3.0, 0.5, 0.2))[None]
    carved = grid.carved_reference(c2w, H, W, K, 0.5, 6.0, torch.zeros(1, H, W, dtype=torch.bool))
    centres = grid.cell_points(0, grid.n_cells).reshape(32, 32, 32, 3)
    around = (centres - torch.tensor(eye)).norm(dim=-1) < 0.4
    assert int(around.sum()) > 50 and not bool((carved & around).any())
    assert int(carved.sum()) > 100
    # the cell that holds the camera is seen by nobody's near plane: not seen at all with near = 0.5
    count = grid.view_counts_reference(c2w, H, W, K, 0.5, 6.0)
    _, c = cells_of(grid, torch.tensor([eye]))
    assert int(count.reshape(-1)[c[0]]) == 0 and int(count.max()) == 1


def test_all_foreground_carves_nothing_and_all_background_only_inside_the_image(hull_scene):
    c2w, grid, _, count, _, _ = hull_scene
    assert not bool(grid.carved_reference(c2w, H, W, K, NEAR, FAR, torch.ones(8, H, W, dtype=torch.bool)).any())
    one = c2w[:1]
    carved = grid.carved_reference(one, H, W, K, NEAR, FAR, torch.zeros(1, H, W, dtype=torch.bool)).reshape(-1)
    # the corners in the camera, in float64
    idx = torch.stack(torch.meshgrid(*[torch.arange(33, dtype=torch.float64)] * 3, indexing="ij"), -1)
    p = -1.5 + idx * (3.0 / 32)
    d = p - one[0, :, 3].double()
    x, y, s = (d * one[0, :, 0].double()).sum(-1), (d * one[0, :, 1].double()).sum(-1), -(d * one[0, :, 2].double()).sum(-1)
    i, j = FOCAL * x / s + 24.0, 24.0 - FOCAL * y / s
    ok = (s > 0) & (i >= 0) & (i <= W - 1) & (j >= 0) & (j <= H - 1)            # per corner of the 33^3 lattice
    whole = torch.ones(32, 32, 32, dtype=torch.bool)
    for ox in (0, 1):
        for oy in (0, 1):
            for oz in (0, 1):
                whole &= ok[ox:ox + 32, oy:oy + 32, oz:oz + 32]
    whole = whole.reshape(-1)
    print(f"all-background: carved {int(carved.sum())} cells, {int(whole.sum())} project inside the image")
    assert int(carved.sum()) > 1000 and bool((whole | ~carved).all())
    # a cell whose rectangle clears the border by more than the margin and a pixel of rounding is carved
    clear = torch.ones(32, 32, 32, dtype=torch.bool)
    inner = (s >= NEAR) & (i >= 2) & (i <= W - 3) & (j >= 2) & (j <= H - 3)
    for ox in (0, 1):
        for oy in (0, 1):
            for oz in (0, 1):
                clear &= inner[ox:ox + 32, oy:oy + 32, oz:oz + 32]
    assert int(clear.sum()) > 1000 and bool((carved | ~clear.reshape(-1)).all())
    # a larger margin carves less and sees more
    wide = grid.carved_reference(one, H, W, K, NEAR, FAR, torch.zeros(1, H, W, dtype=torch.bool), margin_px=3.0).reshape(-1)
    assert bool((carved | ~wide).all()) and int(wide.sum()) < int(carved.sum())
    assert bool((grid.view_counts_reference(c2w, H, W, K, NEAR, FAR, margin_px=3.0) >= count).all())


def test_min_views_and_per_view_intrinsics(hull_scene):
    c2w, grid, masks, count, carved, keep = hull_scene
    two = grid.views_keep_reference(c2w, H, W, K, NEAR, FAR, masks=masks, min_views=2)
    assert bool((keep | ~two).all()) and torch.equal(two, (count >= 2) & ~carved)
    more = npa.OccupancyGrid((-3.0,) * 3, (3.0,) * 3, 24, device=CPU)
    a = more.views_keep_reference(c2w[:3], H, W, K, NEAR, FAR)
    b = more.views_keep_reference(c2w[:3], H, W, K, NEAR, FAR, min_views=2)
    assert bool((a | ~b).all()) and 0 < int(b.sum()) < int(a.sum())
    # K [V, 3, 3] with equal rows is K [3, 3]; a longer lens on one camera sees fewer cells
    assert torch.equal(grid.view_counts_reference(c2w, H, W, K[None].expand(8, 3, 3), NEAR, FAR), count)
    Ks = K[None].repeat(8, 1, 1)
    Ks[0, 0, 0] = Ks[0, 1, 1] = 4.0 * FOCAL
    tele = grid.view_counts_reference(c2w, H, W, Ks, NEAR, FAR)
    assert bool((tele <= count).all()) and int(tele.sum()) < int(count.sum())
    for bad in (0, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="min_views"):
            grid.views_keep_reference(c2w, H, W, K, NEAR, FAR, min_views=bad)
    with pytest.raises(ValueError, match="masks"):
        grid.carved_reference(c2w, H, W, K, NEAR, FAR, masks[:, :-1])
    with pytest.raises(ValueError, match="masks"):
        grid.carved_reference(c2w, H, W, K, NEAR, FAR, None)
    with pytest.raises(ValueError, match="c2w"):
        grid.view_counts_reference(torch.zeros(0, 3, 4), H, W, K, NEAR, FAR)
    with pytest.raises(ValueError, match="K "):
        grid.view_counts_reference(c2w, H, W, K[None].expand(3, 3, 3), NEAR, FAR)
    for bad in (-0.5, NAN, float("inf")):
        with pytest.raises(ValueError, match="margin_px"):
            grid.view_counts_reference(c2w, H, W, K, NEAR, FAR, margin_px=bad)


# ------------------------------------------------------------------------------------------------ restrict
def _dgrid(res=(5, 6, 7), **kw):
    g = npa.DensityGrid((-1, -1, -1), (1, 1, 1), res, device=CPU, sigma_threshold=0.5, **kw)
    g.density = torch.rand(g.n_cells, generator=torch.Generator().manual_seed(3))
    return g


def test_density_grid_restrict_on_the_cpu():
    gen = torch.Generator().manual_seed(5)
    keep = torch.rand(5, 6, 7, generator=gen) < 0.5
    words = npa.occupancy._pack_bits(keep.reshape(-1))
    for dilate in (0, 1):
        g = _dgrid(dilate=dilate)
        free = g._bits_reference()
        keys = set(g.state_dict())
        assert g.keep is None and "keep" not in keys
        # warm-up: the grid is all-occupied, restricted it is the keep mask
        assert g.restrict(keep) is g
        assert torch.equal(g.keep, words) and g.keep.dtype == torch.int32 and torch.equal(g.to_mask(), keep)
        assert torch.equal(g._bits_reference(), free & words)
        assert 0 < int(npa.occupancy._unpack_bits(free & words, g.n_cells).sum()) < int(npa.occupancy._unpack_bits(free, g.n_cells).sum())
        # after an update (stood in for by the definition): restricted bits, and restrict(None) gives back the unrestricted ones
        g.n_updates, g.bits = 1, g._bits_reference()
        state = g.state_dict()
        assert set(state) == keys | {"keep"} and torch.equal(state["keep"], words)
        g.restrict(None)
        assert g.keep is None and torch.equal(g.bits, free) and torch.equal(g._bits_reference(), free) and set(g.state_dict()) == keys
        # round trip
        h = npa.DensityGrid((0, 0, 0), (1, 1, 1), 2, device=CPU).load_state_dict(state)
        assert torch.equal(h.keep, words) and torch.equal(h.bits, free & words) and torch.equal(h._bits_reference(), free & words)
        assert h.load_state_dict(g.state_dict()).keep is None
        # a second restriction replaces the first
        other = torch.rand(5, 6, 7, generator=gen) < 0.5
        h.load_state_dict(state).restrict(other)
        assert torch.equal(h.bits, free & npa.occupancy._pack_bits(other.reshape(-1)))
    # an OccupancyGrid as the restriction, and a plain grid restricted once
    g = _dgrid()
    hull = npa.OccupancyGrid.from_mask(keep, (-1, -1, -1), (1, 1, 1), device=CPU)
    assert torch.equal(g.restrict(hull).bits, words) and g.keep is not hull.bits
    plain = npa.OccupancyGrid.from_mask(torch.rand(5, 6, 7, generator=gen) < 0.7, (-1, -1, -1), (1, 1, 1), device=CPU)
    before = plain.to_mask()
    assert torch.equal(plain.restrict(keep).to_mask(), before & keep) and not hasattr(plain, "keep")
    assert set(plain.state_dict()) == {"lo", "hi", "resolution", "outside", "bits"}
    with pytest.raises(ValueError, match="plain grid"):
        plain.restrict(None)
    # mismatches
    for target in (g, plain):
        with pytest.raises(ValueError, match="box and resolution"):
            target.restrict(npa.OccupancyGrid((-1, -1, -1), (1, 1, 2), (5, 6, 7), device=CPU))
        with pytest.raises(ValueError, match="box and resolution"):
            target.restrict(npa.OccupancyGrid((-1, -1, -1), (1, 1, 1), (5, 6, 8), device=CPU))
        with pytest.raises(ValueError, match="bool"):
            target.restrict(torch.ones(5, 6, 8, dtype=torch.bool))
        with pytest.raises(ValueError, match="bool"):
            target.restrict(torch.ones(5, 6, 7))
    bad = g.state_dict()
    bad["keep"] = bad["keep"][:-1]
    with pytest.raises(ValueError, match="keep"):
        _dgrid().load_state_dict(bad)


def test_the_kernel_forms_need_the_gpu():
    grid = npa.DensityGrid((-1, -1, -1), (1, 1, 1), 4, device=CPU)
    c2w = ring(2)
    for call in (lambda: grid.view_counts(c2w, H, W, K, NEAR, FAR),
                 lambda: grid.carved(c2w, H, W, K, NEAR, FAR, torch.zeros(2, H, W, dtype=torch.bool)),
                 lambda: grid.restrict_to_views(c2w, H, W, K, NEAR, FAR),
                 lambda: npa.OccupancyGrid.from_views(c2w, H, W, K, NEAR, FAR, (-1, -1, -1), (1, 1, 1), 4, device=CPU)):
        with pytest.raises(npa.hip_backend.NerfHipError, match="GPU"):
            call()
    assert grid.keep is None


# ------------------------------------------------------------------------------------------------ exports
def test_the_library_exports_and_binds_the_entry_point():
    hb = npa.hip_backend
    raw = ctypes.CDLL(npa.build.LIB_PATH)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_hip.h")) as f:
        header = f.read()
    assert hasattr(raw, "nerf_occ_view_carve") and "nerf_occ_view_carve" in hb.EXPORTS and "int nerf_occ_view_carve(" in header
    assert "#define NERF_ABI_VERSION 10" in header and hb.ABI_VERSION == 10
    assert list(inspect.signature(hb.occ_view_carve).parameters) == ["desc", "width", "cams", "H", "W", "near_m", "far_m", "margin_px", "sat",
                                                                     "seen", "carved_words", "accumulate"]
    assert list(inspect.signature(npa.OccupancyGrid.from_views).parameters) == [
        "c2w", "H", "W", "K", "near", "far", "lo", "hi", "resolution", "masks", "min_views", "margin_px", "dilate", "outside", "device"]
    assert list(inspect.signature(npa.DensityGrid.restrict_to_views).parameters) == [
        "self", "c2w", "H", "W", "K", "near", "far", "masks", "min_views", "margin_px", "dilate"]
    L = hb.lib()
    assert L.nerf_abi_version() == 10
    # refused before anything is launched or read (host memory stands in for the device buffers)
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    desc = hb.NerfOccGrid((ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_int * 3)(2, 2, 2), 0, ptr)
    width = (ctypes.c_float * 3)(0.5, 0.5, 0.5)

    def call(grid=desc, V=1, H=4, W=4, m=0.5, masks=True, **null):
        a = dict(width=width, cams=ptr, sat=ptr if masks else None, seen=ptr, carved=ptr if masks else None)
        a.update(null)
        return L.nerf_occ_view_carve(None if grid is None else ctypes.byref(grid), a["width"], a["cams"], V, H, W, 2.0, 6.0, m, a["sat"], 0,
                                     a["seen"], a["carved"], None)
    for masks in (True, False):
        for name in ("width", "cams", "seen"):
            assert call(masks=masks, **{name: None}) != 0 and "null" in L.nerf_last_error().decode(), name
        assert call(masks=masks, grid=None) != 0 and "null" in L.nerf_last_error().decode()
        for kw in (dict(V=0), dict(V=-3), dict(H=0), dict(W=0), dict(H=16385), dict(W=16385)):
            assert call(masks=masks, **kw) != 0 and "bad size" in L.nerf_last_error().decode(), kw
        for m in (-1.0, NAN, float("inf")):
            assert call(masks=masks, m=m) != 0 and "margin_px" in L.nerf_last_error().decode(), m
    # the table and the words it fills come together
    assert call(sat=None) != 0 and "null" in L.nerf_last_error().decode()
    assert call(carved=None) != 0 and "null" in L.nerf_last_error().decode()
    big = hb.NerfOccGrid((ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_int * 3)(2, 513, 2), 0, ptr)
    assert call(grid=big) != 0 and "resolution" in L.nerf_last_error().decode()
    assert hb.view_planes(2.0, 6.0) == (float(np.float32(2.0 * (1 - 2.0 ** -10))), float(np.float32(6.0 * (1 + 2.0 ** -10))))
