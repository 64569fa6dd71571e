"""CPU: render_rays(proposal="grid") without a GPU -- the export of nerf_occ_proposal_weights, DensityGrid.proposal_sigma (the
definition the kernel reproduces) on a hand-built 4 x 3 x 5 grid against an explicit Python loop, every guard on CPU tensors with
nothing launched, and the keys of the empty batch."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import nerf_pytorch_amd as npa

CPU = torch.device("cpu")
NET_KW = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
LO, HI, RES = (-1.0, 0.5, 2.0), (1.0, 2.0, 4.5), (4, 3, 5)
THRESHOLD = 0.3


def hand_grid(outside):
    """4 x 3 x 5 cells, every third cell's bit clear, densities -1.5, -1.25, ... (negatives, an exact zero, positives): a value per
    cell that names the cell, so a wrong index order gives a wrong number"""
    g = npa.DensityGrid(LO, HI, RES, outside=outside, device=CPU, sigma_threshold=THRESHOLD)
    mask = (torch.arange(60) % 3 != 1).view(RES)
    g.bits = npa.OccupancyGrid.from_mask(mask, LO, HI, device=CPU).bits.clone()
    g.density = (torch.arange(60, dtype=torch.float32) - 6.0) * 0.25
    return g, mask


def loop_sigma(g, mask, pts):
    """the rule of the issue, one point at a time in numpy fp32 scalars"""
    out = []
    res = g.resolution
    for p in pts.numpy():
        t = [(np.float32(p[a]) - np.float32(g.lo[a])) * np.float32(g.scale[a]) for a in range(3)]
        inside = all(t[a] >= 0 and t[a] < np.float32(res[a]) for a in range(3))       # (a NaN fails both)
        if not inside:
            out.append(np.float32(g.sigma_threshold) if g.outside == "evaluate" else np.float32(0.0))
            continue
        ix, iy, iz = (int(np.floor(v)) for v in t)
        c = (ix * res[1] + iy) * res[2] + iz
        out.append(np.float32(g.density[c]) if bool(mask[ix, iy, iz]) else np.float32(0.0))
    return torch.tensor(np.asarray(out, dtype=np.float32))


def probe_points():
    gen = torch.Generator().manual_seed(4)
    lo, hi = torch.tensor(LO), torch.tensor(HI)
    width = (hi - lo) / torch.tensor(RES, dtype=torch.float32)
    inside = lo + (hi - lo) * torch.rand(400, 3, generator=gen)
    around = lo + (hi - lo) * (torch.rand(200, 3, generator=gen) * 1.6 - 0.3)       # in and out of the box
    # every corner of every cell: exactly ON the faces, the box's own faces (k = 0 and k = R) included
    k = torch.stack(torch.meshgrid(*[torch.arange(r + 1, dtype=torch.float32) for r in RES], indexing="ij"), -1).reshape(-1, 3)
    faces = lo + k * width
    one_axis = inside[:60].clone()
    one_axis[:, 1] = faces[:60, 1]                                                   # on a face of one axis only
    special = torch.tensor([[float("nan"), 1.0, 3.0], [0.0, float("nan"), 3.0], [0.0, 1.0, float("inf")], [0.0, 1.0, -float("inf")],
                            list(LO), list(HI), [1e30, 1.0, 3.0]])
    return torch.cat([inside, around, faces, one_axis, special], 0)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_the_library_exports_and_binds_the_entry_point():
    hb = npa.hip_backend
    assert hasattr(ctypes.CDLL(npa.build.LIB_PATH), "nerf_occ_proposal_weights") and "nerf_occ_proposal_weights" in hb.EXPORTS
    assert callable(hb.occ_proposal_weights) and hb.ABI_VERSION == 10
    L = hb.lib()
    assert L.nerf_abi_version() == 10
    assert L.nerf_occ_proposal_weights(None, None, 0.0, None, 11, None, 1, 1, None, None, None) != 0
    assert "null" in L.nerf_last_error().decode()
    # the limits, refused before anything is launched or read (host memory stands in for the device buffers)
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    desc = hb.NerfOccGrid((ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_int * 3)(2, 2, 2), 0, ptr)
    call = lambda stride, n, S: L.nerf_occ_proposal_weights(ctypes.byref(desc), ptr, 0.0, ptr, stride, ptr, n, S, ptr, None, None)
    for stride, n, S in ((5, 1, 8), (6, 1, 0), (6, 1, 4097), (6, -1, 8)):
        assert call(stride, n, S) != 0 and "bad size" in L.nerf_last_error().decode(), (stride, n, S)
    assert call(6, 0, 4096) == 0          # no rays: nothing to do


@pytest.mark.parametrize("outside", ["evaluate", "skip"])
def test_proposal_sigma_on_a_hand_built_grid_against_a_python_loop(outside):
    g, mask = hand_grid(outside)
    pts = probe_points()
    got = g.proposal_sigma(pts)
    want = loop_sigma(g, mask, pts)
    assert got.dtype == torch.float32 and got.shape == pts.shape[:-1]
    assert bits_equal(got, want), int((got != want).sum())
    # the cases are all there: set bits with negative, zero and positive densities, clear bits, points outside
    occ = g.occupied(pts)
    inside = ((pts >= torch.tensor(LO)) & (pts < torch.tensor(HI))).all(-1)
    hit = got[inside & occ]
    assert bool((hit < 0).any()) and bool((hit == 0).any()) and bool((hit > 0).any())
    assert int((inside & ~occ).sum()) > 50 and bool((got[inside & ~occ] == 0).all())
    out_val = np.float32(THRESHOLD) if outside == "evaluate" else np.float32(0.0)
    assert int((~inside).sum()) > 50 and bool((got[~inside] == float(out_val)).all())
    # on the faces: lo itself is cell 0 (inside), hi itself is outside, a NaN is outside
    assert float(g.proposal_sigma(torch.tensor([LO]))[0]) == float(g.density[0])
    assert float(g.proposal_sigma(torch.tensor([HI]))[0]) == float(out_val)
    assert float(g.proposal_sigma(torch.tensor([[float("nan"), 1.0, 3.0]]))[0]) == float(out_val)
    # leading shapes are kept
    assert bits_equal(g.proposal_sigma(pts[:24].view(2, 3, 4, 3)), want[:24].view(2, 3, 4))
    # the classifier this shares its arithmetic with did not move
    assert torch.equal(occ, torch.where(inside_by_rule(g, pts), mask.reshape(-1)[cell_by_rule(g, pts)], torch.tensor(outside == "evaluate")))


def inside_by_rule(g, pts):
    t = (pts - torch.tensor(g.lo)) * torch.tensor(g.scale)
    return ((t >= 0) & (t < torch.tensor(g.resolution, dtype=torch.float32))).all(-1)


def cell_by_rule(g, pts):
    t = (pts - torch.tensor(g.lo)) * torch.tensor(g.scale)
    i = torch.where(inside_by_rule(g, pts)[:, None], t, torch.zeros_like(t)).floor().long()
    return (i[:, 0] * g.resolution[1] + i[:, 1]) * g.resolution[2] + i[:, 2]


def test_a_fresh_grid_proposes_zero_inside_the_box():
    g = npa.DensityGrid(LO, HI, RES, device=CPU, sigma_threshold=THRESHOLD)
    pts = probe_points()
    got = g.proposal_sigma(pts)
    inside = inside_by_rule(g, pts)
    assert bool((got[inside] == 0).all()) and bool((got[~inside] == float(np.float32(THRESHOLD))).all())
    g.outside = "skip"
    assert bool((g.proposal_sigma(pts) == 0).all())


def _rays(n):
    gen = torch.Generator().manual_seed(1)
    o = torch.tensor([0.0, 1.0, 6.0]) + 0.1 * torch.randn(n, 3, generator=gen)
    d = torch.tensor([0.0, 0.0, -1.0]) + 0.1 * torch.randn(n, 3, generator=gen)
    return torch.cat([o, d, torch.full((n, 1), 2.0), torch.full((n, 1), 6.0), torch.nn.functional.normalize(d, dim=-1)], -1)


def test_proposal_is_keyword_only_and_every_guard_fires_before_a_launch(monkeypatch):
    p = inspect.signature(npa.render_rays).parameters["proposal"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    net, fine = npa.NeRF(**NET_KW), npa.NeRF(**NET_KW)
    dense = npa.NeRF(D=4, W=64, input_ch=3, output_ch=4, skips=[2], input_ch_views=3, use_viewdirs=True)
    assert isinstance(dense, npa.dense.DenseNeRF)
    monkeypatch.setattr(npa.hip_backend, "lib", lambda: pytest.fail("a guard let a call reach the library"))
    rays = _rays(8)
    dgrid, _ = hand_grid("evaluate")
    plain = npa.OccupancyGrid(LO, HI, RES, device=CPU)
    kw = dict(N_samples=8, N_importance=8, network_fine=fine)
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            with pytest.raises(ValueError, match="proposal must be"):
                npa.render_rays(rays, net, None, occupancy=dgrid, proposal="network", **kw)
            with pytest.raises(ValueError, match="proposal must be"):
                npa.render_rays(rays, net, None, proposal=True, **kw)
            with pytest.raises(ValueError, match="DensityGrid"):
                npa.render_rays(rays, net, None, proposal="grid", **kw)
            with pytest.raises(ValueError, match="plain OccupancyGrid"):
                npa.render_rays(rays, net, None, occupancy=plain, proposal="grid", **kw)
            with pytest.raises(ValueError, match="N_importance"):
                npa.render_rays(rays, net, None, occupancy=dgrid, proposal="grid", N_samples=8, N_importance=0)
            with pytest.raises(ValueError, match="N_importance"):
                npa.render_rays(rays, net, None, occupancy=dgrid, proposal="grid", N_samples=8)
            # what the occupancy path refuses stays refused, with its own error
            with pytest.raises(NotImplementedError, match="network_query_fn"):
                npa.render_rays(rays, net, lambda pts, vd, m: None, occupancy=dgrid, proposal="grid", **kw)
            with pytest.raises(NotImplementedError, match="DenseNeRF"):
                npa.render_rays(rays, dense, None, occupancy=dgrid, proposal="grid", N_samples=8, N_importance=8)
    # through the layers that forward keywords: batchify_rays and render hand `proposal` to render_rays as they hand `occupancy`
    with pytest.raises(ValueError, match="plain OccupancyGrid"):
        npa.batchify_rays(rays, 4, network_fn=net, network_query_fn=None, occupancy=plain, proposal="grid", **kw)
    K = np.array([[10.0, 0, 2.0], [0, 10.0, 2.0], [0, 0, 1]])
    with pytest.raises(ValueError, match="proposal must be"):
        npa.render(4, 4, K, chunk=8, rays=(rays[:, 0:3], rays[:, 3:6]), ndc=False, near=2.0, far=6.0, use_viewdirs=True, network_fn=net,
                   network_query_fn=None, occupancy=dgrid, proposal="coarse", **kw)


@pytest.mark.parametrize("retraw", [False, True])
def test_the_empty_batch_has_the_keys_of_the_mode(monkeypatch, retraw):
    net, fine = npa.NeRF(**NET_KW), npa.NeRF(**NET_KW)
    dgrid, _ = hand_grid("evaluate")
    monkeypatch.setattr(dgrid, "_desc", lambda: None)       # (the empty batch validates the grid's device; this grid lives on the CPU)
    kw = dict(N_samples=8, N_importance=16, network_fine=fine, retraw=retraw, occupancy=dgrid)
    out = npa.render_rays(_rays(0), net, None, proposal="grid", **kw)
    assert set(out) == {"rgb_map", "disp_map", "acc_map", "z_std"} | ({"raw"} if retraw else set())
    assert out["rgb_map"].shape == (0, 3) and out["disp_map"].shape == (0,) and out["acc_map"].shape == (0,) and out["z_std"].shape == (0,)
    if retraw:
        assert out["raw"].shape == (0, 24, 4)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0}
    out = npa.render_rays(_rays(0), net, None, proposal="grid", clip_to_occupancy=True, **kw)
    assert "rgb0" not in out and dgrid.last_stats == {"evaluated": 0, "total": 0, "rays_hit": 0, "rays": 0}
    # without the option the empty batch is what it was
    out = npa.render_rays(_rays(0), net, None, **kw)
    assert set(out) == {"rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "z_std"} | ({"raw"} if retraw else set())
