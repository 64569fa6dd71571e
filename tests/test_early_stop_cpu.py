"""CPU: render_rays(early_stop_eps=) without a GPU -- the exports of nerf_occ_stop_depth / nerf_occ_compact_stop, the definition of the
stop depth (occupancy.stop_depth_reference) against an explicit Python loop over fp32 scalars on hand-made rows, what the definition
means in float64, every guard on CPU tensors with nothing launched, and the stats of the empty batch."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import nerf_pytorch_amd as npa

CPU = torch.device("cpu")
NET_KW = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
LO, HI, RES = (-1.0, 0.5, 2.0), (1.0, 2.0, 4.5), (4, 3, 5)
U = 2.0 ** -24          # unit roundoff of fp32
INF = float("inf")


def threshold(eps):
    """fp32(1 - eps), the subtraction in double"""
    return np.float32(1.0 - float(eps))


def loop_stop_depth(z, w, eps):
    """the rule of the issue, one ray and one sample at a time in numpy fp32 scalars: fp32 [N] as a torch tensor"""
    z, w = np.asarray(z, dtype=np.float32), np.asarray(w, dtype=np.float32)
    thr = threshold(eps)
    n, S = z.shape
    out = np.full(n, np.inf, dtype=np.float32)
    with np.errstate(all="ignore"):
        for r in range(n):
            a = np.float32(0.0)
            for i in range(S):
                a = np.float32(a + w[r, i])
                if a >= thr:            # (a NaN is not)
                    if i + 1 < S:
                        out[r] = z[r, i + 1]
                    break
    return torch.from_numpy(out)


HAND_ROWS = ("crossing at 0", "crossing at S - 2", "crossing at S - 1", "no crossing", "sum exactly the threshold", "NaN before the crossing",
             "NaN after the crossing", "all zero", "one infinite weight", "-inf then +inf")


def hand_rows(S, eps):
    """(z fp32 [10, S] strictly increasing per row, w fp32 [10, S]) in the order of HAND_ROWS; an index beyond a short row is left out
    (S = 1: every crossing is the one at S - 1)"""
    thr = threshold(eps)
    k = len(HAND_ROWS)
    z = (2.0 + 4.0 * (np.arange(S, dtype=np.float64)[None, :] + 0.25 * np.arange(k)[:, None] / k) / S).astype(np.float32)
    w = np.zeros((k, S), dtype=np.float32)

    def put(row, i, v):
        if 0 <= i < S:
            w[row, i] = v
    put(0, 0, 1.0)
    put(1, max(S - 2, 0), 1.0)
    put(2, S - 1, 1.0)
    w[3, :] = np.float32(0.5) * thr / np.float32(S)
    if S >= 2:          # two halves of the threshold: the scaling by 0.5 and the one addition are exact
        put(4, 0, np.float32(0.5) * thr)
        put(4, 1, np.float32(0.5) * thr)
    else:
        put(4, 0, thr)
    put(5, 0, np.nan)
    put(5, 1, 1.0)
    put(6, 0, 1.0)
    put(6, 1, np.nan)
    put(8, min(1, S - 1), np.inf)
    put(9, 0, -np.inf)
    put(9, 1, np.inf)
    return torch.from_numpy(z), torch.from_numpy(w)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ exports
def test_the_library_exports_and_binds_both_entry_points():
    hb = npa.hip_backend
    raw = ctypes.CDLL(npa.build.LIB_PATH)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_hip.h")) as f:
        header = f.read()
    for name in ("nerf_occ_stop_depth", "nerf_occ_compact_stop"):
        assert hasattr(raw, name) and name in hb.EXPORTS and f"int {name}(" in header, name
    assert "#define NERF_ABI_VERSION 10" in header and hb.ABI_VERSION == 10
    assert callable(hb.occ_stop_depth) and "z_stop" in inspect.signature(hb.occ_compact).parameters
    assert inspect.signature(hb.occ_compact).parameters["z_stop"].default is None
    L = hb.lib()
    assert L.nerf_abi_version() == 10
    assert L.nerf_occ_stop_depth(None, None, 1, 1, 0.5, None, None) != 0 and "null" in L.nerf_last_error().decode()
    # the limits, refused before anything is launched or read (host memory stands in for the device buffers)
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    for n, S in ((1, 0), (1, 4097), (-1, 8)):
        assert L.nerf_occ_stop_depth(ptr, ptr, n, S, 0.5, ptr, None) != 0 and "bad size" in L.nerf_last_error().decode(), (n, S)
    assert L.nerf_occ_stop_depth(ptr, ptr, 0, 4096, 0.5, ptr, None) == 0           # no rays: nothing to do
    desc = hb.NerfOccGrid((ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_int * 3)(2, 2, 2), 0, ptr)
    compact = lambda z_stop, stride, n, S: L.nerf_occ_compact_stop(ctypes.byref(desc), ptr, stride, ptr, z_stop, n, S, ptr, ptr, ptr, ptr, None)
    assert compact(None, 11, 1, 1) != 0 and "null" in L.nerf_last_error().decode()          # z_stop is not optional
    for stride, n, S in ((10, 1, 1), (11, 1, 0), (11, -1, 1)):
        assert compact(ptr, stride, n, S) != 0 and "bad size" in L.nerf_last_error().decode(), (stride, n, S)
    # the threshold is fp32(1 - eps) with the subtraction in double
    for eps in (1e-4, 1e-3, 1e-2, 0.3, 1 - 1e-6, 1e-9):
        assert hb.stop_threshold(eps) == float(np.float32(1.0 - eps))
    assert hb.stop_threshold(1e-9) == 1.0


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("eps", [1e-4, 0.3])
@pytest.mark.parametrize("S", [1, 2, 3, 6, 64])
def test_stop_depth_reference_on_hand_made_rows_against_a_python_loop(S, eps):
    z, w = hand_rows(S, eps)
    got = npa.occupancy.stop_depth_reference(z, w, eps)
    want = loop_stop_depth(z, w, eps)
    assert got.dtype == torch.float32 and got.shape == (len(HAND_ROWS),)
    assert bits_equal(got, want), (got, want)
    if S >= 3:          # what the rows are there for, spelt out (z[r, i] by hand, not by the loop)
        zz = z.numpy()
        expect = [zz[0, 1], zz[1, S - 1], INF, INF, zz[4, 2], INF, zz[6, 1], INF, zz[8, 2], INF]
        assert got.tolist() == [float(v) for v in expect]
    if S == 1:          # one sample: its interval is the 1e10 one, nothing lies behind it
        assert bool(torch.isinf(got).all()) and bool((got > 0).all())
    # one ulp of the threshold below the exact sum does not stop there: the comparison is >=, not a tolerance (two ulps of the half:
    # the sum is then the threshold's predecessor exactly, no tie to round)
    if S >= 3:
        w2 = w.clone()
        w2[4, 1] = torch.from_numpy(np.nextafter(np.nextafter(w[4, 1:2].numpy(), np.float32(0.0)), np.float32(0.0)))
        assert float(npa.occupancy.stop_depth_reference(z, w2, eps)[4]) == INF
    # tensors of other dtypes / with a graph are taken as values
    assert bits_equal(npa.occupancy.stop_depth_reference(z.double(), w.double().requires_grad_(True), eps), want)


def test_the_definition_means_transmittance_below_eps_in_float64():
    """smooth random weights that sum to below 1: with c = the float64 cumulative sum of the same fp32 weights, 1 - c at the stop index
    i* is < eps and at i* - 1 it is >= eps, both within S * 2^-24 -- the fp32 running sum of S terms that sum to at most 1 is within
    (S - 1) * 2^-24 of the float64 one (first order), and fp32(1 - eps) is within 2^-25 of 1 - eps."""
    g = torch.Generator().manual_seed(3)
    n, S = 400, 64
    slack = S * U
    z = (2.0 + 4.0 * (torch.arange(S, dtype=torch.float64) + 0.5 * torch.rand(n, S, generator=g, dtype=torch.float64)) / S).float()
    centre, width = torch.rand(n, 1, generator=g) * S, 1.0 + 6.0 * torch.rand(n, 1, generator=g)
    bump = torch.exp(-0.5 * ((torch.arange(S)[None, :] - centre) / width) ** 2) + 1e-3
    total = 0.5 + 0.4999 * torch.rand(n, 1, generator=g)          # acc of the ray: 0.5 .. 0.9999
    w = (bump / bump.sum(-1, keepdim=True) * total).float()
    assert float(w.double().sum(-1).max()) < 1.0
    seen = {"stopped": 0, "never": 0}
    for eps in (1e-4, 1e-2, 0.3):
        z_stop = npa.occupancy.stop_depth_reference(z, w, eps)
        c = torch.cumsum(w.double(), -1)
        for r in range(n):
            if np.isfinite(float(z_stop[r])):
                hit = (z[r] == z_stop[r]).nonzero()
                assert hit.numel() == 1
                i = int(hit[0, 0]) - 1
                assert 1.0 - float(c[r, i]) < eps + slack
                seen["stopped"] += 1
            else:           # never crossed, or crossed at the last sample: in front of it the transmittance is still >= eps
                i = S - 1
                seen["never"] += 1
            if i > 0:
                assert 1.0 - float(c[r, i - 1]) >= eps - slack
    assert seen["stopped"] > 200 and seen["never"] > 200


# ------------------------------------------------------------------------------------------------ guards
def _rays(n):
    gen = torch.Generator().manual_seed(1)
    o = torch.tensor([0.0, 1.0, 6.0]) + 0.1 * torch.randn(n, 3, generator=gen)
    d = torch.tensor([0.0, 0.0, -1.0]) + 0.1 * torch.randn(n, 3, generator=gen)
    return torch.cat([o, d, torch.full((n, 1), 2.0), torch.full((n, 1), 6.0), torch.nn.functional.normalize(d, dim=-1)], -1)


def test_early_stop_eps_is_keyword_only_and_every_guard_fires_before_a_launch(monkeypatch):
    p = inspect.signature(npa.render_rays).parameters["early_stop_eps"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    net, fine = npa.NeRF(**NET_KW), npa.NeRF(**NET_KW)
    dense = npa.NeRF(D=4, W=64, input_ch=3, output_ch=4, skips=[2], input_ch_views=3, use_viewdirs=True)
    assert isinstance(dense, npa.dense.DenseNeRF)
    monkeypatch.setattr(npa.hip_backend, "lib", lambda: pytest.fail("a guard let a call reach the library"))
    rays = _rays(8)
    dgrid = npa.DensityGrid(LO, HI, RES, device=CPU)
    plain = npa.OccupancyGrid(LO, HI, RES, device=CPU)
    kw = dict(N_samples=8, N_importance=8, network_fine=fine)
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            for grid in (dgrid, plain):
                for bad in (0, 0.0, 1, 1.0, -1, float("nan"), 2.5, float("inf")):
                    with pytest.raises(ValueError, match="0 < eps < 1"):
                        npa.render_rays(rays, net, None, occupancy=grid, early_stop_eps=bad, **kw)
                with pytest.raises(ValueError, match="N_importance"):
                    npa.render_rays(rays, net, None, occupancy=grid, early_stop_eps=0.01, N_samples=8, N_importance=0)
                with pytest.raises(ValueError, match="N_importance"):
                    npa.render_rays(rays, net, None, occupancy=grid, early_stop_eps=0.01, N_samples=8)
            with pytest.raises(ValueError, match="needs an occupancy grid"):
                npa.render_rays(rays, net, None, early_stop_eps=0.01, **kw)
            with pytest.raises(ValueError, match="needs an occupancy grid"):
                npa.render_rays(rays, net, lambda pts, vd, m: None, early_stop_eps=0.01, **kw)
            # what the grid path refuses stays refused, with its own error
            with pytest.raises(NotImplementedError, match="network_query_fn"):
                npa.render_rays(rays, net, lambda pts, vd, m: None, occupancy=dgrid, early_stop_eps=0.01, **kw)
            with pytest.raises(NotImplementedError, match="DenseNeRF"):
                npa.render_rays(rays, dense, None, occupancy=dgrid, early_stop_eps=0.01, N_samples=8, N_importance=8)
    with pytest.raises(NotImplementedError, match="plain OccupancyGrid"):       # grad mode on, parameters that require grad
        npa.render_rays(rays, net, None, occupancy=plain, early_stop_eps=0.01, **kw)
    # the public kernel wrapper and the definition check eps themselves
    z = torch.linspace(2.0, 6.0, 8).expand(3, 8)
    for fn in (npa.occupancy.stop_depth, npa.occupancy.stop_depth_reference):
        for bad in (0.0, 1.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="0 < eps < 1"):
                fn(z, torch.zeros(3, 8), bad)
    # through the layers that forward keywords: batchify_rays and render hand `early_stop_eps` to render_rays as they hand `occupancy`
    with pytest.raises(ValueError, match="0 < eps < 1"):
        npa.batchify_rays(rays, 4, network_fn=net, network_query_fn=None, occupancy=dgrid, early_stop_eps=1.0, **kw)
    K = np.array([[10.0, 0, 2.0], [0, 10.0, 2.0], [0, 0, 1]])
    with pytest.raises(ValueError, match="needs an occupancy grid"):
        npa.render(4, 4, K, chunk=8, rays=(rays[:, 0:3], rays[:, 3:6]), ndc=False, near=2.0, far=6.0, use_viewdirs=True, network_fn=net,
                   network_query_fn=None, early_stop_eps=0.5, **kw)


def test_the_empty_batch_reports_no_stopped_ray(monkeypatch):
    net, fine = npa.NeRF(**NET_KW), npa.NeRF(**NET_KW)
    dgrid = npa.DensityGrid(LO, HI, RES, device=CPU)
    monkeypatch.setattr(dgrid, "_desc", lambda: None)       # (the empty batch validates the grid's device; this grid lives on the CPU)
    kw = dict(N_samples=8, N_importance=16, network_fine=fine, occupancy=dgrid)
    out = npa.render_rays(_rays(0), net, None, early_stop_eps=0.01, **kw)
    assert set(out) == {"rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "z_std"} and out["rgb_map"].shape == (0, 3)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0, "rays_stopped": 0}
    npa.render_rays(_rays(0), net, None, early_stop_eps=0.01, clip_to_occupancy=True, proposal="grid", **kw)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0, "rays_hit": 0, "rays": 0, "rays_stopped": 0}
    # without the option the empty batch is what it was
    npa.render_rays(_rays(0), net, None, **kw)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0}
    npa.render_rays(_rays(0), net, None, early_stop_eps=None, **kw)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0}
