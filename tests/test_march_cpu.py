"""CPU: render_rays(proposal="march") without a GPU -- the export of nerf_occ_march, the definition of the marched depths
(OccupancyGrid.march_reference) against an explicit Python loop over fp32 scalars on a hand-made grid and hand-made rays, what the
definition promises on the ball scene, every guard on CPU tensors with nothing launched, and the keys and stats of the empty batch."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import nerf_oracle as orc
import nerf_pytorch_amd as npa
from test_gpu_occupancy import BOX_HI, BOX_LO, ball_mask, bits_equal

CPU = torch.device("cpu")
NET_KW = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
INF = float("inf")
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the rule, one scalar at a time
def loop_occupied(grid, mask, p):
    """OccupancyGrid.occupied for one point (three fp32 scalars): per axis one subtraction, one multiplication"""
    idx = []
    for a in range(3):
        t = f32(f32(p[a] - f32(grid.lo[a])) * f32(grid.scale[a]))
        if not (t >= 0 and t < f32(grid.resolution[a])):        # (a NaN is outside)
            return grid.outside == "evaluate"
        idx.append(int(np.floor(t)))
    return bool(mask[idx[0], idx[1], idx[2]])


def loop_march(grid, rays, u, M, S):
    """the definition of the issue, one ray and one candidate at a time in numpy fp32 scalars"""
    rays = np.asarray(rays, dtype=np.float32)
    mask = grid.to_mask().cpu().numpy()
    N = rays.shape[0]
    z_vals, z_stop, truncated = np.zeros((N, S), dtype=np.float32), np.zeros(N, dtype=np.float32), np.zeros(N, dtype=bool)
    with np.errstate(all="ignore"):
        for r in range(N):
            o, d, near, far = rays[r, 0:3], rays[r, 3:6], rays[r, 6], rays[r, 7]
            if not (np.isfinite(rays[r, :8]).all() and near < far):
                z_vals[r], z_stop[r] = far, -np.inf
                continue
            ur = f32(0.5) if u is None else f32(u[r])
            emitted, before = [], False
            for k in range(M):
                t = f32(f32(f32(k) + ur) / f32(M))
                z = f32(f32(near * f32(f32(1.0) - t)) + f32(far * t))
                keep = loop_occupied(grid, mask, [f32(o[a] + f32(d[a] * z)) for a in range(3)])
                if keep or before:          # before and not keep: the closing candidate
                    emitted.append(z)
                before = keep
            n = min(len(emitted), S - 1)
            truncated[r] = len(emitted) > S - 1
            z_stop[r] = emitted[S - 1] if truncated[r] else far
            z_vals[r, :n] = emitted[:n]
            z_vals[r, n:] = z_stop[r]
    return torch.from_numpy(z_vals), torch.from_numpy(z_stop), torch.from_numpy(truncated)


# the hand-made scene: an 8 x 2 x 1 grid over [0, 8] x [0, 2] x [0, 1]; row y = 0 is . # # . . # . . along x, row y = 1 is all occupied.
# A ray along +x from x = 0 with near 0, far 8 and M = 16 puts two candidates into every cell: z_k = (k + u) / 2.
HAND_LO, HAND_HI = (0.0, 0.0, 0.0), (8.0, 2.0, 1.0)
HAND_ROW = [0, 1, 1, 0, 0, 1, 0, 0]
HAND_RAYS = ("pattern row", "full row", "miss", "NaN component", "near == far", "near > far", "infinite direction", "starts outside the box")


def hand_grid(outside):
    mask = torch.zeros(8, 2, 1, dtype=torch.bool)
    mask[:, 0, 0] = torch.tensor(HAND_ROW, dtype=torch.bool)
    mask[:, 1, 0] = True
    return npa.OccupancyGrid.from_mask(mask, HAND_LO, HAND_HI, outside=outside, device=CPU)


def hand_rays():
    r = torch.zeros(len(HAND_RAYS), 11)
    r[:, 1], r[:, 2], r[:, 3], r[:, 7], r[:, 8] = 0.5, 0.5, 1.0, 8.0, 1.0
    r[1, 1] = 1.5
    r[2, 1] = 5.0
    r[3, 4] = float("nan")
    r[4, 6] = 8.0
    r[5, 6], r[5, 7] = 3.0, 1.0
    r[6, 5] = INF
    r[7, 0], r[7, 7] = -2.0, 12.0
    return r


@pytest.mark.parametrize("outside", ["skip", "evaluate"])
@pytest.mark.parametrize("M,S", [(16, 20), (16, 12), (16, 9), (16, 5), (16, 3), (16, 1), (7, 4), (1, 1), (1, 2), (65, 64)])
def test_march_reference_on_hand_made_rays_against_a_python_loop(M, S, outside):
    grid, rays = hand_grid(outside), hand_rays()
    g = torch.Generator().manual_seed(M * 100 + S)
    for u in (None, torch.rand(len(HAND_RAYS), generator=g), torch.zeros(len(HAND_RAYS))):
        got = grid.march_reference(rays, u, M, S)
        want = loop_march(grid, rays.numpy(), None if u is None else u.numpy(), M, S)
        assert got[0].dtype == torch.float32 and got[0].shape == (len(HAND_RAYS), S) and got[1].shape == got[2].shape == (len(HAND_RAYS),)
        assert got[2].dtype == torch.bool
        assert bits_equal(got[0], want[0]), (got[0], want[0])
        assert bits_equal(got[1], want[1]) and torch.equal(got[2], want[2])
    # u = None means 0.5 for every ray
    a, b = grid.march_reference(rays, None, M, S), grid.march_reference(rays, torch.full((len(HAND_RAYS),), 0.5), M, S)
    assert all(bits_equal(x.float(), y.float()) for x, y in zip(a, b))
    # tensors of other dtypes / with a graph are taken as values
    c = grid.march_reference(rays.double().requires_grad_(True), None, M, S)
    assert bits_equal(c[0], a[0]) and not c[0].requires_grad


def test_march_reference_spelt_out():
    """M = 16, u = 0.5: z_k = k / 2 + 0.25, all exact.  The pattern row keeps k = 2..5 and 10, 11 and closes its runs with k = 6 and 12."""
    grid, rays = hand_grid("skip"), hand_rays()
    zk = lambda k: k / 2 + 0.25
    row = lambda *ks: [zk(k) for k in ks]
    far = 8.0
    # two runs with a gap, everything fits: E = 8 <= S - 1 = 11; the closing samples 6 and 12 are there, the tail is `far`
    z, z_stop, tr = grid.march_reference(rays, None, 16, 12)
    assert z[0].tolist() == row(2, 3, 4, 5, 6, 10, 11, 12) + [far] * 4 and float(z_stop[0]) == far and not bool(tr[0])
    # E == S - 1 exactly: fits, one padded slot
    z, z_stop, tr = grid.march_reference(rays, None, 16, 9)
    assert z[0].tolist() == row(2, 3, 4, 5, 6, 10, 11, 12) + [far] and float(z_stop[0]) == far and not bool(tr[0])
    # the closing sample is the one that does not fit: S - 1 = 4 slots take k = 2..5, z_stop = z_6
    z, z_stop, tr = grid.march_reference(rays, None, 16, 5)
    assert z[0].tolist() == row(2, 3, 4, 5) + [zk(6)] and float(z_stop[0]) == zk(6) and bool(tr[0])
    # truncation inside a run: S - 1 = 2 slots take k = 2, 3, z_stop = z_4
    z, z_stop, tr = grid.march_reference(rays, None, 16, 3)
    assert z[0].tolist() == row(2, 3) + [zk(4)] and float(z_stop[0]) == zk(4) and bool(tr[0])
    # S = 1: nothing fits, the one slot holds the stop depth
    z, z_stop, tr = grid.march_reference(rays, None, 16, 1)
    assert z[:3, 0].tolist() == [zk(2), zk(0), far] and z_stop[:3].tolist() == [zk(2), zk(0), far] and tr[:3].tolist() == [True, True, False]
    # a fully occupied ray with M < S - 1: all 16 candidates, no closing sample (nothing lies behind the last candidate), then `far`
    z, z_stop, tr = grid.march_reference(rays, None, 16, 20)
    assert z[1].tolist() == row(*range(16)) + [far] * 4 and float(z_stop[1]) == far and not bool(tr[1])
    # a miss: the row is `far`, z_stop = far, not truncated -- the compaction drops every slot
    assert z[2].tolist() == [far] * 20 and float(z_stop[2]) == far and not bool(tr[2])
    # invalid rays: the row is the ray's own far, z_stop = -inf, not truncated
    for r, own_far in ((3, 8.0), (4, 8.0), (5, 1.0), (6, 8.0)):
        assert z[r].tolist() == [own_far] * 20 and float(z_stop[r]) == -INF and not bool(tr[r]), HAND_RAYS[r]
    # outside="evaluate": the stretch in front of the box (x in [-2, 0), far = 12, step 14 / 16) is walked like occupied space
    ev = hand_grid("evaluate").march_reference(rays, None, 16, 20)
    sk = grid.march_reference(rays, None, 16, 20)
    x = lambda zz: -2.0 + zz
    assert float(x(ev[0][7, 0])) < 0.0 and float(x(sk[0][7, 0])) >= 1.0
    with pytest.raises(ValueError):
        grid.march_reference(rays, None, 0, 4)
    with pytest.raises(ValueError):
        grid.march_reference(rays, None, 4, 0)


# ------------------------------------------------------------------------------------------------ what the definition promises
@pytest.fixture(scope="module")
def ball_scene():
    rays = orc.synthetic_rays(256, seed=21)
    M = 256
    k = torch.arange(M, dtype=torch.float32)[None, :]
    t = (k + 0.5) / torch.tensor(float(M))
    z_all = rays[:, 6:7] * (1.0 - t) + rays[:, 7:8] * t
    return rays, M, z_all


@pytest.mark.parametrize("outside,least", [("skip", {"miss": 16, "fit": 16, "truncated": 16}), ("evaluate", {"fit": 16, "truncated": 16})])
def test_properties_on_the_ball_scene(ball_scene, outside, least):
    rays, M, z_all = ball_scene
    S = 64
    grid = npa.OccupancyGrid.from_mask(ball_mask(), BOX_LO, BOX_HI, outside=outside, device=CPU)
    z, z_stop, tr = grid.march_reference(rays, None, M, S)
    occ_all = grid.occupied(rays[:, None, 0:3] + rays[:, None, 3:6] * z_all[:, :, None])
    # rows are nondecreasing
    assert bool((z[:, 1:] >= z[:, :-1]).all())
    # the evaluated samples: what nerf_occ_compact_stop keeps
    ev = grid.occupied(rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]) & ~(z >= z_stop[:, None])
    assert not bool(ev[:, -1].any())            # the last slot -- the reference's 1e10 interval -- is never evaluated
    # behind every evaluated sample sits the next candidate, or z_stop
    pos = (z_all[:, None, :] == z[:, :, None]).float().argmax(-1)           # the candidate index of every slot that holds one
    nxt = torch.cat([z_all, rays[:, 7:8]], -1).gather(1, (pos + 1).clamp(max=M))
    behind = torch.cat([z[:, 1:], z_stop[:, None]], -1)
    assert bool((behind == nxt)[ev].all()) and int(ev.sum()) > 1000        # (z_stop IS the next candidate where the row ends on a kept one)
    assert int((ev & (behind == z_stop[:, None])).sum()) > 0
    fits = ~tr
    # on the rays that are not truncated the evaluated set is exactly the occupied candidates
    n_ev, n_occ = ev.sum(-1), occ_all.sum(-1)
    assert torch.equal(n_ev[fits], n_occ[fits])
    for r in fits.nonzero()[:, 0].tolist():
        assert torch.equal(z[r][ev[r]], z_all[r][occ_all[r]])
    # on a truncated ray it is a prefix of them (all of them where only a closing sample did not fit)
    for r in tr.nonzero()[:, 0].tolist()[:32]:
        m = int(n_ev[r])
        assert 0 < m <= int(n_occ[r]) and torch.equal(z[r][ev[r]], z_all[r][occ_all[r]][:m])
    assert int((n_ev < n_occ)[tr].sum()) > 0
    miss = fits & (n_occ == 0)
    counts = {"miss": int(miss.sum()), "fit": int((fits & (n_occ > 0)).sum()), "truncated": int(tr.sum())}
    print(outside, counts)
    for k_, v in least.items():
        assert counts[k_] >= v, counts
    assert bool((z[miss] == rays[miss, 7:8]).all()) and bool((z_stop[~tr] == rays[~tr, 7]).all())
    # with room for everything no ray is truncated
    assert int(grid.march_reference(rays, None, M, 192)[2].sum()) == 0


# ------------------------------------------------------------------------------------------------ exports
def test_the_library_exports_and_binds_the_entry_point():
    hb = npa.hip_backend
    raw = ctypes.CDLL(npa.build.LIB_PATH)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_hip.h")) as f:
        header = f.read()
    assert hasattr(raw, "nerf_occ_march") and "nerf_occ_march" in hb.EXPORTS and "int nerf_occ_march(" in header
    assert "#define NERF_ABI_VERSION 10" in header and hb.ABI_VERSION == 10
    assert list(inspect.signature(hb.occ_march).parameters) == ["desc", "rays", "u", "n_steps", "n_slots"]
    assert list(inspect.signature(npa.OccupancyGrid.march).parameters) == ["self", "rays", "n_steps", "n_slots", "u"]
    L = hb.lib()
    assert L.nerf_abi_version() == 10
    # the limits, refused before anything is launched or read (host memory stands in for the device buffers)
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    desc = hb.NerfOccGrid((ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_int * 3)(2, 2, 2), 0, ptr)
    march = lambda rays, stride, n, M, S, out=ptr: L.nerf_occ_march(ctypes.byref(desc), rays, stride, None, n, M, S, out, ptr, ptr, None)
    assert march(None, 8, 1, 4, 4) != 0 and "null" in L.nerf_last_error().decode()
    assert march(ptr, 8, 1, 4, 4, None) != 0 and "null" in L.nerf_last_error().decode()
    for stride, n, M, S in ((7, 1, 4, 4), (8, -1, 4, 4), (8, 1, 0, 4), (8, 1, 16385, 4), (8, 1, 4, 0), (8, 1, 4, 4097)):
        assert march(ptr, stride, n, M, S) != 0 and "bad size" in L.nerf_last_error().decode(), (stride, n, M, S)
    assert march(ptr, 8, 0, 16384, 4096) == 0          # no rays: nothing to do (u is optional)
    grid = npa.OccupancyGrid(HAND_LO, HAND_HI, (8, 2, 1), device=CPU)
    for M, S in ((0, 4), (16385, 4), (4, 0), (4, 4097)):
        with pytest.raises(ValueError, match="n_steps"):
            grid.march(hand_rays(), M, S)


# ------------------------------------------------------------------------------------------------ guards
def _rays(n):
    gen = torch.Generator().manual_seed(1)
    o = torch.tensor([0.0, 1.0, 6.0]) + 0.1 * torch.randn(n, 3, generator=gen)
    d = torch.tensor([0.0, 0.0, -1.0]) + 0.1 * torch.randn(n, 3, generator=gen)
    return torch.cat([o, d, torch.full((n, 1), 2.0), torch.full((n, 1), 6.0), torch.nn.functional.normalize(d, dim=-1)], -1)


LO, HI, RES = (-1.0, 0.5, 2.0), (1.0, 2.0, 4.5), (4, 3, 5)


def test_march_steps_is_keyword_only_and_every_guard_fires_before_a_launch(monkeypatch):
    p = inspect.signature(npa.render_rays).parameters["march_steps"]
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
            with pytest.raises(ValueError, match="occupancy"):
                npa.render_rays(rays, net, None, proposal="march", march_steps=64, **kw)
            for grid in (dgrid, plain):
                with pytest.raises(ValueError, match="march_steps"):
                    npa.render_rays(rays, net, None, occupancy=grid, proposal="march", **kw)
                for bad in (0, -1, 16385, 64.0, "64", True, float("nan")):
                    with pytest.raises(ValueError, match="march_steps"):
                        npa.render_rays(rays, net, None, occupancy=grid, proposal="march", march_steps=bad, **kw)
                for other in (None, "grid"):
                    with pytest.raises(ValueError, match="march_steps"):
                        npa.render_rays(rays, net, None, occupancy=grid, proposal=other, march_steps=64, **kw)
                with pytest.raises(ValueError, match="early_stop_eps"):
                    npa.render_rays(rays, net, None, occupancy=grid, proposal="march", march_steps=64, early_stop_eps=0.01, **kw)
                with pytest.raises(ValueError, match="4096"):
                    npa.render_rays(rays, net, None, occupancy=grid, proposal="march", march_steps=64, N_samples=4000, N_importance=97)
                with pytest.raises(NotImplementedError, match="lindisp"):
                    npa.render_rays(rays, net, None, occupancy=grid, proposal="march", march_steps=64, lindisp=True, **kw)
                with pytest.raises(ValueError, match="proposal must be"):
                    npa.render_rays(rays, net, None, occupancy=grid, proposal="marching", **kw)
                # what the grid path refuses stays refused, with its own error
                with pytest.raises(NotImplementedError, match="network_query_fn"):
                    npa.render_rays(rays, net, lambda pts, vd, m: None, occupancy=grid, proposal="march", march_steps=64, **kw)
                with pytest.raises(NotImplementedError, match="DenseNeRF"):
                    npa.render_rays(rays, dense, None, occupancy=grid, proposal="march", march_steps=64, N_samples=8, N_importance=8)
    with pytest.raises(NotImplementedError, match="plain OccupancyGrid"):       # grad mode on, parameters that require grad
        npa.render_rays(rays, net, None, occupancy=plain, proposal="march", march_steps=64, **kw)
    # through the layers that forward keywords: batchify_rays and render hand `march_steps` to render_rays as they hand `occupancy`
    with pytest.raises(ValueError, match="march_steps"):
        npa.batchify_rays(rays, 4, network_fn=net, network_query_fn=None, occupancy=dgrid, proposal="march", march_steps=0, **kw)
    with pytest.raises(NotImplementedError, match="plain OccupancyGrid"):
        npa.batchify_rays(rays, 4, network_fn=net, network_query_fn=None, occupancy=plain, proposal="march", march_steps=16384, **kw)
    K = np.array([[10.0, 0, 2.0], [0, 10.0, 2.0], [0, 0, 1]])
    geo = dict(rays=(rays[:, 0:3], rays[:, 3:6]), ndc=False, near=2.0, far=6.0, use_viewdirs=True, network_fn=net, network_query_fn=None)
    with pytest.raises(ValueError, match="march_steps"):
        npa.render(4, 2, K, chunk=8, occupancy=dgrid, march_steps=64, **geo, **kw)
    with pytest.raises(NotImplementedError, match="lindisp"):
        npa.render(4, 2, K, chunk=8, occupancy=dgrid, proposal="march", march_steps=64, lindisp=True, **geo, **kw)


@pytest.mark.parametrize("retraw", [False, True])
def test_the_empty_batch_has_the_keys_and_stats_of_the_mode(monkeypatch, retraw):
    net, fine = npa.NeRF(**NET_KW), npa.NeRF(**NET_KW)
    dgrid = npa.DensityGrid(LO, HI, RES, device=CPU)
    monkeypatch.setattr(dgrid, "_desc", lambda: None)       # (the empty batch validates the grid's device; this grid lives on the CPU)
    kw = dict(N_samples=8, N_importance=16, network_fine=fine, retraw=retraw, occupancy=dgrid)
    out = npa.render_rays(_rays(0), net, None, proposal="march", march_steps=64, **kw)
    assert set(out) == {"rgb_map", "disp_map", "acc_map"} | ({"raw"} if retraw else set())
    assert out["rgb_map"].shape == (0, 3) and out["disp_map"].shape == (0,) and out["acc_map"].shape == (0,)
    if retraw:
        assert out["raw"].shape == (0, 24, 4)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0, "rays_truncated": 0}
    out = npa.render_rays(_rays(0), net, None, proposal="march", march_steps=64, clip_to_occupancy=True, **kw)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0, "rays_hit": 0, "rays": 0, "rays_truncated": 0}
    out = npa.render_rays(_rays(0), net, None, proposal="march", march_steps=64, **dict(kw, N_importance=0))
    assert set(out) == {"rgb_map", "disp_map", "acc_map"} | ({"raw"} if retraw else set())
    if retraw:
        assert out["raw"].shape == (0, 8, 4)
    # batchify_rays sums the stats of the mode (no chunk at all: the zeros it starts from)
    npa.batchify_rays(_rays(0), 4, network_fn=net, network_query_fn=None, proposal="march", march_steps=64, **kw)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0, "rays_truncated": 0}
    # without the option the empty batch is what it was
    out = npa.render_rays(_rays(0), net, None, **kw)
    assert set(out) == {"rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "z_std"} | ({"raw"} if retraw else set())
    assert dgrid.last_stats == {"evaluated": 0, "total": 0}
    out = npa.render_rays(_rays(0), net, None, proposal="grid", **kw)
    assert set(out) == {"rgb_map", "disp_map", "acc_map", "z_std"} | ({"raw"} if retraw else set())
    assert dgrid.last_stats == {"evaluated": 0, "total": 0}
