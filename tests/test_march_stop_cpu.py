"""CPU: render_rays(proposal="march", march_stop_eps=eps) without a GPU -- the export of nerf_occ_march_stop and its argument checks,
the definition (DensityGrid.march_stop_reference) against an explicit Python loop over numpy fp32 scalars with the 64-lane scan written
out lane by lane, on the hand-made 8 x 2 x 1 grid of tests/test_march_cpu.py with hand-set densities; what the definition promises on
the ball scene; every guard on CPU tensors with the library unreachable; the keys and stats of the empty batch."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import nerf_oracle as orc
import nerf_pytorch_amd as npa
from test_gpu_occupancy import BOX_HI, BOX_LO, ball_mask, bits_equal
from test_march_cpu import HAND_HI, HAND_LO, HAND_RAYS, LO, HI, NET_KW, RES, _rays, hand_grid, hand_rays

CPU = torch.device("cpu")
INF, NAN = float("inf"), float("nan")
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the rule, one scalar at a time
def loop_cell(grid, p):
    """the cell index (ix, iy, iz) of one point by OccupancyGrid's rule, or None outside the box (a NaN is outside)"""
    idx = []
    for a in range(3):
        t = f32(f32(p[a] - f32(grid.lo[a])) * f32(grid.scale[a]))
        if not (t >= 0 and t < f32(grid.resolution[a])):
            return None
        idx.append(int(np.floor(t)))
    return tuple(idx)


def loop_march_stop(grid, rays, u, M, S, eps):
    """the definition of the issue, one ray, one candidate and one lane at a time in numpy fp32 scalars.  Returns the four outputs and
    k_stop per ray (-1: none)"""
    rays = np.asarray(rays, dtype=np.float32)
    mask = grid.to_mask().cpu().numpy()
    density = grid.density.cpu().numpy().reshape(grid.resolution)
    outside_sigma = f32(grid.sigma_threshold) if grid.outside == "evaluate" else f32(0.0)
    tau = f32(-math.log(float(eps)))
    N = rays.shape[0]
    z_vals, z_stop = np.zeros((N, S), dtype=np.float32), np.zeros(N, dtype=np.float32)
    truncated, stopped, k_stops = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool), np.full(N, -1)
    with np.errstate(all="ignore"):
        for r in range(N):
            o, d, near, far = rays[r, 0:3], rays[r, 3:6], rays[r, 6], rays[r, 7]
            if not (np.isfinite(rays[r, :8]).all() and near < far):
                z_vals[r], z_stop[r] = far, -np.inf
                continue
            ur = f32(0.5) if u is None else f32(u[r])
            zs, keeps, sigmas = [], [], []
            for k in range(M):
                t = f32(f32(f32(k) + ur) / f32(M))
                z = f32(f32(near * f32(f32(1.0) - t)) + f32(far * t))
                cell = loop_cell(grid, [f32(o[a] + f32(d[a] * z)) for a in range(3)])
                if cell is None:
                    keep, sg = grid.outside == "evaluate", outside_sigma
                else:
                    keep = bool(mask[cell])
                    sg = f32(density[cell]) if keep else f32(0.0)
                zs.append(z), keeps.append(keep), sigmas.append(sg if sg > 0 else f32(0.0))       # (a NaN fails the comparison)
            dn = f32(np.sqrt(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))))
            c = [f32(sigmas[k] * f32(f32((zs[k + 1] if k + 1 < M else far) - zs[k]) * dn)) if keeps[k] else f32(0.0) for k in range(M)]
            # the exclusive prefix sum in the order of the wave scan
            A, base = [], f32(0.0)
            for k0 in range(0, M, 64):
                v = [c[k0 + l] if k0 + l < M else f32(0.0) for l in range(64)]
                for step in (1, 2, 4, 8, 16, 32):
                    prev = list(v)
                    for l in range(step, 64):
                        v[l] = f32(prev[l] + prev[l - step])
                for l in range(64):
                    A.append(f32(base + (v[l - 1] if l > 0 else f32(0.0))))
                base = f32(base + v[63])
            k_stop = next((k for k in range(M) if A[k] >= tau), None)
            emitted, before = [], False
            for k in range(M if k_stop is None else k_stop):
                if keeps[k] or before:
                    emitted.append(zs[k])
                before = keeps[k]
            n = min(len(emitted), S - 1)
            truncated[r] = len(emitted) > S - 1
            if truncated[r]:
                z_stop[r] = emitted[S - 1]
            elif k_stop is not None:
                z_stop[r], stopped[r] = zs[k_stop], True
            else:
                z_stop[r] = far
            k_stops[r] = -1 if k_stop is None else k_stop
            z_vals[r, :n] = emitted[:n]
            z_vals[r, n:] = z_stop[r]
    return torch.from_numpy(z_vals), torch.from_numpy(z_stop), torch.from_numpy(truncated), torch.from_numpy(stopped), k_stops


# The hand-made scene of tests/test_march_cpu.py -- an 8 x 2 x 1 grid over [0, 8] x [0, 2] x [0, 1], row y = 0 is . # # . . # . . along x,
# row y = 1 all occupied -- with one density per cell, and two more rays:
#   "closing cut": along +x from x = -2 with near 0, far 65 / 8: at M = 65 the step is 1 / 8, candidates 56 .. 63 lie in cell 5 of the
#                  pattern row and candidate 64 (lane 0 of the second round) in the empty cell 6: a closing candidate;
#   "d = 0":       every candidate is the point (3.5, 1.5, 0.5), cell 3 of the full row.
RAYS = HAND_RAYS + ("closing cut", "d = 0")
EPS = 1e-2          # tau = 4.60517


def stop_rays():
    extra = torch.zeros(2, 11)
    extra[:, 1], extra[:, 2], extra[:, 7], extra[:, 8] = 0.5, 0.5, 8.0, 1.0
    extra[0, 0], extra[0, 3], extra[0, 7] = -2.0, 1.0, 65.0 / 8.0
    extra[1, 0], extra[1, 1] = 3.5, 1.5
    return torch.cat([hand_rays(), extra], 0)


DENSITIES = {
    # 4 per cell: a kept candidate of the M = 16 rays (interval 1 / 2) adds 2
    "run": ([4.0] * 8, [4.0] * 8),
    # pattern row: 0, a negative value, and 5 in cell 5 (eight candidates of "closing cut" at 5 / 8 each: A_63 = 4.375 < tau <= A_64 = 5);
    # full row: 0.6 (sixteen candidates at 0.3: A_15 = 4.5 < tau, the whole sum 4.8 reaches it only behind the last candidate)
    "late": ([0.0, 0.0, -3.0, 0.0, 0.0, 5.0, 0.0, 0.0], [0.6] * 8),
    # a NaN cell in front of a cell of 4; an infinite cell (pattern row: A = inf stops; the d = 0 ray: inf * 0 = NaN never stops)
    "odd": ([0.0, NAN, 4.0, 0.0, 0.0, INF, 0.0, 0.0], [0.0, 0.0, 0.0, INF, 0.0, 0.0, 0.0, 0.0]),
    "zero": ([0.0] * 8, [0.0] * 8),
}


def hand_dgrid(outside, densities):
    g = npa.DensityGrid(HAND_LO, HAND_HI, (8, 2, 1), outside=outside, device=CPU)
    g.bits = hand_grid(outside).bits.clone()
    d = torch.zeros(8, 2, 1)
    d[:, 0, 0], d[:, 1, 0] = torch.tensor(DENSITIES[densities][0]), torch.tensor(DENSITIES[densities][1])
    g.density = d.reshape(-1).contiguous()
    return g


@pytest.mark.parametrize("outside", ["skip", "evaluate"])
@pytest.mark.parametrize("densities", sorted(DENSITIES))
@pytest.mark.parametrize("M,S", [(16, 20), (16, 5), (16, 4), (16, 3), (16, 1), (7, 4), (1, 1), (1, 2), (65, 64), (65, 30), (130, 64)])
def test_march_stop_reference_on_hand_made_rays_against_a_python_loop(M, S, densities, outside):
    grid, rays = hand_dgrid(outside, densities), stop_rays()
    g = torch.Generator().manual_seed(M * 100 + S)
    for u in (None, torch.rand(len(RAYS), generator=g), torch.zeros(len(RAYS))):
        got = grid.march_stop_reference(rays, u, M, S, EPS)
        want = loop_march_stop(grid, rays.numpy(), None if u is None else u.numpy(), M, S, EPS)
        assert got[0].dtype == torch.float32 and got[0].shape == (len(RAYS), S) and got[1].shape == got[2].shape == got[3].shape == (len(RAYS),)
        assert got[2].dtype == got[3].dtype == torch.bool
        assert bits_equal(got[0], want[0]), (got[0], want[0])
        assert bits_equal(got[1], want[1]) and torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
        assert not bool((got[2] & got[3]).any())
        if densities == "zero":         # a grid that was never updated: march_reference, bit for bit
            plain = grid.march_reference(rays, u, M, S)
            assert all(bits_equal(a.float(), b.float()) for a, b in zip(got[:3], plain)) and not bool(got[3].any())
    a, b = grid.march_stop_reference(rays, None, M, S, EPS), grid.march_stop_reference(rays, torch.full((len(RAYS),), 0.5), M, S, EPS)
    assert all(bits_equal(x.float(), y.float()) for x, y in zip(a, b))
    c = grid.march_stop_reference(rays.double().requires_grad_(True), None, M, S, EPS)
    assert bits_equal(c[0], a[0]) and not c[0].requires_grad


def test_march_stop_reference_spelt_out():
    """u = 0.5 (None).  M = 16: z_k = k / 2 + 0.25 and every interval is 1 / 2, all exact."""
    rays = stop_rays()
    zk = lambda k: k / 2 + 0.25
    row = lambda *ks: [zk(k) for k in ks]
    far = 8.0
    run = hand_dgrid("skip", "run")
    # a stop inside a run: the pattern row keeps k = 2 .. 5 at c = 2: A_3 = 2, A_4 = 4, A_5 = 6 >= tau: k = 2, 3, 4 are emitted
    z, z_stop, tr, st = run.march_stop_reference(rays, None, 16, 12, EPS)
    assert z[0].tolist() == row(2, 3, 4) + [zk(5)] * 9 and float(z_stop[0]) == zk(5) and bool(st[0]) and not bool(tr[0])
    # the full row: A_k = 2 k, k_stop = 3, E = 3.  S - 1 = 3: the cut comes first
    z, z_stop, tr, st = run.march_stop_reference(rays, None, 16, 4, EPS)
    assert z[1].tolist() == row(0, 1, 2) + [zk(3)] and float(z_stop[1]) == zk(3) and bool(st[1]) and not bool(tr[1])
    # ... S - 1 = 2: candidate 2 does not fit, in the round of the cut and in front of it: truncated, not stopped
    z, z_stop, tr, st = run.march_stop_reference(rays, None, 16, 3, EPS)
    assert z[1].tolist() == row(0, 1) + [zk(2)] and float(z_stop[1]) == zk(2) and bool(tr[1]) and not bool(st[1])
    # S = 1: whatever emits is truncated (k_stop - 1 is a kept candidate: something is always emitted in front of a cut)
    z, z_stop, tr, st = run.march_stop_reference(rays, None, 16, 1, EPS)
    assert z[:3, 0].tolist() == [zk(2), zk(0), far] and tr[:3].tolist() == [True, True, False] and not bool(st.any())
    # a miss and the invalid rays are march_reference's
    z, z_stop, tr, st = run.march_stop_reference(rays, None, 16, 20, EPS)
    assert z[2].tolist() == [far] * 20 and float(z_stop[2]) == far and not bool(tr[2]) and not bool(st[2])
    for r, own_far in ((3, 8.0), (4, 8.0), (5, 1.0), (6, 8.0)):
        assert z[r].tolist() == [own_far] * 20 and float(z_stop[r]) == -INF and not bool(tr[r]) and not bool(st[r]), RAYS[r]
    # the d = 0 ray: every interval is 0 * |d| = 0: it never stops, whatever the (finite) density
    assert not bool(st[9]) and z[9].tolist() == [zk(k) for k in range(16)] + [far] * 4

    late = hand_dgrid("skip", "late")
    # A reaches tau only behind the last candidate: nothing changes
    got, plain = late.march_stop_reference(rays, None, 16, 20, EPS), late.march_reference(rays, None, 16, 20)
    assert all(bits_equal(a[1:2].float(), b[1:2].float()) for a, b in zip(got[:3], plain)) and not bool(got[3][1])
    # 0 and a negative density add nothing: the pattern row's first run (k = 2 .. 5) does not move A; cell 5 (k = 10, 11 at 2.5) does
    assert got[0][0].tolist() == row(2, 3, 4, 5, 6, 10, 11) + [zk(12)] * 13 and bool(got[3][0]) and float(got[1][0]) == zk(12)
    # the cut at a closing candidate, lane 0 of the second round: M = 65, candidates 56 .. 63 in cell 5, candidate 64 in the empty cell 6
    for outside in ("skip", "evaluate"):
        late = hand_dgrid(outside, "late")
        z, z_stop, tr, st = late.march_stop_reference(rays, None, 65, 64, EPS)
        want = loop_march_stop(late, rays.numpy(), None, 65, 64, EPS)
        assert int(want[4][8]) == 64 and bool(st[8]) and not bool(tr[8])
        z64 = f32(f32(f32(0.0) * f32(f32(1.0) - f32(f32(64.5) / f32(65.0)))) + f32(f32(65.0 / 8.0) * f32(f32(64.5) / f32(65.0))))
        assert float(z_stop[8]) == float(z64)
        assert not bool(late.occupied(rays[8:9, 0:3] + rays[8:9, 3:6] * z_stop[8])[0])            # a closing candidate
        n = int((z[8] < z_stop[8]).sum())
        assert late.occupied(rays[8:9, 0:3] + rays[8:9, 3:6] * z[8, n - 1])[0]                      # behind a kept one

    odd = hand_dgrid("skip", "odd")
    z, z_stop, tr, st = odd.march_stop_reference(rays, None, 16, 20, EPS)
    # the NaN cell (k = 2, 3) counts as 0, cell 2 (k = 4, 5) adds 2 + 2, cell 5 (k = 10) adds inf: the stop is at k = 11
    assert z[0].tolist() == row(2, 3, 4, 5, 6, 10) + [zk(11)] * 14 and bool(st[0]) and float(z_stop[0]) == zk(11)
    # inf * 0 is a NaN: the d = 0 ray in the infinite cell never stops
    assert not bool(st[9]) and float(z_stop[9]) == far and z[9].tolist() == [zk(k) for k in range(16)] + [far] * 4
    with pytest.raises(ValueError):
        odd.march_stop_reference(rays, None, 0, 4, EPS)
    with pytest.raises(ValueError):
        odd.march_stop_reference(rays, None, 4, 0, EPS)
    for bad in (0.0, 1.0, -0.1, NAN, True, 1, "0.01", None):
        with pytest.raises(ValueError, match="march_stop_eps"):
            odd.march_stop_reference(rays, None, 4, 4, bad)


# ------------------------------------------------------------------------------------------------ what the definition promises
def ball_density_grid(outside, scale=4.0, seed=5, device=CPU):
    """the 32^3 ball of tests/test_gpu_occupancy.py as a DensityGrid with density = scale * (0.25 + 1.5 * rand) inside the ball"""
    mask = ball_mask()
    g = npa.DensityGrid(BOX_LO, BOX_HI, tuple(mask.shape), outside=outside, device=device)
    g.bits = npa.OccupancyGrid.from_mask(mask, BOX_LO, BOX_HI, device=device).bits.clone()
    rand = torch.rand(mask.shape, generator=torch.Generator().manual_seed(seed))
    g.density = torch.where(mask, scale * (0.25 + 1.5 * rand), torch.zeros(())).to(torch.float32).reshape(-1).contiguous().to(device)
    return g


@pytest.mark.parametrize("outside,least", [("skip", {"stopped": 16, "truncated": 16, "fit": 16, "miss": 16}),
                                           ("evaluate", {"stopped": 16, "truncated": 16, "fit": 16})])
def test_properties_on_the_ball_scene(outside, least):
    rays = orc.synthetic_rays(256, seed=21)
    M, S, eps = 256, 64, 1e-2
    grid = ball_density_grid(outside)
    z, z_stop, tr, st = grid.march_stop_reference(rays, None, M, S, eps)
    plain = grid.march_reference(rays, None, M, S)
    k = torch.arange(M, dtype=torch.float32)[None, :]
    t = (k + 0.5) / torch.tensor(float(M))
    z_all = rays[:, 6:7] * (1.0 - t) + rays[:, 7:8] * t
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z_all[:, :, None]
    keep = grid.occupied(pts)
    assert bool((z[:, 1:] >= z[:, :-1]).all())
    assert not bool((tr & st).any())
    # the optical depth in float64, summed sequentially: A64[:, k] = the sum over the candidates in front of k
    z_next = torch.cat([z_all[:, 1:], rays[:, 7:8]], -1)
    sigma = grid.proposal_sigma(pts).double().clamp(min=0.0)
    c = torch.where(keep, sigma * (z_next.double() - z_all.double()) * rays[:, 3:6].double().norm(dim=-1, keepdim=True), torch.zeros((), dtype=torch.float64))
    A64 = torch.cat([torch.zeros(rays.shape[0], 1, dtype=torch.float64), torch.cumsum(c, -1)], -1)        # [N, M + 1]
    n_stopped = 0
    for r in st.nonzero()[:, 0].tolist():
        at = (z_all[r] == z_stop[r]).nonzero()[:, 0]
        assert at.numel() == 1
        ks = int(at[0])
        assert ks >= 1 and bool(keep[r, ks - 1])                                # z_stop is the depth of a candidate behind a kept one
        assert math.exp(-float(A64[r, ks])) <= eps * (1 + 1e-5), (r, ks, math.exp(-float(A64[r, ks])))
        assert math.exp(-float(A64[r, ks - 1])) > eps * (1 - 1e-5), (r, ks, math.exp(-float(A64[r, ks - 1])))
        # in front of the stop the row is the plain march's; behind it the padding
        n = int((z[r] < z_stop[r]).sum())
        assert bits_equal(z[r, :n], plain[0][r, :n]) and bool((z[r, n:] == z_stop[r]).all())
        n_stopped += 1
    # a ray that neither stops nor is truncated never reached tau, and is the plain march's ray
    quiet = ~st & ~tr
    assert bool((A64[quiet][:, :M].max(-1).values < -math.log(eps) * (1 + 1e-5)).all())
    assert bits_equal(z[quiet], plain[0][quiet]) and bits_equal(z_stop[quiet], plain[1][quiet]) and not bool(plain[2][quiet].any())
    miss = quiet & ~keep.any(-1)
    counts = {"stopped": n_stopped, "truncated": int(tr.sum()), "fit": int((quiet & keep.any(-1)).sum()), "miss": int(miss.sum())}
    print(outside, counts, "truncated without the stop:", int(plain[2].sum()))
    for k_, v in least.items():
        assert counts[k_] >= v, counts
    assert counts["truncated"] < int(plain[2].sum())
    assert not bool((tr & ~plain[2]).any())             # the stop truncates no ray that fitted
    # density == 0: the plain march, bit for bit, nothing stopped
    grid.density = torch.zeros_like(grid.density)
    zero = grid.march_stop_reference(rays, None, M, S, eps)
    assert all(bits_equal(a.float(), b.float()) for a, b in zip(zero[:3], plain)) and not bool(zero[3].any())


# ------------------------------------------------------------------------------------------------ exports
def test_the_library_exports_and_binds_the_entry_point():
    hb = npa.hip_backend
    raw = ctypes.CDLL(npa.build.LIB_PATH)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_hip.h")) as f:
        header = f.read()
    assert hasattr(raw, "nerf_occ_march_stop") and "nerf_occ_march_stop" in hb.EXPORTS and "int nerf_occ_march_stop(" in header
    assert "#define NERF_ABI_VERSION 10" in header and hb.ABI_VERSION == 10
    assert list(inspect.signature(hb.occ_march_stop).parameters) == ["desc", "density", "outside_sigma", "rays", "u", "n_steps", "n_slots", "eps"]
    assert list(inspect.signature(npa.DensityGrid.march_stop).parameters) == ["self", "rays", "n_steps", "n_slots", "eps", "u"]
    assert not hasattr(npa.OccupancyGrid, "march_stop") and not hasattr(npa.OccupancyGrid, "march_stop_reference")
    assert hb.march_stop_threshold(1e-2) == float(f32(-math.log(1e-2)))
    L = hb.lib()
    assert L.nerf_abi_version() == 10
    # the limits, refused before anything is launched or read (host memory stands in for the device buffers)
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    desc = hb.NerfOccGrid((ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_int * 3)(2, 2, 2), 0, ptr)

    def call(stride=8, n=1, M=4, S=4, tau=1.0, **null):
        a = dict(density=ptr, rays=ptr, z_vals=ptr, z_stop=ptr, truncated=ptr, stopped=ptr)
        a.update(null)
        return L.nerf_occ_march_stop(ctypes.byref(desc), a["density"], 0.0, a["rays"], stride, None, n, M, S, tau, a["z_vals"], a["z_stop"],
                                     a["truncated"], a["stopped"], None)
    for name in ("density", "rays", "z_vals", "z_stop", "truncated", "stopped"):
        assert call(**{name: None}) != 0 and "null" in L.nerf_last_error().decode(), name
    assert L.nerf_occ_march_stop(None, ptr, 0.0, ptr, 8, None, 1, 4, 4, 1.0, ptr, ptr, ptr, ptr, None) != 0 and "null" in L.nerf_last_error().decode()
    for kw in (dict(stride=7), dict(n=-1), dict(M=0), dict(M=16385), dict(S=0), dict(S=4097)):
        assert call(**kw) != 0 and "bad size" in L.nerf_last_error().decode(), kw
    for tau in (0.0, -1.0, NAN):
        assert call(tau=tau) != 0 and "tau" in L.nerf_last_error().decode(), tau
    assert call(n=0, M=16384, S=4096) == 0          # no rays: nothing to do (u is optional)
    grid = npa.DensityGrid(HAND_LO, HAND_HI, (8, 2, 1), device=CPU)
    for M, S in ((0, 4), (16385, 4), (4, 0), (4, 4097)):
        with pytest.raises(ValueError, match="n_steps"):
            grid.march_stop(stop_rays(), M, S, 0.01)
    for bad in (0.0, 1.0, NAN, True, 1):
        with pytest.raises(ValueError, match="march_stop_eps"):
            grid.march_stop(stop_rays(), 4, 4, bad)


# ------------------------------------------------------------------------------------------------ guards
def test_march_stop_eps_is_keyword_only_and_every_guard_fires_before_a_launch(monkeypatch):
    for fn in (npa.render_rays,):
        p = inspect.signature(fn).parameters["march_stop_eps"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    net, fine = npa.NeRF(**NET_KW), npa.NeRF(**NET_KW)
    monkeypatch.setattr(npa.hip_backend, "lib", lambda: pytest.fail("a guard let a call reach the library"))
    rays = _rays(8)
    dgrid = npa.DensityGrid(LO, HI, RES, device=CPU)
    plain = npa.OccupancyGrid(LO, HI, RES, device=CPU)
    kw = dict(N_samples=8, N_importance=8, network_fine=fine)
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            # the option without the march
            for other in (None, "grid"):
                with pytest.raises(ValueError, match="march_stop_eps belongs"):
                    npa.render_rays(rays, net, None, occupancy=dgrid, proposal=other, march_stop_eps=0.01, **kw)
            with pytest.raises(ValueError, match="march_stop_eps belongs"):
                npa.render_rays(rays, net, None, march_stop_eps=0.01, **kw)
            # a value that is not a float in (0, 1)
            for bad in (0.0, 1.0, -0.5, 2.0, NAN, True, False, 1, 0, "0.01", torch.tensor(0.01)):
                with pytest.raises(ValueError, match="march_stop_eps must be a float"):
                    npa.render_rays(rays, net, None, occupancy=dgrid, proposal="march", march_steps=64, march_stop_eps=bad, **kw)
            # a plain OccupancyGrid has no densities: the message form of proposal="grid"
            with pytest.raises(ValueError, match="reads the densities of an occupancy.DensityGrid.*a plain OccupancyGrid has none"):
                npa.render_rays(rays, net, None, occupancy=plain, proposal="march", march_steps=64, march_stop_eps=0.01, **kw)
            # what the march refuses stays refused, with its own error
            with pytest.raises(ValueError, match="early_stop_eps together with"):
                npa.render_rays(rays, net, None, occupancy=dgrid, proposal="march", march_steps=64, march_stop_eps=0.01, early_stop_eps=0.01, **kw)
            with pytest.raises(ValueError, match="march_steps"):
                npa.render_rays(rays, net, None, occupancy=dgrid, proposal="march", march_stop_eps=0.01, **kw)
            with pytest.raises(NotImplementedError, match="lindisp"):
                npa.render_rays(rays, net, None, occupancy=dgrid, proposal="march", march_steps=64, march_stop_eps=0.01, lindisp=True, **kw)
            with pytest.raises(NotImplementedError, match="network_query_fn"):
                npa.render_rays(rays, net, lambda pts, vd, m: None, occupancy=dgrid, proposal="march", march_steps=64, march_stop_eps=0.01, **kw)
    # through the layers that forward keywords
    with pytest.raises(ValueError, match="march_stop_eps must be a float"):
        npa.batchify_rays(rays, 4, network_fn=net, network_query_fn=None, occupancy=dgrid, proposal="march", march_steps=64, march_stop_eps=1.0, **kw)
    K = np.array([[10.0, 0, 2.0], [0, 10.0, 2.0], [0, 0, 1]])
    geo = dict(rays=(rays[:, 0:3], rays[:, 3:6]), ndc=False, near=2.0, far=6.0, use_viewdirs=True, network_fn=net, network_query_fn=None)
    with pytest.raises(ValueError, match="march_stop_eps belongs"):
        npa.render(4, 2, K, chunk=8, occupancy=dgrid, march_stop_eps=0.01, **geo, **kw)
    with pytest.raises(ValueError, match="a plain OccupancyGrid has none"):
        npa.render(4, 2, K, chunk=8, occupancy=plain, proposal="march", march_steps=64, march_stop_eps=0.01, **geo, **kw)


@pytest.mark.parametrize("retraw", [False, True])
def test_the_empty_batch_has_the_keys_and_stats_of_the_mode(monkeypatch, retraw):
    net, fine = npa.NeRF(**NET_KW), npa.NeRF(**NET_KW)
    dgrid = npa.DensityGrid(LO, HI, RES, device=CPU)
    monkeypatch.setattr(dgrid, "_desc", lambda: None)       # (the empty batch validates the grid's device; this grid lives on the CPU)
    kw = dict(N_samples=8, N_importance=16, network_fine=fine, retraw=retraw, occupancy=dgrid, proposal="march", march_steps=64)
    out = npa.render_rays(_rays(0), net, None, march_stop_eps=0.01, **kw)
    assert set(out) == {"rgb_map", "disp_map", "acc_map"} | ({"raw"} if retraw else set())
    assert out["rgb_map"].shape == (0, 3) and out["disp_map"].shape == (0,) and out["acc_map"].shape == (0,)
    if retraw:
        assert out["raw"].shape == (0, 24, 4)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0, "rays_truncated": 0, "rays_stopped": 0}
    npa.render_rays(_rays(0), net, None, march_stop_eps=0.01, clip_to_occupancy=True, **kw)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0, "rays_hit": 0, "rays": 0, "rays_truncated": 0, "rays_stopped": 0}
    # batchify_rays sums the stats of the mode (no chunk at all: the zeros it starts from)
    npa.batchify_rays(_rays(0), 4, network_fn=net, network_query_fn=None, march_stop_eps=0.01, **kw)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0, "rays_truncated": 0, "rays_stopped": 0}
    # without the option the empty batch is what it was
    npa.render_rays(_rays(0), net, None, march_stop_eps=None, **kw)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0, "rays_truncated": 0}
