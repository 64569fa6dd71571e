"""CPU: render_rays(proposal="march", march_step_size=ds, march_fit=J) without a GPU -- the export of nerf_occ_march_step and its
argument checks, both definitions (OccupancyGrid.march_step_reference, DensityGrid.march_step_stop_reference) against an explicit
Python loop over numpy fp32 scalars on the hand-made 8 x 2 x 1 grid of tests/test_march_cpu.py, the equality with march_reference on
a power-of-two geometry, a doubling spelt out by hand, what the definitions promise on the ball scene, every guard on CPU tensors with
the library unreachable, and the keys and stats of the empty batch."""
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
from test_march_cpu import HAND_HI, HAND_LO, HAND_RAYS, LO, HI, NET_KW, RES, _rays, hand_grid, hand_rays, loop_occupied
from test_march_stop_cpu import DENSITIES, hand_dgrid, loop_cell

CPU = torch.device("cpu")
INF, NAN = float("inf"), float("nan")
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the rule, one scalar at a time
def loop_march_step(grid, rays, u, ds, M, S, fit, eps=None):
    """the definition of the issue, one ray, one level, one candidate (and one lane of the scan) at a time in numpy fp32 scalars.
    eps None: the plain form.  Returns (z_vals, z_stop, truncated, level, stopped)."""
    rays = np.asarray(rays, dtype=np.float32)
    mask = grid.to_mask().cpu().numpy()
    if eps is not None:
        density = grid.density.cpu().numpy().reshape(grid.resolution)
        outside_sigma = f32(grid.sigma_threshold) if grid.outside == "evaluate" else f32(0.0)
        tau = f32(-math.log(float(eps)))
    N = rays.shape[0]
    z_vals, z_stop = np.zeros((N, S), dtype=np.float32), np.zeros(N, dtype=np.float32)
    truncated, stopped, level = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool), np.zeros(N, dtype=np.int32)
    with np.errstate(all="ignore"):
        for r in range(N):
            o, d, near, far = rays[r, 0:3], rays[r, 3:6], rays[r, 6], rays[r, 7]
            dn = f32(np.sqrt(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))))
            dz0 = f32(f32(ds) / dn)
            if not (np.isfinite(rays[r, :8]).all() and near < far and dz0 > 0 and np.isfinite(dz0)):
                z_vals[r], z_stop[r] = far, -np.inf
                continue
            ur = f32(0.5) if u is None else f32(u[r])
            for j in range(fit + 1):
                dz = f32(dz0 * f32(2 ** j))
                zs, valid, keeps, sigmas = [], [], [], []
                for k in range(M):
                    z = f32(near + f32(f32(f32(k) + ur) * dz))
                    v = bool(z < far)
                    p = [f32(o[a] + f32(d[a] * z)) for a in range(3)]
                    keep = v and loop_occupied(grid, mask, p)
                    sg = f32(0.0)
                    if eps is not None and keep:
                        cell = loop_cell(grid, p)
                        sg = outside_sigma if cell is None else f32(density[cell])
                    zs.append(z), valid.append(v), keeps.append(keep), sigmas.append(sg if sg > 0 else f32(0.0))     # (a NaN: 0)
                k_stop = None
                if eps is not None:
                    nxt = lambda k: zs[k + 1] if k + 1 < M and valid[k + 1] else far
                    c = [f32(sigmas[k] * f32(f32(nxt(k) - zs[k]) * dn)) if keeps[k] else f32(0.0) for k in range(M)]
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
                    k_stop = next((k for k in range(M) if valid[k] and A[k] >= tau), None)
                emitted, before = [], False
                for k in range(M if k_stop is None else k_stop):
                    if valid[k] and (keeps[k] or before):
                        emitted.append(zs[k])
                    before = keeps[k]
                trunc = len(emitted) > S - 1
                if not trunc:
                    break
            n = min(len(emitted), S - 1)
            truncated[r], level[r] = trunc, j
            if trunc:
                z_stop[r] = emitted[S - 1]
            elif k_stop is not None:
                z_stop[r], stopped[r] = zs[k_stop], True
            else:
                z_stop[r] = far
            z_vals[r, :n] = emitted[:n]
            z_vals[r, n:] = z_stop[r]
    return tuple(torch.from_numpy(a) for a in (z_vals, z_stop, truncated, level, stopped))


# The hand-made scene of tests/test_march_cpu.py -- an 8 x 2 x 1 grid over [0, 8] x [0, 2] x [0, 1], row y = 0 is . # # . . # . . along x,
# row y = 1 all occupied -- its eight rays (pattern row, full row, miss, NaN component, near == far, near > far, infinite direction,
# starts outside the box) and three more:
#   "d = 0":        every candidate would be the point (3.5, 1.5, 0.5): there is no step, the ray is invalid;
#   "fast":         the full row with d = (2, 0, 0) and far = 4: the same points at half the depths, dz0 = ds / 2;
#   "tilted":       from (0.25, 0.25, 0.5) along (1, 0.2, 0): |d| is no power of two, the ray changes rows at x = 4 and leaves through y = 2
#                   at x = 9 (never: far = 7.5 ends it inside).
STEP_RAYS = HAND_RAYS + ("d = 0", "fast", "tilted")


def step_rays():
    extra = torch.zeros(3, 11)
    extra[:, 1], extra[:, 2], extra[:, 7], extra[:, 8] = 1.5, 0.5, 8.0, 1.0
    extra[0, 0] = 3.5
    extra[1, 3], extra[1, 7] = 2.0, 4.0
    extra[2, 0], extra[2, 1], extra[2, 3], extra[2, 4], extra[2, 7] = 0.25, 0.25, 1.0, 0.2, 7.5
    return torch.cat([hand_rays(), extra], 0)


def assert_same(got, want, what):
    assert bits_equal(got[0], want[0]), (what, got[0], want[0])
    assert bits_equal(got[1], want[1]), (what, got[1], want[1])
    assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3]), (what, got[2], want[2], got[3], want[3])
    if len(got) > 4:
        assert torch.equal(got[4], want[4]), (what, got[4], want[4])


SHAPES = [(16, 20), (16, 12), (16, 9), (16, 5), (16, 3), (16, 1), (7, 4), (1, 1), (1, 2), (65, 64), (40, 9)]


@pytest.mark.parametrize("outside", ["skip", "evaluate"])
@pytest.mark.parametrize("fit", [0, 1, 3])
@pytest.mark.parametrize("ds", [0.5, 0.25, 0.37])
def test_march_step_reference_on_hand_made_rays_against_a_python_loop(ds, fit, outside):
    """a miss, a full row, two runs with a gap, truncation inside a run (S = 3), the closing candidate the one that does not fit (S = 5),
    S = 1, the cap M biting before far (M = 7, M = 1), u None / 0 / random, NaN and infinite components, near >= far, d = 0, a ray that
    starts outside the box"""
    grid, rays = hand_grid(outside), step_rays()
    n = len(STEP_RAYS)
    levels = set()
    for M, S in SHAPES:
        g = torch.Generator().manual_seed(M * 100 + S)
        for u in (None, torch.rand(n, generator=g), torch.zeros(n)):
            got = grid.march_step_reference(rays, u, ds, M, S, fit)
            want = loop_march_step(grid, rays.numpy(), None if u is None else u.numpy(), ds, M, S, fit)
            assert len(got) == 4 and got[0].dtype == torch.float32 and got[0].shape == (n, S)
            assert got[1].shape == got[2].shape == got[3].shape == (n,) and got[2].dtype == torch.bool and got[3].dtype == torch.int32
            assert_same(got, want[:4], (M, S, u))
            levels |= set(got[3].tolist())
            # the invalid rays: own far, -inf, no flag, level 0
            for r, own_far in ((3, 8.0), (4, 8.0), (5, 1.0), (6, 8.0), (8, 8.0)):
                assert got[0][r].tolist() == [own_far] * S and float(got[1][r]) == -INF and not bool(got[2][r]) and int(got[3][r]) == 0
            assert int(got[3].max()) <= fit and bool((got[3][got[2]] == fit).all())       # a truncated ray has used every level
        a, b = grid.march_step_reference(rays, None, ds, M, S, fit), grid.march_step_reference(rays, torch.full((n,), 0.5), ds, M, S, fit)
        assert_same(a, b, "u = None is 0.5")
        c = grid.march_step_reference(rays.double().requires_grad_(True), None, ds, M, S, fit)
        assert bits_equal(c[0], a[0]) and not c[0].requires_grad
    assert levels == set(range(fit + 1)), levels        # every level is reached by some ray of some shape


@pytest.mark.parametrize("outside", ["skip", "evaluate"])
@pytest.mark.parametrize("densities", sorted(DENSITIES))
@pytest.mark.parametrize("fit", [0, 1, 3])
def test_march_step_stop_reference_on_hand_made_rays_against_a_python_loop(fit, densities, outside):
    grid, rays = hand_dgrid(outside, densities), step_rays()
    n = len(STEP_RAYS)
    stops = 0
    for ds in (0.5, 0.37):
        for M, S in SHAPES:
            g = torch.Generator().manual_seed(M * 100 + S)
            for u in (None, torch.rand(n, generator=g)):
                got = grid.march_step_stop_reference(rays, u, ds, M, S, 1e-2, fit)
                want = loop_march_step(grid, rays.numpy(), None if u is None else u.numpy(), ds, M, S, fit, eps=1e-2)
                assert len(got) == 5 and got[4].dtype == torch.bool and got[4].shape == (n,)
                assert_same(got, want, (ds, M, S, u))
                assert not bool((got[2] & got[4]).any())            # stopped and truncated are exclusive
                stops += int(got[4].sum())
                if densities == "zero":         # an all-zero density: the plain form, nothing stopped
                    assert_same(got[:4], grid.march_step_reference(rays, u, ds, M, S, fit), "zero density")
                    assert not bool(got[4].any())
    assert (stops > 0) == (densities != "zero")
    for bad in (0.0, 1.0, NAN, True, 1, None):
        with pytest.raises(ValueError, match="march_stop_eps"):
            grid.march_step_stop_reference(rays, None, 0.5, 4, 4, bad)


@pytest.mark.parametrize("outside", ["skip", "evaluate"])
def test_level_zero_equals_march_reference_on_a_power_of_two_geometry(outside):
    """|d| = 1, near = 0, far = 8 = ds * M with ds = 0.5 and M = 16: (k + u) * ds and far * ((k + u) / M) are the same exact scalings, so
    the level-0 depths are march_reference's bit for bit (rays 0-6 of hand_rays(); ray 7 has far = 12)"""
    grid, rays = hand_grid(outside), hand_rays()[:7]
    g = torch.Generator().manual_seed(9)
    for S in (20, 12, 9, 5, 3, 1):
        for u in (None, torch.zeros(7), torch.rand(7, generator=g)):
            got = grid.march_step_reference(rays, u, 0.5, 16, S)
            want = grid.march_reference(rays, u, 16, S)
            assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1]) and torch.equal(got[2], want[2]), (S, u)
            assert not bool(got[3].any())


def test_a_doubling_spelt_out_by_hand():
    """the full row (ray 1: near 0, far 8, |d| = 1), ds = 0.25, u = 0.5, S = 9 (8 slots in front of the stop depth's), fit = 3.
    Level 0: z_k = (k + 0.5) / 4, 32 candidates in front of far, all kept: 32 > 8.  Level 1: step 0.5, 16 > 8.  Level 2: step 1,
    z_k = k + 0.5 for k = 0 .. 7, 8 <= 8: the ray fits, nothing closes its run (no valid candidate lies behind it), z_stop = far."""
    grid, rays = hand_grid("skip"), hand_rays()
    for fit, level, row, stop, trunc in ((3, 2, [k + 0.5 for k in range(8)] + [8.0], 8.0, False),
                                         (2, 2, [k + 0.5 for k in range(8)] + [8.0], 8.0, False),
                                         (1, 1, [k / 2 + 0.25 for k in range(8)] + [4.25], 4.25, True),
                                         (0, 0, [k / 4 + 0.125 for k in range(8)] + [2.125], 2.125, True)):
        z, z_stop, tr, lv = grid.march_step_reference(rays, None, 0.25, 64, 9, fit)
        assert z[1].tolist() == row and float(z_stop[1]) == stop and bool(tr[1]) == trunc and int(lv[1]) == level, fit
    # the counts per level, from the definition's own level-0 form with room for everything
    counts = [int((grid.march_step_reference(rays, None, 0.25 * 2 ** j, 64, 64)[0][1] < 8.0).sum()) for j in range(4)]
    assert counts == [32, 16, 8, 4] and min(j for j in range(4) if counts[j] <= 8) == 2
    # the pattern row at the same settings: 8 + 1 closing + 4 + 1 closing = 14 > 8 at level 0; level 1: 4 + 1 + 2 + 1 = 8: fits
    z, z_stop, tr, lv = grid.march_step_reference(rays, None, 0.25, 64, 9, 3)
    assert int(lv[0]) == 1 and not bool(tr[0]) and z[0].tolist() == [1.25, 1.75, 2.25, 2.75, 3.25, 5.25, 5.75, 6.25, 8.0]
    # the cap M bites before far: M = 4 candidates of the full row at step 0.25, all kept, then nothing (no closing candidate either)
    z, z_stop, tr, lv = grid.march_step_reference(rays, None, 0.25, 4, 9, 3)
    assert z[1].tolist() == [0.125, 0.375, 0.625, 0.875] + [8.0] * 5 and float(z_stop[1]) == 8.0 and int(lv[1]) == 0
    with pytest.raises(ValueError):
        grid.march_step_reference(rays, None, 0.25, 0, 4)
    with pytest.raises(ValueError):
        grid.march_step_reference(rays, None, 0.25, 4, 0)
    for bad in (0.0, -1.0, NAN, INF, True, "0.5", None, 1e-60, 1e60):
        with pytest.raises(ValueError, match="march_step_size"):
            grid.march_step_reference(rays, None, bad, 4, 4)
    for bad in (-1, 9, 1.0, True, "1", None):
        with pytest.raises(ValueError, match="march_fit"):
            grid.march_step_reference(rays, None, 0.25, 4, 4, bad)


# ------------------------------------------------------------------------------------------------ what the definitions promise
DS_BALL, M_BALL, S_BALL = 1.0 / 64, 1024, 32


@pytest.fixture(scope="module")
def ball_scene():
    rays = orc.synthetic_rays(256, seed=21)
    grid = npa.OccupancyGrid.from_mask(ball_mask(), BOX_LO, BOX_HI, outside="skip", device=CPU)
    return rays, grid, {fit: grid.march_step_reference(rays, None, DS_BALL, M_BALL, S_BALL, fit) for fit in (0, 2, 3)}


def candidates_of(rays, level, M):
    """z_k of every ray at its own level, by the definition's expression, and which of them are valid"""
    d = rays[:, 3:6]
    dn = torch.sqrt((d[:, 0:1] * d[:, 0:1] + d[:, 1:2] * d[:, 1:2] + d[:, 2:3] * d[:, 2:3]).double()).float()    # (correctly rounded)
    dz = (torch.tensor(DS_BALL) / dn) * (2.0 ** level.float())[:, None]
    z_all = rays[:, 6:7] + (torch.arange(M, dtype=torch.float32)[None, :] + 0.5) * dz
    return z_all, z_all < rays[:, 7:8]


def test_properties_on_the_ball_scene(ball_scene):
    """orc.synthetic_rays(256, seed=21), the 32^3 ball, outside="skip", ds = 1 / 64, M = 1024, S = 32, u = None.  A prototype of the
    definition gave: fit = 3: no ray truncated, levels 0 / 1 / 2 / 3 hold 70 / 13 / 145 / 28 rays; fit = 2: 28 rays stay truncated;
    fit = 0: 186; 51 rays miss.  Asserted as floors only; the counts are printed."""
    rays, grid, runs = ball_scene
    M, S = M_BALL, S_BALL
    z, z_stop, tr, level = runs[3]
    per_level = [int((level == j).sum()) for j in range(4)]
    n_miss = int((z[:, 0] == rays[:, 7]).sum())
    print(f"fit=3: truncated {int(tr.sum())}, levels {per_level}; fit=2: truncated {int(runs[2][2].sum())}; fit=0: truncated "
          f"{int(runs[0][2].sum())}; miss {n_miss}")
    assert min(per_level) >= 8 and int(tr.sum()) == 0 and int(runs[2][2].sum()) > 0 and int(runs[0][2].sum()) > int(runs[2][2].sum())
    for fit, (z, z_stop, tr, level) in runs.items():
        assert int(level.max()) <= fit and bool((level[tr] == fit).all())
        z_all, valid = candidates_of(rays, level, M)
        occ_all = grid.occupied(rays[:, None, 0:3] + rays[:, None, 3:6] * z_all[:, :, None]) & valid
        # rows are nondecreasing
        assert bool((z[:, 1:] >= z[:, :-1]).all())
        # the evaluated samples: what nerf_occ_compact_stop keeps
        ev = grid.occupied(rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]) & ~(z >= z_stop[:, None])
        assert not bool(ev[:, -1].any())            # the last slot is never evaluated
        # behind every evaluated slot sits the next candidate of that ray's level, or z_stop
        pos = (z_all[:, None, :] == z[:, :, None]).float().argmax(-1)
        assert bool((z_all.gather(1, pos) == z)[ev].all())                                  # an evaluated slot holds a candidate
        nxt_valid = torch.cat([valid, torch.zeros_like(valid[:, :1])], -1).gather(1, (pos + 1).clamp(max=M))
        nxt = torch.where(nxt_valid, torch.cat([z_all, rays[:, 7:8]], -1).gather(1, (pos + 1).clamp(max=M)), rays[:, 7:8].expand(-1, S))
        behind = torch.cat([z[:, 1:], z_stop[:, None]], -1)
        assert bool((behind == nxt)[ev].all()) and int(ev.sum()) > 1000
        # on the rays that fit, the evaluated set is exactly the occupied valid candidates of their level
        fits = ~tr
        n_ev, n_occ = ev.sum(-1), occ_all.sum(-1)
        assert torch.equal(n_ev[fits], n_occ[fits])
        for r in fits.nonzero()[:, 0].tolist():
            assert torch.equal(z[r][ev[r]], z_all[r][occ_all[r]]), (fit, r)
        assert bool((n_ev[tr] <= S - 1).all()) and bool((z_stop[fits] == rays[fits, 7]).all())
        # a ray at level j > 0 was truncated at level j - 1: its occupied candidates there alone may not say so (closing candidates count),
        # but at level 0 of the fit = 0 run it was
        assert bool(runs[0][2][level > 0].all())
    # the levels of a smaller fit are those of a larger one, capped
    assert torch.equal(runs[2][3], runs[3][3].clamp(max=2)) and torch.equal(runs[0][3], torch.zeros_like(runs[0][3]))
    same = runs[3][3] <= 2
    assert bits_equal(runs[2][0][same], runs[3][0][same])


def ball_dgrid_cpu(value):
    mask = ball_mask()
    g = npa.DensityGrid(BOX_LO, BOX_HI, tuple(mask.shape), outside="skip", device=CPU)
    g.bits = npa.OccupancyGrid.from_mask(mask, BOX_LO, BOX_HI, device=CPU).bits.clone()
    g.density = torch.where(mask, torch.tensor(float(value)), torch.zeros(())).to(torch.float32).reshape(-1).contiguous()
    return g


STOP_SPARES_A_DOUBLING = 0     # a ray chosen from the printed list of the test below: level 2 without the stop, level 0 with it


def test_the_stop_form_on_the_ball_scene(ball_scene):
    """a zero density is the plain form at every fit; with a density of 50 inside the ball and eps = 1e-2 (tau = 4.6: a ray stops after
    about 0.09 of the ball) stopped and truncated are exclusive, no ray's level rises, and rays that the slot limit truncated at level 0
    without the stop fit at a lower level with it"""
    rays, _, runs = ball_scene
    zero = ball_dgrid_cpu(0.0)
    for fit in (0, 3):
        got = zero.march_step_stop_reference(rays, None, DS_BALL, M_BALL, S_BALL, 1e-2, fit)
        assert_same(got[:4], runs[fit], fit)
        assert not bool(got[4].any())
    dense = ball_dgrid_cpu(50.0)
    z, z_stop, tr, level, st = dense.march_step_stop_reference(rays, None, DS_BALL, M_BALL, S_BALL, 1e-2, 3)
    plain_level = runs[3][3]
    spared = ((plain_level > 0) & (level < plain_level)).nonzero()[:, 0].tolist()
    print(f"density 50, eps 1e-2, fit=3: stopped {int(st.sum())}, truncated {int(tr.sum())}, levels {[int((level == j).sum()) for j in range(4)]}; "
          f"rays at a lower level than without the stop: {len(spared)} (the first: {spared[:8]})")
    assert not bool((tr & st).any()) and int(tr.sum()) == 0
    assert bool((level <= plain_level).all())
    assert len(spared) > 0
    r = STOP_SPARES_A_DOUBLING
    print(f"ray {r}: level {int(plain_level[r])} without the stop, {int(level[r])} with it")
    assert r in spared and bool(runs[0][2][r]) and int(level[r]) < int(plain_level[r]) and bool(st[r]) and not bool(tr[r])
    # in front of its stop a stopped ray at level 0 holds the plain level-0 march's depths
    for r in (st & (level == 0)).nonzero()[:, 0].tolist()[:16]:
        n = int((z[r] < z_stop[r]).sum())
        assert n > 0 and bits_equal(z[r, :n], runs[0][0][r, :n]) and bool((z[r, n:] == z_stop[r]).all())


# ------------------------------------------------------------------------------------------------ exports
def test_the_library_exports_and_binds_the_entry_point():
    hb = npa.hip_backend
    raw = ctypes.CDLL(npa.build.LIB_PATH)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_hip.h")) as f:
        header = f.read()
    assert hasattr(raw, "nerf_occ_march_step") and "nerf_occ_march_step" in hb.EXPORTS and "int nerf_occ_march_step(" in header
    assert "#define NERF_ABI_VERSION 10" in header and hb.ABI_VERSION == 10
    assert list(inspect.signature(hb.occ_march_step).parameters) == ["desc", "density", "outside_sigma", "rays", "u", "step_size", "n_steps",
                                                                     "n_slots", "fit", "eps"]
    assert list(inspect.signature(npa.OccupancyGrid.march_step).parameters) == ["self", "rays", "step_size", "n_steps", "n_slots", "fit", "u"]
    assert list(inspect.signature(npa.DensityGrid.march_step_stop).parameters) == ["self", "rays", "step_size", "n_steps", "n_slots", "eps",
                                                                                   "fit", "u"]
    assert list(inspect.signature(npa.OccupancyGrid.march_step_reference).parameters) == ["self", "rays", "u", "step_size", "n_steps", "n_slots",
                                                                                          "fit"]
    assert list(inspect.signature(npa.DensityGrid.march_step_stop_reference).parameters) == ["self", "rays", "u", "step_size", "n_steps",
                                                                                             "n_slots", "eps", "fit"]
    assert not hasattr(npa.OccupancyGrid, "march_step_stop") and not hasattr(npa.OccupancyGrid, "march_step_stop_reference")
    L = hb.lib()
    assert L.nerf_abi_version() == 10
    # the limits, refused before anything is launched or read (host memory stands in for the device buffers)
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    desc = hb.NerfOccGrid((ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_int * 3)(2, 2, 2), 0, ptr)

    def call(stride=8, n=1, ds=0.5, M=4, S=4, fit=0, tau=1.0, stop=True, **null):
        a = dict(density=ptr if stop else None, rays=ptr, z_vals=ptr, z_stop=ptr, truncated=ptr, level=ptr, stopped=ptr if stop else None)
        a.update(null)
        return L.nerf_occ_march_step(ctypes.byref(desc), a["density"], 0.0, a["rays"], stride, None, n, ds, M, S, fit, tau, a["z_vals"],
                                     a["z_stop"], a["truncated"], a["level"], a["stopped"], None)
    for stop in (True, False):
        for name in ("rays", "z_vals", "z_stop", "truncated", "level"):
            assert call(stop=stop, **{name: None}) != 0 and "null" in L.nerf_last_error().decode(), name
        for kw in (dict(stride=7), dict(n=-1), dict(M=0), dict(M=16385), dict(S=0), dict(S=4097)):
            assert call(stop=stop, **kw) != 0 and "bad size" in L.nerf_last_error().decode(), kw
        for fit in (-1, 9):
            assert call(stop=stop, fit=fit) != 0 and "fit" in L.nerf_last_error().decode(), fit
        for ds in (0.0, -0.5, NAN, INF):
            assert call(stop=stop, ds=ds) != 0 and "step_size" in L.nerf_last_error().decode(), ds
        assert call(stop=stop, n=0, M=16384, S=4096, fit=8) == 0          # no rays: nothing to do (u is optional)
    # stopped comes exactly with the density
    assert call(density=None) != 0 and "null" in L.nerf_last_error().decode()
    assert call(stopped=None) != 0 and "null" in L.nerf_last_error().decode()
    assert L.nerf_occ_march_step(None, ptr, 0.0, ptr, 8, None, 1, 0.5, 4, 4, 0, 1.0, ptr, ptr, ptr, ptr, ptr, None) != 0
    assert "null" in L.nerf_last_error().decode()
    for tau in (0.0, -1.0, NAN):
        assert call(tau=tau) != 0 and "tau" in L.nerf_last_error().decode(), tau
    assert call(stop=False, tau=0.0, n=0) == 0      # the plain form has no threshold
    grid = npa.DensityGrid(HAND_LO, HAND_HI, (8, 2, 1), device=CPU)
    for M, S in ((0, 4), (16385, 4), (4, 0), (4, 4097)):
        with pytest.raises(ValueError, match="n_steps"):
            grid.march_step(step_rays(), 0.5, M, S)
        with pytest.raises(ValueError, match="n_steps"):
            grid.march_step_stop(step_rays(), 0.5, M, S, 0.01)
    for bad in (0.0, NAN, INF, True, "1"):
        with pytest.raises(ValueError, match="march_step_size"):
            grid.march_step(step_rays(), bad, 4, 4)
        with pytest.raises(ValueError, match="march_step_size"):
            grid.march_step_stop(step_rays(), bad, 4, 4, 0.01)
    for bad in (-1, 9, True, 2.0):
        with pytest.raises(ValueError, match="march_fit"):
            grid.march_step(step_rays(), 0.5, 4, 4, fit=bad)
        with pytest.raises(ValueError, match="march_fit"):
            grid.march_step_stop(step_rays(), 0.5, 4, 4, 0.01, fit=bad)
    for bad in (0.0, 1.0, NAN, True, 1):
        with pytest.raises(ValueError, match="march_stop_eps"):
            grid.march_step_stop(step_rays(), 0.5, 4, 4, bad)


# ------------------------------------------------------------------------------------------------ guards
def test_the_options_are_keyword_only_and_every_guard_fires_before_a_launch(monkeypatch):
    params = inspect.signature(npa.render_rays).parameters
    assert params["march_step_size"].kind is inspect.Parameter.KEYWORD_ONLY and params["march_step_size"].default is None
    assert params["march_fit"].kind is inspect.Parameter.KEYWORD_ONLY and params["march_fit"].default == 0
    net, fine = npa.NeRF(**NET_KW), npa.NeRF(**NET_KW)
    monkeypatch.setattr(npa.hip_backend, "lib", lambda: pytest.fail("a guard let a call reach the library"))
    rays = _rays(8)
    dgrid = npa.DensityGrid(LO, HI, RES, device=CPU)
    plain = npa.OccupancyGrid(LO, HI, RES, device=CPU)
    kw = dict(N_samples=8, N_importance=8, network_fine=fine)
    march = dict(proposal="march", march_steps=64)
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            # the options without the march
            for other in (None, "grid"):
                with pytest.raises(ValueError, match="march_step_size belongs"):
                    npa.render_rays(rays, net, None, occupancy=dgrid, proposal=other, march_step_size=0.1, **kw)
                with pytest.raises(ValueError, match="march_fit belongs"):
                    npa.render_rays(rays, net, None, occupancy=dgrid, proposal=other, march_fit=1, **kw)
            with pytest.raises(ValueError, match="march_step_size belongs"):
                npa.render_rays(rays, net, None, march_step_size=0.1, **kw)
            with pytest.raises(ValueError, match="march_fit belongs"):
                npa.render_rays(rays, net, None, march_fit=2, **kw)
            for grid in (dgrid, plain):
                # a step that is not a finite real number > 0
                for bad in (0.0, -0.1, NAN, INF, -INF, True, False, "0.1", torch.tensor(0.1), 1e-60, 0):
                    with pytest.raises(ValueError, match="march_step_size must be"):
                        npa.render_rays(rays, net, None, occupancy=grid, march_step_size=bad, **march, **kw)
                # a fit that is not an int in 0..8
                for bad in (-1, 9, 1.0, True, False, "1", NAN):
                    with pytest.raises(ValueError, match="march_fit must be"):
                        npa.render_rays(rays, net, None, occupancy=grid, march_step_size=0.1, march_fit=bad, **march, **kw)
                    with pytest.raises(ValueError, match="march_fit must be"):
                        npa.render_rays(rays, net, None, occupancy=grid, march_fit=bad, **march, **kw)
                # a fit without a step
                for fit in (1, 8, np.int64(3)):
                    with pytest.raises(ValueError, match="needs march_step_size"):
                        npa.render_rays(rays, net, None, occupancy=grid, march_fit=fit, **march, **kw)
                # what the march refuses stays refused, with its own error
                with pytest.raises(ValueError, match="march_steps"):
                    npa.render_rays(rays, net, None, occupancy=grid, proposal="march", march_step_size=0.1, **kw)
                with pytest.raises(NotImplementedError, match="lindisp"):
                    npa.render_rays(rays, net, None, occupancy=grid, march_step_size=0.1, march_fit=2, lindisp=True, **march, **kw)
                with pytest.raises(ValueError, match="early_stop_eps together with"):
                    npa.render_rays(rays, net, None, occupancy=grid, march_step_size=0.1, early_stop_eps=0.01, **march, **kw)
                with pytest.raises(NotImplementedError, match="network_query_fn"):
                    npa.render_rays(rays, net, lambda pts, vd, m: None, occupancy=grid, march_step_size=0.1, march_fit=2, **march, **kw)
            with pytest.raises(ValueError, match="a plain OccupancyGrid has none"):
                npa.render_rays(rays, net, None, occupancy=plain, march_step_size=0.1, march_stop_eps=0.01, **march, **kw)
    with pytest.raises(NotImplementedError, match="plain OccupancyGrid"):       # grad mode on, parameters that require grad
        npa.render_rays(rays, net, None, occupancy=plain, march_step_size=0.1, march_fit=2, **march, **kw)
    # through the layers that forward keywords
    with pytest.raises(ValueError, match="march_step_size must be"):
        npa.batchify_rays(rays, 4, network_fn=net, network_query_fn=None, occupancy=dgrid, march_step_size=0.0, **march, **kw)
    with pytest.raises(ValueError, match="march_fit must be"):
        npa.batchify_rays(rays, 4, network_fn=net, network_query_fn=None, occupancy=dgrid, march_step_size=0.1, march_fit="2", **march, **kw)
    K = np.array([[10.0, 0, 2.0], [0, 10.0, 2.0], [0, 0, 1]])
    geo = dict(rays=(rays[:, 0:3], rays[:, 3:6]), ndc=False, near=2.0, far=6.0, use_viewdirs=True, network_fn=net, network_query_fn=None)
    with pytest.raises(ValueError, match="march_step_size belongs"):
        npa.render(4, 2, K, chunk=8, occupancy=dgrid, march_step_size=0.1, **geo, **kw)
    with pytest.raises(ValueError, match="needs march_step_size"):
        npa.render(4, 2, K, chunk=8, occupancy=dgrid, march_fit=1, **march, **geo, **kw)


@pytest.mark.parametrize("retraw", [False, True])
def test_the_empty_batch_has_the_keys_and_stats_of_the_mode(monkeypatch, retraw):
    net, fine = npa.NeRF(**NET_KW), npa.NeRF(**NET_KW)
    dgrid = npa.DensityGrid(LO, HI, RES, device=CPU)
    monkeypatch.setattr(dgrid, "_desc", lambda: None)       # (the empty batch validates the grid's device; this grid lives on the CPU)
    kw = dict(N_samples=8, N_importance=16, network_fine=fine, retraw=retraw, occupancy=dgrid, proposal="march", march_steps=64)
    out = npa.render_rays(_rays(0), net, None, march_step_size=0.1, march_fit=2, **kw)
    assert set(out) == {"rgb_map", "disp_map", "acc_map"} | ({"raw"} if retraw else set())
    assert out["rgb_map"].shape == (0, 3) and out["disp_map"].shape == (0,) and out["acc_map"].shape == (0,)
    if retraw:
        assert out["raw"].shape == (0, 24, 4)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0, "rays_truncated": 0, "rays_refit": 0}
    npa.render_rays(_rays(0), net, None, march_step_size=0.1, march_fit=2, march_stop_eps=0.01, clip_to_occupancy=True, **kw)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0, "rays_hit": 0, "rays": 0, "rays_truncated": 0, "rays_stopped": 0, "rays_refit": 0}
    # without a fit there is no counter of refit rays
    npa.render_rays(_rays(0), net, None, march_step_size=0.1, **kw)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0, "rays_truncated": 0}
    # batchify_rays sums the stats of the mode (no chunk at all: the zeros it starts from)
    npa.batchify_rays(_rays(0), 4, network_fn=net, network_query_fn=None, march_step_size=0.1, march_fit=8, march_stop_eps=0.01, **kw)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0, "rays_truncated": 0, "rays_stopped": 0, "rays_refit": 0}
    # without the options the empty batch is what it was
    npa.render_rays(_rays(0), net, None, march_step_size=None, march_fit=0, **kw)
    assert dgrid.last_stats == {"evaluated": 0, "total": 0, "rays_truncated": 0}
