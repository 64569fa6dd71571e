"""Generate tests/golden/march_references.npz: what the four march references returned BEFORE they were put on one shared walk.

Run once, at the commit in front of that change; tests/test_march_references_pin_cpu.py holds the references to it bit for bit.

Scene: the seeded ball DensityGrid of tests/test_march_stop_cpu.py (``ball_density_grid``), outside = "skip" and "evaluate".
Shapes (M, S): (1, 1), (7, 2), (65, 64) -- one candidate into the second round of 64 --, (130, 9) -- three rounds and a slot limit
that bites.  Per (outside, shape) 96 rays, chosen from a seeded pool of random rays through and around the ball: two each of the four
invalid kinds (a NaN component, an infinite component, near == far, d = 0), at least eight misses and (S > 1) eight rays that fit, and what
the conditions below ask for; the rest are misses.  Per (outside, shape) 20 cases on those rays: u given / u = None times
    march                                march_reference
    march_stop                           march_stop_reference, eps = 1e-2
    step       ds in {1/64, 0.37} x fit in {0, 3}     march_step_reference
    step_stop  ds in {1/64, 0.37} x fit in {0, 3}     march_step_stop_reference, eps = 1e-2
The file holds the rays, u, and per case z_vals, z_stop and the flags (truncated, stopped, level; 0 where a form has none).

Conditions, asserted here:
  * every case has at least 8 truncated rays -- rays the case itself flags: at fit = 3 those that no level fits;
  * every fit = 3 case has at least 8 rays at a level > 0;
  * every stop case has at least 8 stopped rays;
  * for every ray fp32 torch.sqrt of dx dx + dy dy + dz dz equals the root taken through float64, bit for bit (pool rays that fail
    are dropped): the file does not depend on how a torch build rounds its fp32 square root.
Some cases cannot meet one of the first three, whatever the rays of the pool; ``can_truncate`` / ``can_stop`` say which and why, and
those counts are printed, not asserted.

    python tests/golden/make_golden_march.py
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
from test_march_stop_cpu import ball_density_grid  # noqa: E402

SHAPES = ((1, 1), (7, 2), (65, 64), (130, 9))
OUTSIDE = ("skip", "evaluate")
STEP_SIZES = (1.0 / 64.0, 0.37)
FITS = (0, 3)
EPS = 1e-2
N_RAYS, N_POOL, POOL_SEED, LEAST = 96, 24000, 20, 8
SIGMA_MAX = 4.0 * 1.75              # ball_density_grid: scale * (0.25 + 1.5 * rand), rand < 1
CHORD_MAX = 2.0 * (1.0 + math.sqrt(3.0) / 16.0)     # the ball's cells have their centres within 1 of the origin and a half diagonal of sqrt(3) / 16
LENGTH_MAX, NORM_MAX = 24.0, 2.0    # ray_pool: far - near and |d| at most


def cases():
    """[(name, form, with_u, ds, fit)] in the order of the stored arrays (twins next to each other: they share most rows)"""
    out = []
    for with_u in (True, False):
        tag = "u" if with_u else "none"
        out.append((f"march {tag}", "march", with_u, None, None))
        out.append((f"march_stop {tag}", "march_stop", with_u, None, None))
        for ds in STEP_SIZES:
            for form in ("step", "step_stop"):
                for fit in FITS:
                    out.append((f"{form} {tag} {ds!r} {fit}", form, with_u, ds, fit))
    return out


def run_case(grid, rays, u, M, S, form, with_u, ds, fit):
    """(z_vals, z_stop, truncated, stopped, level) of one case; stopped / level are zeros where the form has none"""
    uu = u if with_u else None
    zero = torch.zeros(rays.shape[0], dtype=torch.int32)
    if form == "march":
        z, zs, tr = grid.march_reference(rays, uu, M, S)
        return z, zs, tr, zero, zero
    if form == "march_stop":
        z, zs, tr, st = grid.march_stop_reference(rays, uu, M, S, EPS)
        return z, zs, tr, st, zero
    if form == "step":
        z, zs, tr, lv = grid.march_step_reference(rays, uu, ds, M, S, fit)
        return z, zs, tr, zero, lv
    z, zs, tr, lv, st = grid.march_step_stop_reference(rays, uu, ds, M, S, EPS, fit)
    return z, zs, tr, st, lv


def can_truncate(form, outside, S, ds, level):
    """whether any ray of the pool can overflow S - 1 slots at `level`.  A world-space march over a stretch of length L in the scene
    emits at most L / (ds * 2^level) + 1 kept candidates and one closing one; with outside="skip" only the ball is occupied and L is at
    most CHORD_MAX, with outside="evaluate" L is at most the pool's longest ray, LENGTH_MAX * NORM_MAX.  Equal steps shrink with the ray:
    they can emit all M."""
    if form in ("step", "step_stop"):
        return (CHORD_MAX if outside == "skip" else LENGTH_MAX * NORM_MAX) / (ds * 2 ** level) + 2 >= S
    return True


def can_stop(form, M, S, ds, fit):
    """whether any ray can stop.  A_0 = 0, so a cut needs a candidate k >= 1 (M > 1) and at least one kept -- hence emitted --
    candidate in front of it that still fits (S > 1).  A world-space march adds at most SIGMA_MAX * ds * 2^level per kept candidate,
    and at most S - 1 of them fit in front of the cut."""
    if M < 2 or S < 2:
        return False
    if form == "step_stop":
        return (S - 1) * SIGMA_MAX * ds * 2 ** fit >= -math.log(EPS)
    return True


def ray_pool():
    """rays through and around the ball: a point p within 1.9 of the origin is met at a depth inside [near, far]; |d| in [0.5, 2],
    near in [0, 2], far - near log-uniform in [0.2, 24].  u: one offset per ray."""
    rs = np.random.RandomState(POOL_SEED)
    n = N_POOL
    p = rs.normal(size=(n, 3))
    p *= (rs.uniform(0.0, 1.9, size=(n, 1)) / np.linalg.norm(p, axis=-1, keepdims=True))
    d = rs.normal(size=(n, 3))
    d *= (rs.uniform(0.5, 2.0, size=(n, 1)) / np.linalg.norm(d, axis=-1, keepdims=True))
    near = rs.uniform(0.0, 2.0, size=(n, 1))
    length = np.exp(rs.uniform(math.log(0.2), math.log(24.0), size=(n, 1)))
    at = near + length * rs.uniform(0.0, 1.0, size=(n, 1)) ** 2
    rays = torch.tensor(np.concatenate([p - d * at, d, near, near + length], -1), dtype=torch.float32)
    u = torch.tensor(rs.uniform(0.0, 1.0, size=n), dtype=torch.float32).clamp(max=1.0 - 2.0 ** -24)
    return rays[sqrt_is_exact(rays)], u[sqrt_is_exact(rays)]


def sqrt_is_exact(rays):
    d = rays[:, 3:6].to(torch.float32)
    s = d[:, 0:1] * d[:, 0:1] + d[:, 1:2] * d[:, 1:2] + d[:, 2:3] * d[:, 2:3]
    a, b = torch.sqrt(s.contiguous()), torch.sqrt(s.to(torch.float64)).to(torch.float32)
    return (a.view(torch.int32) == b.view(torch.int32))[:, 0]


def invalid_rays():
    base = torch.tensor([[0.0, 0.0, 3.0, 0.0, 0.0, -1.0, 2.0, 4.0], [0.5, 0.0, -3.0, 0.0, 0.25, 1.5, 1.0, 5.0]], dtype=torch.float32)
    out = base.repeat(4, 1)
    out[0, 1], out[1, 4] = float("nan"), float("nan")
    out[2, 0], out[3, 5] = float("inf"), float("-inf")
    out[4, 7], out[5, 7] = out[4, 6], out[5, 6]
    out[6:8, 3:6] = 0.0
    out[6, 0:3] = torch.tensor([0.25, 0.25, 0.25])          # (a point of the ball: the equal-step forms keep every candidate)
    return out, torch.tensor([0.5, 0.25, 0.0, 0.75, 0.125, 0.5, 0.625, 0.875], dtype=torch.float32)


def choose(grid, outside, M, S, pool, pool_u):
    """indices of the pool rays of one (outside, shape): a greedy cover of every condition a case can meet, then misses"""
    needs, free = [], []            # (name, mask over the pool, asserted?)
    plain = None
    for name, form, with_u, ds, fit in cases():
        z, zs, tr, st, lv = run_case(grid, pool, pool_u, M, S, form, with_u, ds, fit)
        if form == "march" and not with_u:
            plain = (z, zs, tr)
        (needs if can_truncate(form, outside, S, ds, fit or 0) else free).append((name + ": truncated", tr.bool()))
        if fit:                     # (a ray at a level > 0 was truncated at level 0)
            (needs if can_truncate(form, outside, S, ds, 0) else free).append((name + ": level > 0", lv > 0))
        if form in ("march_stop", "step_stop"):
            (needs if can_stop(form, M, S, ds, fit) else free).append((name + ": stopped", st.bool()))
    z, zs, tr = plain
    emits = (z < zs[:, None]).any(-1) | tr
    needs.append(("misses", ~emits))
    if S > 1:                       # (with S = 1 whatever emits is truncated)
        needs.append(("fits", emits & ~tr))
    short = torch.stack([(m.sum() < LEAST) for _, m in needs])
    assert not bool(short.any()), [(n, int(m.sum())) for n, m in needs if m.sum() < LEAST]
    have = torch.stack([m for _, m in needs], 0)            # [conditions, pool]
    left = torch.full((len(needs),), LEAST)
    picked = []
    while bool((left > 0).any()):
        gain = (have & (left > 0)[:, None]).sum(0)
        gain[picked] = -1
        best = int(gain.argmax())
        assert int(gain[best]) > 0
        picked.append(best)
        left = left - have[:, best].to(left.dtype)
    assert len(picked) <= N_RAYS - 8, (outside, M, S, len(picked))
    misses = [i for i in (~emits).nonzero()[:, 0].tolist() if i not in set(picked)]
    picked += misses[:N_RAYS - 8 - len(picked)]
    assert len(picked) == N_RAYS - 8
    return sorted(picked), [n for n, _ in needs], [n for n, _ in free]


def main():
    pool, pool_u = ray_pool()
    print(f"pool: {pool.shape[0]} of {N_POOL} rays have an exact fp32 sqrt in this torch build")
    bad, bad_u = invalid_rays()
    rec = {"cases": np.array([c[0] for c in cases()]), "eps": np.float64(EPS)}
    for outside in OUTSIDE:
        grid = ball_density_grid(outside)
        rec[f"density_checksum/{outside}"] = np.float64(grid.density.double().sum())
        for M, S in SHAPES:
            idx, asserted, free = choose(grid, outside, M, S, pool, pool_u)
            rays, u = torch.cat([pool[idx], bad], 0), torch.cat([pool_u[idx], bad_u], 0)
            assert rays.shape == (N_RAYS, 8) and bool(sqrt_is_exact(rays[:N_RAYS - 8]).all()) and bool(sqrt_is_exact(rays[-2:]).all())
            key = f"{outside}/{M}x{S}"
            z_all, zs_all, flags = [], [], []
            for name, form, with_u, ds, fit in cases():
                z, zs, tr, st, lv = run_case(grid, rays, u, M, S, form, with_u, ds, fit)
                counts = {"truncated": int(tr.sum()), "stopped": int(st.sum()), "level > 0": int((lv > 0).sum())}
                for what in ("truncated", "stopped", "level > 0"):
                    if f"{name}: {what}" in asserted:
                        assert counts[what] >= LEAST, (key, name, what, counts)
                print(f"{key:>16} {name:<34} {counts}" + ("" if not any(f.startswith(name + ":") for f in free) else "   (cannot: " +
                      ", ".join(f.split(": ")[1] for f in free if f.startswith(name + ":")) + ")"))
                z_all.append(z.numpy()), zs_all.append(zs.numpy())
                flags.append(torch.stack([tr.to(torch.int8), st.to(torch.int8), lv.to(torch.int8)], -1).numpy())
            rec[f"rays/{key}"], rec[f"u/{key}"] = rays.numpy(), u.numpy()
            rec[f"z_vals/{key}"], rec[f"z_stop/{key}"], rec[f"flags/{key}"] = np.stack(z_all), np.stack(zs_all), np.stack(flags)
    path = os.path.join(HERE, "march_references.npz")
    np.savez_compressed(path, **rec)
    print(f"-> {path} ({os.path.getsize(path)} B)")
    assert os.path.getsize(path) < 200 * 1000


if __name__ == "__main__":
    main()
