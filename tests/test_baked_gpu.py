"""GPU tests (-m gpu) of nerf_baked_render against its definition, BakedField.render_rays_reference.

THE DEFINITION is render_rays_reference(dtype=float64), run on the CPU on the fp32 inputs the kernel sees.  THE YARDSTICK of the
tolerance is the same function with dtype=float32 against its own float64 run (the project's rule, tests/test_gpu_distortion.py): over
each case set -- one grid, one ray count, one degree; u None and given, white_bkgd off and on -- the kernel's largest absolute error in
rgb_map and acc_map may be at most max(4 x the yardstick's, 2^-22), 2^-22 being one ulp of the largest value either can take (rgb and
acc lie in [0, 1], rgb + 1 - acc too); for depth_map = sum w z <= far the floor is 2^-22 times the largest far of the set.  The discrete
outputs are exact: n_samples equals the definition's (the geometry is the same fp32 expressions on both sides) and disp_map is
1 / max(1e-10, depth / acc), NaN kept, evaluated in fp32 on the kernel's own depth_map and acc_map.

Shapes.  Grids 5 x 6 x 7 and 8^3 with cells of edge 1/4 over boxes that are not centred on the origin (scale = 4 exactly, so a ray can run
along a cell plane with t an exact integer), masks of share about 0.3 that hold cells on all six faces (the node index R).  1, 5 and
130 rays: blocks of four rays, the last one partly filled.  Ray kinds, row i being kind i % 10: rays through the box with 130, 65, 64 and
63 valid candidates (the rounds of 64), a ray that starts inside with one candidate, rays along each axis on cell planes, a ray that
misses the box, and an invalid ray (a NaN, near >= far, d = 0 in turn).  The sigma column has both signs (the ReLU acts behind the
blend); the colour coefficients reach logits of +-30."""
import numpy as np
import pytest
import torch

import nerf_pytorch_amd
from nerf_pytorch_amd.baked import BakedField
from nerf_pytorch_amd.occupancy import OccupancyGrid
from test_gpu_occupancy import bits_equal
from test_gpu_parity import dev, maxdiff, npa  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")
F64 = torch.float64
FLOOR = 2.0 ** -22
DS = 0.02
GRIDS = {"5x6x7": ((5, 6, 7), (-0.75, 0.5, 1.0)), "8x8x8": ((8, 8, 8), (1.0, -2.5, 0.25))}
COUNTS = [1, 5, 130]
KINDS = ("130 candidates", "65 candidates", "64 candidates", "63 candidates", "inside, 1 candidate", "along x", "along y", "along z", "miss",
         "invalid")
CANDIDATES = {0: 130, 1: 65, 2: 64, 3: 63, 4: 1}


def box_of(name):
    res, lo = GRIDS[name]
    return res, lo, tuple(l + 0.25 * r for l, r in zip(lo, res))


def mask_of(name, seed):
    res = GRIDS[name][0]
    m = torch.rand(res, generator=torch.Generator().manual_seed(seed)) < 0.3
    m[0, 1, 2] = m[-1, 2, 1] = m[1, 0, 3] = m[2, -1, 2] = m[3, 2, 0] = m[1, 3, -1] = True      # a cell on each of the six faces
    m[2, 3, :] = True       # the rows the axis rays run along
    m[:, 3, 2] = True
    m[2, :, 2] = True
    return m


def nodes_of(name, degree, seed):
    """fp32 [Rx + 1, Ry + 1, Rz + 1, 1 + 3B]: sigma of both signs, coefficients whose DC term alone reaches logits of +-30"""
    res = GRIDS[name][0]
    B = (degree + 1) ** 2
    g = torch.Generator().manual_seed(seed)
    nodes = torch.randn(tuple(r + 1 for r in res) + (1 + 3 * B,), generator=g)
    nodes[..., 0] = 12.0 * nodes[..., 0] + 4.0
    nodes[..., 1:] *= 2.0
    for c in range(3):
        nodes[..., 1 + c * B] *= 106.0 / 2.0 / 2.0         # 0.282 * 106 = 30 at two standard deviations
    return nodes


def rays_of(name, n, seed, with_u):
    """(rays fp32 [n, 11], u fp32 [n] or None, the planned number of valid candidates per ray: -1 where it is not planned)"""
    res, lo, hi = box_of(name)
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=F64)
    lo64, hi64 = torch.tensor(lo, dtype=F64), torch.tensor(hi, dtype=F64)
    centre, half = 0.5 * (lo64 + hi64), 0.5 * (hi64 - lo64)
    u = 0.7 * rnd(n) if with_u else None            # (below 0.75: far = near + (C - 1/4) dz then holds C candidates for every u)
    rays = torch.zeros(n, 11, dtype=F64)
    planned = torch.full((n,), -1, dtype=torch.int64)
    for i in range(n):
        kind, j = i % len(KINDS), i // len(KINDS)
        e = torch.randn(3, generator=g, dtype=F64)
        e = e / e.norm()
        L = 0.5 + 1.5 * float(rnd(1))               # |d|: the ray directions are not normalised
        target = centre + half * (1.6 * rnd(3) - 0.8)
        view = torch.randn(3, generator=g, dtype=F64)
        view = view / view.norm()
        near = 0.25 * float(rnd(1))
        if kind in CANDIDATES:
            C = CANDIDATES[kind]
            start = target if kind == 4 else target - e * (0.35 * C * DS)          # the box lies inside the candidates' span
            o = start - e * L * near
            far = near + (C - 0.25) * (DS / L)
            planned[i] = C
            rays[i] = torch.cat([o, e * L, torch.tensor([near, far], dtype=F64), view])
        elif kind in (5, 6, 7):                     # along an axis, on cell planes of the two other axes, through the rows the mask keeps
            a = kind - 5
            cell = {0: (None, 3, 2), 1: (2, None, 2), 2: (2, 3, None)}[a]
            o = torch.tensor([lo[b] + 0.25 * (cell[b] if cell[b] is not None else -2.0) for b in range(3)], dtype=F64)
            d = torch.zeros(3, dtype=F64)
            d[a] = L if j % 2 == 0 else 1.0
            rays[i] = torch.cat([o, d, torch.tensor([0.0, 4.0 / float(d[a])], dtype=F64), view])
        elif kind == 8:                             # parallel to the box, outside it
            o = torch.tensor([lo[0] - 1.0, hi[1] + 0.3, centre[2]], dtype=F64)
            rays[i] = torch.cat([o, torch.tensor([L, 0.0, 0.0], dtype=F64), torch.tensor([0.0, 6.0], dtype=F64), view])
        else:
            o = centre - e * 2.0
            rays[i] = torch.cat([o, e * L, torch.tensor([0.0, 4.0], dtype=F64), view])
            if j % 3 == 0:
                rays[i, 1] = float("nan")
            elif j % 3 == 1:
                rays[i, 6] = rays[i, 7]
            else:
                rays[i, 3:6] = 0.0
    return rays.float(), None if u is None else u.float(), planned


def field_of(name, degree, device, **kw):
    res, lo, hi = box_of(name)
    grid = OccupancyGrid.from_mask(mask_of(name, 17), lo, hi, device=device)
    return BakedField.from_nodes(grid, nodes_of(name, degree, 100 + degree), degree, step_size=DS, **kw)


def empty_of(ns):
    return (ns == 0).cpu()


def kernel(hb, field, rays, u, white, max_steps=1 << 14, stop_eps=None):
    return hb.baked_render(field.grid._desc(), field.index, field.table, field.sh_degree, rays, u, field.step_size, max_steps,
                           field.stop_eps if stop_eps is None else stop_eps, white)


@pytest.fixture(scope="module")
def measured(npa, dev):
    """every case once: {(grid, n, degree): [rows]}, a row holding the kernel's outputs, the float64 definition and the errors of the
    kernel and of the float32 definition against it"""
    hb = npa.hip_backend
    out = {}
    for name in GRIDS:
        for degree in (0, 1, 2):
            f_cpu, f_dev = field_of(name, degree, CPU), field_of(name, degree, dev)
            assert f_cpu.grid.scale.tolist() == [4.0, 4.0, 4.0]
            for n in COUNTS:
                rows = []
                for with_u in (False, True):
                    rays, u, planned = rays_of(name, n, 1000 * n + degree, with_u)
                    for white in (False, True):
                        for max_steps in ((1 << 14, 64) if n == 130 and not white else (1 << 14,)):
                            r64 = f_cpu.render_rays_reference(rays, u, white, max_steps, F64)
                            r32 = f_cpu.render_rays_reference(rays, u, white, max_steps, torch.float32)
                            got = kernel(hb, f_dev, rays.to(dev), None if u is None else u.to(dev), white, max_steps)
                            rows.append(dict(rays=rays, u=u, planned=planned, white=white, max_steps=max_steps, r64=r64, r32=r32, got=got,
                                             err={"rgb_map": maxdiff(got[0], r64["rgb_map"]), "acc_map": maxdiff(got[2], r64["acc_map"]),
                                                  "depth_map": maxdiff(got[3], r64["depth_map"])},
                                             yard={k: maxdiff(r32[k], r64[k]) for k in ("rgb_map", "acc_map", "depth_map")}))
                out[(name, n, degree)] = rows
    return out


def test_the_cases_are_what_they_claim(measured):
    """the planned numbers of valid candidates are met in fp32, every kind is sampled or empty as said, the blended sigma takes both signs
    and the logits reach the sigmoid's tails"""
    for (name, n, degree), rows in measured.items():
        f = field_of(name, degree, CPU)
        for r in rows:
            rr, ok, uu, dn, M, _ = OccupancyGrid._march_rays("test", r["rays"], r["u"], 1 << 14, 1)
            dz = torch.tensor(DS, dtype=torch.float32) / dn
            z, valid = OccupancyGrid._world_steps(rr, ok & torch.isfinite(dz[:, 0]) & (dz[:, 0] > 0), uu, dz, M)
            counts = valid.sum(-1)
            plan = r["planned"]
            assert torch.equal(counts[plan >= 0], plan[plan >= 0]), (name, n, degree)
            ns = r["r64"]["n_samples"]
            kinds = torch.arange(n) % len(KINDS)
            assert bool((ns[kinds >= 8] == 0).all())
            if r["max_steps"] == 64:
                assert bool((ns <= 64).all())
                continue
            for k in (5, 6, 7):             # an axis ray crosses its kept row: at least the cells' worth of steps
                assert bool((ns[kinds == k] >= 20).all()), (name, k, ns[kinds == k])
            if n == 130:
                assert bool((ns[kinds == 0] > 0).any()) and int(ns.max()) > 64
    nodes = nodes_of("8x8x8", 2, 102)
    assert float(nodes[..., 0].min()) < -10.0 and float(nodes[..., 0].max()) > 10.0
    assert float((0.28209479 * nodes[..., 1]).abs().max()) > 30.0


@pytest.mark.parametrize("name", list(GRIDS))
@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("n", COUNTS)
def test_the_kernel_against_the_definition(measured, name, degree, n):
    rows = measured[(name, n, degree)]
    far = max(float(r["rays"][:, 7][torch.isfinite(r["rays"][:, 7])].max()) for r in rows)
    err = {k: max(r["err"][k] for r in rows) for k in ("rgb_map", "acc_map", "depth_map")}
    yard = {k: max(r["yard"][k] for r in rows) for k in ("rgb_map", "acc_map", "depth_map")}
    print(f"\n{name}, {n} rays, degree {degree}: kernel vs float64 definition " + ", ".join(
        f"{k} {err[k]:.3e} (float32 definition {yard[k]:.3e}, ratio {err[k] / max(yard[k], 1e-300):.2f})" for k in err))
    for r in rows:
        rgb, disp, acc, depth, ns, stopped = r["got"]
        assert rgb.shape == (n, 3) and disp.shape == acc.shape == depth.shape == ns.shape == (n,) and ns.dtype == torch.int32
        # exact outputs
        assert torch.equal(ns.cpu(), r["r64"]["n_samples"]), (name, n, degree, r["white"], r["max_steps"])
        assert not bool(stopped.any())
        d, a = depth.cpu(), acc.cpu()
        ratio = d / a
        want = 1.0 / torch.max(torch.full_like(ratio, 1e-10), ratio)
        nan = torch.isnan(want)         # (0 / 0 where nothing has weight: a NaN on both sides, whatever its sign bit)
        assert torch.equal(torch.isnan(disp.cpu()), nan) and torch.equal(nan, a == 0) and bool(nan[empty_of(ns)].all())
        assert bits_equal(disp.cpu()[~nan], want[~nan])
        empty = empty_of(ns)
        assert not bool(a[empty].any()) and not bool(d[empty].any())
        assert torch.equal(rgb.cpu()[empty], torch.full((int(empty.sum()), 3), 1.0 if r["white"] else 0.0))
        assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(acc).all()) and bool(torch.isfinite(depth).all())
    assert err["rgb_map"] <= max(4.0 * yard["rgb_map"], FLOOR), (err, yard)
    assert err["acc_map"] <= max(4.0 * yard["acc_map"], FLOOR), (err, yard)
    assert err["depth_map"] <= max(4.0 * yard["depth_map"], FLOOR * far), (err, yard, far)


def test_render_rays_is_the_kernel_and_counts_its_samples(npa, dev, measured):
    hb = npa.hip_backend
    field = field_of("5x6x7", 1, dev)
    r = measured[("5x6x7", 130, 1)][-1]
    rgb, disp, acc, depth, ns, _ = kernel(hb, field, r["rays"].to(dev), r["u"].to(dev), True)
    out = field.render_rays(r["rays"].to(dev), u=r["u"].to(dev), white_bkgd=True)
    assert list(out) == ["rgb_map", "disp_map", "acc_map", "depth_map"]
    for k, v in zip(out, (rgb, disp, acc, depth)):
        assert bits_equal(out[k], v) and not out[k].requires_grad, k
    assert field.last_stats == {"rays": 130, "samples": int(ns.sum()), "rays_stopped": 0} and field.last_stats["samples"] > 1000
    # a ray record wider than 11 columns is addressed by its stride
    wide = torch.cat([r["rays"], torch.full((130, 3), float("nan"))], -1).to(dev)
    again = field.render_rays(wide, u=r["u"].to(dev), white_bkgd=True)
    assert all(bits_equal(again[k], out[k]) for k in out)


def test_the_stop(npa, dev):
    """on an opaque field: within stop_eps (what is dropped weighs at most T at the stop) plus the kernels' own fp32 noise of the unstopped
    kernel, fewer samples, rays stopped; with stop_eps = 0 a second launch gives the same bits"""
    hb = npa.hip_backend
    eps = 1e-2
    res, lo, hi = box_of("8x8x8")
    grid = OccupancyGrid.from_mask(torch.ones(res, dtype=torch.bool), lo, hi, device=dev)
    nodes = nodes_of("8x8x8", 2, 7)
    nodes[..., 0] = 25.0            # T after one round of 64 steps of 0.02: exp(-32)
    free = BakedField.from_nodes(grid, nodes, 2, step_size=0.02)
    stop = BakedField.from_nodes(grid, nodes, 2, step_size=0.02, stop_eps=eps)
    rays, u, _ = rays_of("8x8x8", 130, 5, True)
    rays, u = rays.to(dev), u.to(dev)
    a = free.render_rays(rays, u=u)
    sa = free.last_stats
    b = stop.render_rays(rays, u=u)
    sb = stop.last_stats
    tol = eps + 1e-5
    assert maxdiff(a["rgb_map"], b["rgb_map"]) <= tol and maxdiff(a["acc_map"], b["acc_map"]) <= tol
    assert sa["rays_stopped"] == 0 and sb["rays_stopped"] > 0 and 0 < sb["samples"] < sa["samples"]
    # the count of a stopped ray is whole rounds' worth of kept candidates: the stop acts between rounds
    ns_free = kernel(hb, free, rays, u, False)[4]
    ns_stop, stopped = kernel(hb, stop, rays, u, False)[4:6]
    assert int(stopped.sum()) == sb["rays_stopped"] and bool((ns_stop <= ns_free).all()) and bool((ns_stop[~stopped] == ns_free[~stopped]).all())
    ref = BakedField.from_nodes(OccupancyGrid.from_mask(torch.ones(res, dtype=torch.bool), lo, hi, device=CPU), nodes, 2, step_size=0.02,
                                stop_eps=eps).render_rays_reference(rays.cpu(), u.cpu())
    clear = (ns_stop.cpu() == ref["n_samples"])         # (a T next to eps may fall either side of it in fp32 and float64)
    assert int(clear.sum()) >= 120
    # deterministic: no atomics
    for f in (free, stop):
        x, y = kernel(hb, f, rays, u, True), kernel(hb, f, rays, u, True)
        assert all(bits_equal(p, q) if p.dtype == torch.float32 else torch.equal(p, q) for p, q in zip(x, y))


def test_no_rays(npa, dev):
    field = field_of("5x6x7", 2, dev)
    out = field.render_rays(torch.zeros(0, 11, device=dev))
    assert out["rgb_map"].shape == (0, 3) and all(out[k].shape == (0,) for k in ("disp_map", "acc_map", "depth_map"))
    assert field.last_stats == {"rays": 0, "samples": 0, "rays_stopped": 0}
