"""GPU tests (-m gpu) of the baked field's training path (csrc/baked_train.hip, baked.BakedTrainer) against its definition.

FORWARD: the trainer's rgb_map / acc_map / depth_map are nerf_baked_render's bits with stop_eps = 0 and nerf_baked_count is its n_samples.

GRADIENT.  THE DEFINITION is float64 autograd of BakedTrainer.render_rays_reference on the CPU, at the fp16 table's values, of the loss
sum G . rgb_map + g_acc acc_map + g_depth depth_map with seeded random G, g_acc, g_depth.  THE YARDSTICK is the same autograd in float32
against float64 (the project's rule, tests/test_gpu_distortion.py, tests/test_baked_gpu.py): over each case set -- one grid, one ray
count, one degree; u None and given, white_bkgd off and on -- the kernels' largest absolute error over the table's gradient may be at
most max(4 x the yardstick's, 2^-22 x the largest |gradient| of the definition).
Condition on the inputs, asserted: no kept sample's float64 blend has |v0| < 1e-4 -- an fp32 blend on the other side of the ReLU's kink
would change the gradient by O(1) and say nothing about the kernels.  The seed of the node values is chosen on the CPU, per grid and
degree, as the first one from 100 + degree on at which every case of the set meets the condition; no sample is left out.

Shapes: tests/test_baked_gpu.py's -- grids 5 x 6 x 7 and 8^3 at DS = 0.02, 1 / 5 / 130 rays of the ten kinds (63 / 64 / 65 / 130
candidates, axis rays on cell planes, a miss, invalid rays): the smallest at which rounds of 64 records, partly filled blocks and edge
nodes can go wrong."""
import numpy as np
import pytest
import torch

from nerf_pytorch_amd.baked import BakedField
from nerf_pytorch_amd.occupancy import OccupancyGrid
from test_baked_gpu import COUNTS, DS, GRIDS, KINDS, box_of, field_of, mask_of, nodes_of, rays_of
from test_gpu_occupancy import bits_equal
from test_gpu_parity import dev, maxdiff, npa  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")
F64 = torch.float64
KINK = 1e-4
OUT = ("rgb_map", "acc_map", "depth_map")


def kept_blend(field, rays, u, max_steps=1 << 14):
    """(v0 float64 [S], cell int64 [S]) of the kept samples of `rays`: the reference's geometry (its fp32 expressions) and its blend of
    the sigma column in float64"""
    grid = field.grid
    r, ok, uu, dn, M, _ = OccupancyGrid._march_rays("test", rays, u, max_steps, 1)
    dz = torch.tensor(field.step_size, dtype=torch.float32) / dn
    z, valid = OccupancyGrid._world_steps(r, ok & torch.isfinite(dz[:, 0]) & (dz[:, 0] > 0), uu, dz, M)
    pts = r[:, None, 0:3] + r[:, None, 3:6] * z[:, :, None]
    f32 = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))
    t = (pts - f32(grid.lo)) * f32(grid.scale)
    inside, _, bit = grid._classify(pts)
    rows, cols = (valid & inside & bit).nonzero(as_tuple=True)
    tk = t[rows, cols]
    cell = torch.floor(tk)
    f, ci = (tk - cell).to(F64), cell.to(torch.int64)
    ny, nz = grid.resolution[1] + 1, grid.resolution[2] + 1
    sigma = field.table[:, 0].to(F64)
    v0 = torch.zeros(rows.numel(), dtype=F64)
    for c in range(8):
        ox, oy, oz = (c >> 2) & 1, (c >> 1) & 1, c & 1
        node = ((ci[:, 0] + ox) * ny + (ci[:, 1] + oy)) * nz + (ci[:, 2] + oz)
        w = (f[:, 0] if ox else 1.0 - f[:, 0]) * (f[:, 1] if oy else 1.0 - f[:, 1]) * (f[:, 2] if oz else 1.0 - f[:, 2])
        v0 = v0 + w * sigma[field.index[node].to(torch.int64)]
    return v0, (ci[:, 0] * grid.resolution[1] + ci[:, 1]) * grid.resolution[2] + ci[:, 2]


def cases_of(name, degree):
    """[(n, rays, u, white)]: the case sets of one grid and degree"""
    out = []
    for n in COUNTS:
        for with_u in (False, True):
            rays, u, _ = rays_of(name, n, 1000 * n + degree, with_u)
            out += [(n, rays, u, white) for white in (False, True)]
    return out


def fields_of(name, degree, device):
    """(the CPU field, the same field on `device`, its node seed): the first seed at which no kept sample of any case lies at the kink"""
    res, lo, hi = box_of(name)
    cases = cases_of(name, degree)
    for seed in range(100 + degree, 140 + degree):
        make = lambda d: BakedField.from_nodes(OccupancyGrid.from_mask(mask_of(name, 17), lo, hi, device=d), nodes_of(name, degree, seed), degree,
                                               step_size=DS)
        cpu = make(CPU)
        blends = [kept_blend(cpu, rays, u)[0] for n, rays, u, white in cases if not white]
        if all(v0.numel() == 0 or float(v0.abs().min()) >= KINK for v0 in blends):
            return cpu, make(device), seed
    raise AssertionError("no node seed keeps every kept sample off the ReLU's kink")


def upstream(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)


def definition(trainer, rays, u, white, G, dtype):
    """autograd's gradient of the reference at the fp16 table's values, in dtype, on the CPU"""
    values = trainer.table.to(dtype).requires_grad_(True)
    out = trainer.render_rays_reference(rays, u, white, dtype=dtype, values=values)
    loss = (out["rgb_map"] * G[0].to(dtype)).sum() + (out["acc_map"] * G[1].to(dtype)).sum() + (out["depth_map"] * G[2].to(dtype)).sum()
    grad, = torch.autograd.grad(loss, values, allow_unused=True)
    return torch.zeros_like(values) if grad is None else grad


def kernels(trainer, rays, u, white, G, max_steps=1 << 14):
    """(the outputs, the gradient of `values`) of the trainer on the GPU"""
    d = trainer.device
    out = trainer.render_rays(rays.to(d), None if u is None else u.to(d), white, max_steps)
    grad, = torch.autograd.grad([out[k] for k in OUT], [trainer.values], [g.to(d) for g in G], retain_graph=True)
    return out, grad


def measure(cpu_trainer, gpu_trainer, rays, u, white, seed):
    n = rays.shape[0]
    G = upstream(n, seed)
    g64 = definition(cpu_trainer, rays, u, white, G, F64)
    g32 = definition(cpu_trainer, rays, u, white, G, torch.float32)
    out, grad = kernels(gpu_trainer, rays, u, white, G)
    return dict(n=n, rays=rays, u=u, white=white, G=G, g64=g64, out=out, grad=grad, stats=dict(gpu_trainer.last_stats),
                err=maxdiff(grad, g64), yard=maxdiff(g32, g64), top=float(g64.abs().max()))


def within(rows, label):
    err, yard, top = max(r["err"] for r in rows), max(r["yard"] for r in rows), max(r["top"] for r in rows)
    print(f"\n{label}: kernels vs float64 autograd {err:.3e} (float32 autograd {yard:.3e}, ratio {err / max(yard, 1e-300):.2f}; "
          f"largest |gradient| {top:.3e}, floor {2.0 ** -22 * top:.3e})")
    assert err <= max(4.0 * yard, 2.0 ** -22 * top), (label, err, yard, top)


@pytest.fixture(scope="module")
def measured(npa, dev):
    """every case once: {(grid, n, degree): [rows]} and the fields {(grid, degree): (cpu, gpu, seed)}"""
    out, fields = {}, {}
    for name in GRIDS:
        for degree in (0, 1, 2):
            cpu, gpu, seed = fields_of(name, degree, dev)
            fields[(name, degree)] = (cpu, gpu, seed)
            ct, gt = cpu.trainable(), gpu.trainable()
            for i, (n, rays, u, white) in enumerate(cases_of(name, degree)):
                out.setdefault((name, n, degree), []).append(measure(ct, gt, rays, u, white, 7 * i + degree))
    return out, fields


def test_the_condition_on_the_inputs(measured):
    """no kept sample at the kink, none left out, and the sigma column of the kept samples takes both signs"""
    rows, fields = measured
    for (name, n, degree), rs in rows.items():
        cpu = fields[(name, degree)][0]
        for r in rs:
            v0, _ = kept_blend(cpu, r["rays"], r["u"])
            assert v0.numel() == r["stats"]["samples"] and r["stats"]["rays"] == n
            assert v0.numel() == 0 or float(v0.abs().min()) >= KINK, (name, n, degree, fields[(name, degree)][2])
            if n == 130:
                assert float(v0.min()) < -1.0 and float(v0.max()) > 1.0 and v0.numel() > 1000


@pytest.mark.parametrize("name", list(GRIDS))
@pytest.mark.parametrize("degree", [0, 1, 2])
def test_the_forward_is_the_render_without_a_stop(npa, dev, measured, name, degree):
    hb = npa.hip_backend
    rows, fields = measured
    field = fields[(name, degree)][1]
    desc = field.grid._desc()
    for n in COUNTS:
        for r in rows[(name, n, degree)]:
            rays, u = r["rays"].to(dev), None if r["u"] is None else r["u"].to(dev)
            rgb, _, acc, depth, ns, stopped = hb.baked_render(desc, field.index, field.table, degree, rays, u, DS, 1 << 14, 0.0, r["white"])
            assert list(r["out"]) == list(OUT) and all(r["out"][k].requires_grad for k in OUT)
            assert bits_equal(r["out"]["rgb_map"], rgb) and bits_equal(r["out"]["acc_map"], acc) and bits_equal(r["out"]["depth_map"], depth)
            counts = hb.baked_count(desc, rays, u, DS, 1 << 14)
            assert counts.dtype == torch.int32 and torch.equal(counts, ns) and not bool(stopped.any())
            assert r["stats"] == {"rays": n, "samples": int(ns.sum())}
    # a shorter walk, a field whose stop_eps is set (never used in training) and a wider ray record; under no_grad nothing carries grad
    r = rows[(name, 130, degree)][-1]
    rays, u = r["rays"].to(dev), r["u"].to(dev)
    stopping = BakedField(field.grid, field.index, field.table, degree, DS, stop_eps=0.5).trainable()
    wide = torch.cat([rays, torch.full((130, 2), float("nan"), device=dev)], -1)
    for max_steps in (64, 100):
        rgb, _, acc, depth, ns, _ = hb.baked_render(desc, field.index, field.table, degree, rays, u, DS, max_steps, 0.0, True)
        assert torch.equal(hb.baked_count(desc, wide, u, DS, max_steps), ns)
        with torch.no_grad():
            got = stopping.render_rays(wide, u, True, max_steps)
        assert not any(got[k].requires_grad for k in OUT)
        assert bits_equal(got["rgb_map"], rgb) and bits_equal(got["acc_map"], acc) and bits_equal(got["depth_map"], depth)


@pytest.mark.parametrize("name", list(GRIDS))
@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("n", COUNTS)
def test_the_gradient_against_the_definition(measured, name, degree, n):
    rows = measured[0][(name, n, degree)]
    assert len(rows) == 4 and [r["white"] for r in rows] == [False, True, False, True] and rows[0]["u"] is None and rows[2]["u"] is not None
    for r in rows:
        assert r["grad"].shape == r["g64"].shape and r["grad"].dtype == torch.float32 and bool(torch.isfinite(r["grad"]).all())
    if n > 1:
        assert max(r["top"] for r in rows) > 0.0
    within(rows, f"{name}, {n} rays, degree {degree}")


def test_exact_zeros(npa, dev, measured):
    rows, fields = measured
    for (name, n, degree), rs in rows.items():
        cpu = fields[(name, degree)][0]
        V = 1 + 3 * (degree + 1) ** 2
        res = cpu.grid.resolution
        ny, nz = res[1] + 1, res[2] + 1
        for r in rs:
            grad = r["grad"].cpu()
            assert not bool(grad[0].any()) and not bool(grad[:, V:].any())
            _, cells = kept_blend(cpu, r["rays"], r["u"])
            cells = torch.unique(cells)
            ix, iy, iz = cells // (res[1] * res[2]), (cells // res[2]) % res[1], cells % res[2]
            touched = torch.zeros(cpu.n_rows, dtype=torch.bool)
            for c in range(8):
                touched[cpu.index[((ix + ((c >> 2) & 1)) * ny + iy + ((c >> 1) & 1)) * nz + iz + (c & 1)].to(torch.int64)] = True
            assert not bool(grad[~touched].any()), (name, n, degree)
            if n == 130:
                assert 10 < int(touched.sum()) and bool(grad[touched][:, :V].any())
    # only rays that miss or are invalid: an all-zero gradient; no rays at all: the same
    cpu, gpu, _ = fields[("8x8x8", 1)]
    rays, u, _ = rays_of("8x8x8", 130, 4, True)
    empty = torch.arange(130) % len(KINDS) >= 8
    trainer = gpu.trainable()
    for rr, uu in ((rays[empty], u[empty]), (rays[:0], u[:0]), (rays[:0], None)):
        out, grad = kernels(trainer, rr, uu, True, upstream(rr.shape[0], 1))
        assert trainer.last_stats == {"rays": rr.shape[0], "samples": 0}
        assert out["rgb_map"].shape == (rr.shape[0], 3) and bool((out["rgb_map"] == 1.0).all()) and not bool(out["acc_map"].any())
        assert grad.shape == trainer.values.shape and not bool(grad.any())
        (out["rgb_map"].sum() + out["depth_map"].sum()).backward()          # through .backward() as well: a zero .grad, not None
        assert trainer.values.grad is not None and not bool(trainer.values.grad.any())
        trainer.values.grad = None


def test_saturation(npa, dev):
    """the opaque field of test_baked_gpu.test_the_stop (sigma = 25: T after one round of 64 steps is exp(-32)): finite, within the tolerance"""
    res, lo, hi = box_of("8x8x8")
    nodes = nodes_of("8x8x8", 2, 7)
    nodes[..., 0] = 25.0
    make = lambda d: BakedField.from_nodes(OccupancyGrid.from_mask(torch.ones(res, dtype=torch.bool), lo, hi, device=d), nodes, 2, step_size=0.02)
    ct, gt = make(CPU).trainable(), make(dev).trainable()
    rays, u, _ = rays_of("8x8x8", 130, 5, True)
    rows = [measure(ct, gt, rays, u, white, 3 + white) for white in (False, True)]
    for r in rows:
        assert bool(torch.isfinite(r["grad"]).all()) and r["top"] > 0.0 and r["stats"]["samples"] > 64 * 50
    within(rows, "sigma = 25, 130 rays, degree 2")


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_two_backward_calls_give_the_same_bits(npa, dev, measured, degree):
    rows, fields = measured
    for name in GRIDS:
        trainer = fields[(name, degree)][1].trainable()
        r = rows[(name, 130, degree)][-1]
        a = kernels(trainer, r["rays"], r["u"], r["white"], r["G"])[1]
        b = kernels(trainer, r["rays"], r["u"], r["white"], r["G"])[1]
        assert bits_equal(a, b) and bits_equal(a, r["grad"]) and bool(a.any())


def test_the_loop_closes(npa, dev):
    """20 Adam steps of a noised copy towards its teacher's rgb_map lower the loss; the committed table renders the trainer's bits"""
    teacher = field_of("8x8x8", 1, dev)
    rays, u, _ = rays_of("8x8x8", 130, 11, True)
    rays, u = rays.to(dev), u.to(dev)
    target = teacher.render_rays(rays, u=u)["rgb_map"]
    trainer = teacher.trainable()
    with torch.no_grad():
        trainer.values[1:, :13] += (0.5 * torch.randn(trainer.values[1:, :13].shape, generator=torch.Generator().manual_seed(3))).to(dev)
    trainer.commit()
    opt = torch.optim.Adam(trainer.parameters(), lr=0.05)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = ((trainer.render_rays(rays, u)["rgb_map"] - target) ** 2).mean()
        loss.backward()
        opt.step()
        trainer.commit()
        losses.append(float(loss.detach()))
    print(f"\nloss {losses[0]:.4e} -> {losses[-1]:.4e} in 20 Adam steps (ratio {losses[-1] / losses[0]:.3f})")
    assert losses[-1] < losses[0]
    with torch.no_grad():
        last = trainer.render_rays(rays, u)
    field = trainer.to_field()
    got = field.render_rays(rays, u=u)
    assert all(bits_equal(got[k], last[k]) for k in OUT) and field.last_stats["samples"] == trainer.last_stats["samples"]
