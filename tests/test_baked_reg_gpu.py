"""GPU tests (-m gpu) of the regularisers of a baked field's table (csrc/baked_reg.hip, BakedTrainer.regularizers) against their definition.

THE DEFINITION is float64 autograd of baked.regularizer_reference on the CPU, at the fp32 master's values, of the loss g . (tv_sigma,
tv_sh, sparsity) with three seeded random weights g.  THE YARDSTICK is the same function in float32 against its float64 run (the
project's rule, tests/test_baked_train_gpu.py): over each case set -- one grid, one degree; eps 1e-9 and 1e-2, cubic cells and cells of
edges 0.25 / 0.5 / 1.0 -- the kernels' largest absolute error, in the gradient and in each of the three scalars, may be at most
max(4 x the yardstick's, 2^-22 x the largest |value| of the definition).

Shapes: tests/test_baked_gpu.py's grids 5 x 6 x 7 and 8^3 with its masks, which store 283 of 336 and 612 of 729 nodes; the stored nodes have
0 / 1 / 2 / 3 stored forward neighbours, and as many kinds of backward neighbours, lattice-border nodes among them, so every branch of
the gather occurs; 284 and 613 rows take more than one block and end inside one, and 613 rows end inside a wave at every degree (16 /
4 / 2 rows per wave).
The master is nodes_of's values plus seeded noise, so it is not representable in fp16; row 0 and the padding columns hold noise too,
which must not reach any result."""
import numpy as np
import pytest
import torch

from nerf_pytorch_amd.baked import BakedField
from nerf_pytorch_amd.occupancy import OccupancyGrid
from test_baked_gpu import DS, GRIDS, box_of, field_of, mask_of, nodes_of, rays_of
from test_gpu_occupancy import bits_equal
from test_gpu_parity import dev, maxdiff, npa  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")
F64 = torch.float64
KEYS = ("tv_sigma", "tv_sh", "sparsity")
EPS = (1e-9, 1e-2)
BOXES = ("cubic", "anisotropic")
EDGES = {"cubic": (0.25, 0.25, 0.25), "anisotropic": (0.25, 0.5, 1.0)}
SCALES = {"cubic": (1.0, 1.0, 1.0), "anisotropic": (1.0, 0.5, 0.25)}


def trainer_of(name, degree, box, device, master=True):
    """the trainer of the fixture's mask on a box of the given cell edges; master: nodes_of's values plus noise in every column and row"""
    res, lo, _ = box_of(name)
    hi = tuple(l + e * r for l, e, r in zip(lo, EDGES[box], res))
    grid = OccupancyGrid.from_mask(mask_of(name, 17), lo, hi, device=device)
    nodes = nodes_of(name, degree, 100 + degree)
    trainer = BakedField.from_nodes(grid, nodes, degree, step_size=DS).trainable()
    if master:
        V = nodes.shape[-1]
        stored = BakedField.stored_nodes(OccupancyGrid.from_mask(mask_of(name, 17), lo, hi, device=CPU))
        values = torch.randn(trainer.values.shape, generator=torch.Generator().manual_seed(7 + degree))
        values[1:, :V] = 0.01 * values[1:, :V] + nodes[stored]
        with torch.no_grad():
            trainer.values.copy_(values.to(device))
    return trainer


def neighbour_counts(stored):
    """(forward, backward): per stored node the number of its stored neighbours ahead and behind, as histograms over 0 .. 3"""
    fw, bw = torch.zeros(stored.shape, dtype=torch.int64), torch.zeros(stored.shape, dtype=torch.int64)
    fw[:-1] += stored[1:]
    fw[:, :-1] += stored[:, 1:]
    fw[:, :, :-1] += stored[:, :, 1:]
    bw[1:] += stored[:-1]
    bw[:, 1:] += stored[:, :-1]
    bw[:, :, 1:] += stored[:, :, :-1]
    return [int(((fw == c) & stored).sum()) for c in range(4)], [int(((bw == c) & stored).sum()) for c in range(4)]


def upstream(seed):
    return torch.randn(3, generator=torch.Generator().manual_seed(seed))


def definition(trainer, eps, g, dtype):
    """(the three scalars, autograd's gradient of g . scalars) of the reference at the master's values, in dtype, on the CPU"""
    values = trainer.values.detach().to(dtype).requires_grad_(True)
    out = trainer.regularizers_reference(values, eps, dtype)
    grad, = torch.autograd.grad(sum(g[i].to(dtype) * out[k] for i, k in enumerate(KEYS)), values)
    return torch.stack([out[k].detach() for k in KEYS]), grad


def kernels(trainer, eps, g):
    out = trainer.regularizers(eps)
    grad, = torch.autograd.grad([out[k] for k in KEYS], [trainer.values], [g[i].to(trainer.device) for i in range(3)])
    return torch.stack([out[k].detach() for k in KEYS]), grad


def measure(cpu, gpu, eps, seed):
    g = upstream(seed)
    s64, g64 = definition(cpu, eps, g, F64)
    s32, g32 = definition(cpu, eps, g, torch.float32)
    s, grad = kernels(gpu, eps, g)
    row = dict(eps=eps, g=g, s64=s64, g64=g64, s=s, grad=grad, err=maxdiff(grad, g64), yard=maxdiff(g32, g64), top=float(g64.abs().max()))
    for i, k in enumerate(KEYS):
        row[k] = dict(err=maxdiff(s[i], s64[i]), yard=maxdiff(s32[i], s64[i]), top=abs(float(s64[i])))
    return row


def within(rows, label):
    for what, pick in [("gradient", lambda r: r)] + [(k, lambda r, k=k: r[k]) for k in KEYS]:
        err, yard, top = max(pick(r)["err"] for r in rows), max(pick(r)["yard"] for r in rows), max(pick(r)["top"] for r in rows)
        print(f"\n{label}, {what}: kernels vs float64 {err:.3e} (float32 {yard:.3e}, ratio {err / max(yard, 1e-300):.2f}; "
              f"largest |value| {top:.3e}, floor {2.0 ** -22 * top:.3e})")
        assert err <= max(4.0 * yard, 2.0 ** -22 * top), (label, what, err, yard, top)


@pytest.fixture(scope="module")
def measured(npa, dev):
    """every case once: {(grid, degree): [rows]} in the order of EPS x BOXES, and the trainers {(grid, degree, box): (cpu, gpu)}"""
    out, trainers = {}, {}
    for name in GRIDS:
        for degree in (0, 1, 2):
            for box in BOXES:
                trainers[(name, degree, box)] = (trainer_of(name, degree, box, CPU), trainer_of(name, degree, box, dev))
            for i, eps in enumerate(EPS):
                for j, box in enumerate(BOXES):
                    cpu, gpu = trainers[(name, degree, box)]
                    out.setdefault((name, degree), []).append(dict(measure(cpu, gpu, eps, 11 * degree + 2 * i + j), box=box))
    return out, trainers


def test_the_fixtures_hold_every_branch_of_the_gather():
    """on the CPU: the stored nodes, their forward and backward neighbours, and the partly filled last wave"""
    want = {"5x6x7": (283, 336, [7, 25, 85, 166], [9, 22, 85, 167]), "8x8x8": (612, 729, [8, 53, 169, 382], [9, 46, 180, 377])}
    for name in GRIDS:
        for box in BOXES:
            trainer = trainer_of(name, 0, box, CPU, master=False)
            stored = (trainer.index > 0).view(trainer._field.node_resolution)
            n, total, ahead, behind = want[name]
            assert (int(stored.sum()), stored.numel(), trainer.n_rows) == (n, total, n + 1)
            assert neighbour_counts(stored) == (ahead, behind), (name, neighbour_counts(stored))
            assert trainer.axis_scale == SCALES[box]
            # border nodes that are stored: a neighbour outside the lattice on either side of every axis
            assert all(bool(stored.select(a, 0).any()) and bool(stored.select(a, -1).any()) for a in range(3))
    # 284 and 613 rows: more than one block and a partly filled last block at every row width; 613 rows end inside a wave at every width
    for W in (4, 16, 32):
        assert all(rows * W > 256 and (rows * W) % 256 != 0 for rows in (284, 613)) and (613 * W) % 64 != 0


@pytest.mark.parametrize("name", list(GRIDS))
@pytest.mark.parametrize("degree", [0, 1, 2])
def test_the_losses_and_the_gradient_against_the_definition(measured, name, degree):
    rows = measured[0][(name, degree)]
    assert [(r["eps"], r["box"]) for r in rows] == [(e, b) for e in EPS for b in BOXES]
    for r in rows:
        assert r["grad"].shape == r["g64"].shape and r["grad"].dtype == torch.float32 and bool(torch.isfinite(r["grad"]).all())
        assert r["s"].dtype == torch.float32 and r["s"].shape == (3,) and r["top"] > 0.0 and all(r[k]["top"] > 0.0 for k in KEYS)
    within(rows, f"{name}, degree {degree}")


def test_exact_zeros(npa, dev, measured):
    rows, trainers = measured
    for (name, degree), rs in rows.items():
        V = 1 + 3 * (degree + 1) ** 2
        for r in rs:
            grad = r["grad"].cpu()
            assert not bool(grad[0].any()) and not bool(grad[:, V:].any()) and bool(grad[1:, :V].any())
        # the sparsity term alone: nothing outside column 0, nothing in a row of negative density
        gpu = trainers[(name, degree, "cubic")][1]
        _, grad = kernels(gpu, 1e-9, torch.tensor([0.0, 0.0, 1.0]))
        sigma = gpu.values.detach()[:, 0].cpu()
        negative, positive = sigma < 0, sigma > 0
        negative[0] = positive[0] = False
        grad = grad.cpu()
        assert int(negative.sum()) > 50 and int(positive.sum()) > 50
        assert not bool(grad[negative].any()) and not bool(grad[:, 1:].any()) and not bool(grad[0].any()) and bool((grad[positive, 0] > 0).all())


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_a_constant_master(npa, dev, degree):
    """every difference is 0: a bit-exact zero TV gradient; every term is sqrtf(eps), so tv_sigma is that value exactly and tv_sh within
    the log2(W) fp32 additions of the row's butterfly (2^-24 relative each)"""
    hb = npa.hip_backend
    trainer = trainer_of("5x6x7", degree, "anisotropic", dev, master=False)
    B, V = trainer.n_basis, 1 + 3 * trainer.n_basis
    row = torch.tensor([1.7] + [0.3] * B + [-0.2] * B + [0.1] * B, device=dev)
    with torch.no_grad():
        trainer.values[1:, :V] = row
    for eps in (1e-9, 1e-2):
        root = float(np.sqrt(np.float32(eps)))
        terms = hb.baked_reg_fwd(trainer.grid._desc(), trainer.index, trainer.row_node, trainer.values.detach(), degree, trainer.axis_scale, eps)
        assert terms.shape == (trainer.n_rows, 3) and not bool(terms[0].any()) and bool((terms[1:, 0] == root).all())
        out, grad = kernels(trainer, eps, torch.tensor([1.0, 1.0, 0.0]))
        assert float(out[0]) == root and abs(float(out[1]) - root) <= 5 * 2.0 ** -24 * root
        assert grad.shape == trainer.values.shape and not bool(grad.any())
        assert abs(float(out[2]) - np.log1p(2.0 * 1.7 ** 2)) <= 2.0 ** -22 * 2.0


def test_an_empty_grid_and_a_single_cell(npa, dev):
    # no occupied cell: one row, three zeros, a zero gradient of the table's shape
    grid = OccupancyGrid.from_mask(torch.zeros((3, 2, 2), dtype=torch.bool), [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], device=dev)
    trainer = BakedField.from_nodes(grid, torch.ones(4, 3, 3, 13), 1).trainable()
    assert trainer.n_rows == 1
    with torch.no_grad():
        trainer.values.fill_(3.0)               # row 0 is never read
    out = trainer.regularizers()
    assert all(out[k].dtype == torch.float32 and out[k].dim() == 0 and float(out[k].detach()) == 0.0 for k in KEYS)
    sum(out.values()).backward()
    assert trainer.values.grad.shape == (1, 16) and not bool(trainer.values.grad.any())
    # one occupied cell in the middle of a 3 x 3 x 3 grid: eight rows, each with 0 .. 3 neighbours ahead and 3 .. 0 behind
    rows = []
    for degree in (0, 1, 2):
        mask = torch.zeros((3, 3, 3), dtype=torch.bool)
        mask[1, 1, 1] = True
        V = 1 + 3 * (degree + 1) ** 2
        make = lambda d: BakedField.from_nodes(OccupancyGrid.from_mask(mask, [0.0, 0.0, 0.0], [0.75, 1.5, 3.0], device=d),
                                               torch.zeros(4, 4, 4, V), degree).trainable()
        cpu, gpu = make(CPU), make(dev)
        assert cpu.n_rows == 9 and cpu.axis_scale == (1.0, 0.5, 0.25)
        values = torch.randn(cpu.values.shape, generator=torch.Generator().manual_seed(degree))
        with torch.no_grad():
            cpu.values.copy_(values)
            gpu.values.copy_(values.to(dev))
        rows += [measure(cpu, gpu, eps, 5 + degree) for eps in EPS]
        assert not bool(rows[-1]["grad"][0].any()) and not bool(rows[-1]["grad"][:, V:].any()) and bool(rows[-1]["grad"][1:, :V].all())
    within(rows, "a single cell, degrees 0 1 2")


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_two_calls_give_the_same_bits(npa, dev, measured, degree):
    rows, trainers = measured
    for name in GRIDS:
        r = rows[(name, degree)][1]             # eps = 1e-9, anisotropic
        gpu = trainers[(name, degree, "anisotropic")][1]
        a, b = kernels(gpu, r["eps"], r["g"]), kernels(gpu, r["eps"], r["g"])
        assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1]) and bits_equal(a[0], r["s"]) and bits_equal(a[1], r["grad"]) and bool(a[1].any())


def test_under_no_grad_only_the_forward_runs(npa, dev, measured):
    hb = npa.hip_backend
    gpu = measured[1][("8x8x8", 1, "cubic")][1]
    assert hb.TIMER is None
    hb.TIMER = hb.KernelTimer()
    try:
        with torch.no_grad():
            out = gpu.regularizers()
        quiet = [r[0] for r in hb.TIMER.records]
        out2 = gpu.regularizers()
        sum(out2.values()).backward()
        both = [r[0] for r in hb.TIMER.records]
        summary = hb.TIMER.summary()
    finally:
        hb.TIMER = None
    gpu.values.grad = None
    assert quiet == ["baked_reg_fwd_kernel"] and both == ["baked_reg_fwd_kernel"] * 2 + ["baked_reg_bwd_kernel"]
    assert not any(out[k].requires_grad for k in KEYS) and all(out2[k].requires_grad and bits_equal(out[k], out2[k].detach()) for k in KEYS)
    rows, nodes = gpu.n_rows, gpu.index.numel()
    assert summary["baked_reg_fwd_kernel"]["bytes"] == 2 * (64.0 * rows + 12.0 * rows + 4.0 * rows + 4.0 * nodes)
    assert summary["baked_reg_bwd_kernel"]["bytes"] == 128.0 * rows + 4.0 * rows + 4.0 * nodes


def test_adam_on_the_total_variation_lowers_it(npa, dev):
    trainer = trainer_of("8x8x8", 1, "cubic", dev)
    opt = torch.optim.Adam(trainer.parameters(), lr=0.05)
    seen = []
    for _ in range(20):
        opt.zero_grad()
        reg = trainer.regularizers()
        (reg["tv_sigma"] + reg["tv_sh"]).backward()
        opt.step()
        trainer.commit()
        seen.append((float(reg["tv_sigma"].detach()), float(reg["tv_sh"].detach())))
    with torch.no_grad():
        last = trainer.regularizers()
    print(f"\ntv_sigma {seen[0][0]:.4f} -> {float(last['tv_sigma']):.4f}, tv_sh {seen[0][1]:.4f} -> {float(last['tv_sh']):.4f} in 20 Adam steps")
    assert float(last["tv_sigma"]) < seen[0][0] and float(last["tv_sh"]) < seen[0][1]
    assert all(b[0] < a[0] and b[1] < a[1] for a, b in zip(seen, seen[1:]))


def test_the_loop_closes_with_the_regularisers(npa, dev):
    """5 steps of mse(render_rays) + lambda . regularizers with commit(); the committed table renders the trainer's bits"""
    teacher = field_of("8x8x8", 1, dev)
    rays, u, _ = rays_of("8x8x8", 130, 11, True)
    rays, u = rays.to(dev), u.to(dev)
    target = teacher.render_rays(rays, u=u)["rgb_map"]
    trainer = teacher.trainable()
    opt = torch.optim.Adam(trainer.parameters(), lr=0.05)
    for _ in range(5):
        opt.zero_grad()
        reg = trainer.regularizers()
        loss = ((trainer.render_rays(rays, u)["rgb_map"] - target) ** 2).mean() + 1e-3 * reg["tv_sigma"] + 1e-4 * reg["tv_sh"] + 1e-5 * reg["sparsity"]
        loss.backward()
        assert trainer.values.grad is not None and bool(torch.isfinite(trainer.values.grad).all()) and bool(trainer.values.grad.any())
        opt.step()
        trainer.commit()
    assert bool(torch.isfinite(loss.detach()))
    with torch.no_grad():
        last = trainer.render_rays(rays, u)
    field = trainer.to_field()
    got = field.render_rays(rays, u=u)
    assert all(bits_equal(got[k], last[k]) for k in ("rgb_map", "acc_map", "depth_map")) and not torch.equal(field.table, teacher.table)
