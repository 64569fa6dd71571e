"""CPU: fine-tuning a baked field without a GPU -- BakedTrainer.render_rays_reference against BakedField's and against autograd's own
checks, the closed form of one ray through a constant field, the inverted index against a brute-force loop, commit(), checkpoints,
to_field(), and the export of the four entry points of csrc/baked_train.hip with their argument errors."""
import ctypes
import io
import math
import os

import pytest
import torch

import nerf_pytorch_amd as npa
from nerf_pytorch_amd.baked import BakedField, BakedTrainer, inverted_index
from test_baked_cpu import constant_field, unit_grid, x_ray
from test_baked_gpu import field_of, rays_of

CPU = torch.device("cpu")
F64 = torch.float64
NAN, INF = float("nan"), float("inf")
NEW = ("nerf_baked_count", "nerf_baked_train_fwd", "nerf_baked_train_bwd_samples", "nerf_baked_train_bwd_rows")


def bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64 if a.dtype == F64 else torch.int32),
                                                                      b.contiguous().view(torch.int64 if b.dtype == F64 else torch.int32))


def small_trainer(seed=0, degree=1):
    """a 2 x 2 x 2 grid, every cell occupied, sigma well above the ReLU's kink"""
    g = torch.Generator().manual_seed(seed)
    nodes = torch.randn(3, 3, 3, 1 + 3 * (degree + 1) ** 2, generator=g)
    nodes[..., 0] = 1.0 + 2.0 * torch.rand(3, 3, 3, generator=g)
    return BakedField.from_nodes(unit_grid(2), nodes, degree).trainable()


def through_the_box(n, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([-0.5, 0.3, 0.4]) + 0.2 * torch.rand(n, 3, generator=g)
    target = 0.2 + 0.6 * torch.rand(n, 3, generator=g)
    d = target - o
    view = torch.randn(n, 3, generator=g)
    return torch.cat([o, d, torch.zeros(n, 1), torch.full((n, 1), 2.5), view / view.norm(dim=-1, keepdim=True)], -1)


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("degree", [0, 1, 2])
def test_the_reference_is_the_fields_reference_without_a_stop(degree):
    rays, u, _ = rays_of("5x6x7", 130, 3 + degree, True)
    plain = field_of("5x6x7", degree, CPU)
    stopping = field_of("5x6x7", degree, CPU, stop_eps=0.25)
    for white in (False, True):
        for dtype in (F64, torch.float32):
            want = plain.render_rays_reference(rays, u, white, 1 << 14, dtype)
            assert int(want["n_samples"].sum()) > 1000
            for field in (plain, stopping):          # a field's stop_eps is carried, never used
                trainer = field.trainable()
                assert isinstance(trainer, BakedTrainer) and trainer.stop_eps == field.stop_eps
                got = trainer.render_rays_reference(rays, u, white, dtype=dtype)
                assert list(got) == ["rgb_map", "acc_map", "depth_map", "n_samples"]
                assert torch.equal(got["n_samples"], want["n_samples"])
                assert all(bits(got[k], want[k]) for k in ("rgb_map", "acc_map", "depth_map"))
                # values standing in for the table: the same numbers give the same bits
                again = trainer.render_rays_reference(rays, u, white, dtype=dtype, values=trainer.table.to(dtype))
                assert all(bits(again[k], want[k]) for k in ("rgb_map", "acc_map", "depth_map"))
    assert stopping.render_rays_reference(rays, u)["rays_stopped"] > 0


def test_gradcheck_of_the_reference():
    trainer = small_trainer()
    rays = through_the_box(3, 5)
    assert int(trainer.render_rays_reference(rays)["n_samples"].min()) >= 2
    values = trainer.table.to(F64).requires_grad_(True)

    def fn(v):
        out = trainer.render_rays_reference(rays, white_bkgd=True, values=v)
        return torch.cat([out["rgb_map"].reshape(-1), out["acc_map"], out["depth_map"]])
    assert torch.autograd.gradcheck(fn, (values,), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_one_ray_through_a_constant_field_against_the_closed_form():
    """acc = 1 - exp(-sigma n ds) up to the 1e-10 terms, and every sample's corner weights add up to 1: the gradient's sigma column adds
    up to d acc / d sigma = n ds exp(-sigma n ds); the colours are constant, so acc carries no gradient to them"""
    sigma = 1.5
    trainer = constant_field(sigma, (0.3, -0.2, 0.1), degree=1).trainable()
    rays = torch.tensor([x_ray(0.3, 0.6)])
    values = trainer.table.to(F64).requires_grad_(True)
    out = trainer.render_rays_reference(rays, values=values)
    n, ds = int(out["n_samples"][0]), float(torch.tensor(trainer.step_size, dtype=torch.float32))
    assert n == 8 and ds == 0.125
    assert abs(float(out["acc_map"][0].detach()) - (1.0 - math.exp(-sigma * n * ds))) <= 1e-8
    out["acc_map"].sum().backward()
    want = n * ds * math.exp(-sigma * n * ds)
    assert abs(float(values.grad[:, 0].sum()) - want) <= 1e-8 * want + 1e-9
    assert float(values.grad[:, 1:].abs().max()) == 0.0 and float(values.grad[0].abs().max()) == 0.0
    # depth: sum w z has d/dsigma by the same closed form, checked against a finite difference of the formula itself
    z = [1.0 + (k + 0.5) * ds for k in range(n)]
    depth = lambda s: sum((1.0 - math.exp(-s * ds)) * math.exp(-s * ds * k) * z[k] for k in range(n))
    values.grad = None
    trainer.render_rays_reference(rays, values=values)["depth_map"].sum().backward()
    fd = (depth(sigma + 1e-6) - depth(sigma - 1e-6)) / 2e-6
    assert abs(float(values.grad[:, 0].sum()) - fd) <= 1e-7


# ------------------------------------------------------------------------------------------------ the inverted index
def test_the_inverted_index_against_a_loop():
    g = torch.Generator().manual_seed(9)
    for n_cells, S in ((7, 0), (7, 1), (30, 500), (3, 64)):
        cells = torch.randint(0, n_cells, (S,), generator=g, dtype=torch.int32)
        order, start = inverted_index(cells, n_cells)
        assert order.dtype == start.dtype == torch.int32 and order.shape == (S,) and start.shape == (n_cells + 1,)
        want_order, want_start = [], [0]
        for c in range(n_cells):
            want_order += [s for s in range(S) if int(cells[s]) == c]         # ascending sample number inside a cell: (ray, k)
            want_start.append(len(want_order))
        assert order.tolist() == want_order and start.tolist() == want_start


# ------------------------------------------------------------------------------------------------ the trainer object
def test_the_trainer_holds_a_master_copy_and_the_inverse_of_the_index():
    field = field_of("5x6x7", 1, CPU)
    trainer = field.trainable()
    assert isinstance(trainer.values, torch.nn.Parameter) and trainer.values.dtype == torch.float32 and trainer.values.requires_grad
    assert trainer.values.shape == (field.n_rows, 16) and torch.equal(trainer.values.detach(), field.table.float())
    assert trainer.parameters() == [trainer.values] and trainer.parameters()[0] is trainer.values
    assert trainer.table.dtype == torch.float16 and torch.equal(trainer.table, field.table) and trainer.table is not field.table
    assert trainer.sh_degree == 1 and trainer.step_size == field.step_size and trainer.grid is not field.grid
    assert trainer.row_node.dtype == torch.int32 and trainer.row_node.shape == (field.n_rows,) and int(trainer.row_node[0]) == -1
    nodes = trainer.row_node[1:].to(torch.int64)
    assert torch.equal(field.index[nodes], torch.arange(1, field.n_rows, dtype=torch.int32))
    assert int((field.index > 0).sum()) == field.n_rows - 1
    with pytest.raises(ValueError, match="BakedField"):
        BakedTrainer(trainer)


def test_commit_zeroes_rounds_and_clamps():
    trainer = field_of("8x8x8", 1, CPU).trainable()
    V = 13
    with torch.no_grad():
        trainer.values += 0.3 * torch.randn(trainer.values.shape, generator=torch.Generator().manual_seed(2))
        trainer.values[5, 2] = INF
        trainer.values[6, 0] = -INF
        trainer.values[7, 3] = 1e6
        master = trainer.values.detach().clone()
    assert bool(trainer.values[0].abs().max() > 0) and bool(trainer.values[:, V:].abs().max() > 0)
    assert trainer.commit() is trainer
    v = trainer.values.detach()
    assert not bool(v[0].any()) and not bool(v[:, V:].any()) and not bool(trainer.table[0].any()) and not bool(trainer.table[:, V:].any())
    assert float(v[5, 2]) == 65504.0 and float(v[6, 0]) == -65504.0 and float(v[7, 3]) == 65504.0
    assert bool(torch.isfinite(trainer.table).all())
    assert torch.equal(trainer.table, v.to(torch.float16))                      # the table is the rounded master ...
    keep = torch.ones_like(v, dtype=torch.bool)
    keep[0] = False
    keep[:, V:] = False
    keep[5, 2] = keep[6, 0] = keep[7, 3] = False
    assert torch.equal(v[keep], master[keep]) and not torch.equal(v, trainer.table.float())      # ... and the master keeps its digits
    assert trainer.values.requires_grad and trainer.values.grad is None


def test_state_dict_round_trip():
    trainer = field_of("5x6x7", 2, CPU, stop_eps=0.125).trainable()
    with torch.no_grad():
        trainer.values[1:, :28] += 1e-4             # below an fp16 ulp of most values: only the master can carry it
    trainer.commit()
    buf = io.BytesIO()
    torch.save(trainer.state_dict(), buf)
    buf.seek(0)
    state = torch.load(buf, weights_only=False)
    assert set(state) == {"grid", "index", "table", "sh_degree", "step_size", "stop_eps", "values"}
    other = BakedField.from_nodes(npa.OccupancyGrid([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], (5, 6, 7), device=CPU), torch.zeros(6, 7, 8, 28), 2).trainable()
    assert other.load_state_dict(state) is other
    assert torch.equal(other.values.detach(), trainer.values.detach()) and torch.equal(other.table, trainer.table)
    assert torch.equal(other.index, trainer.index) and torch.equal(other.row_node, trainer.row_node) and other.stop_eps == 0.125
    assert isinstance(other.values, torch.nn.Parameter) and other.values.requires_grad
    rays, u, _ = rays_of("5x6x7", 5, 1, True)
    a, b = trainer.render_rays_reference(rays, u), other.render_rays_reference(rays, u)
    assert all(bits(a[k], b[k]) for k in ("rgb_map", "acc_map", "depth_map"))
    # a field's state has no master: the table stands in
    fresh = field_of("5x6x7", 2, CPU).trainable().load_state_dict(trainer.to_field().state_dict())
    assert torch.equal(fresh.values.detach(), trainer.table.float())
    with pytest.raises(ValueError, match="sh_degree"):
        field_of("5x6x7", 1, CPU).trainable().load_state_dict(state)


def test_to_field_is_independent_of_later_steps():
    trainer = field_of("8x8x8", 1, CPU, stop_eps=0.25).trainable()
    field = trainer.to_field()
    assert type(field) is BakedField and field.stop_eps == 0.25 and field.sh_degree == 1 and field.step_size == trainer.step_size
    table, index, bits_ = field.table.clone(), field.index.clone(), field.grid.bits.clone()
    opt = torch.optim.SGD(trainer.parameters(), lr=1.0)
    trainer.values.grad = torch.ones_like(trainer.values)
    opt.step()
    trainer.commit()
    trainer.grid.bits.zero_()
    assert not torch.equal(trainer.table, table)
    assert torch.equal(field.table, table) and torch.equal(field.index, index) and torch.equal(field.grid.bits, bits_)
    assert field.table.data_ptr() != trainer.table.data_ptr() and field.grid is not trainer.grid


def test_a_cpu_trainer_renders_by_the_reference_only():
    trainer = constant_field(1.0, (0.0, 0.0, 0.0)).trainable()
    with pytest.raises(npa.hip_backend.NerfHipError, match="on the GPU"):
        trainer.render_rays(torch.tensor([x_ray()] * 4))
    with pytest.raises(ValueError, match="max_steps"):
        trainer.render_rays(torch.tensor([x_ray()]), max_steps=0)
    with pytest.raises(ValueError, match="11"):
        trainer.render_rays(torch.zeros(2, 8))


# ------------------------------------------------------------------------------------------------ exports
def test_the_library_exports_and_binds_the_four_entry_points():
    hb = npa.hip_backend
    raw = ctypes.CDLL(npa.build.LIB_PATH)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(raw, name) and name in hb.EXPORTS and f"int {name}(" in header, name
    assert "#define NERF_ABI_VERSION 10" in header and hb.ABI_VERSION == 10 and hb.lib().nerf_abi_version() == 10
    assert "baked_train.hip" in npa.build.SOURCES and "baked_device.h" in npa.build.HEADERS
    assert "BakedTrainer" in npa.__all__ and npa.BakedTrainer is BakedTrainer
    rows = {k: v for k, v in npa.build.resource_usage().items() if v["source"] == "baked_train.hip"}
    assert len(rows) == 8 and not any("baked_render_kernel" in k for k in rows), sorted(rows)          # count, 3 fwd, samples, 3 rows
    for k, v in rows.items():
        assert v["scratch_bytes_per_lane"] == 0 and v.get("vgpr_spills", 0) == 0 and v.get("sgpr_spills", 0) == 0 and v["lds_bytes"] == 0, (k, v)


def test_every_limit_is_refused_before_a_launch():
    """host memory stands in for the device buffers: nothing is launched or read"""
    hb = npa.hip_backend
    L = hb.lib()
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 15) & ~15
    desc = hb.NerfOccGrid((ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_int * 3)(2, 2, 2), 0, ptr)
    err = lambda: L.nerf_last_error().decode()
    BIG = (1 << 30) + 1

    def count(grid=True, stride=11, n=1, ds=0.5, M=4, **null):
        a = dict(rays=ptr, counts=ptr)
        a.update(null)
        return L.nerf_baked_count(ctypes.byref(desc) if grid else None, a["rays"], stride, None, n, ds, M, a["counts"], None)

    def fwd(grid=True, rows=1, degree=0, stride=11, n=1, ds=0.5, M=4, total=1, **null):
        a = dict(index=ptr, table=ptr, rays=ptr, offsets=ptr, records=ptr, rgb=ptr, acc=ptr, depth=ptr)
        a.update(null)
        return L.nerf_baked_train_fwd(ctypes.byref(desc) if grid else None, a["index"], a["table"], rows, degree, a["rays"], stride, None, n, ds, M,
                                      0, a["offsets"], total, a["records"], a["rgb"], a["acc"], a["depth"], None)

    def samples(n=1, total=1, ds=0.5, **null):
        a = dict(records=ptr, offsets=ptr, g_rgb=ptr, g_acc=ptr, g_depth=ptr, out=ptr)
        a.update(null)
        return L.nerf_baked_train_bwd_samples(a["records"], a["offsets"], n, total, ds, 0, a["g_rgb"], a["g_acc"], a["g_depth"], a["out"], None)

    def rows_(grid=True, rows=1, degree=0, stride=11, n=1, total=1, **null):
        a = dict(row_node=ptr, rays=ptr, records=ptr, grads=ptr, order=ptr, start=ptr, grad=ptr)
        a.update(null)
        return L.nerf_baked_train_bwd_rows(ctypes.byref(desc) if grid else None, a["row_node"], rows, degree, a["rays"], stride, n, a["records"],
                                           a["grads"], a["order"], a["start"], total, a["grad"], None)

    for call, names in ((count, ("rays", "counts")), (fwd, ("index", "table", "rays", "offsets", "records", "rgb", "acc", "depth")),
                        (samples, ("records", "offsets", "g_rgb", "g_acc", "g_depth", "out")),
                        (rows_, ("row_node", "rays", "records", "grads", "order", "start", "grad"))):
        for name in names:
            assert call(**{name: None}) == -1 and "null" in err(), (call.__name__, name)
    for call in (count, fwd, rows_):
        assert call(grid=False) == -1 and "null" in err(), call.__name__
        assert call(stride=10) == -1 and "11 columns" in err(), call.__name__
        assert call(n=-1) == -1 and "bad size" in err(), call.__name__
    assert samples(n=-1) == -1 and "bad size" in err()
    for call in (fwd, rows_):
        for degree in (-1, 3):
            assert call(degree=degree) == -1 and "sh_degree" in err(), (call.__name__, degree)
        for r in (0, -1):
            assert call(rows=r) == -1 and "n_rows" in err(), (call.__name__, r)
    assert rows_(rows=(1 << 26) + 1) == -1 and "n_rows" in err()
    for call in (count, fwd, samples):
        for ds in (0.0, -0.5, NAN, INF):
            assert call(ds=ds) == -1 and "step_size" in err(), (call.__name__, ds)
    for call in (count, fwd):
        for M in (0, -4, (1 << 24) + 1):
            assert call(M=M) == -1 and "max_steps" in err(), (call.__name__, M)
    for call in (fwd, samples, rows_):
        for total in (-1, BIG):
            assert call(total=total) == -1 and "2^30" in err(), (call.__name__, total)
    assert fwd(table=ptr + 8) == -1 and "aligned" in err()
    assert fwd(records=ptr + 4) == -1 and "aligned" in err()
    assert samples(records=ptr + 8) == -1 and "aligned" in err() and samples(out=ptr + 8) == -1 and "aligned" in err()
    assert rows_(records=ptr + 8) == -1 and "aligned" in err() and rows_(grads=ptr + 4) == -1 and "aligned" in err()
    # no rays: nothing to do (the row pass would write zeros to device memory: tests/test_baked_train_gpu.py)
    assert count(n=0, M=1 << 14) == 0
    for degree in (0, 1, 2):
        assert fwd(n=0, degree=degree, total=0, M=1 << 14) == 0
    assert samples(n=0, total=0) == 0 and samples(n=1, total=0) == 0
