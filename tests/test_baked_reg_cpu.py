"""CPU: the regularisers of a baked field's table without a GPU -- baked.regularizer_reference (the definition) against a naive loop over
the nodes, against autograd's own check and against closed forms (a constant field, a ramp, an anisotropic box), the rule that a missing
neighbour is left out, the gather form of the gradient that csrc/baked_reg.hip computes against autograd of the definition, and the
export of the two entry points with their argument errors."""
import ctypes
import math
import os

import pytest
import torch

import nerf_pytorch_amd as npa
from nerf_pytorch_amd.baked import BakedField, regularizer_reference
from test_baked_cpu import constant_field

CPU = torch.device("cpu")
F64 = torch.float64
NAN, INF = float("nan"), float("inf")
NEW = ("nerf_baked_reg_fwd", "nerf_baked_reg_bwd")
KEYS = ("tv_sigma", "tv_sh", "sparsity")


def holed_trainer(degree, seed=0, res=(3, 4, 5), hi=(1.0, 1.0, 1.0)):
    """a 3 x 4 x 5 grid of which about four cells in ten are occupied, so that stored nodes have missing neighbours on every side; the master
    gets random values in every column, padding and row 0 included"""
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(res, generator=g) < 0.4
    mask[0, 0, 0] = mask[-1, -1, -1] = True
    grid = npa.OccupancyGrid.from_mask(mask, [0.0, 0.0, 0.0], list(hi), device=CPU)
    trainer = BakedField.from_nodes(grid, torch.zeros(tuple(r + 1 for r in res) + (1 + 3 * (degree + 1) ** 2,)), degree).trainable()
    with torch.no_grad():
        trainer.values.copy_(torch.randn(trainer.values.shape, generator=g))
    return trainer


def full_trainer(res, hi, nodes, degree=0):
    grid = npa.OccupancyGrid([0.0, 0.0, 0.0], list(hi), res, device=CPU)
    trainer = BakedField.from_nodes(grid, nodes, degree).trainable()
    with torch.no_grad():
        trainer.values[1:, :nodes.shape[-1]] = nodes.reshape(-1, nodes.shape[-1])        # the fp32 values, not their fp16 rounding
    return trainer


def loop(trainer, values, eps):
    """the three scalars and the per-node terms by a loop over the nodes, in Python floats"""
    nx, ny, nz = trainer._field.node_resolution
    V = 1 + 3 * trainer.n_basis
    s = trainer.axis_scale
    index = trainer.index.view(nx, ny, nz).tolist()
    v = values.to(F64).tolist()
    sums = [0.0, 0.0, 0.0]
    for i in range(nx):
        for j in range(ny):
            for k in range(nz):
                r = index[i][j][k]
                if r == 0:
                    continue
                ahead = [index[i + 1][j][k] if i + 1 < nx else 0, index[i][j + 1][k] if j + 1 < ny else 0, index[i][j][k + 1] if k + 1 < nz else 0]
                for c in range(V):
                    sq = sum((s[a] * (v[ahead[a]][c] - v[r][c])) ** 2 for a in range(3) if ahead[a])
                    sums[0 if c == 0 else 1] += math.sqrt(sq + eps)
                sums[2] += math.log1p(2.0 * max(v[r][0], 0.0) ** 2)
    M = trainer.n_rows - 1
    return sums[0] / M, sums[1] / (3 * trainer.n_basis * M), sums[2] / M


def gather(trainer, values, eps, g):
    """the gradient of g[0] tv_sigma + g[1] tv_sh + g[2] sparsity in the form the kernel computes it: per stored node and column its own
    three differences and those of the up to three stored nodes behind it -- a gather, no node writes to another"""
    nx, ny, nz = trainer._field.node_resolution
    V, B, M = 1 + 3 * trainer.n_basis, trainer.n_basis, trainer.n_rows - 1
    s = trainer.axis_scale
    index = trainer.index.view(nx, ny, nz).tolist()
    v = values.to(F64).tolist()
    w = [g[0] / M] + [g[1] / (3 * B * M)] * (V - 1)
    E = ((1, 0, 0), (0, 1, 0), (0, 0, 1))

    def row(i, j, k):
        return index[i][j][k] if 0 <= i < nx and 0 <= j < ny and 0 <= k < nz else 0

    def diffs(i, j, k, c):
        r = row(i, j, k)
        d = [s[a] * (v[row(i + E[a][0], j + E[a][1], k + E[a][2])][c] - v[r][c]) if row(i + E[a][0], j + E[a][1], k + E[a][2]) else 0.0 for a in range(3)]
        return d, math.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2 + eps)

    grad = torch.zeros(values.shape, dtype=F64)
    for i in range(nx):
        for j in range(ny):
            for k in range(nz):
                r = row(i, j, k)
                if r == 0:
                    continue
                for c in range(V):
                    d, t = diffs(i, j, k, c)
                    total = -sum(s[a] * d[a] / t for a in range(3))
                    for a in range(3):
                        m = (i - E[a][0], j - E[a][1], k - E[a][2])
                        if row(*m):
                            dm, tm = diffs(*m, c)
                            total += s[a] * dm[a] / tm
                    grad[r, c] = w[c] * total
                sg = max(v[r][0], 0.0)
                grad[r, 0] += g[2] / M * 4.0 * sg / (1.0 + 2.0 * sg * sg)
    return grad


def autograd(trainer, values, eps, g, dtype=F64):
    x = values.detach().to(dtype).requires_grad_(True)
    out = trainer.regularizers_reference(x, eps, dtype)
    grad, = torch.autograd.grad(sum(gi * out[k] for gi, k in zip(g, KEYS)), x)
    return {k: v.detach() for k, v in out.items()}, grad


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("degree", [0, 1, 2])
def test_the_reference_against_a_loop_over_the_nodes(degree):
    trainer = holed_trainer(degree, seed=degree)
    M = trainer.n_rows - 1
    stored = (trainer.index > 0).view(trainer._field.node_resolution)
    assert 20 < M < stored.numel() and bool(stored[1:][~stored[:-1]].any()) and bool(stored[:-1][~stored[1:]].any())
    for eps in (1e-9, 1e-2):
        got = trainer.regularizers_reference(eps=eps)
        assert list(got) == list(KEYS) and all(got[k].dtype == F64 and got[k].dim() == 0 and got[k].requires_grad for k in KEYS)
        got = {k: v.detach() for k, v in got.items()}
        want = loop(trainer, trainer.values.detach(), eps)
        for k, w in zip(KEYS, want):
            assert abs(float(got[k]) - w) <= 1e-13 * abs(w), (k, float(got[k]), w)
    # the function itself, on the trainer's pieces; float32 gives float32
    direct = regularizer_reference(trainer.values.detach(), trainer.index, trainer._field.node_resolution, degree, trainer.axis_scale)
    assert all(float(direct[k]) == float(trainer.regularizers_reference()[k].detach()) for k in KEYS)
    low = trainer.regularizers_reference(trainer.values.detach(), dtype=torch.float32)
    assert all(low[k].dtype == torch.float32 and abs(float(low[k]) - float(direct[k])) <= 1e-5 * float(direct[k]) for k in KEYS)
    assert npa.regularizer_reference is regularizer_reference and "regularizer_reference" in npa.__all__


def test_gradcheck_of_the_reference():
    trainer = holed_trainer(1, seed=4, res=(2, 3, 2), hi=(0.5, 1.5, 2.0))
    assert len(set(trainer.axis_scale)) == 3
    values = trainer.values.detach().to(F64).requires_grad_(True)
    fn = lambda v: torch.stack([trainer.regularizers_reference(v, eps=1e-2)[k] for k in KEYS])
    assert torch.autograd.gradcheck(fn, (values,), eps=1e-6, atol=1e-8, rtol=1e-5)


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_the_gather_form_of_the_gradient_is_autograds(degree):
    """what csrc/baked_reg.hip computes per row -- own differences and the differences of the nodes behind -- is the gradient of the
    definition; row 0 and the padding columns get none"""
    trainer = holed_trainer(degree, seed=10 + degree, hi=(0.75, 2.0, 5.0))
    V = 1 + 3 * trainer.n_basis
    for eps in (1e-9, 1e-2):
        g = (0.7, -1.3, 0.4)
        _, want = autograd(trainer, trainer.values, eps, g)
        got = gather(trainer, trainer.values.detach(), eps, g)
        assert float(want.abs().max()) > 1e-3 and float((got - want).abs().max()) <= 1e-14
        assert not bool(want[0].any()) and not bool(want[:, V:].any())


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("degree", [0, 2])
def test_a_constant_field_has_terms_of_root_eps_and_no_tv_gradient(degree):
    trainer = constant_field(1.5, (0.3, -0.2, 0.1), degree=degree, mask=torch.rand((4, 4, 4), generator=torch.Generator().manual_seed(1)) < 0.4).trainable()
    B = trainer.n_basis
    with torch.no_grad():
        trainer.values[1:, :1 + 3 * B] = torch.tensor([1.7] + [0.3] * B + [-0.2] * B + [0.1] * B)
    for eps in (1e-9, 1e-2, 0.25):
        out, grad = autograd(trainer, trainer.values, eps, (1.0, 1.0, 0.0))
        assert abs(float(out["tv_sigma"]) - math.sqrt(eps)) <= 1e-15 and abs(float(out["tv_sh"]) - math.sqrt(eps)) <= 1e-15
        assert not bool(grad.any())            # exactly: every difference is 0
    out, grad = autograd(trainer, trainer.values, 1e-9, (0.0, 0.0, 1.0))
    assert abs(float(out["sparsity"]) - math.log1p(2.0 * 1.7 ** 2)) <= 1e-6       # (1.7 as an fp32 value)
    M = trainer.n_rows - 1
    assert float((grad[1:, 0] - 4.0 * 1.7 / (1.0 + 2.0 * 1.7 ** 2) / M).abs().max()) <= 1e-8 and not bool(grad[:, 1:].any())


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_ramp_against_the_closed_form_on_cubic_and_anisotropic_cells(axis):
    res = (3, 4, 2)
    N = tuple(r + 1 for r in res)
    p, eps = 0.75, 1e-4
    coord = torch.arange(N[axis], dtype=torch.float32).view([-1 if a == axis else 1 for a in range(3)]).expand(N)
    nodes = torch.zeros(N + (4,))
    nodes[..., 0] = p * coord
    nodes[..., 2] = -2.0 * p * coord
    for hi, scales in ((tuple(0.5 * r for r in res), (1.0, 1.0, 1.0)), ((0.25 * res[0], 0.5 * res[1], 1.0 * res[2]), (1.0, 0.5, 0.25))):
        trainer = full_trainer(res, hi, nodes)
        assert trainer.axis_scale == scales
        M = N[0] * N[1] * N[2]
        assert trainer.n_rows - 1 == M
        plane = M // N[axis]
        s = scales[axis]
        out = trainer.regularizers_reference(eps=eps)
        want_sigma = ((M - plane) * math.sqrt(p * p * s * s + eps) + plane * math.sqrt(eps)) / M
        want_sh = ((M - plane) * math.sqrt(4.0 * p * p * s * s + eps) + plane * math.sqrt(eps) + 2 * M * math.sqrt(eps)) / (3 * M)
        assert abs(float(out["tv_sigma"]) - want_sigma) <= 1e-14 and abs(float(out["tv_sh"]) - want_sh) <= 1e-14


def test_a_missing_neighbour_is_left_out():
    """the value a dropped node would have had changes nothing, and a stored node next to it is not pulled towards 0"""
    mask = torch.zeros((3, 3, 3), dtype=torch.bool)
    mask[0, 0, 0] = True
    grid = npa.OccupancyGrid.from_mask(mask, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], device=CPU)
    g = torch.Generator().manual_seed(5)
    outs = []
    for fill in (0.0, 100.0):
        nodes = torch.full((4, 4, 4, 4), fill)
        nodes[:2, :2, :2] = 3.0
        trainer = BakedField.from_nodes(grid, nodes, 0).trainable()
        assert trainer.n_rows - 1 == 8
        outs.append(autograd(trainer, trainer.values, 1e-9, (1.0, 1.0, 1.0)))
    for k in KEYS:
        assert float(outs[0][0][k]) == float(outs[1][0][k])
    assert torch.equal(outs[0][1], outs[1][1])
    assert abs(float(outs[0][0]["tv_sigma"]) - math.sqrt(1e-9)) <= 1e-15        # the eight nodes agree: the hull's zeros are not seen
    # row 0 stands in for the dropped nodes: whatever it holds, nothing reads it and it gets no gradient
    with torch.no_grad():
        trainer.values[0] = torch.randn(4, generator=g)
    again = autograd(trainer, trainer.values, 1e-9, (1.0, 1.0, 1.0))
    assert all(float(again[0][k]) == float(outs[1][0][k]) for k in KEYS) and torch.equal(again[1], outs[1][1]) and not bool(again[1][0].any())


def test_negative_densities_have_no_sparsity_gradient():
    trainer = holed_trainer(1, seed=3)
    out, grad = autograd(trainer, trainer.values, 1e-9, (0.0, 0.0, 1.0))
    sigma = trainer.values.detach()[:, 0]
    negative, positive = sigma < 0, sigma > 0
    negative[0] = positive[0] = False
    assert int(negative.sum()) > 5 and int(positive.sum()) > 5 and float(out["sparsity"]) > 0.0
    assert not bool(grad[negative].any()) and bool((grad[positive, 0] > 0).all()) and not bool(grad[:, 1:].any())


def test_an_empty_table_gives_zeros():
    grid = npa.OccupancyGrid.from_mask(torch.zeros((2, 2, 2), dtype=torch.bool), [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], device=CPU)
    trainer = BakedField.from_nodes(grid, torch.ones(3, 3, 3, 13), 1).trainable()
    assert trainer.n_rows == 1
    out = trainer.regularizers_reference()
    assert all(float(out[k]) == 0.0 and out[k].dtype == F64 for k in KEYS)


def test_bad_arguments_of_the_reference():
    trainer = holed_trainer(0)
    for eps in (0.0, -1e-9, NAN, INF, 1e-60, None, True):
        with pytest.raises(ValueError, match="eps"):
            trainer.regularizers_reference(eps=eps)
        with pytest.raises(ValueError, match="eps"):
            trainer.regularizers(eps=eps)
    with pytest.raises(ValueError, match="axis_scale"):
        regularizer_reference(trainer.values, trainer.index, (4, 5, 6), 0, (1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="sh_degree"):
        regularizer_reference(trainer.values, trainer.index, (4, 5, 6), 3, (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="lattice node"):
        regularizer_reference(trainer.values, trainer.index, (4, 5, 7), 0, (1.0, 1.0, 1.0))


def test_a_cpu_trainer_has_the_reference_only():
    trainer = constant_field(1.0, (0.0, 0.0, 0.0)).trainable()
    with pytest.raises(npa.hip_backend.NerfHipError, match="on the GPU"):
        trainer.regularizers()
    with torch.no_grad(), pytest.raises(npa.hip_backend.NerfHipError, match="on the GPU"):
        trainer.regularizers(eps=1e-2)


# ------------------------------------------------------------------------------------------------ exports
def test_the_library_exports_and_binds_the_two_entry_points():
    hb = npa.hip_backend
    raw = ctypes.CDLL(npa.build.LIB_PATH)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(raw, name) and name in hb.EXPORTS and f"int {name}(const NerfOccGrid* grid, const int* node_index, const int* row_node" in header, name
        assert callable(getattr(hb, name[len("nerf_"):]))
    assert "#define NERF_ABI_VERSION 10" in header and hb.ABI_VERSION == 10 and hb.lib().nerf_abi_version() == 10
    assert "baked_reg.hip" in npa.build.SOURCES
    rows = {k: v for k, v in npa.build.resource_usage().items() if v["source"] == "baked_reg.hip"}
    assert len(rows) == 6 and sum("baked_reg_fwd_kernel" in k for k in rows) == 3 and sum("baked_reg_bwd_kernel" in k for k in rows) == 3, sorted(rows)
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

    def fwd(grid=True, rows=2, degree=0, s=(1.0, 1.0, 1.0), eps=1e-9, **null):
        a = dict(index=ptr, row_node=ptr, values=ptr, terms=ptr)
        a.update(null)
        return L.nerf_baked_reg_fwd(ctypes.byref(desc) if grid else None, a["index"], a["row_node"], a["values"], rows, degree, s[0], s[1], s[2], eps,
                                    a["terms"], None)

    def bwd(grid=True, rows=2, degree=0, s=(1.0, 1.0, 1.0), eps=1e-9, **null):
        a = dict(index=ptr, row_node=ptr, values=ptr, g=ptr, grad=ptr)
        a.update(null)
        return L.nerf_baked_reg_bwd(ctypes.byref(desc) if grid else None, a["index"], a["row_node"], a["values"], rows, degree, s[0], s[1], s[2], eps,
                                    a["g"], a["grad"], None)

    for call, names in ((fwd, ("index", "row_node", "values", "terms")), (bwd, ("index", "row_node", "values", "g", "grad"))):
        for name in names:
            assert call(**{name: None}) == -1 and "null" in err(), (call.__name__, name)
        assert call(grid=False) == -1 and "null" in err(), call.__name__
        for degree in (-1, 3):
            assert call(degree=degree) == -1 and "sh_degree" in err(), (call.__name__, degree)
        for r in (0, -1, (1 << 26) + 1):
            assert call(rows=r) == -1 and "n_rows" in err(), (call.__name__, r)
        for eps in (0.0, -1e-9, NAN, INF):
            assert call(eps=eps) == -1 and "eps" in err(), (call.__name__, eps)
        for axis in range(3):
            for bad in (0.0, -1.0, NAN, INF):
                s = [1.0, 1.0, 1.0]
                s[axis] = bad
                assert call(s=s) == -1 and "scale" in err(), (call.__name__, axis, bad)
        for off in (4, 8):
            assert call(values=ptr + off) == -1 and "aligned" in err(), (call.__name__, off)
    assert bwd(grad=ptr + 8) == -1 and "aligned" in err()
    bad_grid = hb.NerfOccGrid((ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_int * 3)(2, 0, 2), 0, ptr)
    assert L.nerf_baked_reg_fwd(ctypes.byref(bad_grid), ptr, ptr, ptr, 2, 0, 1.0, 1.0, 1.0, 1e-9, ptr, None) == -1 and "resolution" in err()
