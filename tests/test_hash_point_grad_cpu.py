"""CPU: the gradient of the hash-grid encoding with respect to its points without a GPU -- the exports and the binding,
the argument errors, HashEncoding.point_grad_reference against float64 autograd of encode_reference on the four-level fixture and on the
odd box, the clamp rule on outside axes and faces, views_grad_reference against float64 autograd of the view embedding, and the flag
through HashNeRF, create_nerf, the state_dict and query_points."""
import copy
import ctypes
import inspect
import os

import pytest
import torch

import nerf_pytorch_amd as npa
from nerf_pytorch_amd.hashgrid import HashEncoding, HashNeRF, views_grad_reference
from test_hash_cpu import FOUR, HI, LO, box_points, four_level, hash_args
from test_hash_edges_cpu import encoding

F64 = torch.float64
MARGIN = 2.0 ** -10


def safe_points(enc, n, seed):
    """points over 1.2 x the box, rejection-sampled: on every axis the unclamped t = (x - lo) inv_extent lies at least 2^-10 from 0 and
    1, and -- where the axis is inside -- u R at least 2^-10 from an integer on every level.  There the encoding is differentiable and
    fp32 and float64 pick the same cells.  Returns (points, the fraction of the draws that survived)."""
    pts = box_points(n, seed, spread=1.2, lo=enc.lo, hi=enc.hi)
    t = (pts.double() - enc._lo32.double()) * enc._inv32.double()
    ok = ((t.abs() >= MARGIN) & ((t - 1.0).abs() >= MARGIN)).all(1)
    inside = (t > 0.0) & (t < 1.0)
    for R in sorted(set(enc.level_resolution)):
        p = t.clamp(0.0, 1.0) * R
        ok &= (((p - p.round()).abs() >= MARGIN) | ~inside).all(1)
    return pts[ok].contiguous(), float(ok.double().mean())


def assert_precondition(enc, pts):
    t = (pts.double() - enc._lo32.double()) * enc._inv32.double()
    assert float(torch.minimum(t.abs(), (t - 1.0).abs()).min()) >= MARGIN
    inside = (t > 0.0) & (t < 1.0)
    for R in enc.level_resolution:
        p = t.clamp(0.0, 1.0) * R
        assert float((p - p.round()).abs()[inside].min()) >= MARGIN
    # fp32 and float64 locate every point in the same cell on every level
    for l in range(enc.n_levels):
        assert torch.equal(enc._corners(pts, l, torch.float32)[0], enc._corners(pts, l, F64)[0])


def autograd_point_grad(enc, pts, d_out, dtype):
    x = pts.to(dtype).requires_grad_(True)
    (enc.encode_reference(x, dtype, enc.embeddings.detach().to(dtype)) * d_out.to(dtype)).sum().backward()
    return x.grad


def make(name, F):
    """the four-level fixture, or the odd configuration (R = 3, 5, 10, 19, 37 on a box whose extents are no powers of two)"""
    return four_level(F=F) if name == "FOUR" else encoding(name, F)


# ------------------------------------------------------------------------------------------------ exports
def test_the_library_exports_and_binds_the_entry_point():
    hb = npa.hip_backend
    raw = ctypes.CDLL(npa.build.LIB_PATH)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_hip.h")) as f:
        header = f.read()
    assert hasattr(raw, "nerf_hash_input_grad") and "nerf_hash_input_grad" in hb.EXPORTS
    assert "int nerf_hash_input_grad(const NerfHashGrid* grid, const float* embeddings" in header
    assert hasattr(raw, "nerf_hash_input_grad_workspace_floats") and "nerf_hash_input_grad_workspace_floats" in hb.EXPORTS
    assert "size_t nerf_hash_input_grad_workspace_floats(long n_points);" in header
    assert "#define NERF_ABI_VERSION 10" in header and hb.ABI_VERSION == 10
    assert "hash_input_grad.hip" in npa.build.SOURCES and "hash_host.h" in npa.build.HEADERS
    assert list(inspect.signature(hb.hash_input_grad).parameters) == ["desc", "embeddings", "d_x", "col", "points", "rays", "z_vals", "views_col",
                                                                      "multires_views", "accumulate"]
    assert callable(views_grad_reference) and callable(HashEncoding.point_grad_reference)
    rows = {k: v for k, v in npa.build.resource_usage().items() if v.get("source") == "hash_input_grad.hip"}
    assert len(rows) == 4, sorted(rows)         # the point kernel for F = 1, 2, 4; the per-ray fold
    for k, v in rows.items():
        assert v["scratch_bytes_per_lane"] == 0 and v.get("vgpr_spills", 0) == 0 and v.get("sgpr_spills", 0) == 0 and v["lds_bytes"] == 0, (k, v)


def test_argument_errors_are_codes_not_crashes():
    L = npa.hip_backend.lib()
    d = four_level().desc()
    g = ctypes.byref(d)
    call = L.nerf_hash_input_grad
    err = lambda: L.nerf_last_error()
    assert L.nerf_hash_input_grad_workspace_floats(0) == 0 and L.nerf_hash_input_grad_workspace_floats(1000) == 3000
    assert call(None, None, None, None, 0, None, 1, 0, None, 8, -1, -1, None, None, None, 0, None) == -1 and b"null grid" in err()
    assert call(g, None, None, None, 0, None, 1, 0, None, 8, -1, -1, None, None, None, 0, None) == 0            # no points: nothing to do
    assert call(g, None, None, None, 0, None, 1, 0, None, 7, -1, -1, None, None, None, 0, None) == -1 and b"ld_d_x" in err()
    assert call(g, None, None, None, 0, None, 1, 5, None, 8, -1, -1, None, None, None, 0, None) == -1           # points without a pointer
    # point mode: every pointer, no view columns, no accumulate, no d_rays
    assert call(g, 0x1000, 0x2000, None, 0, None, 1, 5, None, 8, -1, -1, 0x4000, None, None, 0, None) == -1 and b"null pointer" in err()
    assert call(g, 0x1000, 0x2000, None, 0, None, 1, 5, 0x3000, 8, -1, -1, None, None, None, 0, None) == -1 and b"null pointer" in err()
    assert call(g, 0x1000, 0x2000, None, 0, None, 1, 5, 0x3000, 35, 8, 4, 0x4000, None, None, 0, None) == -1 and b"ray mode" in err()
    assert call(g, 0x1000, 0x2000, None, 0, None, 1, 5, 0x3000, 8, -1, -1, 0x4000, None, None, 1, None) == -1 and b"accumulate" in err()
    assert call(g, 0x1000, 0x2000, None, 0, None, 1, 5, 0x3000, 8, -1, -1, 0x4000, 0x5000, None, 0, None) == -1 and b"d_rays" in err()
    assert call(g, 0x1002, 0x2000, None, 0, None, 1, 5, 0x3000, 8, -1, -1, 0x4000, None, None, 0, None) == -1 and b"aligned" in err()
    assert call(g, 0x1000, 0x2000, 0x6000, 11, 0x7000, 1, 5, 0x3000, 8, -1, -1, 0x4000, None, None, 0, None) == -1 and b"points OR rays" in err()
    # ray mode: d_rays and the workspace, a whole number of rays, the view columns behind the encoding's and inside the rows, 11-column records
    ray = lambda **kw: call(*[dict(dict(grid=g, emb=0x1000, points=None, rays=0x6000, stride=11, z=0x7000, S=4, P=8, d_x=0x3000, ld=35, vc=8, mv=4,
                                        d_points=None, d_rays=0x5000, work=0x8000, acc=0, stream=None), **kw)[k]
                              for k in ("grid", "emb", "points", "rays", "stride", "z", "S", "P", "d_x", "ld", "vc", "mv", "d_points", "d_rays", "work",
                                        "acc", "stream")])
    assert ray(d_rays=None) == -1 and b"workspace" in err()
    assert ray(work=None) == -1 and b"workspace" in err()
    assert ray(d_points=0x4000) == -1 and b"point mode" in err()
    assert ray(P=9) == -1 and b"multiple of n_samples" in err()
    assert ray(vc=7) == -1 and b"view columns" in err()
    assert ray(ld=34) == -1 and b"view columns" in err()
    assert ray(mv=17) == -1 and b"multires_views" in err()
    assert ray(stride=8) == -1 and b"11 columns" in err()
    assert ray(z=None) == -1 and b"null pointer" in err()
    with pytest.raises(npa.hip_backend.NerfHipError):       # no eager fall-back: CPU tensors are refused
        enc = four_level()
        npa.hip_backend.hash_input_grad(enc.desc(), enc.embeddings.detach(), torch.zeros(3, 8), 0, torch.zeros(3, 3), None, None, -1, -1)


# ------------------------------------------------------------------------------------------------ point_grad_reference
@pytest.mark.parametrize("F", [1, 2, 4])
@pytest.mark.parametrize("name", ["FOUR", "ODD"])
def test_point_grad_reference_against_float64_autograd(name, F):
    enc = make(name, F)
    pts, kept = safe_points(enc, 700, seed=31)
    print(f"{name} F={F}: {kept:.3f} of the draws survive")
    assert kept >= 0.9 and pts.shape[0] >= 600
    assert_precondition(enc, pts)
    d_out = torch.randn(pts.shape[0], enc.out_dim, generator=torch.Generator().manual_seed(32))
    want = autograd_point_grad(enc, pts, d_out, F64)
    scale = float(want.abs().max())
    got64 = enc.point_grad_reference(pts, d_out, F64)
    assert got64.dtype == F64 and got64.shape == (pts.shape[0], 3) and scale > 0.0
    rel64 = float((got64 - want).abs().max()) / scale
    # the outside axes are exact zeros on both sides (torch.clamp's backward is inclusive at its bounds only)
    t = (pts.double() - enc._lo32.double()) * enc._inv32.double()
    outside = (t < 0.0) | (t > 1.0)
    assert bool(outside.any()) and float(want[outside].abs().max()) == 0.0 and float(got64[outside].abs().max()) == 0.0
    got32 = enc.point_grad_reference(pts, d_out)
    assert got32.dtype == torch.float32
    err = float((got32.double() - want).abs().max())
    own = float((autograd_point_grad(enc, pts, d_out, torch.float32).double() - want).abs().max())
    print(f"{name} F={F}: float64 closed form {rel64:.2e} relative; float32 definition {err / scale:.2e}, float32 autograd's own {own / scale:.2e}")
    assert rel64 <= 1e-12
    assert own > 0.0 and err <= 4.0 * own
    assert torch.equal(got32, enc.point_grad_reference(pts, d_out))
    # linear in d_out, and another table is accepted
    other = torch.ones_like(enc.embeddings.detach())
    flat = enc.point_grad_reference(pts, d_out, F64, embeddings=other.double())
    assert float(flat.abs().max()) <= 1e-9 * scale          # a constant table: the encoding does not depend on the point


def test_an_outside_axis_is_exactly_zero_and_a_face_has_its_cells_derivative():
    enc = four_level()
    lo, hi = torch.tensor(LO), torch.tensor(HI)
    inside, _ = safe_points(enc, 60, seed=41)
    t = (inside - lo) / (hi - lo)
    inside = inside[((t > 0) & (t < 1)).all(1)][:40]
    d_out = torch.randn(inside.shape[0], enc.out_dim, generator=torch.Generator().manual_seed(42))
    base = enc.point_grad_reference(inside, d_out)
    assert float(base.abs().min()) > 0.0
    for axis in range(3):
        for side, far in ((lo, -7.0), (hi, 9.0), (lo, -1e30), (hi, 1e-3)):
            out, on = inside.clone(), inside.clone()
            out[:, axis] = side[axis] + far
            on[:, axis] = side[axis]
            g_out, g_on = enc.point_grad_reference(out, d_out), enc.point_grad_reference(on, d_out)
            others = [a for a in range(3) if a != axis]
            assert float(g_out[:, axis].abs().max()) == 0.0 and float(g_out[:, others].abs().min()) > 0.0
            # the other axes see the clamped point; on the face itself the derivative is that of the cell the forward picks
            assert torch.equal(g_out[:, others], g_on[:, others]) and float(g_on[:, axis].abs().min()) > 0.0
            # ... which is the cell just inside: the derivative along an axis is constant in that axis within a cell
            nudge = on.clone()
            nudge[:, axis] = side[axis] + (0.01 if side is lo else -0.01)
            assert torch.allclose(enc.point_grad_reference(nudge, d_out, F64)[:, axis], enc.point_grad_reference(on, d_out, F64)[:, axis],
                                  rtol=1e-12, atol=0.0)
    # right-continuous at a lattice plane: node 2 of level 0's x axis equals the derivative just above it on that level
    one = torch.zeros(1, enc.out_dim)
    one[0, 0] = 1.0
    node = torch.tensor([[LO[0] + 2 * (HI[0] - LO[0]) / 4, 0.3, 1.7]])
    above, below = node + torch.tensor([[1e-3, 0.0, 0.0]]), node - torch.tensor([[1e-3, 0.0, 0.0]])
    g = [enc.point_grad_reference(p, one, F64)[0, 0] for p in (node, above, below)]
    assert abs(float(g[0] - g[1])) <= 1e-12 * abs(float(g[0])) and abs(float(g[0] - g[2])) > 1e-6 * abs(float(g[0]))


# ------------------------------------------------------------------------------------------------ views_grad_reference
def embed_views(v, Lv):
    """the view columns as nerf_build_inputs writes them: [v, sin 2^0 v, cos 2^0 v, ..]"""
    cols = [v]
    for k in range(max(Lv, 0)):
        cols += [torch.sin(v * 2.0 ** k), torch.cos(v * 2.0 ** k)]
    return torch.cat(cols, -1)


@pytest.mark.parametrize("Lv", [-1, 0, 1, 4])
def test_views_grad_reference_against_float64_autograd(Lv):
    g = torch.Generator().manual_seed(51 + Lv)
    v = torch.nn.functional.normalize(torch.randn(65, 3, generator=g), dim=-1)
    d = torch.randn(65, 3 + 6 * max(Lv, 0), generator=g)
    v64 = v.double().requires_grad_(True)
    (embed_views(v64, Lv) * d.double()).sum().backward()
    scale = float(v64.grad.abs().max())
    got64 = views_grad_reference(v, d, Lv, F64)
    assert float((got64 - v64.grad).abs().max()) <= 1e-13 * scale
    v32 = v.clone().requires_grad_(True)
    (embed_views(v32, Lv) * d).sum().backward()
    own = float((v32.grad.double() - v64.grad).abs().max())
    got32 = views_grad_reference(v, d, Lv)
    assert got32.dtype == torch.float32 and got32.shape == (65, 3)
    err = float((got32.double() - v64.grad).abs().max())
    print(f"Lv={Lv}: float32 definition {err:.2e}, float32 autograd's own {own:.2e}")
    assert err <= 4.0 * own if Lv > 0 else torch.equal(got32, d[:, :3])
    with pytest.raises(ValueError):
        views_grad_reference(v, d[:, :2], Lv)


# ------------------------------------------------------------------------------------------------ the flag
def test_the_flag_through_the_host_objects(tmp_path):
    assert inspect.signature(HashEncoding.__init__).parameters["point_grad"].default is False
    assert inspect.signature(HashNeRF.__init__).parameters["point_grad"].default is False
    plain, flagged = HashNeRF(LO, HI, **FOUR), HashNeRF(LO, HI, point_grad=True, **FOUR)
    assert plain.point_grad is False and plain.encoding.point_grad is False
    assert flagged.point_grad is True and flagged.encoding.point_grad is True
    assert list(flagged.state_dict()) == list(plain.state_dict())
    assert [n for n, _ in flagged.named_parameters()] == [n for n, _ in plain.named_parameters()]
    flagged.load_state_dict(plain.state_dict())                 # the flag is not part of a checkpoint
    assert flagged.point_grad is True
    clone = copy.deepcopy(flagged)
    assert clone.point_grad is True and clone.encoding._desc is None and copy.deepcopy(plain).point_grad is False
    assert isinstance(flagged, npa.dense.DenseNeRF)
    # create_nerf
    assert npa.config_parser().parse_args([]).hash_point_grad is False
    train = npa.create_nerf(hash_args(tmp_path, "--hash_point_grad"), device=torch.device("cpu"))[0]
    assert train["network_fn"].point_grad is True and train["network_fine"].point_grad is True
    train = npa.create_nerf(hash_args(tmp_path), device=torch.device("cpu"))[0]
    assert train["network_fn"].point_grad is False and train["network_fine"].point_grad is False
    a = hash_args(tmp_path)
    delattr(a, "hash_point_grad")       # a namespace without the flag reads its default
    assert npa.create_nerf(a, device=torch.device("cpu"))[0]["network_fn"].point_grad is False


def test_query_points_and_the_mesh_functions_name_the_flag():
    plain = HashNeRF(LO, HI, **FOUR)
    pts = torch.zeros(4, 3, requires_grad=True)
    vd = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="point_grad=True"):
        npa.query_points(plain, pts, vd)
    with pytest.raises(NotImplementedError, match="point_grad=True"):
        npa.query_points(plain, pts.detach(), vd.requires_grad_(True))
    with pytest.raises(NotImplementedError, match="point_grad=True"):
        npa.mesh.vertex_normals(plain, torch.zeros(4, 3))
    dense = npa.dense.DenseNeRF(D=2, W=32, input_ch=3, input_ch_views=3, use_viewdirs=True)
    with pytest.raises(NotImplementedError, match="fused-kernel NeRF module is required"):
        npa.mesh.density_volume(dense, LO, HI, 5)
