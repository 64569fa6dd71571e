"""CPU: the hash-grid field without a GPU -- the exports, the level tables, the hash, HashEncoding.encode_reference on nodes, faces and
outside points, table_grad_reference against float64 autograd, create_nerf(--i_embed 1) and the state_dict."""
import ctypes
import inspect
import io
import math
import os

import pytest
import torch

import nerf_pytorch_amd as npa
from nerf_pytorch_amd.hashgrid import HashEncoding, HashNeRF, hash_slot, level_tables

F64 = torch.float64
LO, HI = (-1.0, -0.5, 0.0), (1.0, 1.5, 4.0)         # (extents 2, 2, 4: a lattice node is an exact fp32 point)
FOUR = dict(n_levels=4, log2_hashmap_size=10, base_resolution=4, finest_resolution=32)


def four_level(F=2, seed=0):
    torch.manual_seed(seed)
    enc = HashEncoding(LO, HI, n_features=F, **FOUR)
    with torch.no_grad():       # values large enough for a rounding error to show
        enc.embeddings.copy_(torch.randn(enc.embeddings.shape, generator=torch.Generator().manual_seed(seed + 1)))
    return enc


def box_points(n, seed, spread=1.0, lo=LO, hi=HI):
    """points over the box [lo, hi], `spread` > 1 reaching outside"""
    u = torch.rand(n, 3, generator=torch.Generator().manual_seed(seed), dtype=F64)
    lo, hi = torch.tensor(lo, dtype=F64), torch.tensor(hi, dtype=F64)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    return (mid + (2.0 * u - 1.0) * half * spread).float()


# ------------------------------------------------------------------------------------------------ exports
def test_the_library_exports_and_binds_the_entry_points():
    hb = npa.hip_backend
    raw = ctypes.CDLL(npa.build.LIB_PATH)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_hip.h")) as f:
        header = f.read()
    for name in ("nerf_hash_encode_fwd", "nerf_hash_encode_bwd"):
        assert hasattr(raw, name) and name in hb.EXPORTS and f"int {name}(const NerfHashGrid* grid" in header, name
    assert hasattr(raw, "nerf_hash_scratch_words") and "nerf_hash_scratch_words" in hb.EXPORTS
    assert "#define NERF_ABI_VERSION 10" in header and hb.ABI_VERSION == 10
    assert "hash_encode.hip" in npa.build.SOURCES and "hash_device.h" in npa.build.HEADERS
    assert list(inspect.signature(hb.hash_encode_fwd).parameters) == ["desc", "embeddings", "out", "col", "points", "rays", "z_vals"]
    assert list(inspect.signature(hb.hash_encode_bwd).parameters) == ["desc", "d_out", "col", "points", "rays", "z_vals", "scratch", "phases",
                                                                      "d_embeddings"]
    for name in ("HashEncoding", "HashNeRF", "hashgrid"):
        assert name in npa.__all__ and getattr(npa, name) is not None
    rows = {k: v for k, v in npa.build.resource_usage().items() if v.get("source") == "hash_encode.hip"}
    assert len(rows) == 8, sorted(rows)         # forward and scatter for F = 1, 2, 4; the maximum; the finishing pass
    for k, v in rows.items():
        assert v["scratch_bytes_per_lane"] == 0 and v.get("vgpr_spills", 0) == 0 and v.get("sgpr_spills", 0) == 0 and v["lds_bytes"] == 0, (k, v)


def test_argument_errors_are_codes_not_crashes():
    L = npa.hip_backend.lib()
    enc = four_level()
    d = enc.desc()
    assert L.nerf_hash_scratch_words(ctypes.byref(d)) == enc.rows_total * 2 + 1
    assert L.nerf_hash_encode_fwd(None, None, None, None, 0, None, 1, 0, None, 8, None) == -1 and b"null grid" in L.nerf_last_error()
    assert L.nerf_hash_encode_fwd(ctypes.byref(d), None, None, None, 0, None, 1, 0, None, 8, None) == 0         # no points: nothing to do
    assert L.nerf_hash_encode_fwd(ctypes.byref(d), None, None, None, 0, None, 1, 0, None, 7, None) == -1 and b"ld_out" in L.nerf_last_error()
    assert L.nerf_hash_encode_fwd(ctypes.byref(d), None, None, None, 0, None, 1, 5, None, 8, None) == -1        # points without a pointer
    assert L.nerf_hash_encode_bwd(ctypes.byref(d), None, None, 0, None, 1, 0, None, 8, None, None, 3, None) == -1 and b"null pointer" in L.nerf_last_error()
    assert L.nerf_hash_encode_bwd(ctypes.byref(d), None, None, 0, None, 1, 0, None, 8, 0x1000, 0x2000, 4, None) == -1 and b"phases" in L.nerf_last_error()
    bad = npa.hip_backend.NerfHashGrid.from_buffer_copy(d)
    bad.level_dense[2] = 1          # 17^3 rows do not fit 2^10
    assert L.nerf_hash_encode_fwd(ctypes.byref(bad), None, None, None, 0, None, 1, 0, None, 8, None) == -1 and b"level_dense" in L.nerf_last_error()
    bad = npa.hip_backend.NerfHashGrid.from_buffer_copy(d)
    bad.level_offset[3] += 1
    assert L.nerf_hash_encode_fwd(ctypes.byref(bad), None, None, None, 0, None, 1, 0, None, 8, None) == -1 and b"prefix sum" in L.nerf_last_error()
    with pytest.raises(npa.hip_backend.NerfHipError):       # no eager fall-back: CPU tensors are refused
        enc(torch.zeros(3, 3))


# ------------------------------------------------------------------------------------------------ level tables and the hash
def test_level_tables_of_the_four_level_configuration():
    enc = four_level()
    assert enc.level_resolution == [4, 8, 16, 32]
    assert enc.level_dense == [True, True, False, False]           # 5^3 = 125 and 9^3 = 729 fit 1024 rows, 17^3 does not
    assert enc.level_offset == [0, 125, 125 + 729, 125 + 729 + 1024, 125 + 729 + 2048]
    assert enc.rows_total == 2902 and tuple(enc.embeddings.shape) == (2902, 2) and enc.out_dim == 8
    assert enc.embeddings.dtype == torch.float32
    fresh = HashEncoding(LO, HI, **FOUR)
    E = fresh.embeddings.detach()
    assert float(E.abs().max()) <= 1e-4 and float(E.min()) < 0.0 < float(E.max())
    assert [n for n, _ in fresh.named_parameters()] == ["embeddings"]


def test_level_tables_of_one_level_and_of_the_default():
    res, off, dense = level_tables(1, 10, 4, 32)
    assert (res, off, dense) == ([4], [0, 125], [True])
    res, off, dense = level_tables(1, 4, 7, 7)
    assert (res, off, dense) == ([7], [0, 16], [False])
    enc = HashEncoding(LO, HI)
    assert enc.n_levels == 16 and enc.n_features == 2 and enc.log2_hashmap_size == 19 and enc.out_dim == 32
    R = enc.level_resolution
    assert R[0] == 16 and R[-1] == 512 and all(a < b for a, b in zip(R, R[1:]))
    b = math.exp((math.log(512) - math.log(16)) / 15)
    assert R[:-1] == [int(math.floor(16 * b ** l)) for l in range(15)]
    T = 1 << 19
    assert enc.level_dense == [(r + 1) ** 3 <= T for r in R] and enc.level_dense[:7] == [True] * 7 and not any(enc.level_dense[7:])
    assert enc.level_offset[0] == 0
    assert [b_ - a for a, b_ in zip(enc.level_offset, enc.level_offset[1:])] == [(r + 1) ** 3 if d else T for r, d in zip(R, enc.level_dense)]
    for bad in (dict(n_levels=0), dict(n_levels=33), dict(n_features=3), dict(log2_hashmap_size=3), dict(log2_hashmap_size=25),
                dict(base_resolution=0), dict(base_resolution=64, finest_resolution=32)):
        with pytest.raises(ValueError):
            HashEncoding(LO, HI, **bad)
    with pytest.raises(ValueError):
        HashEncoding((0.0, 0.0, 0.0), (1.0, 0.0, 1.0))


def test_the_hash_of_three_hand_written_coordinates():
    # iy * 2654435761 and iz * 805459861 reduced mod 2^32 by hand, then xor, then the low bits
    #   (1, 0, 0): 1
    #   (0, 1, 0): 2654435761 = 0x9E3779B1 -> low 10 bits 0x1B1 = 433
    #   (3, 5, 7): 5 * 2654435761 = 13272178805 = 3 * 2^32 + 387276917 -> 0x17156075;  7 * 805459861 = 5638219027 = 2^32 + 1343251731 ->
    #              0x50106513;  3 ^ 0x17156075 ^ 0x50106513 = 0x47050565 -> low 10 bits 0x165 = 357
    assert hash_slot(1, 0, 0, 10) == 1
    assert hash_slot(0, 1, 0, 10) == 433
    assert hash_slot(3, 5, 7, 10) == 357 and hash_slot(3, 5, 7, 24) == 0x050565
    t = torch.tensor([[1, 0, 0], [0, 1, 0], [3, 5, 7]], dtype=torch.int64)
    assert hash_slot(t[:, 0], t[:, 1], t[:, 2], 10).tolist() == [1, 433, 357]


# ------------------------------------------------------------------------------------------------ encode_reference
def node_points(enc, level):
    """five lattice nodes of one level over the encoding's own box (indices capped at R: a level coarser than 3 cells has no node 3)"""
    R = enc.level_resolution[level]
    idx = torch.tensor([[0, 0, 0], [1, 2, 3], [R, R, R], [R, 0, 1], [2, R - 1, R]], dtype=torch.int64).clamp(max=R)
    lo, hi = torch.tensor(enc.lo, dtype=F64), torch.tensor(enc.hi, dtype=F64)
    return idx, (lo + idx.to(F64) / R * (hi - lo)).float()


def test_at_a_node_of_a_dense_level_the_output_is_the_stored_row():
    enc = four_level()
    for level in (0, 1):
        R = enc.level_resolution[level]
        idx, pts = node_points(enc, level)
        out = enc.encode_reference(pts)
        rows = enc.level_offset[level] + idx[:, 0] + idx[:, 1] * (R + 1) + idx[:, 2] * (R + 1) ** 2
        # (R a power of two and the box's extents too: u R is exact, so the weights are exactly 0 and 1)
        assert torch.equal(out[:, 2 * level:2 * level + 2], enc.embeddings.detach()[rows])


def test_the_weights_sum_to_one():
    enc = four_level()
    pts = box_points(500, 3, spread=1.2)
    for level in range(4):
        rows, w = enc._corners(pts, level, torch.float32)
        assert rows.shape == (500, 8) and int(rows.min()) >= enc.level_offset[level] and int(rows.max()) < enc.level_offset[level + 1]
        assert float(w.min()) >= 0.0 and float(w.max()) <= 1.0
        # eight products of three factors in [0, 1], each off by at most 3.5 ulp of a value <= 1, summed
        assert float((w.sum(1) - 1.0).abs().max()) <= 8 * 4 * 2.0 ** -24


def test_faces_and_outside_points_equal_their_clamped_points():
    enc = four_level()
    lo, hi = torch.tensor(LO), torch.tensor(HI)
    inside = box_points(40, 5)
    cases = []
    for axis in range(3):
        for side, far in ((lo, -7.0), (hi, 9.0)):
            on, out = inside.clone(), inside.clone()
            on[:, axis] = side[axis]
            out[:, axis] = side[axis] + far
            cases.append((on, out))
    cases.append((hi.expand(3, 3).clone(), hi.expand(3, 3) + torch.tensor([[0.5, 0.0, 0.0], [1.0, 2.0, 3.0], [0.0, 0.0, 1e30]])))
    cases.append((lo.expand(2, 3).clone(), lo.expand(2, 3) - torch.tensor([[0.5, 1e20, 0.0], [1.0, 2.0, 3.0]])))
    for on, out in cases:
        a, b = enc.encode_reference(on), enc.encode_reference(out)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    # the upper face: i = R - 1 and f = 1 exactly
    rows, w = enc._corners(hi[None], 3, torch.float32)
    assert w[0].tolist() == [0.0] * 7 + [1.0]
    assert int(rows[0, 7]) == enc.level_offset[3] + hash_slot(32, 32, 32, 10)


def test_encode_reference_is_linear_in_the_table_and_accepts_another():
    enc = four_level(F=4)
    pts = box_points(50, 7, spread=1.1).view(5, 10, 3)
    out = enc.encode_reference(pts)
    assert out.shape == (5, 10, 16) and out.dtype == torch.float32
    other = torch.ones_like(enc.embeddings)
    one = enc.encode_reference(pts, embeddings=other)
    assert float((one - 1.0).abs().max()) <= 8 * 4 * 2.0 ** -24            # a constant table gives the weights' sum
    assert enc.encode_reference(pts, dtype=F64).dtype == F64


# ------------------------------------------------------------------------------------------------ table_grad_reference
@pytest.mark.parametrize("F", [1, 2, 4])
def test_table_grad_reference_against_float64_autograd(F):
    torch.manual_seed(0)
    enc = HashEncoding(LO, HI, n_features=F, **FOUR)
    pts = box_points(700, 11, spread=1.05)
    d_out = torch.randn(700, 4 * F, generator=torch.Generator().manual_seed(12))
    E64 = enc.embeddings.detach().double().requires_grad_(True)
    (enc.encode_reference(pts, F64, E64) * d_out.double()).sum().backward()
    E32 = enc.embeddings.detach().clone().requires_grad_(True)
    (enc.encode_reference(pts, torch.float32, E32) * d_out).sum().backward()
    got = enc.table_grad_reference(pts, d_out)
    assert got.shape == E32.grad.shape and got.dtype == torch.float32
    own = float((E32.grad.double() - E64.grad).abs().max())
    err = float((got.double() - E64.grad).abs().max())
    print(f"F={F}: fixed-point error {err:.3e}, float32 autograd's own {own:.3e}")
    assert own > 0.0 and err <= 4.0 * own
    assert torch.equal(got, enc.table_grad_reference(pts, d_out))
    untouched = E64.grad.abs().sum(1) == 0
    assert bool(untouched.any()) and float(got[untouched].abs().max()) == 0.0


def test_table_grad_reference_edge_cases():
    enc = four_level()
    pts = box_points(20, 13)
    zero = enc.table_grad_reference(pts, torch.zeros(20, 8))
    assert zero.shape == (enc.rows_total, 2) and float(zero.abs().max()) == 0.0
    d = torch.ones(20, 8)
    d[3, 5] = float("nan")
    assert bool(torch.isnan(enc.table_grad_reference(pts, d)).all())
    d[3, 5] = float("inf")
    assert bool(torch.isnan(enc.table_grad_reference(pts, d)).all())
    assert float(enc.table_grad_reference(pts[:0], d[:0]).abs().max()) == 0.0
    # one point, one unit of gradient on level 0: the eight weights, exactly (M = 1: q = 60, every weight a multiple of 2^-60)
    g = torch.zeros(1, 8)
    g[0, 0] = 1.0
    rows, w = enc._corners(pts[:1], 0, torch.float32)
    got = enc.table_grad_reference(pts[:1], g)
    want = torch.zeros_like(got)
    want[:, 0].index_add_(0, rows[0], w[0])
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ host objects
def hash_args(tmp_path, *extra):
    return npa.config_parser().parse_args(["--expname", "h", "--basedir", str(tmp_path), "--i_embed", "1", "--use_viewdirs", "--N_importance", "8",
                                           "--N_samples", "8", "--netdepth", "2", "--netwidth", "64", "--netdepth_fine", "3", "--netwidth_fine", "32",
                                           "--hash_levels", "4", "--log2_hashmap_size", "10", "--base_resolution", "4",
                                           "--finest_resolution", "32", *extra])


def test_create_nerf_with_i_embed_1_builds_hash_networks(tmp_path):
    d = npa.config_parser().parse_args([])
    assert (d.hash_levels, d.hash_features, d.log2_hashmap_size, d.base_resolution, d.finest_resolution, d.hash_bound) == (16, 2, 19, 16, 512, 1.5)
    embed, ch = npa.get_embedder(10, 1)
    x = torch.randn(4, 3)
    assert ch == 3 and embed(x) is x
    train, test, start, grad_vars, opt = npa.create_nerf(hash_args(tmp_path, "--hash_bound", "2.0"), device=torch.device("cpu"))
    nc, nf = train["network_fn"], train["network_fine"]
    assert isinstance(nc, HashNeRF) and isinstance(nf, HashNeRF) and nc is not nf and start == 0
    assert isinstance(nc, npa.dense.DenseNeRF)        # render_rays' general-network path takes it
    assert nc.encoding.embeddings is not nf.encoding.embeddings and nc.encoding.lo == (-2.0,) * 3 and nc.encoding.hi == (2.0,) * 3
    assert (nc.D, nc.W, nf.D, nf.W) == (2, 64, 3, 32) and nc.input_ch == 8 and nc.input_ch_views == 27 and nc.mlp.input_ch == 8
    assert nc.mlp.output_ch == 5 and nc.skips == []
    assert any(p is nc.encoding.embeddings for p in grad_vars) and any(p is nf.encoding.embeddings for p in grad_vars)
    assert len(grad_vars) == len(list(nc.parameters())) + len(list(nf.parameters()))
    assert type(opt) is torch.optim.Adam
    assert sum(len(g["params"]) for g in opt.param_groups) == len(grad_vars)
    # the table stays out of the layer stack's parameter list, whose order is the reference's
    ref = npa.dense.DenseNeRF(D=2, W=64, input_ch=8, input_ch_views=27, output_ch=5, skips=[], use_viewdirs=True)
    assert [n for n, _ in nc.mlp.named_parameters()] == [n for n, _ in ref.named_parameters()]
    assert [n for n, _ in nc.named_parameters()] == ["encoding.embeddings"] + ["mlp." + n for n, _ in ref.named_parameters()]
    # a namespace without the new flags reads their defaults
    a = hash_args(tmp_path)
    for name in ("hash_levels", "hash_features", "log2_hashmap_size", "base_resolution", "finest_resolution", "hash_bound"):
        delattr(a, name)
    a.N_importance = 0
    train = npa.create_nerf(a, device=torch.device("cpu"))[0]
    assert train["network_fine"] is None and train["network_fn"].encoding.n_levels == 16 and train["network_fn"].encoding.hi == (1.5,) * 3
    # the reference's choices are untouched
    assert npa.get_embedder(10, -1)[1] == 3 and npa.get_embedder(10, 0)[1] == 63


def test_hash_nerf_defaults_and_refusals():
    net = HashNeRF(LO, HI, **FOUR)
    assert (net.D, net.W, net.skips, net.use_viewdirs, net.input_ch, net.input_ch_views, net.output_ch) == (2, 64, [], True, 8, 27, 4)
    assert net.multires_views == 4
    with pytest.raises(NotImplementedError):
        net.multires
    plain = HashNeRF(LO, HI, use_viewdirs=False, **FOUR)
    assert plain.input_ch_views == 0 and plain.multires_views == -1
    # the density head starts open: the raw density of a zero encoding is INITIAL_DENSITY whatever the layers' draw
    for seed in range(4):
        torch.manual_seed(seed)
        for m, head, row in ((HashNeRF(LO, HI, **FOUR).mlp, "alpha_linear", 0), (HashNeRF(LO, HI, D=3, use_viewdirs=False, **FOUR).mlp, "output_linear", 3)):
            h = torch.zeros(1, 8)
            for lin in m.pts_linears:
                h = torch.relu(lin(h))
            assert abs(float(getattr(m, head)(h).detach()[0, row]) - HashNeRF.INITIAL_DENSITY) <= 1e-6
    with pytest.raises(ValueError):
        net(torch.zeros(5, 31))
    with pytest.raises(NotImplementedError):
        HashNeRF(LO, HI, input_ch_views=10, **FOUR)


def test_state_dict_round_trips_through_torch_save(tmp_path):
    enc = four_level(F=4, seed=3)
    buf = io.BytesIO()
    torch.save(enc.state_dict(), buf)
    buf.seek(0)
    other = HashEncoding(LO, HI, n_features=4, **FOUR)
    assert not torch.equal(other.embeddings, enc.embeddings)
    other.load_state_dict(torch.load(buf))
    assert list(other.state_dict()) == ["embeddings"] and torch.equal(other.embeddings, enc.embeddings)
    pts = box_points(30, 17)
    assert torch.equal(other.encode_reference(pts), enc.encode_reference(pts))
    with pytest.raises(RuntimeError):       # another configuration has another number of rows
        HashEncoding(LO, HI, n_features=4, **dict(FOUR, log2_hashmap_size=11)).load_state_dict(enc.state_dict())
    # a checkpoint saved the way the reference saves it reloads through create_nerf
    a = hash_args(tmp_path)
    train, _, _, grad_vars, opt = npa.create_nerf(a, device=torch.device("cpu"))
    with torch.no_grad():
        for p in grad_vars:
            p.add_(0.25)
    os.makedirs(os.path.join(str(tmp_path), "h"), exist_ok=True)
    torch.save({"global_step": 7, "network_fn_state_dict": train["network_fn"].state_dict(),
                "network_fine_state_dict": train["network_fine"].state_dict(), "optimizer_state_dict": opt.state_dict()},
               os.path.join(str(tmp_path), "h", "000007.tar"))
    again, _, start, grad_vars2, _ = npa.create_nerf(a, device=torch.device("cpu"))
    assert start == 7 and len(grad_vars2) == len(grad_vars)
    assert all(torch.equal(p, q) for p, q in zip(grad_vars, grad_vars2))
    import copy
    clone = copy.deepcopy(train["network_fn"])
    assert torch.equal(clone.encoding.embeddings, train["network_fn"].encoding.embeddings) and clone.encoding._scratch == {}
