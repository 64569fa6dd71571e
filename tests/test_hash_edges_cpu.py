"""CPU: the conditions the hash-grid edge tests (test_hash_edges_gpu.py) stand on, checked without a GPU -- the level tables of the edge
configurations, that their u R really rounds (and the four-level fixture's does not), that TINY's corners collide inside one point,
table_grad_reference against float64 autograd on each of them and at three magnitudes of max |d_out|, and the saturated row."""
import math

import pytest
import torch

from nerf_pytorch_amd.hashgrid import HashEncoding
from test_hash_cpu import box_points, four_level, node_points

F64 = torch.float64
ODD_LO, ODD_HI = (-1.5, -1.3, -0.7), (1.5, 1.7, 2.4)        # extents 3, 3, 3.1: no power of two, and 1 / extent is not an fp32 number
CUBE_LO, CUBE_HI = (-1.5,) * 3, (1.5,) * 3                  # create_nerf's default box (--hash_bound 1.5)
# name: (lo, hi, HashEncoding's arguments, the values of n_features that run)
CONFIGS = {
    "ODD": (ODD_LO, ODD_HI, dict(n_levels=5, log2_hashmap_size=10, base_resolution=3, finest_resolution=37), (1, 2, 4)),
    "TINY": (ODD_LO, ODD_HI, dict(n_levels=1, log2_hashmap_size=4, base_resolution=7, finest_resolution=7), (1, 4)),
    "ALL_DENSE_32": (ODD_LO, ODD_HI, dict(n_levels=32, log2_hashmap_size=8, base_resolution=5, finest_resolution=5), (1,)),
    "MIXED_32": (ODD_LO, ODD_HI, dict(n_levels=32, log2_hashmap_size=8, base_resolution=2, finest_resolution=300), (1,)),
    "DEFAULT": (CUBE_LO, CUBE_HI, dict(), (2,)),
    "FINE": (CUBE_LO, CUBE_HI, dict(n_levels=2, log2_hashmap_size=12, base_resolution=1 << 20, finest_resolution=1 << 24), (2,)),
}
SMALL = [(name, F) for name in ("ODD", "TINY", "ALL_DENSE_32", "MIXED_32") for F in CONFIGS[name][3]]       # (cheap enough for every test)
BACKWARD_SIZES = (1, 64, 256, 257, 1024)        # ceil(log2 P) at powers of two and behind them
BACKWARD_SEED = 400                             # (+ P: the one point of P = 1 then has two corners in one of TINY's rows)
MAGNITUDES = (1e-41, 1e-30, 2.0 ** 100)         # of d_out = randn * s: the first makes max |d_out| a denormal
SATURATED_NODE = (-0.5, 0.0, 1.0)               # node (1, 1, 1) of FOUR's level 0, a node of every finer level too
SATURATED_ROW = 1 + 1 * 5 + 1 * 25
SATURATED_P = 4096


def encoding(name, F, seed=0):
    """a fresh HashEncoding of one configuration with a seeded randn table, as four_level makes it"""
    lo, hi, kw, features = CONFIGS[name]
    assert F in features
    enc = HashEncoding(lo, hi, n_features=F, **kw)
    with torch.no_grad():
        enc.embeddings.copy_(torch.randn(enc.embeddings.shape, generator=torch.Generator().manual_seed(seed + 1)))
    return enc


def special_points(enc):
    """hi, a point on each of the six faces, points outside, lo, five lattice nodes of every distinct resolution -- over the encoding's
    own box.  On the odd box a node is not an fp32 point: it lies within an ulp of a cell boundary, on either side."""
    lo, hi = torch.tensor(enc.lo), torch.tensor(enc.hi)
    faces = box_points(6, 21, lo=enc.lo, hi=enc.hi)
    for k in range(6):
        faces[k, k // 2] = (lo, hi)[k % 2][k // 2]
    outside = torch.stack([hi + torch.tensor([0.5, 0.0, 0.0]), lo - torch.tensor([0.0, 3.0, 0.25]), hi + 1e30, lo - 7.0,
                           torch.tensor([0.0, 9.0, 1.0]), torch.tensor([-40.0, 0.25, 2.0])])
    first = [enc.level_resolution.index(r) for r in sorted(set(enc.level_resolution))]
    return torch.cat([hi[None], faces, outside, lo[None]] + [node_points(enc, level)[1] for level in first])


def edge_points(enc, P, seed):
    """[P, 3]: draws over 1.1 x the box first (at least a quarter of the points), then the special points"""
    special = special_points(enc)
    n = max(P - special.shape[0], (P + 3) // 4)
    return torch.cat([box_points(n, seed, spread=1.1, lo=enc.lo, hi=enc.hi), special])[:P].contiguous()


def own_corner_collisions(enc, pts, level=0):
    """the number of points two of whose eight corners on `level` share a row"""
    rows, _ = enc._corners(pts, level, torch.float32)
    return int(((rows[:, :, None] == rows[:, None, :]).sum((1, 2)) > 8).sum())


def float64_errors(enc, pts, d_out, got):
    """(max |got - float64 autograd|, max |float32 autograd - float64 autograd|) of the table's gradient"""
    E64 = enc.embeddings.detach().cpu().double().requires_grad_(True)
    (enc.encode_reference(pts, F64, E64) * d_out.double()).sum().backward()
    E32 = enc.embeddings.detach().cpu().clone().requires_grad_(True)
    (enc.encode_reference(pts, torch.float32, E32) * d_out).sum().backward()
    return float((got.double() - E64.grad).abs().max()), float((E32.grad.double() - E64.grad).abs().max())


def saturated_case(alternating):
    """4096 copies of one node of FOUR's every level, d_out = +-float32(1.9999999) = 2 - 2^-23: a full mantissa, P M in one row"""
    pts = torch.tensor(SATURATED_NODE).expand(SATURATED_P, 3).contiguous()
    d_out = torch.full((SATURATED_P, 4 * 2), 1.9999999)
    if alternating:
        d_out[1::2] *= -1.0
    return pts, d_out


# ------------------------------------------------------------------------------------------------ level tables
def test_level_tables_of_the_edge_configurations():
    T10 = 1 << 10
    odd = encoding("ODD", 1)
    assert odd.level_resolution == [3, 5, 10, 19, 37] and odd.level_dense == [True, True, False, False, False]
    assert odd.level_offset == [0, 64, 64 + 216, 280 + T10, 280 + 2 * T10, 280 + 3 * T10] and odd.out_dim == 5
    tiny = encoding("TINY", 4)
    assert (tiny.level_resolution, tiny.level_dense, tiny.level_offset, tiny.out_dim) == ([7], [False], [0, 16], 4)
    dense = encoding("ALL_DENSE_32", 1)
    assert dense.level_resolution == [5] * 32 and dense.level_dense == [True] * 32 and dense.rows_total == 32 * 216 and dense.out_dim == 32
    mixed = encoding("MIXED_32", 1)
    R = mixed.level_resolution
    assert len(R) == 32 and R[0] == 2 and R[-3:] == [217, 255, 300] and all(a <= b for a, b in zip(R, R[1:]))
    assert mixed.level_dense == [True] * 7 + [False] * 25 and R[6] <= 5 < R[7]          # 6^3 = 216 <= 2^8 < 7^3
    assert mixed.rows_total == sum((r + 1) ** 3 for r in R[:7]) + 25 * 256
    default = HashEncoding(CUBE_LO, CUBE_HI)                # (no table drawn: the fresh one)
    assert default.level_resolution == [16, 20, 25, 32, 40, 50, 64, 80, 101, 128, 161, 203, 256, 322, 406, 512]
    assert default.rows_total == 5262476 and default.level_offset[-2] > 1 << 22 and default.out_dim == 32
    fine = encoding("FINE", 2)
    assert fine.level_resolution == [1 << 20, 1 << 24] and fine.level_dense == [False, False] and fine.rows_total == 2 << 12


# ------------------------------------------------------------------------------------------------ the rounding these configurations reach
def fused_differs(enc, level, pts):
    """the fraction of coordinates whose f = p - i changes when u R - i is rounded once (a fused multiply-subtract) instead of twice"""
    R = enc.level_resolution[level]
    u = torch.clamp((pts - enc._lo32) * enc._inv32, 0.0, 1.0)
    p = u * float(R)
    i = torch.clamp(torch.floor(p), 0, R - 1)
    f = p - i
    fused = (u.double() * float(R) - i.double()).float()
    return float((fused != f).double().mean())


def test_the_rounding_of_u_R_is_visible_here_and_not_on_the_four_level_fixture():
    four = four_level()
    for level in range(4):
        assert fused_differs(four, level, box_points(2000, 31)) == 0.0
    odd = encoding("ODD", 1)
    assert fused_differs(odd, 4, box_points(2000, 32, lo=ODD_LO, hi=ODD_HI)) >= 1.0 / 3.0           # R = 37
    # the default's finest level is R = 512, where u R is exact whatever the box: the bound holds on each of its ten levels
    # whose R is no power of two (the finest of them R = 406), and the other six show nothing
    default = HashEncoding(CUBE_LO, CUBE_HI)
    pts = box_points(2000, 33, lo=CUBE_LO, hi=CUBE_HI)
    seen = {R: fused_differs(default, level, pts) for level, R in enumerate(default.level_resolution)}
    print({R: round(v, 3) for R, v in seen.items()})
    for R, v in seen.items():
        assert (v == 0.0) if R & (R - 1) == 0 else (v >= 1.0 / 3.0), (R, v)
    assert sum(1 for R in seen if R & (R - 1)) == 10


def test_float32_and_float64_agree_on_the_cell_except_on_FINE():
    """what lets the GPU tests compare with float64 autograd everywhere but on FINE, which is compared with the fp32 definition only"""
    differ = lambda enc, pts: sum(int((enc._corners(pts, level, torch.float32)[0] != enc._corners(pts, level, F64)[0]).any(1).sum())
                                  for level in range(enc.n_levels))
    for name in ("ODD", "TINY", "ALL_DENSE_32", "MIXED_32", "DEFAULT"):
        lo, hi, kw, _ = CONFIGS[name]
        # (draws only: the odd box's lattice nodes are meant to sit within an ulp of a boundary, where the two may part)
        assert differ(HashEncoding(lo, hi, **kw), box_points(1000, 34, spread=1.1, lo=lo, hi=hi)) == 0, name
    assert differ(encoding("FINE", 2), box_points(1000, 34, spread=1.1, lo=CUBE_LO, hi=CUBE_HI)) > 200         # of 2000 point-levels


def test_two_corners_of_one_point_share_a_row_on_TINY():
    for F in CONFIGS["TINY"][3]:
        enc = encoding("TINY", F)
        for P in BACKWARD_SIZES:
            assert own_corner_collisions(enc, edge_points(enc, P, seed=BACKWARD_SEED + P)) >= 1, P


# ------------------------------------------------------------------------------------------------ table_grad_reference
@pytest.mark.parametrize("name,F", SMALL + [("DEFAULT", 2)])
def test_table_grad_reference_against_float64_autograd(name, F):
    enc = encoding(name, F)
    pts = edge_points(enc, 1000, seed=35)
    d_out = torch.randn(1000, enc.out_dim, generator=torch.Generator().manual_seed(36))
    got = enc.table_grad_reference(pts, d_out)
    err, own = float64_errors(enc, pts, d_out, got)
    print(f"{name} F={F}: fixed-point error {err:.3e}, float32 autograd's own {own:.3e}, ratio {err / own:.2f}")
    assert own > 0.0 and err <= 4.0 * own


@pytest.mark.parametrize("s", MAGNITUDES)
def test_table_grad_reference_at_three_magnitudes(s):
    enc = encoding("ODD", 2)
    pts = edge_points(enc, 1000, seed=37)
    d_out = torch.randn(1000, enc.out_dim, generator=torch.Generator().manual_seed(38)) * s
    M = float(d_out.abs().max())
    assert 0.0 < M < math.inf and (M < 2.0 ** -126) == (s == 1e-41)
    got = enc.table_grad_reference(pts, d_out)
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0.0
    # float64 autograd with both factors scaled to order one (a power of two for the last, so the scaling is exact there)
    E64 = enc.embeddings.detach().double().requires_grad_(True)
    (enc.encode_reference(pts, F64, E64) * (d_out.double() / s)).sum().backward()
    rel = float((got.double() / s - E64.grad).abs().max() / E64.grad.abs().max())
    print(f"s={s:g}: M={M:.3e}, relative error {rel:.3e}")
    assert rel <= 2e-4


@pytest.mark.parametrize("alternating", [False, True])
def test_a_row_that_receives_P_M(alternating):
    enc = four_level()
    pts, d_out = saturated_case(alternating)
    rows, w = enc._corners(pts[:1], 0, torch.float32)
    assert int(rows[0, 0]) == SATURATED_ROW and w[0].tolist() == [1.0] + [0.0] * 7
    got = enc.table_grad_reference(pts, d_out)
    g = float(torch.tensor(1.9999999))
    assert g == 2.0 - 2.0 ** -23
    want = 0.0 if alternating else SATURATED_P * g         # 2^13 - 2^-11: 24 bits, an fp32 number
    assert got[SATURATED_ROW].tolist() == [want, want]
    assert int((got != 0).sum()) == (0 if alternating else 4 * 2)          # one row per level
