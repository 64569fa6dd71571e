"""CPU: OccupancyGrid's semantics -- the classification rule in plain torch (the definition the kernels reproduce), the bit layout,
checkpoints, and the masked oracle the GPU tests compare with."""
import io

import numpy as np
import pytest
import torch

import nerf_oracle as orc
import nerf_pytorch_amd as npa

CPU = torch.device("cpu")


def _grid(mask, outside="evaluate"):
    return npa.OccupancyGrid.from_mask(mask, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), outside=outside, device=CPU)


@pytest.mark.parametrize("outside", ["evaluate", "skip"])
def test_occupied_on_hand_placed_points(outside):
    """4^3 cells of width 0.5 over [-1, 1]^3; occupied: cells (0, 0, 0), (1, 1, 1) and (3, 3, 3).  A cell owns its lower faces
    (0 <= t, floor), `hi` itself is outside (t < R), a NaN is outside; what `outside` points get is the mode's choice."""
    mask = torch.zeros(4, 4, 4, dtype=torch.bool)
    mask[0, 0, 0] = mask[1, 1, 1] = mask[3, 3, 3] = True
    g = _grid(mask, outside)
    out = outside == "evaluate"
    nan = float("nan")
    cases = [
        ((-1.0, -1.0, -1.0), True),        # exactly lo: cell (0, 0, 0)
        ((-0.5, -0.5, -0.5), True),        # the corner shared by 8 cells belongs to (1, 1, 1)
        ((-0.5000001, -0.5, -0.5), False),  # one ulp below it on x: cell (0, 1, 1), empty
        ((-0.75, -0.75, -0.75), True),     # centre of (0, 0, 0)
        ((0.0, 0.0, 0.0), False),          # corner owned by (2, 2, 2), empty
        ((0.5, 0.5, 0.5), True),           # lower corner of (3, 3, 3)
        ((0.875, 0.99999, 0.75), True),
        ((0.99999994, 0.75, 0.75), out),   # the last fp32 below hi: p - lo rounds to 2.0 in fp32, t == R, outside BY THE RULE
        ((1.0, 1.0, 1.0), out),            # exactly hi: outside
        ((0.75, 0.75, 1.0), out),          # one axis on the upper face: outside
        ((-1.0000001, 0.0, 0.0), out),     # one ulp below lo
        ((nan, 0.75, 0.75), out),          # NaN: outside
        ((0.75, 0.75, nan), out),
        ((1e30, 0.0, 0.0), out), ((0.0, -float("inf"), 0.0), out),
    ]
    pts = torch.tensor([c[0] for c in cases], dtype=torch.float32)
    got = g.occupied(pts)
    assert got.dtype == torch.bool and got.tolist() == [c[1] for c in cases]
    # any leading shape
    assert torch.equal(g.occupied(pts.view(3, 5, 3)), got.view(3, 5))
    # a fresh grid is all-occupied; outside follows the mode
    fresh = npa.OccupancyGrid((-1, -1, -1), (1, 1, 1), 4, outside=outside, device=CPU)
    assert fresh.fraction_occupied() == 1.0
    assert fresh.occupied(pts).tolist() == [True] * 7 + [out] * 8


def test_scale_is_the_fp32_rounding_of_the_float64_quotient():
    g = npa.OccupancyGrid((0.1, -0.3, 0.0), (0.7, 1.1, 3.0), (7, 5, 512), device=CPU)
    lo, hi = np.float32([0.1, -0.3, 0.0]).astype(np.float64), np.float32([0.7, 1.1, 3.0]).astype(np.float64)
    assert g.scale.dtype == np.float32 and np.array_equal(g.scale, (np.float64([7, 5, 512]) / (hi - lo)).astype(np.float32))
    assert g.resolution == (7, 5, 512)
    for bad in (0, 513, (4, 4), (4, 0, 4)):
        with pytest.raises(ValueError):
            npa.OccupancyGrid((0, 0, 0), (1, 1, 1), bad, device=CPU)
    with pytest.raises(ValueError):
        npa.OccupancyGrid((0, 0, 0), (1, 0, 1), 4, device=CPU)
    with pytest.raises(ValueError):
        npa.OccupancyGrid((0, 0, 0), (1, 1, 1), 4, outside="ignore", device=CPU)


def test_word_and_bit_layout_and_mask_round_trip():
    """cell (ix, iy, iz) -> c = (ix Ry + iy) Rz + iz -> bit c & 31 of word c >> 5; 3 x 5 x 7 = 105 cells = 3 words + 9 bits"""
    R = (3, 5, 7)
    mask = torch.zeros(R, dtype=torch.bool)
    cells = [(0, 0, 0), (0, 0, 6), (0, 4, 3), (1, 0, 0), (2, 4, 6), (1, 2, 5)]
    for c in cells:
        mask[c] = True
    g = npa.OccupancyGrid.from_mask(mask, (0, 0, 0), (3, 5, 7), device=CPU)
    assert g.bits.dtype == torch.int32 and g.bits.shape == (4,) and g.resolution == R
    want = [0, 0, 0, 0]
    for ix, iy, iz in cells:
        c = (ix * 5 + iy) * 7 + iz
        want[c >> 5] |= 1 << (c & 31)
    assert [int(w) & 0xffffffff for w in g.bits] == want
    assert want[3] >> 9 == 0        # the tail bits of the last word stay clear
    assert torch.equal(g.to_mask(), mask)
    assert abs(g.fraction_occupied() - len(cells) / 105) < 1e-7
    # bit 31 (the sign bit of the int32 word) round-trips: cell c = 31
    m2 = torch.zeros(R, dtype=torch.bool)
    m2[0, 4, 3] = True
    g2 = npa.OccupancyGrid.from_mask(m2, (0, 0, 0), (3, 5, 7), device=CPU)
    assert int(g2.bits[0]) == -(1 << 31) and torch.equal(g2.to_mask(), m2)
    # a random mask, and occupied() at every cell centre reads it back
    rm = torch.rand(R, generator=torch.Generator().manual_seed(3)) < 0.4
    g3 = npa.OccupancyGrid.from_mask(rm, (0, 0, 0), (3, 5, 7), device=CPU)
    assert torch.equal(g3.to_mask(), rm)
    centres = g3.cell_points(0, 105)
    assert centres.shape == (105, 1, 3) and torch.equal(g3.occupied(centres[:, 0]), rm.reshape(-1))
    pts = g3.cell_points(0, 105, 4, torch.Generator().manual_seed(1))
    assert torch.equal(pts[:, 0], centres[:, 0]) and torch.equal(g3.occupied(pts), rm.reshape(-1, 1).expand(105, 4))


def test_state_dict_round_trip():
    rm = torch.rand(5, 3, 9, generator=torch.Generator().manual_seed(7)) < 0.5
    g = npa.OccupancyGrid.from_mask(rm, (-1.5, 0.25, 2.0), (1.0, 0.75, 6.5), outside="skip", device=CPU)
    buf = io.BytesIO()
    torch.save({"occupancy": g.state_dict()}, buf)      # travels with a checkpoint
    buf.seek(0)
    state = torch.load(buf)["occupancy"]
    h = npa.OccupancyGrid((0, 0, 0), (1, 1, 1), 2, device=CPU).load_state_dict(state)
    assert h.resolution == (5, 3, 9) and h.outside == "skip"
    assert np.array_equal(h.lo, g.lo) and np.array_equal(h.hi, g.hi) and np.array_equal(h.scale, g.scale)
    assert torch.equal(h.bits, g.bits) and torch.equal(h.to_mask(), rm)
    pts = torch.randn(200, 3, generator=torch.Generator().manual_seed(2)) * 3
    assert torch.equal(h.occupied(pts), g.occupied(pts))
    g.bits.zero_()          # a copy, not a view
    assert torch.equal(h.to_mask(), rm)
    bad = dict(state, bits=state["bits"][:-1])
    with pytest.raises(ValueError):
        h.load_state_dict(bad)


_PLAIN_QUERY_FIELD = orc.query_field


def masked_query_field(grid):
    """the reference's network_query_fn with the rows of skipped samples replaced by zeros"""
    plain = _PLAIN_QUERY_FIELD

    def q(P, pts, viewdirs, *a, **k):
        raw = plain(P, pts, viewdirs, *a, **k)
        return torch.where(grid.occupied(pts)[..., None], raw, torch.zeros_like(raw))
    return q


@pytest.mark.parametrize("white", [False, True])
def test_oracle_under_masking_is_well_defined(monkeypatch, white):
    """trace_rays with the masked query: rays through a fully EMPTY box come back with acc_map == 0 and the background colour; an
    all-occupied grid changes nothing."""
    Pc, Pf = orc.scene_params()
    rays = orc.synthetic_rays(24, seed=3)
    plain = orc.trace_rays(rays, Pc, Pf, 16, 16, white_bkgd=white)
    empty = npa.OccupancyGrid.from_mask(torch.zeros(4, 4, 4, dtype=torch.bool), (-8, -8, -8), (8, 8, 8), device=CPU)
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * plain["_z_vals"][..., None]
    assert not empty.occupied(pts).any()        # every sample lies in the box
    monkeypatch.setattr(orc, "query_field", masked_query_field(empty))
    out = orc.trace_rays(rays, Pc, Pf, 16, 16, white_bkgd=white, retraw=True)
    assert torch.equal(out["acc_map"], torch.zeros(24)) and torch.equal(out["acc0"], torch.zeros(24))
    assert torch.equal(out["rgb_map"], torch.full((24, 3), 1.0 if white else 0.0))
    assert torch.equal(out["raw"], torch.zeros(24, 32, 4))
    assert float(plain["acc_map"].max()) > 0.5   # (the scene itself is not empty)
    monkeypatch.setattr(orc, "query_field", masked_query_field(npa.OccupancyGrid((-8, -8, -8), (8, 8, 8), 4, device=CPU)))
    full = orc.trace_rays(rays, Pc, Pf, 16, 16, white_bkgd=white)
    for k in ("rgb_map", "acc_map", "disp_map", "rgb0"):
        assert torch.equal(full[k].nan_to_num(nan=-1.0), plain[k].nan_to_num(nan=-1.0)), k     # (disp of an empty ray is 0 / 0, as in the reference)


def test_render_rays_takes_occupancy_as_a_keyword_only_argument():
    """like `randoms`: keyword-only, default None"""
    import inspect
    sig = inspect.signature(npa.render_rays)
    assert sig.parameters["occupancy"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["occupancy"].default is None
