"""CPU: DensityGrid's semantics in plain torch -- the density step (_update_reference: decay, maximum, NaN), the bits of the whole grid
(_bits_reference: the threshold's strict >, dilation recomputed from the densities), the cursor arithmetic of update(), maybe_update's
schedule, checkpoints, the export list, and that the library resolves the three entry points of the training path."""
import ctypes
import io

import pytest
import torch

import nerf_pytorch_amd as npa

CPU = torch.device("cpu")
NAN, INF = float("nan"), float("inf")


def grid(res=4, **kw):
    return npa.DensityGrid((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), res, device=CPU, **kw)


def test_export_and_a_new_grid():
    assert "DensityGrid" in npa.__all__ and issubclass(npa.DensityGrid, npa.OccupancyGrid)
    g = grid(5)
    assert g.density.shape == (125,) and g.density.dtype == torch.float32 and bool((g.density == 0).all())
    assert g.fraction_occupied() == 1.0 and g.cursor == 0 and g.n_updates == 0
    assert (g.decay, g.sigma_threshold, g.dilate, g.update_every, g.warmup_steps) == (0.95, 0.01, 0, 16, 256)
    for bad in (dict(decay=1.5), dict(dilate=-1), dict(update_every=0), dict(warmup_steps=-1)):
        with pytest.raises(ValueError):
            grid(**bad)


def test_density_step_on_hand_made_numbers():
    g = grid(2, decay=0.5)
    g.density[:] = torch.tensor([4.0, 4.0, 4.0, -4.0, 0.0, 4.0, 1.0, 2.0])
    #                      cell:  0     1     2     3     4    5      6    7
    sigma = torch.tensor([[1.0, 0.5], [3.0, 2.5], [NAN, 1.0], [-3.0, -9.0], [-1.0, NAN], [NAN, NAN], [INF, 0.0], [1.0, 1.0]])
    g._update_reference(sigma.reshape(-1), 0, 8)
    # decay wins (2 > 1), the maximum wins (3 > 2), a NaN sample is ignored (max(2, 1)), negative densities decay TOWARDS zero and a
    # larger negative sample still loses (-2 > -3), 0 * decay = 0 > -1, all-NaN = -inf: the decayed value stays, inf is a maximum like any
    assert g.density.tolist() == [2.0, 3.0, 2.0, -2.0, 0.0, 2.0, INF, 1.0]
    # a run inside the grid touches only its cells; one fp32 multiplication: 0.1f * 0.95f
    h = grid(4, decay=0.95)
    h.density[:] = 0.1
    h._update_reference(torch.full((32,), -INF), 32, 64)
    want = (torch.tensor(0.1, dtype=torch.float32) * torch.tensor(0.95, dtype=torch.float32)).item()
    assert bool((h.density[32:64] == want).all()) and bool((h.density[:32] == torch.tensor(0.1)).all()) and bool((h.density[64:] == torch.tensor(0.1)).all())


def test_bits_threshold_is_strict_and_dilation_does_not_accumulate():
    g = grid(7, sigma_threshold=0.5, dilate=0, decay=1.0)
    g.density[0], g.density[1], g.density[2] = 0.5, 0.5000001, NAN
    g.bits = g._bits_reference()
    assert g.to_mask().reshape(-1)[:3].tolist() == [False, True, False] and int(g.to_mask().sum()) == 1
    # a lone cell, dilate = 1, two updates: one ring (27 cells) both times, because the bits are recomputed from the densities
    d = grid(7, sigma_threshold=0.5, dilate=1, decay=1.0)
    centre = (3 * 7 + 3) * 7 + 3
    sigma = torch.zeros(d.n_cells)
    sigma[centre] = 2.0
    for _ in range(2):
        d._update_reference(sigma, 0, d.n_cells)
        d.bits = d._bits_reference()
        m = d.to_mask()
        assert int(m.sum()) == 27 and bool(m[2:5, 2:5, 2:5].all())
    d.dilate = 2
    d.bits = d._bits_reference()
    assert int(d.to_mask().sum()) == 125
    # a corner cell: neighbours beyond the faces do not exist
    c = grid(3, sigma_threshold=0.0, dilate=1)
    c.density[0] = 1.0
    c.bits = c._bits_reference()
    assert int(c.to_mask().sum()) == 8 and bool(c.to_mask()[:2, :2, :2].all())


def test_cursor_arithmetic():
    g = grid(8)                     # 512 cells = 16 words
    assert g._next_runs(0.25) == [(0, 512)] and g.cursor == 0 and g.n_updates == 1      # the first visit: every cell, whatever fraction says
    seen = torch.zeros(16, dtype=torch.int64)
    for call in range(4):
        runs = g._next_runs(0.25)
        assert len(runs) == 1 and runs[0][0] == 128 * call and runs[0][0] % 32 == 0
        for a, b in runs:
            seen[a // 32:(b + 31) // 32] += 1
    assert seen.tolist() == [1] * 16 and g.cursor == 0 and g.n_updates == 5
    # a fraction that does not divide the grid wraps: 0.3 * 16 words rounds up to 5
    starts = []
    for _ in range(4):
        runs = g._next_runs(0.3)
        starts.append(runs)
        assert all(a % 32 == 0 for a, _ in runs) and sum(b - a for a, b in runs) == 160
    assert starts == [[(0, 160)], [(160, 320)], [(320, 480)], [(480, 512), (0, 128)]] and g.cursor == 128
    # a cell count that is no multiple of 32: the last word is short
    odd = grid((3, 5, 7))           # 105 cells = 4 words
    assert odd._next_runs(1.0) == [(0, 105)]
    assert odd._next_runs(0.5) == [(0, 64)] and odd._next_runs(0.5) == [(64, 105)] and odd.cursor == 0
    assert odd._next_runs(0.75) == [(0, 96)] and odd._next_runs(0.75) == [(96, 105), (0, 64)] and odd.cursor == 64
    assert odd._next_runs(1e-9) == [(64, 96)]       # at least one word
    with pytest.raises(ValueError):
        odd._next_runs(0.0)


def test_maybe_update_schedule(monkeypatch):
    g = grid(4, warmup_steps=8, update_every=4)
    calls = []
    monkeypatch.setattr(g, "update", lambda model, **kw: calls.append((model, kw)))
    done = [s for s in range(20) if g.maybe_update("net", s, fraction=0.5)]
    assert done == [8, 12, 16] and calls == [("net", dict(fraction=0.5))] * 3
    assert g.fraction_occupied() == 1.0      # (all-occupied through the warm-up, and here throughout: update was replaced)
    h = grid(4, warmup_steps=0, update_every=1)
    monkeypatch.setattr(h, "update", lambda model, **kw: calls.append(model))
    assert h.maybe_update("n", 0) is True and g.maybe_update("n", 7) is False


def test_update_refuses_what_from_network_refuses():
    g = grid(4)
    with pytest.raises(NotImplementedError):
        g.update(torch.nn.Linear(3, 4))
    kw = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    with pytest.raises(npa.hip_backend.NerfHipError, match="GPU"):
        g.update(npa.NeRF(**kw))
    assert g.n_updates == 0 and g.cursor == 0


def test_state_dict_round_trip_and_loading_into_a_plain_grid():
    gen = torch.Generator().manual_seed(3)
    g = npa.DensityGrid((-1.5, 0.25, 2.0), (1.0, 0.75, 6.5), (3, 5, 7), outside="skip", device=CPU, decay=0.9, sigma_threshold=0.3, dilate=1,
                        update_every=4, warmup_steps=12)
    g._next_runs(1.0)
    g._next_runs(0.5)
    g._update_reference(torch.rand(g.n_cells, generator=gen), 0, g.n_cells)
    g.bits = g._bits_reference()
    buf = io.BytesIO()
    torch.save(g.state_dict(), buf)
    buf.seek(0)
    state = torch.load(buf, weights_only=False)
    h = npa.DensityGrid((0, 0, 0), (1, 1, 1), 2, device=CPU).load_state_dict(state)
    assert h.resolution == (3, 5, 7) and h.outside == "skip" and torch.equal(h.bits, g.bits) and torch.equal(h.density, g.density)
    assert (h.cursor, h.n_updates) == (g.cursor, g.n_updates) == (64, 2)
    assert (h.decay, h.sigma_threshold, h.dilate, h.update_every, h.warmup_steps) == (0.9, 0.3, 1, 4, 12)
    assert (h.lo == g.lo).all() and (h.hi == g.hi).all() and (h.scale == g.scale).all()
    assert h._next_runs(0.5) == g._next_runs(0.5)
    # into a plain OccupancyGrid: the fields that class knows
    p = npa.OccupancyGrid((0, 0, 0), (1, 1, 1), 2, device=CPU).load_state_dict(state)
    assert p.resolution == (3, 5, 7) and p.outside == "skip" and torch.equal(p.bits, g.bits) and not hasattr(p, "density")
    pts = torch.rand(200, 3, generator=gen) * 6 - 2
    assert torch.equal(p.occupied(pts), g.occupied(pts))
    # the other way round there is no density to load
    with pytest.raises(ValueError, match="DensityGrid"):
        npa.DensityGrid((0, 0, 0), (1, 1, 1), 2, device=CPU).load_state_dict(p.state_dict())
    bad = dict(state, density=torch.zeros(7))
    with pytest.raises(ValueError, match="density"):
        npa.DensityGrid((0, 0, 0), (1, 1, 1), 2, device=CPU).load_state_dict(bad)


def test_from_mask_gives_a_density_grid_with_the_masks_bits():
    mask = torch.rand(4, 4, 4, generator=torch.Generator().manual_seed(1)) < 0.5
    g = npa.DensityGrid.from_mask(mask, (-1, -1, -1), (1, 1, 1), device=CPU)
    assert isinstance(g, npa.DensityGrid) and torch.equal(g.to_mask(), mask) and bool((g.density == 0).all())


def test_library_resolves_the_training_entry_points():
    """the build exports nerf_occ_gather / nerf_occ_fold_rays / nerf_occ_density_update, they are bound, and bad arguments are codes"""
    lib = ctypes.CDLL(npa.build.LIB_PATH)
    names = ("nerf_occ_gather", "nerf_occ_fold_rays", "nerf_occ_density_update")
    for name in names:
        assert hasattr(lib, name) and name in npa.hip_backend.EXPORTS
    L = npa.hip_backend.lib()
    assert L.nerf_abi_version() == 10
    assert L.nerf_occ_gather(None, None, 4, None, None) != 0
    assert L.nerf_occ_fold_rays(None, None, None, 1, 1, None, 0, None) != 0
    assert L.nerf_occ_density_update(None, 1, 1, 0.5, None, None) != 0
    assert "null" in L.nerf_last_error().decode()
