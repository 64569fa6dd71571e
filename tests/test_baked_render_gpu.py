"""GPU tests (-m gpu) of the public chain of baked fields: BakedField.from_network against the same values written out from the public
pieces, render_rays(baked=) / batchify_rays / render / render_path against BakedField.render_rays on the same ray records, the one
random draw of perturb, and -- baked=None: nothing changes -- the sequence of library calls of a dense render_rays call against
tests/golden/baked_off_call_trace.json.

The fixture holds the NAMES of the C entry points a dense two-network render_rays call makes, in order, without a gradient and with a
backward, on the fp32 and the fp16x3 datapath (launches only: is_launch below).  It was recorded by `record_trace` below on the commit
BEFORE the baked path existed:

    NERF_RECORD_BAKED_OFF_TRACE=tests/golden/baked_off_call_trace.json python -m pytest -m gpu tests/test_baked_render_gpu.py"""
import json
import math
import os

import numpy as np
import pytest
import torch

import nerf_oracle as orc
from test_gpu_occupancy import BOX_HI, BOX_LO, bits_equal
from test_gpu_occupancy_train import positive_median_density
from test_gpu_parity import dev, nets, npa  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "baked_off_call_trace.json")
RES, N_DIRS, DEGREE = 12, 16, 2
H, W, FOCAL = 12, 10, 14.0
MAPS = ["rgb_map", "disp_map", "acc_map", "depth_map"]
NO_NET = dict(network_fn=None, network_query_fn=None, N_samples=64)


def pose(x=0.0):
    """a camera at (x, 0, 4) looking down -z at the scene around the origin"""
    return torch.tensor([[1.0, 0.0, 0.0, x], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 4.0]])


def intrinsics():
    return np.array([[FOCAL, 0.0, 0.5 * W], [0.0, FOCAL, 0.5 * H], [0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def scene(npa, dev, nets):
    """(grid, field, rays [130, 11]): the fixture fine network baked into a 12^3 grid over [-2, 2]^3 whose cells are those above the median
    positive density (no dilation: about half of the box)"""
    nf = nets[1]
    thr = positive_median_density(npa, nf, dev, RES)
    grid = npa.OccupancyGrid.from_network(nf, BOX_LO, BOX_HI, RES, sigma_threshold=thr, dilate=0)
    assert 0.05 < grid.fraction_occupied() < 0.95
    field = npa.BakedField.from_network(nf, grid, sh_degree=DEGREE, n_dirs=N_DIRS)
    return grid, field, orc.synthetic_rays(130, seed=21).to(dev)


def test_from_network_equals_the_public_pieces(npa, dev, nets, scene):
    """BIT FOR BIT: the test evaluates ALL 13^3 nodes in one batch, from_network the stored ones in its own batches; the field kernels
    evaluate a point independently of its batch, and both sides add over the directions left to right, one multiplication and one
    addition per term, so not one fp16 entry may differ.  A second bake in chunks of 1000 (node, direction) pairs gives the same table."""
    grid, field, _ = scene
    nf = nets[1]
    n = RES + 1
    i = torch.arange(N_DIRS, dtype=torch.float64)
    z = 1.0 - (2.0 * i + 1.0) / N_DIRS
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    s = torch.sqrt(1.0 - z * z)
    dirs = torch.stack([s * torch.cos(phi), s * torch.sin(phi), z], -1).float().to(dev)
    fit = npa.BakedField.sh_fit_matrix(N_DIRS, DEGREE).to(dev)
    pts = npa.mesh.lattice_points(BOX_LO, BOX_HI, n, 0, n ** 3, dev)
    with torch.no_grad():
        raw = npa.query_points(nf, pts.repeat_interleave(N_DIRS, 0), dirs.repeat(n ** 3, 1)).view(n ** 3, N_DIRS, 4)
        sigma = torch.zeros(n ** 3, device=dev)
        coef = torch.zeros(n ** 3, 3, 9, device=dev)
        for k in range(N_DIRS):
            sigma = sigma + torch.relu(raw[:, k, 3])
            coef = coef + raw[:, k, :3, None] * fit[None, None, :, k]
    nodes = torch.cat([(sigma / N_DIRS)[:, None], coef.reshape(-1, 27)], -1).view(n, n, n, 28)
    want = npa.BakedField.from_nodes(grid, nodes, DEGREE)
    assert field.table.shape == want.table.shape == (field.n_rows, 32) and 1 < field.n_rows < n ** 3 + 1
    assert torch.equal(field.index, want.index)
    assert torch.equal(field.table.view(torch.int16), want.table.view(torch.int16))
    assert bool((field.table[1:, 0] >= 0).all()) and float(field.table[1:, 0].max()) > 0.0         # sigma behind the ReLU
    assert abs(field.step_size - 0.5 * 4.0 / RES) < 1e-6 and field.stop_eps == 0.0 and field.device == grid.device
    again = npa.BakedField.from_network(nf, grid, sh_degree=DEGREE, n_dirs=N_DIRS, chunk=1000)
    assert torch.equal(again.table.view(torch.int16), field.table.view(torch.int16)) and torch.equal(again.index, field.index)


def same_maps(got, want):
    assert list(got) == MAPS
    for k in MAPS:
        assert got[k].shape == want[k].shape and bits_equal(got[k], want[k]), k


def test_the_chain_equals_the_field(npa, dev, scene):
    _, field, rays = scene
    want = field.render_rays(rays)
    stats = dict(field.last_stats)
    assert stats["rays"] == 130 and stats["samples"] > 130 and float(want["acc_map"].max()) > 0.01
    field.last_stats = None
    same_maps(npa.render_rays(rays, None, None, N_samples=64, baked=field), want)
    assert field.last_stats == stats
    field.last_stats = None
    same_maps(npa.batchify_rays(rays, 48, baked=field, **NO_NET), want)        # chunks of 48, 48 and 34 rays
    assert field.last_stats == stats
    white = field.render_rays(rays, white_bkgd=True)
    same_maps(npa.render_rays(rays, None, None, N_samples=64, white_bkgd=True, baked=field), white)
    assert not bits_equal(white["rgb_map"], want["rgb_map"])
    # render: the ray records of one camera, in chunks of 40
    K = intrinsics()
    records = npa.hip_backend.make_rays(H, W, K, pose(), None, False, 2.0, 6.0, dev)
    frame = field.render_rays(records)
    stats = dict(field.last_stats)
    field.last_stats = None
    out = npa.render(H, W, K, chunk=40, c2w=pose(), ndc=False, near=2.0, far=6.0, use_viewdirs=True, baked=field, **NO_NET)
    assert len(out) == 4 and list(out[3]) == ["depth_map"]
    for got, k in zip(out[:3] + [out[3]["depth_map"]], MAPS):
        assert got.shape == (H, W) + tuple(frame[k].shape[1:]) and bits_equal(got.reshape(frame[k].shape), frame[k]), k
    assert field.last_stats == stats and stats["rays"] == H * W and stats["samples"] > 0
    # under grad mode with rays that need none: the same, detached
    got = npa.render_rays(rays, None, None, N_samples=64, baked=field)
    assert not any(v.requires_grad for v in got.values())
    with pytest.raises(ValueError, match="no backward"):
        npa.render_rays(rays.clone().requires_grad_(True), None, None, N_samples=64, baked=field)


def test_perturb_draws_one_offset_per_ray(npa, dev, scene):
    _, field, rays = scene
    torch.manual_seed(1234)
    got = npa.render_rays(rays, None, None, N_samples=64, perturb=1.0, baked=field)
    after = torch.cuda.get_rng_state(dev)
    torch.manual_seed(1234)
    u = torch.rand(rays.shape[0], device=dev)
    assert torch.equal(torch.cuda.get_rng_state(dev), after)                # exactly one torch.rand(N)
    same_maps(got, field.render_rays(rays, u=u))
    assert not bits_equal(got["depth_map"], field.render_rays(rays)["depth_map"])
    torch.manual_seed(1234)             # no draw without perturb
    before = torch.cuda.get_rng_state(dev)
    npa.render_rays(rays, None, None, N_samples=64, perturb=0.0, baked=field)
    assert torch.equal(torch.cuda.get_rng_state(dev), before)


def test_render_path_renders_frames(npa, dev, scene):
    _, field, _ = scene
    poses = torch.stack([pose(0.0), pose(0.3)]).to(dev)
    kw = dict(NO_NET, baked=field, ndc=False, near=2.0, far=6.0, use_viewdirs=True, white_bkgd=True)
    rgbs, disps = npa.render_path(poses, (H, W, FOCAL), intrinsics(), 64, kw)
    assert rgbs.shape == (2, H, W, 3) and disps.shape == (2, H, W)
    first = npa.render(H, W, intrinsics(), chunk=64, c2w=poses[0], **kw)
    assert np.array_equal(rgbs[0], first[0].cpu().numpy()) and not np.array_equal(rgbs[0], rgbs[1])


# ------------------------------------------------------------------------------------------------ baked=None: nothing changes
TRACE_N, TRACE_C, TRACE_F = 96, 16, 24
TRACE_ROWS = [f"{p}/{m}" for p in ("fp32", "fp16x3") for m in ("no_grad", "backward")]


def is_launch(name):
    """what the trace keeps: not the host-side size queries, and neither the parameter repack (cached per network) nor the range
    monitor's scans (scheduled by the monitor's own state), which depend on what ran before"""
    return not ("pack" in name or name.endswith(("_floats", "_floats_dp", "_words", "_supported"))
                or name in ("nerf_last_error", "nerf_buffer_layout", "nerf_range_scan"))


def record_trace(npa_mod, device, nc, nf, extra):
    """{row: [the names of the C entry points one dense render_rays call makes, in order]}; extra: keyword arguments added to the call"""
    hb = npa_mod.hip_backend
    real = hb.lib()
    names = []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            return lambda *a, **k: (names.append(name), fn(*a, **k))[1]
    rays = orc.synthetic_rays(TRACE_N, seed=3).to(device)
    rnd = {k: v.to(device) for k, v in orc.synthetic_randoms(TRACE_N, TRACE_C, TRACE_F, seed=4).items()}
    kw = dict(N_samples=TRACE_C, N_importance=TRACE_F, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, randoms=rnd, **extra)
    mp = pytest.MonkeyPatch()
    prev = npa_mod.get_precision()
    out = {}
    try:
        mp.setattr(hb, "lib", lambda: Spy())
        # a fresh range monitor, as a new process has it: which form of the delta chain a backward launches follows the monitor's schedule
        mp.setattr(hb, "RANGE_MONITOR", hb.RangeMonitor())
        for row in TRACE_ROWS:
            prec, mode = row.split("/")
            npa_mod.set_precision(prec)
            hb.WORKSPACE.clear()
            del names[:]
            if mode == "no_grad":
                with torch.no_grad():
                    npa_mod.render_rays(rays, nc, None, **kw)
            else:
                ret = npa_mod.render_rays(rays, nc, None, **kw)
                (ret["rgb_map"].sum() + ret["rgb0"].sum()).backward()
                for m in (nc, nf):
                    for p in m.parameters():
                        p.grad = None
            torch.cuda.synchronize()
            out[row] = [n for n in names if is_launch(n)]
    finally:
        mp.undo()
        npa_mod.set_precision(prev)
        hb.WORKSPACE.clear()
    return out


def test_without_a_baked_field_the_library_calls_are_the_parents(npa, dev, nets):
    nc, nf, _, _ = nets
    off = record_trace(npa, dev, nc, nf, {})
    record = os.environ.get("NERF_RECORD_BAKED_OFF_TRACE")
    if record:
        with open(record, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in off.items()) + "\n}\n")
    with open(FIXTURE) as f:
        golden = json.load(f)
    none = record_trace(npa, dev, nc, nf, dict(baked=None))
    for row in TRACE_ROWS:
        assert len(off[row]) >= 1 and not any(n.startswith("nerf_baked") for n in off[row] + none[row]), row
        assert off[row] == golden[row], row
        assert none[row] == golden[row], row
