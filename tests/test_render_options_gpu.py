"""GPU (-m gpu): the dict render_rays returns, pinned in one place for every path -- the fused node with and without a needed gradient,
a user network_query_fn, general (DenseNeRF) networks, an occupancy grid without and with gradients, proposal="grid", the march, a
baked field -- crossed with retraw, distortion and interlevel where the path accepts them: the keys IN ORDER (batchify_rays and
render() iterate the dict, the reference's train() asks `'rgb0' in extras`), the trailing shape of every value and the keys of the
grid's last_stats, for 64 rays, for the empty batch and through batchify_rays in two chunks.  64 rays, 8 (+ 8) samples, 8^3 grids:
the smallest call that still takes every branch."""
import itertools

import pytest
import torch

import nerf_oracle as orc
from test_baked_cpu import constant_field
from test_gpu_parity import dev, nets, npa  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

N_RAYS, N_C = 64, 8
LO, HI = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)

# the orders in which the paths list their keys, every optional key present ("raw": retraw, "distortion" / "interlevel": the options)
FUSED = ["rgb_map", "disp_map", "acc_map", "raw", "rgb0", "disp0", "acc0", "z_std", "distortion", "interlevel"]
STAGED = ["rgb0", "disp0", "acc0", "z_std", "rgb_map", "disp_map", "acc_map", "raw", "distortion", "interlevel"]
ONE_PASS = ["rgb_map", "disp_map", "acc_map", "raw", "distortion"]
PROPOSAL = ["z_std", "rgb_map", "disp_map", "acc_map", "raw", "distortion"]
PROPOSAL_EMPTY = ["rgb_map", "disp_map", "acc_map", "raw", "z_std", "distortion"]
BAKED = ["rgb_map", "disp_map", "acc_map", "depth_map"]
BASE = ["evaluated", "total"]

MARCH = dict(proposal="march", march_steps=32)
FIT = dict(MARCH, march_stop_eps=0.01, march_step_size=0.25, march_fit=2, clip_to_occupancy=True)

# id: (path, N_importance, keywords, keys with rays, keys without rays, last_stats keys with rays, last_stats keys of the empty batch and of
# batchify_rays).  path: networks / grad mode / query function / grid of the call (call_of)
CASES = {
    "fused-grad": ("grad", 8, {}, FUSED, FUSED, None, None),
    "fused-grad-coarse-only": ("grad", 0, {}, ONE_PASS, ONE_PASS, None, None),
    "fused-no-grad": ("no_grad", 8, {}, FUSED, FUSED, None, None),
    "fused-no-grad-coarse-only": ("no_grad", 0, {}, ONE_PASS, ONE_PASS, None, None),
    "hook": ("hook", 8, {}, STAGED, FUSED, None, None),
    "hook-coarse-only": ("hook", 0, {}, ONE_PASS, ONE_PASS, None, None),
    "dense": ("dense", 8, {}, STAGED, STAGED, None, None),
    "dense-coarse-only": ("dense", 0, {}, ONE_PASS, ONE_PASS, None, None),
    "grid-no-grad": ("plain", 8, {}, STAGED, FUSED, BASE, BASE),
    "grid-no-grad-coarse-only": ("plain", 0, {}, ONE_PASS, ONE_PASS, BASE, BASE),
    "grid-no-grad-clip-stop": ("plain", 8, dict(clip_to_occupancy=True, early_stop_eps=0.01), STAGED, FUSED,
                               BASE + ["rays_stopped", "rays_hit", "rays"], BASE + ["rays_hit", "rays", "rays_stopped"]),
    "grid-grad": ("density", 8, {}, STAGED, FUSED, BASE, BASE),
    "grid-grad-coarse-only": ("density", 0, {}, ONE_PASS, ONE_PASS, BASE, BASE),
    "grid-grad-clip-stop": ("density", 8, dict(clip_to_occupancy=True, early_stop_eps=0.01), STAGED, FUSED,
                            BASE + ["rays_stopped", "rays_hit", "rays"], BASE + ["rays_hit", "rays", "rays_stopped"]),
    "proposal-grid-no-grad": ("density_no_grad", 8, dict(proposal="grid"), PROPOSAL, PROPOSAL_EMPTY, BASE, BASE),
    "proposal-grid-grad": ("density", 8, dict(proposal="grid", early_stop_eps=0.01), PROPOSAL, PROPOSAL_EMPTY,
                           BASE + ["rays_stopped"], BASE + ["rays_stopped"]),
    "march-no-grad": ("plain", 8, MARCH, ONE_PASS, ONE_PASS, BASE + ["rays_truncated"], BASE + ["rays_truncated"]),
    "march-grad": ("density", 8, MARCH, ONE_PASS, ONE_PASS, BASE + ["rays_truncated"], BASE + ["rays_truncated"]),
    "march-grad-no-importance": ("density", 0, dict(MARCH, march_stop_eps=0.01), ONE_PASS, ONE_PASS,
                                 BASE + ["rays_stopped", "rays_truncated"], BASE + ["rays_truncated", "rays_stopped"]),
    "march-fit-no-grad": ("density_no_grad", 8, FIT, ONE_PASS, ONE_PASS, BASE + ["rays_stopped", "rays_truncated", "rays_refit", "rays_hit", "rays"],
                          BASE + ["rays_hit", "rays", "rays_truncated", "rays_stopped", "rays_refit"]),
    "march-fit-grad": ("density", 8, FIT, ONE_PASS, ONE_PASS, BASE + ["rays_stopped", "rays_truncated", "rays_refit", "rays_hit", "rays"],
                       BASE + ["rays_hit", "rays", "rays_truncated", "rays_stopped", "rays_refit"]),
    "baked": ("baked", 8, {}, BAKED, BAKED, None, None),
}


@pytest.fixture(scope="module")
def world(npa, dev, nets):
    dense_kw = dict(D=4, W=64, input_ch=63, output_ch=4, skips=[2], input_ch_views=27, use_viewdirs=True)
    torch.manual_seed(3)
    dense = (npa.NeRF(**dense_kw).to(dev), npa.NeRF(**dense_kw).to(dev))
    assert isinstance(dense[0], npa.dense.DenseNeRF)
    return dict(fused=nets[:2], dense=dense, rays=orc.synthetic_rays(N_RAYS, seed=11).to(dev),
                plain=npa.OccupancyGrid(LO, HI, 8, device=dev), density=npa.DensityGrid(LO, HI, 8, device=dev),
                baked=constant_field(1.0, (0.5, 0.5, 0.5)).to(dev),
                hook=lambda pts, viewdirs, net: npa.run_network(pts, viewdirs, net, None, None))


def call_of(world, path, n_f, kw):
    """(positional arguments behind the rays, keywords, grad mode, the grid whose last_stats the call writes) of a case"""
    net, fine = world["dense" if path == "dense" else "fused"]
    kw = dict(N_samples=N_C, N_importance=n_f, network_fine=fine, **kw)
    grid = None
    if path in ("plain", "density", "density_no_grad"):
        grid = kw["occupancy"] = world["density" if path == "density_no_grad" else path]
    if path == "baked":
        kw["baked"] = world["baked"]
    return (net, world["hook"] if path == "hook" else None), kw, path in ("grad", "hook", "dense", "density"), grid


def combos_of(path, n_f, kw):
    """(retraw, distortion, interlevel) the case accepts: interlevel needs two network passes, a baked field none of the three"""
    if path == "baked":
        return [(False, False, False)]
    inter = (False, True) if n_f > 0 and "proposal" not in kw else (False,)
    return list(itertools.product((False, True), (False, True), inter))


def check(out, full, retraw, distortion, interlevel, n, slots):
    dropped = {k for k, on in (("raw", retraw), ("distortion", distortion), ("interlevel", interlevel)) if not on}
    assert list(out) == [k for k in full if k not in dropped]
    tails = {"rgb_map": (3,), "rgb0": (3,), "raw": (slots, 4)}
    for k, v in out.items():
        assert tuple(v.shape) == (n,) + tails.get(k, ()) and v.dtype == torch.float32, k


@pytest.mark.parametrize("case", CASES)
def test_keys_shapes_and_stats_with_rays(npa, world, case):
    path, n_f, kw, full, _, stats, _ = CASES[case]
    args, kwargs, grad, grid = call_of(world, path, n_f, kw)
    for retraw, distortion, interlevel in combos_of(path, n_f, kw):
        opts = {} if path == "baked" else dict(retraw=retraw, distortion=distortion, interlevel=interlevel)
        if grid is not None:
            grid.last_stats = None
        with torch.set_grad_enabled(grad):
            out = npa.render_rays(world["rays"], *args, **kwargs, **opts)
        check(out, full, retraw, distortion, interlevel, N_RAYS, N_C + n_f)
        if grid is not None:
            assert list(grid.last_stats) == stats and grid.last_stats["total"] > 0


@pytest.mark.parametrize("case", CASES)
def test_keys_shapes_and_stats_of_the_empty_batch(npa, world, case):
    path, n_f, kw, _, full, _, stats = CASES[case]
    args, kwargs, grad, grid = call_of(world, path, n_f, kw)
    for retraw, distortion, interlevel in combos_of(path, n_f, kw):
        opts = {} if path == "baked" else dict(retraw=retraw, distortion=distortion, interlevel=interlevel)
        if grid is not None:
            grid.last_stats = None
        with torch.set_grad_enabled(grad):
            out = npa.render_rays(world["rays"][:0], *args, **kwargs, **opts)
        check(out, full, retraw, distortion, interlevel, 0, N_C + n_f)
        if grid is not None:
            assert list(grid.last_stats) == stats and set(grid.last_stats.values()) == {0}


@pytest.mark.parametrize("case", CASES)
def test_batchify_rays_in_two_chunks_has_the_keys_and_the_summed_stats(npa, world, case):
    path, n_f, kw, full, _, _, stats = CASES[case]
    (net, query), kwargs, grad, grid = call_of(world, path, n_f, kw)
    opts = {} if path == "baked" else dict(retraw=True, distortion=True, interlevel=n_f > 0 and "proposal" not in kw)
    owner = world["baked"] if path == "baked" else grid
    with torch.set_grad_enabled(grad):
        want = []
        for half in (world["rays"][:32], world["rays"][32:]):
            npa.render_rays(half, net, query, **kwargs, **opts)
            want.append(None if owner is None else dict(owner.last_stats))
        out = npa.batchify_rays(world["rays"], 32, network_fn=net, network_query_fn=query, **kwargs, **opts)
    check(out, full, True, True, opts.get("interlevel", False), N_RAYS, N_C + n_f)
    if owner is not None:
        assert owner.last_stats == {k: want[0][k] + want[1][k] for k in want[0]}
        if grid is not None:
            assert list(grid.last_stats) == stats
