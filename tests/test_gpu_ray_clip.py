"""GPU tests (-m gpu) of clipping rays to the occupied span of an occupancy grid: the kernel nerf_occ_ray_span against the float64
definition OccupancyGrid.ray_span_reference on every ray, against the classifier on the device, and render_rays(clip_to_occupancy=True)
against clipping by hand -- bit for bit, in inference and in training."""
import numpy as np
import pytest
import torch

import nerf_oracle as orc
from test_gpu_occupancy import bits_equal
from test_gpu_occupancy_train import datapath_fp16x3, fresh_nets, grads_of, loss_of, positive_median_density, zero_grads  # noqa: F401  (fixture, helpers)
from test_gpu_parity import BOUNDARY_DATAPATHS, datapath, dev, nets, npa  # noqa: F401  (fixtures)
from test_ray_clip_cpu import (BOX_HI, BOX_LO, CLEAR, all_rays, ball_mask, check_span, make_grid, one_cell_mask,
                               two_balls_mask)

pytestmark = pytest.mark.gpu

# ball128: the share-0.25 ball of DESIGN.md section 3.9 at 128^3 -- 2 Mi cells, the bits spread over 64 Ki words
KERNEL_MASKS = {"ball": ball_mask, "two_balls": two_balls_mask, "ball128": lambda: ball_mask(128, 0.811), "one_cell_32x20x48": one_cell_mask}


# ------------------------------------------------------------------------------------------------ 1. the kernel against the definition
@pytest.mark.parametrize("outside", ["evaluate", "skip"])
@pytest.mark.parametrize("mask", sorted(KERNEL_MASKS))
def test_kernel_lies_between_the_two_hulls_on_every_ray(npa, dev, mask, outside):
    """1024 synthetic rays + 64 hand-made ones (axis-aligned, origin inside the box, pointing away, zero components, NaN / inf,
    near == far, near > far), no ray left out: check_span (tests/test_ray_clip_cpu.py) holds hit and both ends to the float64 hulls,
    near <= near' < far' <= far, a miss to the untouched row; a second launch gives the same bits.  The bounds are the issue's: the
    kernel's pad is 2^-10 cell, its fp32 end points err by at most 2^-11 cell (R <= 512), so an end lies within 2 pads of the hull
    of all occupied segments and never inside the hull of the segments longer than 2^-9 cell."""
    m = KERNEL_MASKS[mask]()
    grid, cpu_grid = make_grid(m, outside, dev), make_grid(m, outside)
    rays = all_rays()
    span, hit = grid.ray_span(rays.to(dev))
    assert span.is_cuda and hit.is_cuda and not span.requires_grad
    n_hit, n_differ = check_span(cpu_grid, rays, span.cpu(), hit.cpu())
    print(f"\n[{mask}, {outside}] {n_hit} of {rays.shape[0]} rays hit; the two hulls differ on {n_differ}")
    assert 0 < n_hit < rays.shape[0]
    span2, hit2 = grid.ray_span(rays.to(dev))
    assert bits_equal(span, span2) and torch.equal(hit, hit2)
    # the binding: int32 flags, a wider record stride reads the same eight columns, an empty batch launches nothing
    hb = npa.hip_backend
    wide = torch.cat([rays, torch.full((rays.shape[0], 3), 7.0)], -1).to(dev)
    s3, h3 = hb.occ_ray_span(grid._desc(), wide)
    assert h3.dtype == torch.int32 and bits_equal(s3, span) and torch.equal(h3.bool(), hit)
    s0, h0 = grid.ray_span(rays[:0].to(dev))
    assert s0.shape == (0, 2) and h0.shape == (0,)


def test_kernel_sizes_that_do_not_fill_a_wave(npa, dev):
    """ray counts around the 32 rays of a wave (two lanes per ray): every count gives the rows of the full launch, and nothing is
    written past the last ray"""
    grid = make_grid(ball_mask(), "skip", dev)
    rays = all_rays().to(dev)
    span, hit = grid.ray_span(rays)
    for n in (1, 2, 31, 32, 33, 63, 65, 1000):
        s, h = grid.ray_span(rays[:n])
        assert bits_equal(s, span[:n]) and torch.equal(h, hit[:n]), n


# ------------------------------------------------------------------------------------------------ 2. conservative against the classifier
@pytest.mark.parametrize("outside", ["evaluate", "skip"])
@pytest.mark.parametrize("mask", ["ball", "two_balls", "ball128"])
def test_span_keeps_every_sample_the_classifier_keeps(npa, dev, mask, outside):
    """The 64 coarse depths of the UNCLIPPED rays (hb.sample_coarse; stratified and perturbed), classified by occupied() on the device:
    every occupied depth whose float64 grid coordinate is at least 2^-8 cell from every cell plane lies in [near', far'] (a miss keeps
    [near, far]).  And the coarse depths of the clipped rays all lie in [near', far'], in disparity sampling within 8 * 2^-24 relative."""
    hb = npa.hip_backend
    grid = make_grid(KERNEL_MASKS[mask](), outside, dev)
    rays = all_rays().to(dev)
    span, hit = grid.ray_span(rays)
    clipped, hit2 = grid.clip_rays(rays)
    assert torch.equal(hit, hit2) and bits_equal(clipped[:, 6:8], span) and bits_equal(clipped[:, :6], rays[:, :6]) and bits_equal(clipped[:, 8:], rays[:, 8:])
    t_lin = torch.linspace(0.0, 1.0, 64, device=dev)
    t_rand = torch.rand(rays.shape[0], 64, generator=torch.Generator().manual_seed(9)).to(dev)
    counted_total = 0
    for lindisp, tr in ((False, None), (False, t_rand), (True, t_rand)):
        ok = rays[:, 6] <= rays[:, 7]       # (near > far: the depths run from near DOWN to far, no interval contains them)
        if lindisp:
            ok = ok & (rays[:, 6] > 0)      # (1 / near)
        z = hb.sample_coarse(rays, t_lin, lindisp, tr)
        occ = grid.occupied(rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None])
        r64, z64 = rays.double(), z.double()
        g = (r64[:, None, 0:3] + r64[:, None, 3:6] * z64[..., None] - torch.tensor(grid.lo.astype(np.float64), device=dev)) \
            * torch.tensor(grid.scale.astype(np.float64), device=dev)
        counted = occ & ((g - torch.round(g)).abs() >= CLEAR).all(-1) & ok[:, None]
        counted_total += int(counted.sum())
        kept = (z >= span[:, 0:1]) & (z <= span[:, 1:2])
        assert bool((kept | ~counted).all()), torch.nonzero((counted & ~kept).any(-1)).reshape(-1).tolist()
        # the depths of the CLIPPED rays.  Linear in depth they lie in [near', far'] exactly (near' (1 - t) + far' t is monotone under
        # rounding and gives the ends back at t = 0 and 1).  In disparity a depth is 1 / (1 / near' (1 - t) + 1 / far' t): seven
        # rounded operations (1 - t, two reciprocals, two products, a sum, a reciprocal), each within u = 2^-24 relative, and every
        # error passes to the result with a factor <= 1 -- 8 u covers them to first order and beyond.
        slack = 8 * 2.0 ** -24 if lindisp else 0.0
        zc = hb.sample_coarse(clipped, t_lin, lindisp, tr).double()
        inside = (zc >= span[:, 0:1].double() * (1 - slack)) & (zc <= span[:, 1:2].double() * (1 + slack))
        live = hit & ok
        assert bool((inside | ~live[:, None]).all()), (lindisp, torch.nonzero((~inside).any(-1) & live).reshape(-1).tolist())
    assert counted_total > 1000


# ------------------------------------------------------------------------------------------------ 3. the keyword == clipping by hand
def _scene(dev, n=512):
    rays = orc.synthetic_rays(n, seed=12).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, 64, 128, seed=5).items()}
    return rays, rnd


@pytest.mark.parametrize("datapath", BOUNDARY_DATAPATHS, indirect=True)
@pytest.mark.parametrize("perturb,noise,lindisp", [(0.0, 0.0, False), (1.0, 1.0, False), (1.0, 0.0, True)])
def test_keyword_equals_clipping_by_hand_bit_for_bit(npa, dev, nets, datapath, perturb, noise, lindisp):
    """render_rays(rays, occupancy=g, clip_to_occupancy=True) == render_rays(g.clip_rays(rays)[0], occupancy=g): every returned tensor,
    last_stats' evaluated / total, and rays_hit == hit.sum(); the clipped render evaluates more points than the unclipped one (all 64
    coarse samples land in the hull)."""
    nc, nf, _, _ = nets
    rays, rnd = _scene(dev)
    grid = make_grid(ball_mask(), "skip", dev)
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=perturb, raw_noise_std=noise, lindisp=lindisp,
              retraw=True, randoms=rnd)
    with torch.no_grad():
        by_hand_rays, hit = grid.clip_rays(rays)
        want = npa.render_rays(by_hand_rays, nc, None, occupancy=grid, **kw)
        want_stats = dict(grid.last_stats)
        got = npa.render_rays(rays, nc, None, occupancy=grid, clip_to_occupancy=True, **kw)
        got_stats = dict(grid.last_stats)
        plain = npa.render_rays(rays, nc, None, occupancy=grid, **kw)
        plain_stats = dict(grid.last_stats)
    assert list(got) == list(want) and set(got) == {"rgb_map", "disp_map", "acc_map", "raw", "rgb0", "disp0", "acc0", "z_std"}
    for k in want:
        assert bits_equal(got[k], want[k]), k
    assert set(want_stats) == {"evaluated", "total"} and set(plain_stats) == {"evaluated", "total"}
    assert got_stats == dict(want_stats, rays_hit=int(hit.sum()), rays=rays.shape[0])
    assert 0 < got_stats["rays_hit"] < rays.shape[0]
    assert got_stats["evaluated"] > plain_stats["evaluated"] and not bits_equal(got["rgb_map"], plain["rgb_map"])
    # coarse only
    with torch.no_grad():
        a = npa.render_rays(by_hand_rays, nc, None, occupancy=grid, **dict(kw, N_importance=0))
        b = npa.render_rays(rays, nc, None, occupancy=grid, clip_to_occupancy=True, **dict(kw, N_importance=0))
    assert list(a) == list(b) and all(bits_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("datapath", BOUNDARY_DATAPATHS, indirect=True)
def test_keyword_through_render_with_chunks_and_a_ragged_tail(npa, dev, nets, datapath):
    """render(c2w=..., chunk=150) of a 20 x 20 frame (chunks of 150, 150, 100 rays) with clip_to_occupancy=True in the keyword
    arguments: equal to batchify_rays over the hand-clipped records of the same frame, last_stats summed over the chunks with rays_hit
    == hit.sum(); render_path takes the keyword from render_kwargs."""
    nc, nf, _, _ = nets
    H, W, focal = 20, 20, 25.0
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    c2w = torch.tensor([[1.0, 0, 0, 0.1], [0, 1.0, 0, 0.2], [0, 0, 1.0, 4.0]]).to(dev)      # looks down -z at the ball: it fills part of the frame
    grid = make_grid(ball_mask(), "skip", dev)
    kw = dict(network_fn=nc, network_query_fn=None, N_samples=64, N_importance=128, network_fine=nf, perturb=0., white_bkgd=True, raw_noise_std=0., retraw=True)
    geo = dict(c2w=c2w, ndc=False, near=2., far=6., use_viewdirs=True)
    with torch.no_grad():
        records = npa.hip_backend.make_rays(H, W, K, c2w, None, False, 2., 6., dev)
        by_hand_rays, hit = grid.clip_rays(records)
        want = npa.batchify_rays(by_hand_rays, 150, occupancy=grid, **kw)
        want_stats = dict(grid.last_stats)
        got = npa.render(H, W, K, chunk=150, occupancy=grid, clip_to_occupancy=True, **geo, **kw)
        got_stats = dict(grid.last_stats)
    assert 0 < int(hit.sum()) < H * W
    assert got_stats == dict(want_stats, rays_hit=int(hit.sum()), rays=H * W) and want_stats["total"] == H * W * 256
    flat = dict(zip(("rgb_map", "disp_map", "acc_map"), got[:3]), **got[3])
    assert set(flat) == set(want)
    for k in want:
        assert bits_equal(flat[k].reshape(want[k].shape), want[k]), k
    rkw = dict(kw, ndc=False, near=2., far=6., use_viewdirs=True, occupancy=grid, clip_to_occupancy=True)
    rkw.pop("retraw")
    with torch.no_grad():
        rgbs, _ = npa.render_path(torch.stack([c2w]), (H, W, focal), K, 150, rkw)
    assert np.array_equal(rgbs[0], got[0].cpu().numpy())
    assert grid.last_stats == got_stats


# ------------------------------------------------------------------------------------------------ 4. training
def _ball_dgrid(npa, dev, **kw):
    g = npa.DensityGrid(BOX_LO, BOX_HI, 32, outside="skip", device=dev, **kw)
    g.bits = make_grid(ball_mask(), "skip", dev).bits.clone()
    return g


def test_training_gradients_equal_clipping_by_hand(npa, dev, nets, datapath_fp16x3):
    """a DensityGrid with the ball's bits, rays that require grad: parameter gradients of both networks and the ray gradients are
    bit-identical to the call on hand-clipped rays; the ray gradient's columns 6:8 are exactly 0"""
    n = 256
    rays0 = orc.synthetic_rays(n, seed=21).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, 64, 128, seed=22).items()}
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(77)).to(dev)
    kw = dict(N_samples=64, N_importance=128, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, randoms=rnd)
    grid = _ball_dgrid(npa, dev)
    nc, nf = fresh_nets(npa, dev, nets)
    res = []
    for by_hand in (True, False):
        zero_grads(nc, nf)
        rays = rays0.clone().requires_grad_(True)
        if by_hand:
            clipped, hit = grid.clip_rays(rays)
            assert clipped.requires_grad and 0 < int(hit.sum()) < n
            out = npa.render_rays(clipped, nc, None, network_fine=nf, occupancy=grid, **kw)
        else:
            out = npa.render_rays(rays, nc, None, network_fine=nf, occupancy=grid, clip_to_occupancy=True, **kw)
            assert grid.last_stats["rays_hit"] == int(hit.sum()) and grid.last_stats["rays"] == n
        loss_of(npa, out, target).backward()
        res.append((out, grads_of(nc), grads_of(nf), rays.grad.clone()))
    (o1, c1, f1, r1), (o2, c2, f2, r2) = res
    for k in o1:
        assert bits_equal(o1[k], o2[k]), k
    for a, b in zip(c1 + f1, c2 + f2):
        assert a is not None and bits_equal(a, b)
    assert bits_equal(r1, r2) and bool((r1[:, 6:8] == 0).all()) and float(r1[:, :6].abs().max()) > 0


def test_ten_optimizer_steps_stay_bit_identical(npa, dev, nets, datapath_fp16x3):
    """two copies of the networks and of a DensityGrid that starts from the ball's bits, FlatAdam and maybe_update (every 4 steps
    from step 4 on) on both sides; one side passes clip_to_occupancy=True, the other clips by hand: parameters, density and bits are
    bit-identical after ten steps"""
    n = 128
    thr = positive_median_density(npa, nets[1], dev, 32)
    sides = []
    for _ in range(2):
        nc, nf = fresh_nets(npa, dev, nets)
        sides.append(dict(nc=nc, nf=nf, opt=npa.FlatAdam(list(nc.parameters()) + list(nf.parameters()), lr=1e-5),
                          grid=_ball_dgrid(npa, dev, warmup_steps=4, update_every=4, sigma_threshold=thr),
                          gen=torch.Generator().manual_seed(31), updates=0, hits=[]))
    for step in range(10):
        rays = orc.synthetic_rays(n, seed=100 + step).to(dev)
        rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, 64, 128, seed=200 + step).items()}
        target = torch.rand(n, 3, generator=torch.Generator().manual_seed(300 + step)).to(dev)
        kw = dict(N_samples=64, N_importance=128, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, randoms=rnd)
        for i, s in enumerate(sides):
            s["updates"] += bool(s["grid"].maybe_update(s["nf"], step, fraction=0.5, samples_per_cell=2, generator=s["gen"]))
            if i == 0:
                out = npa.render_rays(rays, s["nc"], None, network_fine=s["nf"], occupancy=s["grid"], clip_to_occupancy=True, **kw)
                s["hits"].append(s["grid"].last_stats["rays_hit"])
            else:
                clipped, hit = s["grid"].clip_rays(rays)
                s["hits"].append(int(hit.sum()))
                out = npa.render_rays(clipped, s["nc"], None, network_fine=s["nf"], occupancy=s["grid"], **kw)
            s["opt"].zero_grad()
            loss_of(npa, out, target).backward()
            s["opt"].step()
    a, b = sides
    assert a["updates"] == b["updates"] == 2 and a["hits"] == b["hits"] and 0 < a["hits"][0] < n
    assert torch.equal(a["grid"].bits, b["grid"].bits) and bits_equal(a["grid"].density, b["grid"].density)
    for net in ("nc", "nf"):
        assert bits_equal(a[net].flat_params(), b[net].flat_params()), net
        assert not bits_equal(a[net].flat_params(), nets[0 if net == "nc" else 1].flat_params())     # (they did train)


# ------------------------------------------------------------------------------------------------ 5. off means off
@pytest.mark.parametrize("datapath", BOUNDARY_DATAPATHS, indirect=True)
def test_false_is_the_call_without_the_keyword(npa, dev, nets, datapath, monkeypatch):
    nc, nf, _, _ = nets
    rays, rnd = _scene(dev, 256)
    grid = make_grid(ball_mask(), "skip", dev)
    kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd)
    calls = []
    real = npa.hip_backend.occ_ray_span
    monkeypatch.setattr(npa.hip_backend, "occ_ray_span", lambda *a: calls.append(1) or real(*a))
    with torch.no_grad():
        a = npa.render_rays(rays, nc, None, occupancy=grid, **kw)
        a_stats = dict(grid.last_stats)
        b = npa.render_rays(rays, nc, None, occupancy=grid, clip_to_occupancy=False, **kw)
        b_stats = dict(grid.last_stats)
        c = npa.batchify_rays(rays, 100, network_fn=nc, network_query_fn=None, occupancy=grid, clip_to_occupancy=False, **kw)
        c_stats = dict(grid.last_stats)
        d = npa.render_rays(rays, nc, None, clip_to_occupancy=False, **kw)         # no grid, the keyword off
        e = npa.render_rays(rays, nc, None, **kw)
    assert not calls
    assert list(a) == list(b) and all(bits_equal(a[k], b[k]) for k in a) and all(bits_equal(a[k], c[k]) for k in a)
    assert a_stats == b_stats == c_stats and set(a_stats) == {"evaluated", "total"}
    assert all(bits_equal(d[k], e[k]) for k in e)
    with torch.no_grad():
        with pytest.raises(ValueError, match="clip_to_occupancy"):
            npa.render_rays(rays, nc, None, clip_to_occupancy=True, **kw)
        e0 = npa.render_rays(rays[:0], nc, None, occupancy=grid, clip_to_occupancy=True, **kw)
    assert e0["rgb_map"].shape == (0, 3) and grid.last_stats == {"evaluated": 0, "total": 0, "rays_hit": 0, "rays": 0}
    assert calls == []


def test_a_refused_call_launches_no_span_kernel(npa, dev, nets, monkeypatch):
    """the guards of the grid path (a user network_query_fn; a plain OccupancyGrid with a needed gradient) come before the clipping"""
    nc, nf, _, _ = nets
    rays = orc.synthetic_rays(64, seed=3).to(dev)
    grid = make_grid(ball_mask(), "skip", dev)
    calls = []
    real = npa.hip_backend.occ_ray_span
    monkeypatch.setattr(npa.hip_backend, "occ_ray_span", lambda *a: calls.append(1) or real(*a))
    kw = dict(N_samples=16, N_importance=16, network_fine=nf, occupancy=grid, clip_to_occupancy=True)
    with pytest.raises(NotImplementedError, match="gradient"):
        npa.render_rays(rays, nc, None, **kw)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="network_query_fn"):
            npa.render_rays(rays, nc, lambda p, v, m: npa.run_network(p, v, m, None, None), **kw)
        assert not calls
        npa.render_rays(rays, nc, None, **kw)
    assert calls == [1]
