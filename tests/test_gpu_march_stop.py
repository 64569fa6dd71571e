"""GPU tests (-m gpu) of render_rays(proposal="march", march_stop_eps=eps): nerf_occ_march_stop alone against its definition
(DensityGrid.march_stop_reference, evaluated on the CPU) as raw bits, then the render -- forward and backward -- against THE CHAIN of
tests/test_gpu_march.py with the stopping march in front: march_stop_reference -> pts = o + d z -> the compacting hook with the extra
predicate z < z_stop -> npa.raw2outputs.  Every comparison is bit for bit."""
import numpy as np
import pytest
import torch

from test_gpu_march import INVALID, M_STEPS, N_KERNEL, N_SLOTS, NOISE_SEED, kernel_scene, scene, stopping_hook
from test_gpu_occupancy import bits_equal
from test_gpu_occupancy_train import ball_dgrid, datapath_fp16x3, flat_of, grads_of, zero_grads  # noqa: F401
from test_gpu_parity import datapath, dev, maxdiff, nets, npa  # noqa: F401  (fixtures)
from test_gpu_ray_grad import rel_l2
from test_march_stop_cpu import DENSITIES, EPS, RAYS, ball_density_grid, hand_dgrid, stop_rays

pytestmark = pytest.mark.gpu

INF = float("inf")
STOP_EPS = 1e-2
KERNEL_DENSITY_SCALE = 20.0     # chosen on the CPU, with the thin slab: see kernel_dgrid


def on_cpu(grid):
    """a copy of a DensityGrid on the CPU: the definition is evaluated there (its one division is IEEE whatever the device's torch does)"""
    g = type(grid)(grid.lo, grid.hi, grid.resolution, outside=grid.outside, device="cpu", sigma_threshold=grid.sigma_threshold)
    g.bits, g.density = grid.bits.cpu().clone(), grid.density.cpu().clone()
    return g


def reference_on_cpu(grid, rays, u, M, S, eps):
    out = on_cpu(grid).march_stop_reference(rays.detach().cpu(), None if u is None else u.cpu(), M, S, eps)
    return tuple(t.to(rays.device) for t in out)


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
N_EXTRA = 160
N_ALL = N_KERNEL + N_EXTRA


def extra_rays(n=N_EXTRA, seed=11):
    """rays that start inside kernel_scene's box in its cleared half, point towards +z with a small tilt and END inside the box, in
    the occupied half: they never leave the box (under outside="evaluate" a ray that does is truncated by the space outside) and cross
    from nothing to about half of the occupied half, so they fit, are truncated or stop depending on what they cross"""
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor((-1.25, 0.5, -3.0)), torch.tensor((1.75, 2.0, 0.2))
    o = lo + (hi - lo) * (torch.tensor([0.1, 0.1, 0.05]) + torch.tensor([0.8, 0.8, 0.4]) * torch.rand(n, 3, generator=g))
    d = torch.cat([0.15 * torch.randn(n, 2, generator=g), 0.6 + 0.8 * torch.rand(n, 1, generator=g)], -1)
    near = 0.2 * torch.rand(n, 1, generator=g)
    z_end = -1.4 + 1.5 * torch.rand(n, 1, generator=g)
    far = torch.maximum((z_end - o[:, 2:3]) / d[:, 2:3], near + 0.3)
    rays = torch.cat([o, d, near, far, torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)], -1)
    return rays, torch.rand(n, generator=g)


def kernel_dgrid(npa, dev, outside, scale=KERNEL_DENSITY_SCALE):
    """tests/test_gpu_march.kernel_scene -- its grid as a DensityGrid with the same bits, its 301 rays -- and N_EXTRA more rays.
    Density per cell: scale * (0.25 + 1.5 * rand), times 0.05 in the slab ix < 12 (a thin region: rays there fit or are truncated
    rather than stop).

    THE CASE MIX.  At (M, S) = (256, 64) every run -- one `outside`, one eps, u random or None -- must put at least 16 DISTINCT rays
    into each of stopped, truncated and fit, by the definition alone; the test asserts that per run.  The 301 rays alone cannot do
    it, whatever the densities: a stop turns a fitting or a truncated ray into a stopped one and never makes a ray fit, and without
    any stop only 12 of them fit under outside="evaluate" (a ray that leaves the box is truncated by the space outside), while under
    "skip" 247 of the 293 valid ones miss the mask and 46 rays cannot fill three classes of 16.  Hence the added rays, which are
    compared bit for bit like the others.  Scale and slab were chosen on the CPU (scales 15 / 20 / 30 with the slab, 13-17 without):
    at 20 the smallest class of any run holds 29 rays (skip, eps 1e-1: 108 stopped / 29 truncated / 60 fit; evaluate, eps 1e-3:
    39 / 251 / 91)."""
    plain, rays, u = kernel_scene(npa, dev, outside)
    more, more_u = extra_rays()
    rays, u = torch.cat([rays, more], 0), torch.cat([u, more_u], 0)
    g = npa.DensityGrid(plain.lo, plain.hi, plain.resolution, outside=outside, device=dev)
    g.bits = plain.bits.clone()
    rand = torch.rand(plain.resolution, generator=torch.Generator().manual_seed(7))
    thin = torch.ones(plain.resolution)
    thin[:12] = 0.05
    g.density = (scale * (0.25 + 1.5 * rand) * thin).to(torch.float32).reshape(-1).contiguous().to(dev)
    return g, plain, rays, u


@pytest.mark.parametrize("outside", ["evaluate", "skip"])
@pytest.mark.parametrize("M,S", [(1, 1), (7, 2), (64, 5), (65, 64), (256, 64), (1024, 192)])
def test_kernel_equals_the_definition_bit_for_bit(npa, dev, outside, M, S):
    """z_vals and z_stop equal march_stop_reference's as raw bits, truncated and stopped are equal: the 301 rays of kernel_scene, the
    invalid ones included, and the 160 of extra_rays; eps 1e-1 and 1e-3; u random and None; ray records of 8 and of 11 columns; the same bits on a second launch"""
    hb = npa.hip_backend
    grid, _, rays, u = kernel_dgrid(npa, dev, outside)
    cpu = on_cpu(grid)
    invalid = torch.tensor(sorted(INVALID.values()))
    valid = torch.ones(N_ALL, dtype=torch.bool)
    valid[invalid] = False
    out_sigma = grid.sigma_threshold if outside == "evaluate" else 0.0
    for eps in (1e-1, 1e-3):
        for uu in (u, None):
            want = cpu.march_stop_reference(rays, uu, M, S, eps)
            for cols in (11, 8):
                r = rays[:, :cols].contiguous().to(dev)
                z, z_stop, tr, st = hb.occ_march_stop(grid._desc(), grid.density, out_sigma, r, None if uu is None else uu.to(dev), M, S, eps)
                torch.cuda.synchronize()
                assert z.shape == (N_ALL, S) and z.dtype == torch.float32 and z_stop.shape == tr.shape == st.shape == (N_ALL,)
                assert tr.dtype == st.dtype == torch.int32
                assert bits_equal(z.cpu(), want[0]), int((z.cpu() != want[0]).sum())
                assert bits_equal(z_stop.cpu(), want[1]) and torch.equal(tr.cpu().bool(), want[2]) and torch.equal(st.cpu().bool(), want[3])
            again = grid.march_stop(rays.to(dev), M, S, eps, u=None if uu is None else uu.to(dev))
            assert bits_equal(again[0], z) and bits_equal(again[1], z_stop) and torch.equal(again[2], tr.bool()) and torch.equal(again[3], st.bool())
            assert again[2].dtype == again[3].dtype == torch.bool
            # the invalid rays: their own far in every slot, -inf, neither flag
            assert bits_equal(z.cpu()[invalid], rays[invalid, 7:8].expand(-1, S).contiguous())
            assert bool((z_stop.cpu()[invalid] == -INF).all()) and not bool(tr.cpu()[invalid].any()) and not bool(st.cpu()[invalid].any())
            assert bool((z.cpu()[valid][:, 1:] >= z.cpu()[valid][:, :-1]).all())
            miss = valid & ~want[2] & ~want[3] & (want[0][:, 0] == rays[:, 7])
            seen = {"stopped": int(want[3].sum()), "truncated": int(want[2].sum()), "fit": int((valid & ~want[2] & ~want[3] & ~miss).sum())}
            if (M, S) == (256, 64):     # the cases are there, in THIS run, as distinct rays
                assert min(seen.values()) >= 16, (eps, uu is None, seen)
            if S == 1:                  # something is always emitted in front of a cut: with one slot nothing stops
                assert seen["stopped"] == 0 and seen["truncated"] > 0


@pytest.mark.parametrize("outside", ["evaluate", "skip"])
def test_zero_density_gives_the_plain_march_bit_for_bit(npa, dev, outside):
    hb = npa.hip_backend
    grid, plain, rays, u = kernel_dgrid(npa, dev, outside, scale=0.0)
    assert not bool(grid.density.any())
    r = rays.to(dev)
    for M, S in ((7, 2), (65, 64), (256, 64)):
        for uu in (u.to(dev), None):
            want = hb.occ_march(plain._desc(), r, uu, M, S)
            got = hb.occ_march_stop(grid._desc(), grid.density, grid.sigma_threshold if outside == "evaluate" else 0.0, r, uu, M, S, 1e-3)
            assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1]) and torch.equal(got[2], want[2]) and not bool(got[3].any())
            assert int(want[2].sum()) > 0


@pytest.mark.parametrize("outside", ["evaluate", "skip"])
@pytest.mark.parametrize("densities", sorted(DENSITIES))
def test_kernel_on_the_hand_made_scene(npa, dev, outside, densities):
    """the hand-made cases of tests/test_march_stop_cpu.py on the device: a stop inside a run, the cut at a closing candidate in lane 0 of
    the second round (M = 65), cut and truncation in one round either way round (S = 4 and 3), A reaching tau only behind the last
    candidate (the lanes k >= M must not cut), densities of 0, below 0, NaN and inf, the d = 0 ray, S = 1"""
    cpu = hand_dgrid(outside, densities)
    grid = hand_dgrid(outside, densities).to(dev)
    rays = stop_rays()
    g = torch.Generator().manual_seed(3)
    stops = 0
    for M, S in ((16, 20), (16, 12), (16, 4), (16, 3), (16, 1), (7, 4), (1, 1), (1, 2), (65, 64), (65, 30), (130, 64)):
        for uu in (None, torch.rand(len(RAYS), generator=g)):
            want = cpu.march_stop_reference(rays, uu, M, S, EPS)
            got = grid.march_stop(rays.to(dev), M, S, EPS, u=None if uu is None else uu.to(dev))
            assert bits_equal(got[0].cpu(), want[0]), (M, S, got[0].cpu(), want[0])
            assert bits_equal(got[1].cpu(), want[1]) and torch.equal(got[2].cpu(), want[2]) and torch.equal(got[3].cpu(), want[3]), (M, S)
            stops += int(want[3].sum())
    assert (stops > 0) == (densities != "zero")


# ------------------------------------------------------------------------------------------------ 2. the render against the chain
def stop_grid(npa, dev, outside="evaluate", scale=4.0):
    """the ball of the render tests as a DensityGrid with density = scale * (0.25 + 1.5 * rand) inside it (tests/test_march_stop_cpu.py)"""
    return ball_density_grid(outside, scale=scale, device=dev)


def chain(npa, grid, rays, u, net, noise, eps=STOP_EPS, M=M_STEPS, S=N_SLOTS, white=True, seen=None):
    """THE YARDSTICK: render_rays(proposal="march", march_stop_eps=eps) from public pieces (tests/test_gpu_march.chain with the stopping
    march in front)"""
    z, z_stop, tr, st = reference_on_cpu(grid, rays, u, M, S, eps)
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]
    raw = stopping_hook(npa, grid, z, z_stop, seen)(pts, rays[:, 8:11], net)
    if noise > 0:
        torch.manual_seed(NOISE_SEED)
    rgb, disp, acc, _, _ = npa.raw2outputs(raw, z, rays[:, 3:6], noise, white)
    return dict(rgb_map=rgb, disp_map=disp, acc_map=acc, raw=raw), z, z_stop, tr, st


@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
@pytest.mark.parametrize("perturb,noise", [(1.0, 1.0), (0.0, 0.0)])
@pytest.mark.parametrize("outside", ["evaluate", "skip"])
def test_no_grad_render_equals_the_chain_bit_for_bit(npa, dev, nets, datapath, perturb, noise, outside):
    """256 rays, M = 256, S = 64: rgb_map, disp_map, acc_map and raw equal the chain's bit for bit; the keys are the march's; N_samples =
    64, N_importance = 0 gives the bits of 16 + 48; last_stats counts what the hook evaluated and the rays the definition truncates and
    stops; fewer points are evaluated and fewer rays truncated than without the option"""
    nc, nf, _, _ = nets
    rays, rnd, _ = scene(dev)
    n = rays.shape[0]
    grid = stop_grid(npa, dev, outside)
    kw = dict(network_fine=nf, white_bkgd=True, perturb=perturb, raw_noise_std=noise, retraw=True, occupancy=grid, proposal="march",
              march_steps=M_STEPS, randoms=rnd)
    seen = []
    with torch.no_grad():
        want, z, z_stop, tr, st = chain(npa, grid, rays, rnd["u_march"] if perturb > 0 else None, nf, noise, seen=seen)
        got = npa.render_rays(rays, nc, None, N_samples=16, N_importance=48, march_stop_eps=STOP_EPS, **kw)
        stats = dict(grid.last_stats)
        again = npa.render_rays(rays, nc, None, N_samples=64, N_importance=0, march_stop_eps=STOP_EPS, **kw)
        assert grid.last_stats == stats
        npa.render_rays(rays, nc, None, N_samples=16, N_importance=48, **kw)
        off = dict(grid.last_stats)
    assert list(got) == list(again) == ["rgb_map", "disp_map", "acc_map", "raw"]
    for k in got:
        assert bits_equal(got[k], want[k]), (k, maxdiff(got[k], want[k]))
        assert bits_equal(got[k], again[k]), k
    assert stats == {"evaluated": seen[0][0], "total": n * N_SLOTS, "rays_truncated": int(tr.sum()), "rays_stopped": int(st.sum())}
    assert stats["rays_stopped"] >= 16 and stats["rays_truncated"] >= 16
    assert set(off) == {"evaluated", "total", "rays_truncated"}
    assert stats["rays_truncated"] < off["rays_truncated"] and 0 < stats["evaluated"] < off["evaluated"]
    assert float(got["acc_map"].max()) > 0.5
    # what is not evaluated is exactly zero: everything at or behind the stop depth
    assert bool((got["raw"][z >= z_stop[:, None]] == 0).all())


# ------------------------------------------------------------------------------------------------ 3. gradients
@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
def test_forward_with_grad_equals_the_no_grad_render(npa, dev, nets, datapath):
    nc, nf, _, _ = nets
    rays, rnd, _ = scene(dev)
    grid = stop_grid(npa, dev)
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd,
              occupancy=grid, proposal="march", march_steps=M_STEPS, march_stop_eps=STOP_EPS)
    with torch.no_grad():
        want = npa.render_rays(rays, nc, None, **kw)
    stats = dict(grid.last_stats)
    grid.last_stats = None
    got = npa.render_rays(rays, nc, None, **kw)
    assert list(got) == list(want) == ["rgb_map", "disp_map", "acc_map", "raw"]
    for k in want:
        assert bits_equal(got[k], want[k]), (k, maxdiff(got[k], want[k]))
    assert grid.last_stats == stats and stats["rays_stopped"] >= 16 and 0 < stats["rays_truncated"] < rays.shape[0]
    assert got["rgb_map"].grad_fn is not None and got["raw"].grad_fn is not None
    del got          # (a graph dropped without backward)


@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
def test_parameter_gradients_equal_the_chains_bit_for_bit(npa, dev, nets, datapath):
    """loss = img2mse(rgb_map, t): .grad of every parameter of the evaluated network equals autograd's through the chain, bit for bit;
    the other network's .grad stays None"""
    nc, nf, _, _ = nets
    rays, rnd, target = scene(dev)
    grid = stop_grid(npa, dev)
    kw = dict(N_samples=16, N_importance=48, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, randoms=rnd, occupancy=grid, proposal="march",
              march_steps=M_STEPS, march_stop_eps=STOP_EPS)
    zero_grads(nc, nf)
    out = npa.render_rays(rays, nc, None, network_fine=nf, **kw)
    assert grid.last_stats["rays_stopped"] >= 16
    loss_g = npa.img2mse(out["rgb_map"], target)
    loss_g.backward()
    assert all(p.grad is None for p in nc.parameters())
    got = grads_of(nf)
    zero_grads(nc, nf)
    loss_h = npa.img2mse(chain(npa, grid, rays, rnd["u_march"], nf, 1.0)[0]["rgb_map"], target)
    loss_h.backward()
    want = grads_of(nf)
    zero_grads(nc, nf)
    assert bits_equal(loss_g.detach(), loss_h.detach())
    assert all(x is not None for x in got) and float(flat_of(got).abs().max()) > 0
    for i, (x, y) in enumerate(zip(got, want)):
        assert bits_equal(x, y), (i, maxdiff(x, y), rel_l2(flat_of(got), flat_of(want)))


def test_an_upstream_gradient_on_a_stopped_slot_reaches_no_parameter(npa, dev, nets, datapath_fp16x3, monkeypatch):
    """loss = sum(raw * G) through retraw: the network's gradient with a random G equals, bit for bit, the one with G zeroed on the slots
    the pass did not evaluate -- among them the slots of the stopped rays that the march without the option evaluates, which did carry
    a nonzero G"""
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    rays, rnd, _ = scene(dev)
    n = rays.shape[0]
    grid = stop_grid(npa, dev)
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, randoms=rnd, retraw=True, occupancy=grid,
              proposal="march", march_steps=M_STEPS)
    slots = []
    real = hb.occ_compact
    monkeypatch.setattr(hb, "occ_compact", lambda *a, **k: (lambda r: (slots.append(r[0].clone()), r)[1])(real(*a, **k)))
    with torch.no_grad():
        npa.render_rays(rays, nc, None, **kw)
    live_off = (slots.pop() >= 0).view(n, N_SLOTS)
    z, z_stop, tr, st = reference_on_cpu(grid, rays, rnd["u_march"], M_STEPS, N_SLOTS, STOP_EPS)
    G = torch.randn(n, N_SLOTS, 4, generator=torch.Generator().manual_seed(5)).to(dev)
    grads = []
    for mask_it in (False, True):
        zero_grads(nc, nf)
        del slots[:]
        raw = npa.render_rays(rays, nc, None, march_stop_eps=STOP_EPS, **kw)["raw"]
        assert len(slots) == 1
        live = (slots[0] >= 0).view(n, N_SLOTS)
        (raw * (G * live[..., None] if mask_it else G)).sum().backward()
        grads.append(flat_of(grads_of(nf)))
        assert all(p.grad is None for p in nc.parameters())
    zero_grads(nc, nf)
    # on a stopped ray the rows agree in front of the stop: the slots the option took away are the ones live without it and dead with it
    taken = live_off & ~live & st[:, None]
    assert int(st.sum()) >= 16 and int(taken.sum()) > 0 and not bool((live & (z >= z_stop[:, None])).any())
    assert float((G * taken[..., None]).abs().max()) > 0
    assert bits_equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0


def test_with_clipping_and_through_render_in_chunks(npa, dev, nets, datapath_fp16x3):
    """clip_to_occupancy=True + march_stop_eps == the same call on grid.clip_rays(rays)[0]; render(chunk=96) == the unchunked call with
    last_stats -- rays_stopped among them -- summed over the chunks.  The density is 16 * (0.25 + 1.5 * rand) here: a clipped ray spends
    its 256 steps on the chord through the ball (at most 2 long), so with 63 slots it covers a quarter of the chord and reaches tau =
    4.6 within them only where the density times that quarter does; at 4 * (...) every clipped ray is truncated first (the definition on
    the CPU, with the float64 span as the clip: 0 stopped at 4, 151 stopped and 54 truncated at 16)."""
    nc, nf, _, _ = nets
    rays, rnd, _ = scene(dev)
    n = rays.shape[0]
    grid = stop_grid(npa, dev, "skip", scale=16.0)
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd,
              occupancy=grid, proposal="march", march_steps=M_STEPS, march_stop_eps=STOP_EPS)
    clipped, hit = grid.clip_rays(rays)
    assert 0 < int(hit.sum()) and not bits_equal(clipped, rays)
    with torch.no_grad():
        got = npa.render_rays(rays, nc, None, clip_to_occupancy=True, **kw)
        stats = dict(grid.last_stats)
        want = npa.render_rays(clipped, nc, None, **kw)
        assert stats == dict(grid.last_stats, rays_hit=int(hit.sum()), rays=n) and stats["rays_stopped"] >= 16 and stats["rays_truncated"] >= 16
        for k in want:
            assert bits_equal(got[k], want[k]), k
        # the chunks on the density of the other render tests (at 16 * (...) no unclipped ray is truncated: the stops come first)
        grid = kw["occupancy"] = stop_grid(npa, dev, "skip")
        whole = npa.render_rays(rays, nc, None, **kw)
        total = dict(grid.last_stats)
        chunked = npa.batchify_rays(rays, 96, network_fn=nc, network_query_fn=None, **kw)
        assert grid.last_stats == total and total["rays_stopped"] >= 16 and 0 < total["rays_truncated"] < n
        for k in whole:
            assert bits_equal(chunked[k], whole[k]), k
        K = np.array([[20.0, 0, 8.0], [0, 20.0, 8.0], [0, 0, 1]])
        geo = dict(rays=(rays[:, 0:3], rays[:, 3:6]), ndc=False, near=2.0, far=6.0, use_viewdirs=True, network_fn=nc, network_query_fn=None)
        one = npa.render(16, 16, K, chunk=1 << 20, **geo, **kw)
        total = dict(grid.last_stats)
        many = npa.render(16, 16, K, chunk=96, **geo, **kw)
        assert grid.last_stats == total and total["rays_stopped"] >= 16 and total["total"] == n * N_SLOTS
        assert set(total) == {"evaluated", "total", "rays_truncated", "rays_stopped"}
        for a, b in zip(one[:3], many[:3]):
            assert bits_equal(a, b)
        assert bits_equal(one[3]["raw"], many[3]["raw"])


# ------------------------------------------------------------------------------------------------ 4. off means off
@pytest.mark.parametrize("grad", [False, True])
def test_none_is_the_march_of_today_and_a_fresh_grid_stops_nothing(npa, dev, nets, datapath_fp16x3, monkeypatch, grad):
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    rays, rnd, _ = scene(dev)
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd,
              proposal="march", march_steps=M_STEPS)
    calls = []
    for name in ("occ_march", "occ_march_stop"):
        real = getattr(hb, name)
        monkeypatch.setattr(hb, name, lambda *a, _n=name, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])
    with torch.set_grad_enabled(grad):
        grid = stop_grid(npa, dev)
        a = npa.render_rays(rays, nc, None, occupancy=grid, **kw)
        stats_a = dict(grid.last_stats)
        b = npa.render_rays(rays, nc, None, occupancy=grid, march_stop_eps=None, **kw)
        assert calls == ["occ_march", "occ_march"] and grid.last_stats == stats_a and set(stats_a) == {"evaluated", "total", "rays_truncated"}
        for k in a:
            assert bits_equal(a[k].detach(), b[k].detach()), k
        # the same draws without `randoms`: u_march, then the noise
        draws = {k_: v for k_, v in kw.items() if k_ != "randoms"}
        torch.manual_seed(17)
        npa.render_rays(rays, nc, None, occupancy=grid, **draws)
        after_off = torch.rand(4, device=dev)
        torch.manual_seed(17)
        npa.render_rays(rays, nc, None, occupancy=grid, march_stop_eps=STOP_EPS, **draws)
        after_on = torch.rand(4, device=dev)
        assert torch.equal(after_off, after_on) and calls[-1] == "occ_march_stop"
        # a grid that was never updated: density 0, the march of today bit for bit, nothing stopped
        fresh = ball_dgrid(npa, dev)
        assert not bool(fresh.density.any())
        c = npa.render_rays(rays, nc, None, occupancy=fresh, **kw)
        stats_c = dict(fresh.last_stats)
        d = npa.render_rays(rays, nc, None, occupancy=fresh, march_stop_eps=STOP_EPS, **kw)
        assert fresh.last_stats == dict(stats_c, rays_stopped=0) and list(c) == list(d)
        for k in c:
            assert bits_equal(c[k].detach(), d[k].detach()), k
