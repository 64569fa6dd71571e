"""GPU tests (-m gpu) of render_rays(proposal="march", march_step_size=ds, march_fit=J): nerf_occ_march_step alone against its
definitions (OccupancyGrid.march_step_reference / DensityGrid.march_step_stop_reference, evaluated on the CPU) as raw bits, then the
render -- forward and backward -- against THE CHAIN of tests/test_gpu_march.py with the world-space march in front: the reference ->
pts = o + d z -> the compacting hook with the extra predicate z < z_stop -> npa.raw2outputs.  Every comparison is bit for bit but
the ray gradients', which keep the bound of DESIGN.md section 3.10."""
import numpy as np
import pytest
import torch

import nerf_oracle as orc
from test_gpu_march import INVALID, N_KERNEL, NOISE_SEED, noise_of, stopping_hook
from test_gpu_occupancy import BOX_HI, BOX_LO, ball_grid, bits_equal
from test_gpu_occupancy_train import U, _small_scene, datapath_fp16x3, flat_of, fresh_nets, grads_of, zero_grads  # noqa: F401
from test_gpu_parity import datapath, dev, maxdiff, nets, npa  # noqa: F401  (fixtures)
from test_gpu_ray_grad import rel_l2
from test_march_cpu import hand_grid, hand_rays
from test_march_stop_cpu import ball_density_grid, hand_dgrid

pytestmark = pytest.mark.gpu

INF = float("inf")


def reference_on_cpu(grid, rays, u, ds, M, S, fit, eps=None):
    """the definition, evaluated on the CPU (its divisions and its square root are IEEE there whatever the device's torch build does), on
    `rays`' device: (z_vals, z_stop, truncated, level, stopped -- all False without eps)"""
    r, uu = rays.detach().cpu(), None if u is None else u.cpu()
    if eps is None:
        out = grid.march_step_reference(r, uu, ds, M, S, fit)
        out = out + (torch.zeros_like(out[2]),)
    else:
        out = grid.march_step_stop_reference(r, uu, ds, M, S, eps, fit)
    return tuple(t.to(rays.device) for t in out)


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
KERNEL_SHAPES = [(1, 1, 0), (7, 2, 0), (64, 5, 1), (65, 64, 0), (1024, 32, 3), (16384, 192, 2)]
KERNEL_DENSITY_SCALE = 20.0
STEP_INVALID = dict(INVALID)
D_ZERO = STEP_INVALID.pop("NaN direction")      # the same ray, now with d = 0: no step


def step_scene():
    """301 rays (four per block: 76 blocks, the last one ragged) at the 32^3 ball: orc.synthetic_rays with |d| rescaled per ray by a factor
    in [0.4, 2.5] (near and far divided by it: the same span in the scene, another one in depth), 40 rays that start inside the box with
    near = 0 and end anywhere, and the eight invalid rays of tests/test_gpu_march.py planted in the first, in middle and in the last
    block, the NaN direction replaced by d = 0.  u holds 0 and the largest fp32 below 1."""
    g = torch.Generator().manual_seed(41)
    n = N_KERNEL
    rays = orc.synthetic_rays(n, seed=33)
    factor = 0.4 * 6.25 ** torch.rand(n, 1, generator=g)
    rays[:, 3:6] *= factor
    rays[:, 6:8] /= factor
    rays[200:240, 0:3] = (torch.rand(40, 3, generator=g) - 0.5) * 3.0
    rays[200:240, 6] = 0.0
    rays[200:240, 7] = 0.3 + 3.0 * torch.rand(40, generator=g)
    rays[STEP_INVALID["NaN origin"], 1] = float("nan")
    rays[D_ZERO, 3:6] = 0.0
    rays[STEP_INVALID["infinite direction"], 5] = INF
    rays[STEP_INVALID["NaN near"], 6] = float("nan")
    rays[STEP_INVALID["infinite far"], 7] = INF
    rays[STEP_INVALID["near == far"], 6] = rays[STEP_INVALID["near == far"], 7]
    rays[STEP_INVALID["near > far"], 6] = rays[STEP_INVALID["near > far"], 7] + 1.0
    rays[STEP_INVALID["-inf origin"], 0] = -INF
    u = torch.rand(n, generator=g)
    u[5], u[6] = 0.0, float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    return rays, u


@pytest.mark.parametrize("outside", ["evaluate", "skip"])
@pytest.mark.parametrize("ds", [1.0 / 64, 0.37])
@pytest.mark.parametrize("M,S,fit", KERNEL_SHAPES)
def test_kernel_equals_the_definitions_bit_for_bit(npa, dev, outside, ds, M, S, fit):
    """z_vals and z_stop equal the reference's as raw bits, truncated, level and stopped are equal: the plain form and the stop form at
    eps 1e-2 and 1e-4 on a density of 20 * (0.25 + 1.5 * rand) inside the ball; u random and None; ray records of 11 and of 8 columns;
    the same bits on a second launch"""
    hb = npa.hip_backend
    grid = ball_density_grid(outside, scale=KERNEL_DENSITY_SCALE, device=dev)
    rays, u = step_scene()
    invalid = torch.tensor(sorted(INVALID.values()))
    valid = torch.ones(N_KERNEL, dtype=torch.bool)
    valid[invalid] = False
    out_sigma = grid.sigma_threshold if outside == "evaluate" else 0.0
    seen = {"refit": 0, "truncated": 0, "stopped": 0}
    for eps in (None, 1e-2, 1e-4):
        for uu in (u, None):
            want = reference_on_cpu(grid, rays, uu, ds, M, S, fit, eps)
            for cols in (11, 8):
                r = rays[:, :cols].contiguous().to(dev)
                z, z_stop, tr, lv, st = hb.occ_march_step(grid._desc(), None if eps is None else grid.density, out_sigma if eps is not None else 0.0,
                                                          r, None if uu is None else uu.to(dev), ds, M, S, fit, eps)
                torch.cuda.synchronize()
                assert z.shape == (N_KERNEL, S) and z.dtype == torch.float32 and z_stop.shape == tr.shape == lv.shape == (N_KERNEL,)
                assert tr.dtype == lv.dtype == torch.int32 and (st is None) == (eps is None)
                assert bits_equal(z.cpu(), want[0]), (eps, uu is None, cols, int((z.cpu() != want[0]).sum()))
                assert bits_equal(z_stop.cpu(), want[1]) and torch.equal(tr.cpu().bool(), want[2]) and torch.equal(lv.cpu(), want[3])
                if eps is not None:
                    assert st.dtype == torch.int32 and torch.equal(st.cpu().bool(), want[4])
            ud = None if uu is None else uu.to(dev)
            again = grid.march_step(rays.to(dev), ds, M, S, fit, u=ud) if eps is None else grid.march_step_stop(rays.to(dev), ds, M, S, eps, fit, u=ud)
            assert bits_equal(again[0], z) and bits_equal(again[1], z_stop) and torch.equal(again[2], tr.bool()) and torch.equal(again[3], lv)
            assert again[2].dtype == torch.bool and again[3].dtype == torch.int32 and len(again) == (4 if eps is None else 5)
            if eps is not None:
                assert torch.equal(again[4], st.bool()) and again[4].dtype == torch.bool and not bool((again[2] & again[4]).any())
            # the invalid rays: their own far in every slot, -inf, no flag, level 0
            assert bits_equal(z.cpu()[invalid], rays[invalid, 7:8].expand(-1, S).contiguous())
            assert bool((z_stop.cpu()[invalid] == -INF).all()) and not bool(tr.cpu()[invalid].any()) and not bool(lv.cpu()[invalid].any())
            assert bool((z.cpu()[valid][:, 1:] >= z.cpu()[valid][:, :-1]).all())
            assert int(want[3].max()) <= fit and bool((want[3][want[2]] == fit).all())
            seen["refit"] += int((want[3] > 0).sum())
            seen["truncated"] += int(want[2].sum())
            seen["stopped"] += int(want[4].sum())
    print(f"\n[{outside} ds={ds:g} M={M} S={S} fit={fit}] over the six runs: {seen}")
    if fit > 0 and ds < 0.1 and S <= 32:        # a chord of the ball is up to 128 steps of 1 / 64: more than 4 or 31 slots take
        assert seen["refit"] > 0
    if S <= 5 and ds < 0.1:
        assert seen["truncated"] > 0
    if S >= 32 and ds < 0.1:        # (with one or four slots nothing is emitted in front of a cut, or the slot limit bites first)
        assert seen["stopped"] > 0


# ------------------------------------------------------------------------------------------------ 1b. the two kinds of steps agree
# Rays 0 .. 6 of tests/test_march_cpu.hand_rays (pattern row, full row, miss, NaN component, near == far, near > far, infinite
# direction) have |d| = 1, near = 0 and far = 8; with ds * M = 8, all powers of two, (k + u) * ds and (k + u) / M * far are the same
# exact scalings and no candidate is cut by z < far before k = M: march_step_reference's docstring promises level 0 equal to
# march_reference, and the same holds for the two stop definitions.
AGREE_STEPS = [(16, 0.5), (128, 1.0 / 16), (1024, 1.0 / 128)]
AGREE_EPS = 1e-2


def agree_references(outside, density, M, ds, S, u):
    """(equal steps, world steps at fit = 0) of the definitions on the CPU, each (z_vals, z_stop, truncated, level, stopped); density
    None: the plain forms (stopped all False), else the stop forms on that hand-made density"""
    rays = hand_rays()[:7]
    if density is None:
        grid = hand_grid(outside)
        a = grid.march_reference(rays, u, M, S)
        a = a + (torch.zeros(7, dtype=torch.int32), torch.zeros_like(a[2]))
        b = grid.march_step_reference(rays, u, ds, M, S, 0)
        return a, b + (torch.zeros_like(b[2]),)
    grid = hand_dgrid(outside, density)
    a = grid.march_stop_reference(rays, u, M, S, AGREE_EPS)
    return a[:3] + (torch.zeros(7, dtype=torch.int32), a[3]), grid.march_step_stop_reference(rays, u, ds, M, S, AGREE_EPS, 0)


def assert_case_mix(want, density, M, S):
    """the rays of an agreement run do what the run is there for: some emit, some are truncated, some stop"""
    z, z_stop, tr, _, st = want
    if S >= 5:
        assert int((z[:, 0] < z_stop).sum()) >= 2, (density, M, S)      # (a padded slot holds z_stop; an invalid ray's z_stop is -inf)
    if (M, S) == (16, 64) and density not in (None, "zero"):
        assert int(st.sum()) >= 1, (density, M, S)
    if (M, S) == (128, 5):
        assert int(tr.sum()) >= 2, (density, M, S)


@pytest.mark.parametrize("outside", ["evaluate", "skip"])
def test_world_steps_at_fit_0_equal_equal_steps_on_a_power_of_two_geometry(npa, dev, outside):
    """hb.occ_march_step(fit=0) equals hb.occ_march, and its stop form hb.occ_march_stop at eps = 1e-2 on the "late", "odd", "run" and
    "zero" densities, as raw bits in z_vals and z_stop, with equal flags and level 0 everywhere -- and both equal both definitions."""
    hb = npa.hip_backend
    rays = hand_rays()[:7].contiguous().to(dev)
    g = torch.Generator().manual_seed(19)
    for density, slots in [(None, (64, 20, 5, 1))] + [(d, (64, 20, 5)) for d in ("late", "odd", "run", "zero")]:
        grid = (hand_grid(outside) if density is None else hand_dgrid(outside, density)).to(dev)
        dens = None if density is None else grid.density
        out_sigma = grid.sigma_threshold if density is not None and outside == "evaluate" else 0.0
        for M, ds in AGREE_STEPS:
            for S in slots:
                for u in (None, torch.rand(7, generator=g)):
                    want, want_step = agree_references(outside, density, M, ds, S, u)
                    assert_same(want_step, want, ("the definitions", density, M, S))
                    assert_case_mix(want, density, M, S)
                    ud = None if u is None else u.to(dev)
                    if density is None:
                        z, z_stop, tr = hb.occ_march(grid._desc(), rays, ud, M, S)
                        st = None
                    else:
                        z, z_stop, tr, st = hb.occ_march_stop(grid._desc(), dens, out_sigma, rays, ud, M, S, AGREE_EPS)
                    zs, zs_stop, trs, lv, sts = hb.occ_march_step(grid._desc(), dens, out_sigma, rays, ud, ds, M, S, 0,
                                                                  None if density is None else AGREE_EPS)
                    torch.cuda.synchronize()
                    what = (density, M, S, u is None)
                    assert bits_equal(zs, z) and bits_equal(zs_stop, z_stop) and torch.equal(trs, tr), what
                    assert not bool(lv.any()) and (sts is None) == (density is None), what
                    if density is not None:
                        assert torch.equal(sts, st), what
                    got = (z.cpu(), z_stop.cpu(), tr.cpu().bool(), lv.cpu(), want[4] if st is None else st.cpu().bool())
                    assert_same(got, want, ("the kernels against the definitions",) + what)


def assert_same(got, want, what):
    assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1]), (what, got[0], want[0], got[1], want[1])
    assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3]) and torch.equal(got[4], want[4]), (what, got[2:], want[2:])


# ------------------------------------------------------------------------------------------------ 2. the render against the chain
DS, M_CAP, N_SLOTS, FIT = 1.0 / 32, 1024, 64, 2
STOP_EPS = 1e-2
STEP_KW = dict(proposal="march", march_steps=M_CAP, march_step_size=DS, march_fit=FIT)


def scene(dev, n=256, S=N_SLOTS):
    rays, _, target = _small_scene(dev, n)
    u = torch.rand(n, generator=torch.Generator().manual_seed(23)).to(dev)
    return rays, {"u_march": u, "noise_f": noise_of(dev, n, S)}, target


def grid_of(npa, dev, kind, outside):
    """plain: an OccupancyGrid; density / stop: the ball as a DensityGrid with density 4 * (0.25 + 1.5 * rand) inside it"""
    return ball_grid(npa, dev, outside) if kind == "plain" else ball_density_grid(outside, scale=4.0, device=dev)


def chain(npa, grid, rays, u, net, noise, eps=None, ds=DS, M=M_CAP, S=N_SLOTS, fit=FIT, white=True, seen=None, taps=None):
    """THE YARDSTICK: render_rays(proposal="march", march_step_size=ds, march_fit=fit[, march_stop_eps=eps]) from public pieces
    (tests/test_gpu_march.chain with the world-space march in front)"""
    z, z_stop, tr, lv, st = reference_on_cpu(grid, rays, u, ds, M, S, fit, eps)
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]
    raw = stopping_hook(npa, grid, z, z_stop, seen, taps)(pts, rays[:, 8:11], net)
    if noise > 0:
        torch.manual_seed(NOISE_SEED)
    rgb, disp, acc, _, _ = npa.raw2outputs(raw, z, rays[:, 3:6], noise, white)
    return dict(rgb_map=rgb, disp_map=disp, acc_map=acc, raw=raw), z, z_stop, tr, lv, st


def stats_of(n, seen, tr, lv, st, eps):
    want = {"evaluated": seen[0][0], "total": n * N_SLOTS, "rays_truncated": int(tr.sum()), "rays_refit": int((lv > 0).sum())}
    if eps is not None:
        want["rays_stopped"] = int(st.sum())
    return want


@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
@pytest.mark.parametrize("perturb,noise", [(1.0, 1.0), (0.0, 0.0)])
@pytest.mark.parametrize("outside", ["evaluate", "skip"])
@pytest.mark.parametrize("kind", ["plain", "density", "stop"])
def test_no_grad_render_equals_the_chain_bit_for_bit(npa, dev, nets, datapath, perturb, noise, outside, kind):
    """256 rays, ds = 1 / 32, M = 1024, S = 64, fit = 2: rgb_map, disp_map, acc_map and raw equal the chain's bit for bit; the keys are
    the march's; N_samples = 64, N_importance = 0 gives the bits of 16 + 48; last_stats counts what the hook evaluated and the rays the
    definition truncates, refits and stops"""
    nc, nf, _, _ = nets
    rays, rnd, _ = scene(dev)
    n = rays.shape[0]
    grid = grid_of(npa, dev, kind, outside)
    eps = STOP_EPS if kind == "stop" else None
    kw = dict(network_fine=nf, white_bkgd=True, perturb=perturb, raw_noise_std=noise, retraw=True, occupancy=grid, randoms=rnd, **STEP_KW)
    if eps is not None:
        kw["march_stop_eps"] = eps
    seen = []
    with torch.no_grad():
        want, z, z_stop, tr, lv, st = chain(npa, grid, rays, rnd["u_march"] if perturb > 0 else None, nf, noise, eps, seen=seen)
        got = npa.render_rays(rays, nc, None, N_samples=16, N_importance=48, **kw)
        stats = dict(grid.last_stats)
        again = npa.render_rays(rays, nc, None, N_samples=64, N_importance=0, **kw)
        assert grid.last_stats == stats
    assert list(got) == list(again) == ["rgb_map", "disp_map", "acc_map", "raw"]
    for k in got:
        assert bits_equal(got[k], want[k]), (k, maxdiff(got[k], want[k]))
        assert bits_equal(got[k], again[k]), k
    assert got["raw"].shape == (n, N_SLOTS, 4)
    print(f"\n[{kind} {outside}] {stats}; levels {[int((lv == j).sum()) for j in range(FIT + 1)]}")
    assert stats == stats_of(n, seen, tr, lv, st, eps)
    assert 0 < stats["evaluated"] < stats["total"] and stats["rays_refit"] < n
    if eps is None:         # a chord of the ball is up to 64 steps of 1 / 32, and its closing step: the longest do not fit 63 slots
        assert stats["rays_refit"] > 0 and stats["rays_truncated"] == 0
    else:                   # (a stopped ray emits less: the stop spares most of them the doubling)
        assert stats["rays_stopped"] >= 16
    assert float(got["acc_map"].max()) > 0.5
    # what is not evaluated is exactly zero: the closing samples, the padding and whatever lies at or behind the stop depth
    assert bool((got["raw"][z >= z_stop[:, None]] == 0).all())


# ------------------------------------------------------------------------------------------------ 3. gradients
@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
@pytest.mark.parametrize("eps", [None, STOP_EPS])
def test_forward_with_grad_equals_the_no_grad_render(npa, dev, nets, datapath, eps):
    nc, nf, _, _ = nets
    rays, rnd, _ = scene(dev)
    grid = grid_of(npa, dev, "density", "evaluate")
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd,
              occupancy=grid, march_stop_eps=eps, **STEP_KW)
    with torch.no_grad():
        want = npa.render_rays(rays, nc, None, **kw)
    stats = dict(grid.last_stats)
    grid.last_stats = None
    got = npa.render_rays(rays, nc, None, **kw)
    assert list(got) == list(want) == ["rgb_map", "disp_map", "acc_map", "raw"]
    for k in want:
        assert bits_equal(got[k], want[k]), (k, maxdiff(got[k], want[k]))
    assert grid.last_stats == stats and "rays_refit" in stats and ("rays_stopped" in stats) == (eps is not None)
    assert stats["rays_refit" if eps is None else "rays_stopped"] > 0
    assert got["rgb_map"].grad_fn is not None and got["raw"].grad_fn is not None
    del got          # (a graph dropped without backward)


@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
@pytest.mark.parametrize("eps", [None, STOP_EPS])
def test_parameter_gradients_equal_the_chains_bit_for_bit(npa, dev, nets, datapath, eps):
    """loss = img2mse(rgb_map, t): .grad of every parameter of the evaluated network equals autograd's through the chain, bit for bit;
    the other network's .grad stays None"""
    nc, nf, _, _ = nets
    rays, rnd, target = scene(dev)
    grid = grid_of(npa, dev, "density", "evaluate")
    kw = dict(N_samples=16, N_importance=48, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, randoms=rnd, occupancy=grid, march_stop_eps=eps,
              **STEP_KW)
    zero_grads(nc, nf)
    out = npa.render_rays(rays, nc, None, network_fine=nf, **kw)
    assert grid.last_stats["rays_refit" if eps is None else "rays_stopped"] > 0
    loss_g = npa.img2mse(out["rgb_map"], target)
    loss_g.backward()
    assert all(p.grad is None for p in nc.parameters())
    got = grads_of(nf)
    zero_grads(nc, nf)
    loss_h = npa.img2mse(chain(npa, grid, rays, rnd["u_march"], nf, 1.0, eps)[0]["rgb_map"], target)
    loss_h.backward()
    want = grads_of(nf)
    zero_grads(nc, nf)
    assert bits_equal(loss_g.detach(), loss_h.detach())
    assert all(x is not None for x in got) and float(flat_of(got).abs().max()) > 0
    for i, (x, y) in enumerate(zip(got, want)):
        assert bits_equal(x, y), (i, maxdiff(x, y), rel_l2(flat_of(got), flat_of(want)))


@pytest.mark.parametrize("datapath", ["fp32", "fp16x3"], indirect=True)
def test_ray_gradients_against_the_float64_fold_of_the_chain(npa, dev, nets, datapath, monkeypatch):
    """rays.requires_grad_(): by the method and at the bound of tests/test_gpu_march.py's test of the same name --
    the float64 fold of the chain's tapped per-point gradients plus the compositing's |d| term, within (S + 1) * 2^-24 * sum|terms| *
    1.01 per element, S = 64.  The depths are constants of the graph (the step's 1 / |d| too): columns 6:8 are exactly 0."""
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    rays0, rnd, target = scene(dev)
    grid = grid_of(npa, dev, "density", "evaluate")
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=0.5, randoms=rnd, occupancy=grid,
              **STEP_KW)
    rg = rays0.clone().requires_grad_(True)
    npa.img2mse(npa.render_rays(rg, nc, None, **kw)["rgb_map"], target).backward()
    got = rg.grad.clone()
    dns, taps = [], []
    bwd = hb.raw2outputs_bwd
    monkeypatch.setattr(hb, "raw2outputs_bwd", lambda *a, **k: (dns.append(k.get("d_rays_d")), bwd(*a, **k))[1])
    rh = rays0.clone().requires_grad_(True)
    ref, z = chain(npa, grid, rh, rnd["u_march"], nf, 0.5, taps=taps)[:2]
    npa.img2mse(ref["rgb_map"], target).backward()
    zero_grads(nc, nf)
    assert len(taps) == 1 and len(dns) == 1 and dns[0] is not None
    n, S, tap = rays0.shape[0], N_SLOTS, taps[0]
    want = torch.zeros(n, 11, dtype=torch.float64, device=dev)
    mag = torch.zeros_like(want)
    ray_of = tap["idx"] // S
    gp, gv, zz = tap["d_pts"].double(), tap["d_viewdirs"].double(), z.reshape(-1)[tap["idx"]].double()[:, None]
    for cols, terms in ((slice(0, 3), gp), (slice(3, 6), zz * gp), (slice(8, 11), gv)):
        want[:, cols] = want[:, cols].index_add(0, ray_of, terms)
        mag[:, cols] = mag[:, cols].index_add(0, ray_of, terms.abs())
    want[:, 3:6] += dns[0].double()
    mag[:, 3:6] += dns[0].double().abs()
    err = (got.double() - want).abs()
    bound = 1.01 * (S + 1) * U * mag
    geo = [0, 1, 2, 3, 4, 5, 8, 9, 10]
    print(f"\n[{datapath}] ray gradient: worst error / bound {float((err[:, geo] / bound[:, geo].clamp(min=1e-300)).max()):.3f}; "
          f"relative L2 vs the chain's own rays.grad {rel_l2(got, rh.grad):.2e}")
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    assert bool((got[:, 6:8] == 0).all())
    assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())


def test_an_upstream_gradient_on_a_dropped_slot_reaches_no_parameter(npa, dev, nets, datapath_fp16x3, monkeypatch):
    """loss = sum(raw * G) through retraw: the network's gradient with a random G equals, bit for bit, the one with G zeroed on the slots
    the pass did not evaluate (slot < 0: closing samples, padding, stopped) -- and those slots did carry a nonzero G"""
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    rays, rnd, _ = scene(dev)
    n = rays.shape[0]
    grid = grid_of(npa, dev, "density", "evaluate")
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, randoms=rnd, retraw=True, occupancy=grid,
              march_stop_eps=STOP_EPS, **STEP_KW)
    slots = []
    real = hb.occ_compact
    monkeypatch.setattr(hb, "occ_compact", lambda *a, **k: (lambda r: (slots.append(r[0].clone()), r)[1])(real(*a, **k)))
    G = torch.randn(n, N_SLOTS, 4, generator=torch.Generator().manual_seed(5)).to(dev)
    grads = []
    for mask_it in (False, True):
        zero_grads(nc, nf)
        del slots[:]
        raw = npa.render_rays(rays, nc, None, **kw)["raw"]
        assert len(slots) == 1
        live = (slots[0] >= 0).view(n, N_SLOTS, 1)
        (raw * (G * live if mask_it else G)).sum().backward()
        grads.append(flat_of(grads_of(nf)))
        assert all(p.grad is None for p in nc.parameters())
    zero_grads(nc, nf)
    assert 0 < int(live.sum()) < n * N_SLOTS and float((G * ~live).abs().max()) > 0
    assert bits_equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 4. chunks, the clip, the empty grid
def test_with_clipping_and_through_render_in_chunks(npa, dev, nets, datapath_fp16x3):
    """clip_to_occupancy=True equals marching grid.clip_rays(rays)[0]; render(chunk=96) == the unchunked call with last_stats --
    rays_refit and rays_stopped among them -- summed over the chunks (batchify_rays slices u_march too)"""
    nc, nf, _, _ = nets
    rays, rnd, _ = scene(dev)
    n = rays.shape[0]
    grid = grid_of(npa, dev, "density", "skip")
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, randoms=rnd,
              occupancy=grid, march_stop_eps=STOP_EPS, **STEP_KW)
    clipped, hit = grid.clip_rays(rays)
    assert 0 < int(hit.sum()) and not bits_equal(clipped, rays)
    with torch.no_grad():
        got = npa.render_rays(rays, nc, None, clip_to_occupancy=True, **kw)
        stats = dict(grid.last_stats)
        want = npa.render_rays(clipped, nc, None, **kw)
        assert stats == dict(grid.last_stats, rays_hit=int(hit.sum()), rays=n) and stats["total"] == n * N_SLOTS
        for k in want:
            assert bits_equal(got[k], want[k]), k
        whole = npa.render_rays(rays, nc, None, **kw)
        total = dict(grid.last_stats)
        assert set(total) == {"evaluated", "total", "rays_truncated", "rays_stopped", "rays_refit"}
        chunked = npa.batchify_rays(rays, 96, network_fn=nc, network_query_fn=None, **kw)
        assert grid.last_stats == total and total["rays_refit"] + total["rays_stopped"] > 0
        for k in whole:
            assert bits_equal(chunked[k], whole[k]), k
        K = np.array([[20.0, 0, 8.0], [0, 20.0, 8.0], [0, 0, 1]])
        geo = dict(rays=(rays[:, 0:3], rays[:, 3:6]), ndc=False, near=2.0, far=6.0, use_viewdirs=True, network_fn=nc, network_query_fn=None)
        for extra in ({}, {"march_stop_eps": None}):
            one = npa.render(16, 16, K, chunk=1 << 20, **geo, **dict(kw, **extra))
            total = dict(grid.last_stats)
            many = npa.render(16, 16, K, chunk=96, **geo, **dict(kw, **extra))
            assert grid.last_stats == total and total["total"] == n * N_SLOTS and 0 < total["evaluated"] < total["total"]
            assert ("rays_stopped" in total) == (not extra) and "rays_refit" in total
            for a, b in zip(one[:3], many[:3]):
                assert bits_equal(a, b)
            assert set(one[3]) == set(many[3]) == {"raw"} and bits_equal(one[3]["raw"], many[3]["raw"])
        assert total["rays_refit"] > 0      # (without the stop the long chords need a doubling)


def test_all_empty_grid_launches_no_field_kernel(npa, dev, nets, monkeypatch):
    """an all-empty grid with outside="skip": every ray misses, m == 0, no field launch, white background, zero gradients, no ray
    truncated, refit or stopped -- with gradients and without"""
    hb = npa.hip_backend
    nc, nf = fresh_nets(npa, dev, nets)
    rays, rnd, target = scene(dev)
    empty = npa.DensityGrid.from_mask(torch.zeros(2, 2, 2, dtype=torch.bool), BOX_LO, BOX_HI, outside="skip", device=dev)
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = hb.field_fwd, hb.field_bwd
    monkeypatch.setattr(hb, "field_fwd", lambda *a, **k: (calls.__setitem__("fwd", calls["fwd"] + 1), fwd(*a, **k))[1])
    monkeypatch.setattr(hb, "field_bwd", lambda *a, **k: (calls.__setitem__("bwd", calls["bwd"] + 1), bwd(*a, **k))[1])
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, randoms=rnd, occupancy=empty, retraw=True,
              march_stop_eps=STOP_EPS, **STEP_KW)
    want = {"evaluated": 0, "total": 256 * N_SLOTS, "rays_truncated": 0, "rays_stopped": 0, "rays_refit": 0}
    r = rays.clone().requires_grad_(True)
    out = npa.render_rays(r, nc, None, **kw)
    assert empty.last_stats == want
    assert bool((out["rgb_map"] == 1).all()) and bool((out["raw"] == 0).all()) and bool((out["acc_map"] == 0).all())
    npa.img2mse(out["rgb_map"], target).backward()
    assert calls == {"fwd": 0, "bwd": 0}
    assert all(p.grad is not None and bool((p.grad == 0).all()) for p in nf.parameters()) and all(p.grad is None for p in nc.parameters())
    assert r.grad is not None and bool(torch.isfinite(r.grad).all())
    with torch.no_grad():
        out = npa.render_rays(rays, nc, None, **kw)
    assert empty.last_stats == want and calls == {"fwd": 0, "bwd": 0}
    assert bool((out["rgb_map"] == 1).all())


# ------------------------------------------------------------------------------------------------ 5. off means off
@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("eps", [None, STOP_EPS])
def test_off_is_the_march_of_today(npa, dev, nets, datapath_fp16x3, grad, eps):
    """march_step_size=None, march_fit=0: the kernel names of the TIMER summary (and their launch counts), the output bits, the stats and
    the draws of a proposal="march" render equal those of the same call without the keywords; with the keywords set the one march kernel
    is the new one"""
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    rays, rnd, _ = scene(dev)
    grid = grid_of(npa, dev, "density", "evaluate")
    kw = dict(N_samples=16, N_importance=48, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, retraw=True, occupancy=grid,
              proposal="march", march_steps=256, march_stop_eps=eps)

    def traced(**extra):
        timer, hb.TIMER = hb.TIMER, hb.KernelTimer()
        try:
            out = npa.render_rays(rays, nc, None, **kw, **extra)
            summary = hb.TIMER.summary()
        finally:
            hb.TIMER = timer
        return {k: v.detach() for k, v in out.items()}, {k: v["launches"] for k, v in summary.items()}, dict(grid.last_stats)
    with torch.set_grad_enabled(grad):
        a, names_a, stats_a = traced(randoms=rnd)
        b, names_b, stats_b = traced(randoms=rnd, march_step_size=None, march_fit=0)
        assert names_a == names_b and list(names_a) == list(names_b) and stats_a == stats_b and "rays_refit" not in stats_a
        old = "occ_march_stop_kernel" if eps is not None else "occ_march_kernel"
        assert names_a[old] == 1 and "occ_march_step_kernel" not in names_a
        assert list(a) == list(b)
        for k in a:
            assert bits_equal(a[k], b[k]), k
        # the same draws without `randoms`
        torch.manual_seed(17)
        traced()
        after_off = torch.rand(4, device=dev)
        torch.manual_seed(17)
        traced(march_step_size=None, march_fit=0)
        after_none = torch.rand(4, device=dev)
        torch.manual_seed(17)
        c, names_c, stats_c = traced(march_step_size=DS, march_fit=FIT)
        after_on = torch.rand(4, device=dev)
        assert torch.equal(after_off, after_none) and torch.equal(after_off, after_on)
        # on: the new kernel stands where the old one stood, everything else of the call is launched as before
        swap = lambda names: {("march" if k in (old, "occ_march_step_kernel") else k): v for k, v in names.items() if not k.startswith(("field_", "wgrad"))}
        assert names_c["occ_march_step_kernel"] == 1 and old not in names_c and swap(names_c) == swap(names_a)
        assert "rays_refit" in stats_c and (eps is not None or stats_c["rays_refit"] > 0)
        # a fit of 0 has no counter
        _, _, stats_d = traced(randoms=rnd, march_step_size=DS)
        assert "rays_refit" not in stats_d and set(stats_d) == set(stats_a)
