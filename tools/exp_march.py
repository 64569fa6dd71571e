"""render(proposal="march") -- depths placed by marching the occupancy grid, one network evaluated, no coarse pass, no sample_pdf, no
sort -- against proposal="grid" and against the two-network grid render, in the same run on the same DensityGrids (fp16x3, 4096 rays,
S = 64 + 128 = 192 slots):
  * the whole TRAINING step (forward, img2mse, backward, FlatAdam.step) and the no_grad render at the ball masks of
    tools/exp_grid_proposal.py (evaluated shares of about 0.5 / 0.25 / 0.1 of the two-network render, outside skipped), the march at
    M = 256, 512 and 1024 steps;
  * per march row the evaluated points per ray and rays_truncated (last_stats): what the sample budget is spent on;
  * the march with march_stop_eps = 1e-3 and 1e-2 (the stop on the grid's own transmittance) at the same M, next to the
    march_stop_eps=None rows of the same run: ms, evaluated points per ray, rays truncated and rays stopped (left out when the tree
    under --root has no such option); with --density-scale F, because the fixture scene is a fog on which next to nothing stops,
    the eps = 1e-2 rows once more on a copy of every grid whose densities are multiplied by F -- a stand-in for surfaces that says
    what a stop saves in TIME only: the network is not scaled with the grid, so the image of those rows means nothing;
  * nerf_occ_march alone at 128^3 for the three M (HIP events around 100 launches), and nerf_occ_march_stop next to it;
  * with --step-size DS, next to the fixed-M rows of the same run, the march in world-space steps of DS (march_step_size=DS, the cap
    march_steps = 1024) at march_fit = 0 and 3, and at march_fit = 3 with march_stop_eps = 1e-2: ms, evaluated points per ray, rays
    truncated, refit and stopped; and nerf_occ_march_step alone.  Half a cell of the 128^3 grid over [-2, 2]^3 is 1 / 64.
Per row: ms (median of --reps alternating repetitions, min and max = the spread), the evaluated points, field and occupancy kernel ms.
The learning rate is 0 (the optimizer does all of its work; the scene and every share stay put).

    python tools/exp_march.py --out profiles/r14_exp_march.json
    python tools/exp_march.py --density-scale 16 --out profiles/r17_exp_march.json
    python tools/exp_march.py --step-size 0.015625 --out profiles/r18_exp_march_step.json
"""
import grid_exp as gx

ap = gx.parser(__doc__, steps="training steps / renders between two HIP events")
ap.add_argument("--density-scale", type=float, default=None,
                help="also time march_stop_eps = 1e-2 on a copy of every grid with its densities multiplied by this (time and counts only)")
ap.add_argument("--step-size", type=float, default=None,
                help="also time the march in world-space steps of this length (march_step_size, cap 1024) at march_fit 0 and 3")
args = ap.parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_march")
S = gx.Scene(wl, npa, dev, perturb=1., target=True, records=True)
LO, HI, R, N_RAYS, nc, nf = S.LO, S.HI, S.R, S.N_RAYS, S.nc, S.nf
N_C, N_F = 64, 128
MARCH_STEPS = (256, 512, 1024)
STOP_EPS = (1e-3, 1e-2)
STEP_CAP, STEP_FITS = 1024, (0, 3)
HAVE_STOP = hasattr(npa.DensityGrid, "march_stop")      # (--root of a tree without the option: the rows of that tree only)
opt_two, opt_one = S.adam(nc, nf), S.adam(nf)


def render(grid, mode):
    """mode: None (two networks), "grid", the march's step count, (step count, march_stop_eps), or a dict of march keywords"""
    if isinstance(mode, dict):
        return S.render(occupancy=grid, proposal="march", **mode)
    if mode == "grid":
        return S.render(occupancy=grid, proposal="grid")
    if isinstance(mode, tuple):
        return S.render(occupancy=grid, proposal="march", march_steps=mode[0], march_stop_eps=mode[1])
    if mode is not None:
        return S.render(occupancy=grid, proposal="march", march_steps=mode)
    return S.render(occupancy=grid)


def step(grid, mode):
    S.fit(render(grid, mode), opt_two if mode is None else opt_one, rgb0=mode is None)


def infer(grid, mode):
    with torch.no_grad():
        render(grid, mode)


def share_of(grid):
    torch.manual_seed(0)
    infer(grid, None)
    return gx.evaluated_share(grid)


def time_all(fn, configs, k, reps):
    """alternate the configurations inside every repetition; HIP events around k calls each"""
    times = gx.time_alternating([(name, lambda g=g, m=m: fn(g, m)) for name, g, m in configs], k, reps, warmup=3)
    rows = {}
    for name, grid, mode in configs:
        rows[name] = gx.row_stats(times[name], N_RAYS)
        summ = gx.kernel_summary(hb, lambda: fn(grid, mode))      # a separate call with HIP events around every launch
        stats = grid.last_stats
        rows[name].update(evaluated=stats["evaluated"], total=stats["total"], evaluated_per_ray=stats["evaluated"] / N_RAYS,
                          occ_kernels_ms=gx.kernel_ms(summ, "occ_"), field_ms=gx.kernel_ms(summ, ("field_", "wgrad")))
        for key in ("rays_truncated", "rays_stopped", "rays_refit"):
            if key in stats:
                rows[name][key] = stats[key]
    return rows


result = {"precision": "fp16x3", "rays": N_RAYS, "slots": f"{N_C} + {N_F}", "grid_resolution": R, "tree": args.label,
          "step": "render() forward, img2mse (two without a proposal), backward, FlatAdam.step (lr = 0)", "calls_per_timing": args.steps}
with torch.no_grad():
    density = npa.DensityGrid(LO, HI, R, device=dev).update(nf).density
configs = []
grids = []
for want in (0.5, 0.25, 0.1):
    g, radius = S.ball_with_share(npa.DensityGrid, share_of, want)
    g.density = density.clone()
    grids.append(g)
    name = f"share {want} (ball r = {radius:.3f}, outside skipped)"
    configs.append((name + ", two networks", g, None))
    configs.append((name + ", proposal=grid", g, "grid"))
    for M in MARCH_STEPS:
        configs.append((name + f", proposal=march M={M}", g, M))
    if args.step_size is not None:
        for fit in STEP_FITS:
            configs.append((name + f", proposal=march M={STEP_CAP} march_step_size={args.step_size:g} march_fit={fit}", g,
                            dict(march_steps=STEP_CAP, march_step_size=args.step_size, march_fit=fit)))
        configs.append((name + f", proposal=march M={STEP_CAP} march_step_size={args.step_size:g} march_fit={STEP_FITS[-1]} march_stop_eps=0.01", g,
                        dict(march_steps=STEP_CAP, march_step_size=args.step_size, march_fit=STEP_FITS[-1], march_stop_eps=1e-2)))
    if not HAVE_STOP:
        continue
    for M in MARCH_STEPS:
        for eps in STOP_EPS:
            configs.append((name + f", proposal=march M={M} march_stop_eps={eps:g}", g, (M, eps)))
    if args.density_scale is not None:
        dense = S.ball(npa.DensityGrid, radius)
        dense.density = density * args.density_scale
        for M in MARCH_STEPS:
            configs.append((name + f", proposal=march M={M} march_stop_eps=0.01, grid density x {args.density_scale:g}", dense, (M, 1e-2)))
result["train_step_4096_rays"] = time_all(step, configs, args.steps, args.reps)
result["no_grad_render_4096_rays"] = time_all(infer, configs, args.steps, args.reps)
g = grids[1]
rays_rec = S.records
SLOTS = N_C + N_F
kernel = {}
for M in MARCH_STEPS:
    us = gx.time_launches(lambda: g.march(rays_rec, M, SLOTS), args.reps)
    nbytes = (32 + 4 * SLOTS + 8) * N_RAYS
    kernel[f"M={M}"] = dict(us, rays=N_RAYS, slots=SLOTS, bytes_model=nbytes, gbytes_per_s_model=nbytes / us["us_median"] / 1e3,
                            rays_truncated=int(g.march(rays_rec, M, SLOTS)[2].sum()))
kernel["note"] = "host-timed back-to-back launches (allocation of the outputs included)"
result["march_kernel_128_cubed"] = kernel
kernel = {}
for M in MARCH_STEPS if HAVE_STOP else ():
    for eps in STOP_EPS:
        us = gx.time_launches(lambda: g.march_stop(rays_rec, M, SLOTS, eps), args.reps)
        out = g.march_stop(rays_rec, M, SLOTS, eps)
        kernel[f"M={M} eps={eps:g}"] = dict(us, rays=N_RAYS, slots=SLOTS, rays_truncated=int(out[2].sum()), rays_stopped=int(out[3].sum()))
if HAVE_STOP:
    kernel["note"] = "host-timed back-to-back launches (allocation of the outputs included)"
    result["march_stop_kernel_128_cubed"] = kernel
if args.step_size is not None:
    kernel = {}
    for fit in STEP_FITS:
        us = gx.time_launches(lambda: g.march_step(rays_rec, args.step_size, STEP_CAP, SLOTS, fit), args.reps)
        out = g.march_step(rays_rec, args.step_size, STEP_CAP, SLOTS, fit)
        kernel[f"ds={args.step_size:g} M={STEP_CAP} fit={fit}"] = dict(us, rays=N_RAYS, slots=SLOTS, rays_truncated=int(out[2].sum()),
                                                                     rays_refit=int((out[3] > 0).sum()))
    us = gx.time_launches(lambda: g.march_step_stop(rays_rec, args.step_size, STEP_CAP, SLOTS, 1e-2, STEP_FITS[-1]), args.reps)
    out = g.march_step_stop(rays_rec, args.step_size, STEP_CAP, SLOTS, 1e-2, STEP_FITS[-1])
    kernel[f"ds={args.step_size:g} M={STEP_CAP} fit={STEP_FITS[-1]} eps=0.01"] = dict(
        us, rays=N_RAYS, slots=SLOTS, rays_truncated=int(out[2].sum()), rays_refit=int((out[3] > 0).sum()), rays_stopped=int(out[4].sum()))
    kernel["note"] = "host-timed back-to-back launches (allocation of the outputs included)"
    result["march_step_kernel_128_cubed"] = kernel
gx.emit(result, args.out)
