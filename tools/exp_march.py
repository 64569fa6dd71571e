"""render(proposal="march") -- depths placed by marching the occupancy grid, one network evaluated, no coarse pass, no sample_pdf, no
sort -- against proposal="grid" and against the two-network grid render, in the same run on the same DensityGrids (fp16x3, 4096 rays,
S = 64 + 128 = 192 slots):
  * the whole TRAINING step (forward, img2mse, backward, FlatAdam.step) and the no_grad render at the ball masks of
    tools/exp_grid_proposal.py (evaluated shares of about 0.5 / 0.25 / 0.1 of the two-network render, outside skipped), the march at
    M = 256, 512 and 1024 steps;
  * per march row the evaluated points per ray and rays_truncated (last_stats): what the sample budget is spent on;
  * nerf_occ_march alone at 128^3 for the three M (HIP events around 100 launches).
Per row: ms (median of --reps alternating repetitions, min and max = the spread), the evaluated points, field and occupancy kernel ms.
The learning rate is 0 (the optimizer does all of its work; the scene and every share stay put).

    python tools/exp_march.py --out profiles/r14_exp_march.json
"""
import grid_exp as gx

args = gx.parser(__doc__, steps="training steps / renders between two HIP events").parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_march")
S = gx.Scene(wl, npa, dev, perturb=1., target=True, records=True)
LO, HI, R, N_RAYS, nc, nf = S.LO, S.HI, S.R, S.N_RAYS, S.nc, S.nf
N_C, N_F = 64, 128
MARCH_STEPS = (256, 512, 1024)
opt_two, opt_one = S.adam(nc, nf), S.adam(nf)


def render(grid, mode):
    """mode: None (two networks), "grid", or the march's step count"""
    if mode == "grid":
        return S.render(occupancy=grid, proposal="grid")
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
        if "rays_truncated" in stats:
            rows[name]["rays_truncated"] = stats["rays_truncated"]
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
gx.emit(result, args.out)
