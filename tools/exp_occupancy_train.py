"""The TRAINING step through render() with a DensityGrid against the same step without one (fp16x3, 4096 rays x (64 + 128) samples):
forward, two img2mse, backward, FlatAdam.step.  Grids: all-occupied, the ball masks of tools/exp_occupancy.py bisected to evaluated
shares of about 0.5 / 0.25 / 0.1 (outside skipped), and a DensityGrid updated once from the scene_params networks.  Per row: ms (median
of --reps alternating repetitions, min and max = the spread), rays/s, the evaluated share, the bytes of saved activations the step
leases (and what M points need exactly), the time of the occupancy launches.  Also: one full update() of the 128^3 grid.
The learning rate is 0: the optimizer does all of its work, the fragment repack follows every step as in training, and the scene -- so
every share -- stays what the bisection found.

    python tools/exp_occupancy_train.py --out profiles/r10_exp_occupancy_train.json
    python tools/exp_occupancy_train.py --root <checkout of the parent commit> --label "parent commit" --out profiles/r10_exp_occupancy_train_parent.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/exp_occupancy_train.py --trace     # a short run for the kernel table
    python tools/exp_occupancy_train.py --psnr-run 2000 --out profiles/r10_exp_occupancy_train_run.json   # a measurement, not a gate
(a tree without DensityGrid times the dense row only)
"""
import sys

import grid_exp as gx

ap = gx.parser(__doc__, steps="training steps between two HIP events", trace="a short untimed run (dense and share 0.25) for a profiler")
ap.add_argument("--psnr-run", type=int, default=0, metavar="STEPS",
                help="instead of the timing: fit a student to a teacher scene for STEPS steps with and without a DensityGrid "
                     "(defaults of the class) and report held-out PSNR and the evaluated share over time")
args = ap.parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_occupancy_train")
HAVE_GRID = hasattr(npa, "DensityGrid")
S = gx.Scene(wl, npa, dev, perturb=1., target=True)
LO, HI, R, N_RAYS, nc, nf = S.LO, S.HI, S.R, S.N_RAYS, S.nc, S.nf
opt = S.adam(nc, nf)


def render(grid):
    return S.render(**(dict(occupancy=grid) if grid is not None else {}))


def step(grid):
    S.fit(render(grid), opt, rgb0=True)


def share_of(grid):
    torch.manual_seed(0)
    with torch.no_grad():
        render(grid)
    return gx.evaluated_share(grid)


def ball_with_share(want):
    return S.ball_with_share(npa.DensityGrid, share_of, want)


def time_all(configs, k, reps):
    """alternate the configurations inside every repetition; HIP events around k steps each"""
    times = gx.time_alternating([(name, lambda grid=grid: step(grid)) for name, grid in configs], k, reps, warmup=3)
    rows = {}
    for name, grid in configs:
        rows[name] = gx.row_stats(times[name], N_RAYS)
        if grid is None:
            rows[name].update(evaluated_share=1.0, saved_activation_bytes=hb.saved_bytes(N_RAYS, 64, 128, "fp16x3"))
            continue
        # a separate step with HIP events around every launch, and the save buffers the forward leases
        leased, exact = [], []
        fwd = hb.field_fwd

        def counted(packed, r_, z_, *a, **kw):
            if kw.get("act") is not None:
                leased.append(4 * kw["act"].numel())
                exact.append(4 * hb.act_floats(r_.shape[0], z_.shape[1], "fp16x3"))
            return fwd(packed, r_, z_, *a, **kw)
        hb.field_fwd = counted
        try:
            summ = gx.kernel_summary(hb, lambda: step(grid))
        finally:
            hb.field_fwd = fwd
        rows[name].update(evaluated_share=gx.evaluated_share(grid), points=grid.last_stats["total"],
                          saved_activation_bytes=sum(leased), saved_activation_bytes_exact=sum(exact),
                          occ_kernels_ms=gx.kernel_ms(summ, "occ_"), field_ms=gx.kernel_ms(summ, ("field_", "wgrad")),
                          fraction_occupied=grid.fraction_occupied())
    return rows


if args.trace:
    configs = [None] + ([ball_with_share(0.25)[0]] if HAVE_GRID else [])
    for _ in range(5):
        for g in configs:
            step(g)
    torch.cuda.synchronize()
    sys.exit(0)

if args.psnr_run > 0:
    # the converging pair of bench.py --long: a student that starts as scene_params(seed=6) is fitted to the scene of
    # scene_params(seed=5); fresh batches every step, targets = the teacher's no_grad render of the same rays, Adam 5e-4; held out: a
    # batch never trained on
    tkw, (Pc, Pf), held, held_target = S.teacher_and_held_out()
    runs = {}
    # third run: the threshold set, at the grid's first update, to the median of the densities it has just seen (half of the cells stay)
    for label, use_grid, quantile in (("no grid", False, None),
                                      ("DensityGrid (defaults: decay 0.95, sigma > 0.01, every 16 steps after 256)", True, None),
                                      ("DensityGrid, sigma_threshold = median density at the first update", True, 0.5)):
        if use_grid and not HAVE_GRID:
            continue
        nc.load_state_dict(Pc)
        nf.load_state_dict(Pf)
        adam = S.adam(nc, nf, lr=5e-4)
        grid = npa.DensityGrid(LO, HI, R, device=dev) if use_grid else None
        torch.manual_seed(7)
        log = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for it in range(args.psnr_run + 1):
            if it % 250 == 0:
                with torch.no_grad():
                    rgb = S.render(held, perturb=0.)[0]
                    row = {"step": it, "held_out_psnr_db": float(wl.psnr(npa.img2mse(rgb, held_target)))}
                    if grid is not None:
                        rgb_g = S.render(held, perturb=0., occupancy=grid)[0]
                        row.update(held_out_psnr_db_rendered_through_the_grid=float(wl.psnr(npa.img2mse(rgb_g, held_target))),
                                   fraction_occupied=grid.fraction_occupied(), sigma_threshold=grid.sigma_threshold,
                                   evaluated_share=gx.evaluated_share(grid))
                log.append(row)
            if it == args.psnr_run:
                break
            batch = wl.lego_batch(N_RAYS, seed=it).to(dev)
            with torch.no_grad():
                tgt = S.render(batch, **tkw)[0]
            kw = {}
            if grid is not None:
                if grid.maybe_update(nf, it) and quantile is not None and grid.n_updates == 1:
                    grid.sigma_threshold = float(grid.density.quantile(quantile))
                    grid.bits = hb.occ_mark(grid.density, 1, grid.sigma_threshold, torch.empty_like(grid.bits))
                kw["occupancy"] = grid
            rgb, _, _, extras = S.render(batch, **kw)
            loss = npa.img2mse(rgb, tgt) + npa.img2mse(extras["rgb0"], tgt)
            adam.zero_grad()
            loss.backward()
            adam.step()
        e1.record()
        torch.cuda.synchronize()
        runs[label] = {"wall_s_including_teacher_renders_and_evaluations": e0.elapsed_time(e1) / 1e3, "log": log}
    gx.emit({"precision": "fp16x3", "rays_per_step": N_RAYS, "steps": args.psnr_run, "tree": args.label, "lr": 5e-4,
             "task": "student scene_params(seed=6) fitted to the scene of scene_params(seed=5) (the pair of bench.py --long), fresh lego_batch "
                     "every step, held-out batch of 4096 rays",
             "runs": runs}, args.out)
    sys.exit(0)

result = {"precision": "fp16x3", "rays": N_RAYS, "samples": "64 + 128", "grid_resolution": R if HAVE_GRID else None, "tree": args.label,
          "have_density_grid": HAVE_GRID, "step": "render() forward, two img2mse, backward, FlatAdam.step (lr = 0)", "steps_per_timing": args.steps}
configs = [("dense (no grid)", None)]
if HAVE_GRID:
    configs.append(("DensityGrid share 1.0 (all occupied)", npa.DensityGrid(LO, HI, R, device=dev)))
    for want in (0.5, 0.25, 0.1):
        g, radius = ball_with_share(want)
        configs.append((f"DensityGrid share {want} (ball r = {radius:.3f}, outside skipped)", g))
    net_grid = npa.DensityGrid(LO, HI, R, device=dev).update(nf)
    configs.append(("DensityGrid.update(network_fine) (sigma > 0.01, dilate 0)", net_grid))
result["train_step_4096_rays"] = time_all(configs, args.steps, args.reps)
if HAVE_GRID:
    g = npa.DensityGrid(LO, HI, R, device=dev)
    g.update(nf)
    ts = gx.time_alternating([("update", lambda: g.update(nf))], 1, args.reps, warmup=0)["update"]
    stats = gx.row_stats(ts)
    result["update_128_cubed"] = dict(stats, cells=g.n_cells, ms_per_step_at_update_every_16=stats["ms_median"] / 16.0)
gx.emit(result, args.out)
