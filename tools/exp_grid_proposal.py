"""render(proposal="grid") -- importance samples drawn from the DensityGrid's own densities, one network evaluated -- against the same
call without it, on the same DensityGrid (fp16x3, 4096 rays x (64 + 128) samples):
  * the whole TRAINING step (forward, img2mse, backward, FlatAdam.step) and the no_grad render, at the evaluated shares of
    tools/exp_occupancy_train.py: all-occupied and the ball masks bisected to about 0.5 / 0.25 / 0.1 (outside skipped).  Every grid
    carries the densities of one update() on the fine network (the bits stay the mask's).  The two-network step has two losses and an
    optimizer over both networks; the proposal step has one loss and an optimizer over the evaluated network -- each what a user runs;
  * nerf_occ_proposal_weights alone at 128^3 (HIP events around 100 launches).
Per row: ms (median of --reps alternating repetitions, min and max = the spread), the evaluated points, field and occupancy kernel ms.
The learning rate is 0 (the optimizer does all of its work; the scene and every share stay put).

    python tools/exp_grid_proposal.py --out profiles/r12_exp_grid_proposal.json
    python tools/exp_grid_proposal.py --root <checkout of the parent commit> --label "parent commit" --out ...   # its rows without the option
    python tools/exp_grid_proposal.py --psnr-run 2000 --out profiles/r12_exp_grid_proposal_run.json              # a record, not a gate
"""
import inspect

import grid_exp as gx

ap = gx.parser(__doc__, steps="training steps / renders between two HIP events")
ap.add_argument("--psnr-run", type=int, default=0, metavar="STEPS",
                help="instead of the timing: fit a student to a teacher scene for STEPS steps through a DensityGrid (class defaults, "
                     "maybe_update every step) once with two networks and once with proposal=\"grid\"; report held-out PSNR")
args = ap.parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_grid_proposal")
HAVE_PROPOSAL = "proposal" in inspect.signature(npa.render_rays).parameters
S = gx.Scene(wl, npa, dev, perturb=1., target=True, records=True)
LO, HI, R, N_RAYS, nc, nf = S.LO, S.HI, S.R, S.N_RAYS, S.nc, S.nf
opt_two, opt_one = S.adam(nc, nf), S.adam(nf)


def render(grid, proposal, batch=None, **over):
    if proposal:
        over["proposal"] = "grid"
    return S.render(batch, occupancy=grid, **over)


def step(grid, proposal):
    S.fit(render(grid, proposal), opt_one if proposal else opt_two, rgb0=not proposal)


def infer(grid, proposal):
    with torch.no_grad():
        render(grid, proposal)


def share_of(grid):
    torch.manual_seed(0)
    infer(grid, False)
    return gx.evaluated_share(grid)


def time_all(fn, configs, k, reps):
    """alternate the configurations inside every repetition; HIP events around k calls each"""
    times = gx.time_alternating([(name, lambda g=g, p=p: fn(g, p)) for name, g, p in configs], k, reps, warmup=3)
    rows = {}
    for name, grid, proposal in configs:
        rows[name] = gx.row_stats(times[name], N_RAYS)
        summ = gx.kernel_summary(hb, lambda: fn(grid, proposal))      # a separate call with HIP events around every launch
        rows[name].update(evaluated=grid.last_stats["evaluated"], total=grid.last_stats["total"],
                          occ_kernels_ms=gx.kernel_ms(summ, "occ_"), field_ms=gx.kernel_ms(summ, ("field_", "wgrad")))
    return rows


if args.psnr_run > 0:
    # the converging pair of bench.py --long (tools/exp_occupancy_train.py --psnr-run): a student that starts as scene_params(seed=6) is
    # fitted to the scene of scene_params(seed=5); fresh batches every step, targets = the teacher's no_grad render of the same rays,
    # Adam 5e-4; held out: a batch never trained on, rendered the way the run trains
    tkw, (Sc, Sf), held, held_target = S.teacher_and_held_out()
    runs = {}
    for label, proposal in (("two networks through the DensityGrid", False), ("proposal=\"grid\": the fine network alone", True)):
        if proposal and not HAVE_PROPOSAL:
            continue
        nc.load_state_dict(Sc)
        nf.load_state_dict(Sf)
        adam = S.adam(nf, *([] if proposal else [nc]), lr=5e-4)
        grid = npa.DensityGrid(LO, HI, R, device=dev)
        torch.manual_seed(7)
        log = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for it in range(args.psnr_run + 1):
            if it % 250 == 0:
                with torch.no_grad():
                    rgb = render(grid, proposal, held, perturb=0.)[0]
                log.append({"step": it, "held_out_psnr_db": float(wl.psnr(npa.img2mse(rgb, held_target))),
                            "fraction_occupied": grid.fraction_occupied(),
                            "evaluated_share": gx.evaluated_share(grid)})
            if it == args.psnr_run:
                break
            batch = wl.lego_batch(N_RAYS, seed=it).to(dev)
            with torch.no_grad():
                tgt = S.render(batch, **tkw)[0]
            grid.maybe_update(nf, it)
            rgb, _, _, extras = render(grid, proposal, batch)
            loss = npa.img2mse(rgb, tgt)
            if not proposal:
                loss = loss + npa.img2mse(extras["rgb0"], tgt)
            adam.zero_grad()
            loss.backward()
            adam.step()
        e1.record()
        torch.cuda.synchronize()
        runs[label] = {"wall_s_including_teacher_renders_and_evaluations": e0.elapsed_time(e1) / 1e3, "grid_updates": grid.n_updates, "log": log}
    result = {"precision": "fp16x3", "rays_per_step": N_RAYS, "steps": args.psnr_run, "tree": args.label, "lr": 5e-4,
              "task": "student scene_params(seed=6) fitted to the scene of scene_params(seed=5) (the pair of bench.py --long), fresh lego_batch "
                      "every step, DensityGrid 128^3 with the class defaults and maybe_update every step, held-out batch of 4096 rays "
                      "rendered the way the run trains",
              "runs": runs}
else:
    result = {"precision": "fp16x3", "rays": N_RAYS, "samples": "64 + 128", "grid_resolution": R, "tree": args.label, "have_proposal": HAVE_PROPOSAL,
              "step": "render() forward, img2mse (two without the option), backward, FlatAdam.step (lr = 0)", "calls_per_timing": args.steps}
    with torch.no_grad():
        density = npa.DensityGrid(LO, HI, R, device=dev).update(nf).density
    grids = [("share 1.0 (all occupied)", npa.DensityGrid(LO, HI, R, device=dev))]
    for want in (0.5, 0.25, 0.1):
        g, radius = S.ball_with_share(npa.DensityGrid, share_of, want)
        grids.append((f"share {want} (ball r = {radius:.3f}, outside skipped)", g))
    configs = []
    for name, g in grids:
        g.density = density.clone()
        configs.append((name + ", two networks", g, False))
        if HAVE_PROPOSAL:
            configs.append((name + ", proposal=grid", g, True))
    result["train_step_4096_rays"] = time_all(step, configs, args.steps, args.reps)
    result["no_grad_render_4096_rays"] = time_all(infer, configs, args.steps, args.reps)
    if HAVE_PROPOSAL:
        g = grids[2][1]
        rays_rec = S.records
        z = hb.sample_coarse(rays_rec, torch.linspace(0., 1., 64, device=dev), False, None)
        P = N_RAYS * 64
        us = gx.time_launches(lambda: g.proposal_weights(rays_rec, z), args.reps)
        result["proposal_weights_kernel_128_cubed"] = dict(us, rays=N_RAYS, samples=64, bytes_model=24 * N_RAYS + 16 * P,
                                                           gbytes_per_s_model=(24 * N_RAYS + 16 * P) / us["us_median"] / 1e3,
                                                           note="host-timed back-to-back launches (allocation of the output included)")
gx.emit(result, args.out)
