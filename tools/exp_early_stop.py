"""render(early_stop_eps=eps) -- the refining pass stopped where the coarse pass's transmittance estimate falls below eps -- against the
same call with early_stop_eps=None, in the same run (fp16x3, 4096 rays x (64 + 128) samples, DensityGrid at 128^3).

The scene has SURFACES, which the fixture fogs do not: both fixture networks get a constant on the density head's bias (--opaque,
default 60: the density before the ReLU is positive and large everywhere) and the grid is a ball mask with the outside skipped, so a
ray sees empty space, then an opaque ball.  The grid carries the densities of one update() on the fine network (bits stay the mask's),
which is what proposal="grid" reads.  Sweep: eps in {1e-4, 1e-3, 1e-2} and None, with and without proposal="grid".  Per row:
  * the refining pass's evaluated points and their share of n * (64 + 128), the rays stopped;
  * ms of the no_grad render and of the whole TRAINING step (forward, img2mse (two without the proposal), backward, FlatAdam.step with
    lr = 0): median of --reps alternating repetitions, min and max = the spread;
  * the PSNR of the stopped image against the unstopped one (same depths: perturb = 0 for that render).
And nerf_occ_stop_depth / nerf_occ_compact_stop alone (HIP events around 100 launches) next to nerf_occ_compact.

    python tools/exp_early_stop.py --out profiles/r13_exp_early_stop.json
    python tools/exp_early_stop.py --root <checkout of the parent commit> --label "parent commit" --out ...      # its rows with the option off
"""
import inspect

import grid_exp as gx

ap = gx.parser(__doc__, steps="training steps / renders between two HIP events")
ap.add_argument("--radius", type=float, default=1.0, help="radius of the opaque ball")
ap.add_argument("--opaque", type=float, default=60.0, help="constant added to both networks' density-head bias")
args = ap.parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_early_stop")
HAVE_STOP = "early_stop_eps" in inspect.signature(npa.render_rays).parameters
S = gx.Scene(wl, npa, dev, perturb=1., target=True, records=True)
LO, HI, R, N_RAYS, nc, nf = S.LO, S.HI, S.R, S.N_RAYS, S.nc, S.nf
N_C, N_F = 64, 128
with torch.no_grad():
    nc.alpha_linear.bias += args.opaque
    nf.alpha_linear.bias += args.opaque
opt_two, opt_one = S.adam(nc, nf), S.adam(nf)

grid = S.ball(npa.DensityGrid, args.radius)
with torch.no_grad():
    grid.density = npa.DensityGrid(LO, HI, R, device=dev).update(nf).density


def render(eps, proposal, **over):
    if proposal:
        over["proposal"] = "grid"
    if eps is not None:
        over["early_stop_eps"] = eps
    return S.render(occupancy=grid, **over)


def step(eps, proposal):
    S.fit(render(eps, proposal), opt_one if proposal else opt_two, rgb0=not proposal)


def infer(eps, proposal):
    with torch.no_grad():
        render(eps, proposal)


def time_all(fn, configs, k, reps):
    """alternate the configurations inside every repetition; HIP events around k calls each"""
    times = gx.time_alternating([(name, lambda e=e, p=p: fn(e, p)) for name, e, p in configs], k, reps, warmup=3)
    rows = {}
    for name, eps, proposal in configs:
        rows[name] = gx.row_stats(times[name], N_RAYS)
        summ = gx.kernel_summary(hb, lambda: fn(eps, proposal))      # a separate call with HIP events around every launch
        with torch.no_grad():       # the counts at perturb = 0, where the coarse pass's own count is known (coarse_evaluated)
            render(eps, proposal, perturb=0.)
        refine = grid.last_stats["evaluated"] - (0 if proposal else coarse_evaluated[0])
        rows[name].update(evaluated=grid.last_stats["evaluated"], total=grid.last_stats["total"], rays_stopped=grid.last_stats.get("rays_stopped"),
                          refining_pass_evaluated=refine, refining_pass_share=refine / (N_RAYS * (N_C + N_F)),
                          occ_kernels_ms=gx.kernel_ms(summ, "occ_"), stop_depth_ms=gx.kernel_ms(summ, "occ_stop_depth"),
                          field_ms=gx.kernel_ms(summ, ("field_", "wgrad")))
    return rows


def psnr_vs_unstopped(eps, proposal):
    with torch.no_grad():
        a = render(eps, proposal, perturb=0.)[0]
        b = render(None, proposal, perturb=0.)[0]
    return {"psnr_db": gx.psnr_db(a, b), "max_abs_difference": float((a - b).abs().max())}


# the coarse pass's evaluated points (the stop never touches it): the two-network render with N_importance = 0
with torch.no_grad():
    S.render(occupancy=grid, N_importance=0, network_fine=None, perturb=0.)
coarse_evaluated = [grid.last_stats["evaluated"]]

result = {"precision": "fp16x3", "rays": N_RAYS, "samples": "64 + 128", "grid_resolution": R, "tree": args.label, "have_early_stop": HAVE_STOP,
          "scene": f"fixture networks with {args.opaque} added to the density-head bias, ball mask r = {args.radius}, outside skipped",
          "fraction_occupied": grid.fraction_occupied(), "coarse_pass_evaluated_perturb_0": coarse_evaluated[0],
          "step": "render() forward, img2mse (two without the proposal), backward, FlatAdam.step (lr = 0)", "calls_per_timing": args.steps}
configs = []
for proposal in (False, True):
    tag = ", proposal=grid" if proposal else ", two networks"
    configs.append(("early_stop_eps=None" + tag, None, proposal))
    if HAVE_STOP:
        configs += [(f"early_stop_eps={eps:g}" + tag, eps, proposal) for eps in (1e-4, 1e-3, 1e-2)]
result["no_grad_render_4096_rays"] = time_all(infer, configs, args.steps, args.reps)
result["train_step_4096_rays"] = time_all(step, configs, args.steps, args.reps)
if HAVE_STOP:
    result["image_vs_unstopped_perturb_0"] = {name: psnr_vs_unstopped(eps, proposal) for name, eps, proposal in configs if eps is not None}
    # the two new launches alone, on the refining pass's own inputs
    rec = S.records
    z_c = hb.sample_coarse(rec, torch.linspace(0., 1., N_C, device=dev), False, None)
    w = grid.proposal_weights(rec, z_c)
    z_f = hb.sample_fine(z_c, w, N_F, None, torch.linspace(0., 1., N_F, device=dev))[0]
    z_stop = hb.occ_stop_depth(z_c, w, 1e-3)
    desc = grid._desc()
    slot_ws, rec_ws = torch.empty(N_RAYS * (N_C + N_F), device=dev), torch.empty(11 * N_RAYS * (N_C + N_F), device=dev)
    launches = {"nerf_occ_stop_depth (4096 x 64)": lambda: hb.occ_stop_depth(z_c, w, 1e-3),
                "nerf_occ_compact (4096 x 192)": lambda: hb.occ_compact(desc, rec, z_f, slot_ws, rec_ws),
                "nerf_occ_compact_stop (4096 x 192)": lambda: hb.occ_compact(desc, rec, z_f, slot_ws, rec_ws, z_stop)}
    alone = {name: dict(gx.time_launches(fn, args.reps), note="host-timed back-to-back calls (allocation of the small outputs included)")
             for name, fn in launches.items()}
    alone["rays_stopped_at_1e-3"] = int(torch.isfinite(z_stop).sum())
    result["launches_alone"] = alone
gx.emit(result, args.out)
