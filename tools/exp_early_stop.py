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
import argparse
import inspect
import json
import math
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this commit", help="what --root is, for the record")
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=10, help="training steps / renders between two HIP events")
ap.add_argument("--radius", type=float, default=1.0, help="radius of the opaque ball")
ap.add_argument("--opaque", type=float, default=60.0, help="constant added to both networks' density-head bias")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
import workloads as wl  # noqa: E402
import nerf_pytorch_amd as npa  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("exp_early_stop: needs the GPU (no timing without one)")
hb = npa.hip_backend
dev = torch.device("cuda", 0)
HAVE_STOP = "early_stop_eps" in inspect.signature(npa.render_rays).parameters
Pc, Pf = wl.scene_params()
kwn = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
nc, nf = npa.NeRF(**kwn).to(dev), npa.NeRF(**kwn).to(dev)
nc.load_state_dict(Pc)
nf.load_state_dict(Pf)
with torch.no_grad():
    nc.alpha_linear.bias += args.opaque
    nf.alpha_linear.bias += args.opaque
npa.set_precision("fp16x3")
LO, HI, R = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), 128
N_RAYS, N_C, N_F = 4096, 64, 128
KW = dict(network_fn=nc, network_query_fn=None, N_samples=N_C, N_importance=N_F, network_fine=nf, perturb=1., white_bkgd=True, raw_noise_std=0.)
H = W = 800
K = wl.intrinsics(dict(H=H, W=W, focal=1111.0))
GEO = dict(chunk=32768, ndc=False, near=2., far=6., use_viewdirs=True)
rays = wl.lego_batch(N_RAYS, seed=1).to(dev)
target = torch.rand(N_RAYS, 3, generator=torch.Generator().manual_seed(2)).to(dev)
opt_two = npa.FlatAdam(list(nc.parameters()) + list(nf.parameters()), lr=0.0)
opt_one = npa.FlatAdam(list(nf.parameters()), lr=0.0)

c = LO[0] + (torch.arange(R, dtype=torch.float64) + 0.5) * (HI[0] - LO[0]) / R
x, y, z = torch.meshgrid(c, c, c, indexing="ij")
grid = npa.DensityGrid.from_mask((x * x + y * y + z * z) <= args.radius ** 2, LO, HI, outside="skip", device=dev)
with torch.no_grad():
    grid.density = npa.DensityGrid(LO, HI, R, device=dev).update(nf).density


def render(eps, proposal, **over):
    kw = dict(KW, occupancy=grid, **over)
    if proposal:
        kw["proposal"] = "grid"
    if eps is not None:
        kw["early_stop_eps"] = eps
    return npa.render(H, W, K, rays=rays, **GEO, **kw)


def step(eps, proposal):
    rgb, _, _, extras = render(eps, proposal)
    loss = npa.img2mse(rgb, target)
    if not proposal:
        loss = loss + npa.img2mse(extras["rgb0"], target)
    opt = opt_one if proposal else opt_two
    opt.zero_grad()
    loss.backward()
    opt.step()


def infer(eps, proposal):
    with torch.no_grad():
        render(eps, proposal)


def time_all(fn, configs, k, reps):
    """alternate the configurations inside every repetition; HIP events around k calls each"""
    times = {name: [] for name, _, _ in configs}
    for _, eps, proposal in configs:
        for _ in range(3):
            fn(eps, proposal)
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, eps, proposal in configs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                fn(eps, proposal)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / k)
    rows = {}
    for name, eps, proposal in configs:
        ms = statistics.median(times[name])
        rows[name] = {"ms_median": ms, "ms_min": min(times[name]), "ms_max": max(times[name]), "rays_per_s": N_RAYS / ms * 1e3}
        timer = hb.TIMER
        hb.TIMER = hb.KernelTimer()         # a separate call with HIP events around every launch
        try:
            fn(eps, proposal)
            summ = hb.TIMER.summary()
        finally:
            hb.TIMER = timer
        with torch.no_grad():       # the counts at perturb = 0, where the coarse pass's own count is known (coarse_evaluated)
            render(eps, proposal, perturb=0.)
        refine = grid.last_stats["evaluated"] - (0 if proposal else coarse_evaluated[0])
        rows[name].update(evaluated=grid.last_stats["evaluated"], total=grid.last_stats["total"], rays_stopped=grid.last_stats.get("rays_stopped"),
                          refining_pass_evaluated=refine, refining_pass_share=refine / (N_RAYS * (N_C + N_F)),
                          occ_kernels_ms=sum(v["ms"] for kname, v in summ.items() if kname.startswith("occ_")),
                          stop_depth_ms=sum(v["ms"] for kname, v in summ.items() if kname.startswith("occ_stop_depth")),
                          field_ms=sum(v["ms"] for kname, v in summ.items() if kname.startswith(("field_", "wgrad"))))
    return rows


def psnr_vs_unstopped(eps, proposal):
    with torch.no_grad():
        a = render(eps, proposal, perturb=0.)[0]
        b = render(None, proposal, perturb=0.)[0]
    mse = float(((a.double() - b.double()) ** 2).mean())
    return {"psnr_db": None if mse == 0.0 else -10.0 * math.log10(mse), "max_abs_difference": float((a - b).abs().max())}


# the coarse pass's evaluated points (the stop never touches it): the two-network render with N_importance = 0
with torch.no_grad():
    npa.render(H, W, K, rays=rays, **GEO, **dict(KW, occupancy=grid, N_importance=0, network_fine=None, perturb=0.))
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
    rec = wl.synthetic_rays(N_RAYS, 1).to(dev).contiguous()
    z_c = hb.sample_coarse(rec, torch.linspace(0., 1., N_C, device=dev), False, None)
    w = grid.proposal_weights(rec, z_c)
    z_f = hb.sample_fine(z_c, w, N_F, None, torch.linspace(0., 1., N_F, device=dev))[0]
    z_stop = hb.occ_stop_depth(z_c, w, 1e-3)
    desc = grid._desc()
    slot_ws, rec_ws = torch.empty(N_RAYS * (N_C + N_F), device=dev), torch.empty(11 * N_RAYS * (N_C + N_F), device=dev)
    launches = {"nerf_occ_stop_depth (4096 x 64)": lambda: hb.occ_stop_depth(z_c, w, 1e-3),
                "nerf_occ_compact (4096 x 192)": lambda: hb.occ_compact(desc, rec, z_f, slot_ws, rec_ws),
                "nerf_occ_compact_stop (4096 x 192)": lambda: hb.occ_compact(desc, rec, z_f, slot_ws, rec_ws, z_stop)}
    alone = {}
    for name, fn in launches.items():
        for _ in range(3):
            fn()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 100 * 1e3)
        alone[name] = {"us_median": statistics.median(ts), "us_min": min(ts), "us_max": max(ts),
                       "note": "host-timed back-to-back calls (allocation of the small outputs included)"}
    alone["rays_stopped_at_1e-3"] = int(torch.isfinite(z_stop).sum())
    result["launches_alone"] = alone
text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
