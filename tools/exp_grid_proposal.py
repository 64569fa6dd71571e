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
import argparse
import inspect
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this commit", help="what --root is, for the record")
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=10, help="training steps / renders between two HIP events")
ap.add_argument("--psnr-run", type=int, default=0, metavar="STEPS",
                help="instead of the timing: fit a student to a teacher scene for STEPS steps through a DensityGrid (class defaults, "
                     "maybe_update every step) once with two networks and once with proposal=\"grid\"; report held-out PSNR")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
import workloads as wl  # noqa: E402
import nerf_pytorch_amd as npa  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("exp_grid_proposal: needs the GPU (no timing without one)")
hb = npa.hip_backend
dev = torch.device("cuda", 0)
HAVE_PROPOSAL = "proposal" in inspect.signature(npa.render_rays).parameters
Pc, Pf = wl.scene_params()
kwn = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
nc, nf = npa.NeRF(**kwn).to(dev), npa.NeRF(**kwn).to(dev)
nc.load_state_dict(Pc)
nf.load_state_dict(Pf)
npa.set_precision("fp16x3")
LO, HI, R = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), 128
N_RAYS = 4096
KW = dict(network_fn=nc, network_query_fn=None, N_samples=64, N_importance=128, network_fine=nf, perturb=1., white_bkgd=True, raw_noise_std=0.)
H = W = 800
K = wl.intrinsics(dict(H=H, W=W, focal=1111.0))
GEO = dict(chunk=32768, ndc=False, near=2., far=6., use_viewdirs=True)
rays = wl.lego_batch(N_RAYS, seed=1).to(dev)
target = torch.rand(N_RAYS, 3, generator=torch.Generator().manual_seed(2)).to(dev)
opt_two = npa.FlatAdam(list(nc.parameters()) + list(nf.parameters()), lr=0.0)
opt_one = npa.FlatAdam(list(nf.parameters()), lr=0.0)


def render(grid, proposal, batch=rays, **over):
    kw = dict(KW, occupancy=grid, **over)
    if proposal:
        kw["proposal"] = "grid"
    return npa.render(H, W, K, rays=batch, **GEO, **kw)


def step(grid, proposal):
    rgb, _, _, extras = render(grid, proposal)
    loss = npa.img2mse(rgb, target)
    if not proposal:
        loss = loss + npa.img2mse(extras["rgb0"], target)
    opt = opt_one if proposal else opt_two
    opt.zero_grad()
    loss.backward()
    opt.step()


def infer(grid, proposal):
    with torch.no_grad():
        render(grid, proposal)


def ball(radius):
    c = LO[0] + (torch.arange(R, dtype=torch.float64) + 0.5) * (HI[0] - LO[0]) / R
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    return npa.DensityGrid.from_mask((x * x + y * y + z * z) <= radius * radius, LO, HI, outside="skip", device=dev)


def share_of(grid, proposal=False):
    torch.manual_seed(0)
    infer(grid, proposal)
    return grid.last_stats["evaluated"] / grid.last_stats["total"]


def ball_with_share(want):
    lo, hi = 0.0, 4.0
    for _ in range(14):
        mid = 0.5 * (lo + hi)
        if share_of(ball(mid)) < want:
            lo = mid
        else:
            hi = mid
    return ball(hi), hi


def time_all(fn, configs, k, reps):
    """alternate the configurations inside every repetition; HIP events around k calls each"""
    times = {name: [] for name, _, _ in configs}
    for _, grid, proposal in configs:
        for _ in range(3):
            fn(grid, proposal)
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, grid, proposal in configs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                fn(grid, proposal)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / k)
    rows = {}
    for name, grid, proposal in configs:
        ms = statistics.median(times[name])
        rows[name] = {"ms_median": ms, "ms_min": min(times[name]), "ms_max": max(times[name]), "rays_per_s": N_RAYS / ms * 1e3}
        timer = hb.TIMER
        hb.TIMER = hb.KernelTimer()         # a separate call with HIP events around every launch
        try:
            fn(grid, proposal)
            summ = hb.TIMER.summary()
        finally:
            hb.TIMER = timer
        rows[name].update(evaluated=grid.last_stats["evaluated"], total=grid.last_stats["total"],
                          occ_kernels_ms=sum(v["ms"] for kname, v in summ.items() if kname.startswith("occ_")),
                          field_ms=sum(v["ms"] for kname, v in summ.items() if kname.startswith(("field_", "wgrad"))))
    return rows


if args.psnr_run > 0:
    # the converging pair of bench.py --long (tools/exp_occupancy_train.py --psnr-run): a student that starts as scene_params(seed=6) is
    # fitted to the scene of scene_params(seed=5); fresh batches every step, targets = the teacher's no_grad render of the same rays,
    # Adam 5e-4; held out: a batch never trained on, rendered the way the run trains
    Tc, Tf = wl.scene_params(seed=5)
    Sc, Sf = wl.scene_params(seed=6)
    tc, tf = npa.NeRF(**kwn).to(dev), npa.NeRF(**kwn).to(dev)
    tc.load_state_dict(Tc)
    tf.load_state_dict(Tf)
    tkw = dict(KW, network_fn=tc, network_fine=tf, perturb=0.)
    held = wl.lego_batch(N_RAYS, seed=10 ** 6).to(dev)
    with torch.no_grad():
        held_target = npa.render(H, W, K, rays=held, **GEO, **tkw)[0]
    runs = {}
    for label, proposal in (("two networks through the DensityGrid", False), ("proposal=\"grid\": the fine network alone", True)):
        if proposal and not HAVE_PROPOSAL:
            continue
        nc.load_state_dict(Sc)
        nf.load_state_dict(Sf)
        adam = npa.FlatAdam(list(nf.parameters()) + ([] if proposal else list(nc.parameters())), lr=5e-4)
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
                            "evaluated_share": grid.last_stats["evaluated"] / grid.last_stats["total"]})
            if it == args.psnr_run:
                break
            batch = wl.lego_batch(N_RAYS, seed=it).to(dev)
            with torch.no_grad():
                tgt = npa.render(H, W, K, rays=batch, **GEO, **tkw)[0]
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
        g, radius = ball_with_share(want)
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
        rays_rec = wl.synthetic_rays(N_RAYS, 1).to(dev).contiguous()       # (the records render() makes of `rays`)
        z = hb.sample_coarse(rays_rec, torch.linspace(0., 1., 64, device=dev), False, None)
        ts = []
        for _ in range(3):
            g.proposal_weights(rays_rec, z)
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100):
                g.proposal_weights(rays_rec, z)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 100 * 1e3)
        P = N_RAYS * 64
        us = statistics.median(ts)
        result["proposal_weights_kernel_128_cubed"] = {"us_median": us, "us_min": min(ts), "us_max": max(ts), "rays": N_RAYS, "samples": 64,
                                                       "bytes_model": 24 * N_RAYS + 16 * P, "gbytes_per_s_model": (24 * N_RAYS + 16 * P) / us / 1e3,
                                                       "note": "host-timed back-to-back launches (allocation of the output included)"}
text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
