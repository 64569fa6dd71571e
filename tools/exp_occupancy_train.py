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
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this commit", help="what --root is, for the record")
ap.add_argument("--out", default=None)
ap.add_argument("--trace", action="store_true", help="a short untimed run (dense and share 0.25) for a profiler")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=10, help="training steps between two HIP events")
ap.add_argument("--psnr-run", type=int, default=0, metavar="STEPS",
                help="instead of the timing: fit a student to a teacher scene for STEPS steps with and without a DensityGrid "
                     "(defaults of the class) and report held-out PSNR and the evaluated share over time")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
import workloads as wl  # noqa: E402
import nerf_pytorch_amd as npa  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("exp_occupancy_train: needs the GPU (no timing without one)")
hb = npa.hip_backend
dev = torch.device("cuda", 0)
HAVE_GRID = hasattr(npa, "DensityGrid")
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
rays = wl.lego_batch(N_RAYS, seed=1).to(dev)
target = torch.rand(N_RAYS, 3, generator=torch.Generator().manual_seed(2)).to(dev)
opt = npa.FlatAdam(list(nc.parameters()) + list(nf.parameters()), lr=0.0)


def render(grid):
    kw = dict(KW, occupancy=grid) if grid is not None else KW
    return npa.render(H, W, K, chunk=32768, rays=rays, ndc=False, near=2., far=6., use_viewdirs=True, **kw)


def step(grid):
    rgb, _, _, extras = render(grid)
    loss = npa.img2mse(rgb, target) + npa.img2mse(extras["rgb0"], target)
    opt.zero_grad()
    loss.backward()
    opt.step()


def ball(radius):
    c = LO[0] + (torch.arange(R, dtype=torch.float64) + 0.5) * (HI[0] - LO[0]) / R
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    return npa.DensityGrid.from_mask((x * x + y * y + z * z) <= radius * radius, LO, HI, outside="skip", device=dev)


def share_of(grid):
    torch.manual_seed(0)
    with torch.no_grad():
        render(grid)
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


def time_all(configs, k, reps):
    """alternate the configurations inside every repetition; HIP events around k steps each"""
    times = {name: [] for name, _ in configs}
    for name, grid in configs:
        for _ in range(3):
            step(grid)
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, grid in configs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                step(grid)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / k)
    rows = {}
    for name, grid in configs:
        ms = statistics.median(times[name])
        rows[name] = {"ms_median": ms, "ms_min": min(times[name]), "ms_max": max(times[name]), "rays_per_s": N_RAYS / ms * 1e3}
        if grid is None:
            rows[name].update(evaluated_share=1.0, saved_activation_bytes=hb.saved_bytes(N_RAYS, 64, 128, "fp16x3"))
            continue
        # a separate step with HIP events around every launch, and the save buffers the forward leases
        leased, exact = [], []
        fwd, timer = hb.field_fwd, hb.TIMER

        def counted(packed, r_, z_, *a, **kw):
            if kw.get("act") is not None:
                leased.append(4 * kw["act"].numel())
                exact.append(4 * hb.act_floats(r_.shape[0], z_.shape[1], "fp16x3"))
            return fwd(packed, r_, z_, *a, **kw)
        hb.field_fwd, hb.TIMER = counted, hb.KernelTimer()
        try:
            step(grid)
            summ = hb.TIMER.summary()
        finally:
            hb.field_fwd, hb.TIMER = fwd, timer
        rows[name].update(evaluated_share=grid.last_stats["evaluated"] / grid.last_stats["total"], points=grid.last_stats["total"],
                          saved_activation_bytes=sum(leased), saved_activation_bytes_exact=sum(exact),
                          occ_kernels_ms=sum(v["ms"] for kname, v in summ.items() if kname.startswith("occ_")),
                          field_ms=sum(v["ms"] for kname, v in summ.items() if kname.startswith(("field_", "wgrad"))),
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
    Tc, Tf = wl.scene_params(seed=5)
    Pc, Pf = wl.scene_params(seed=6)
    tc, tf = npa.NeRF(**kwn).to(dev), npa.NeRF(**kwn).to(dev)
    tc.load_state_dict(Tc)
    tf.load_state_dict(Tf)
    geo = dict(chunk=32768, ndc=False, near=2., far=6., use_viewdirs=True)
    tkw = dict(KW, network_fn=tc, network_fine=tf, perturb=0.)
    held = wl.lego_batch(N_RAYS, seed=10 ** 6).to(dev)
    with torch.no_grad():
        held_target = npa.render(H, W, K, rays=held, **geo, **tkw)[0]
    runs = {}
    # third run: the threshold set, at the grid's first update, to the median of the densities it has just seen (half of the cells stay)
    for label, use_grid, quantile in (("no grid", False, None),
                                      ("DensityGrid (defaults: decay 0.95, sigma > 0.01, every 16 steps after 256)", True, None),
                                      ("DensityGrid, sigma_threshold = median density at the first update", True, 0.5)):
        if use_grid and not HAVE_GRID:
            continue
        nc.load_state_dict(Pc)
        nf.load_state_dict(Pf)
        adam = npa.FlatAdam(list(nc.parameters()) + list(nf.parameters()), lr=5e-4)
        grid = npa.DensityGrid(LO, HI, R, device=dev) if use_grid else None
        torch.manual_seed(7)
        log = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for it in range(args.psnr_run + 1):
            if it % 250 == 0:
                with torch.no_grad():
                    rgb = npa.render(H, W, K, rays=held, **geo, **dict(KW, perturb=0.))[0]
                    row = {"step": it, "held_out_psnr_db": float(wl.psnr(npa.img2mse(rgb, held_target)))}
                    if grid is not None:
                        rgb_g = npa.render(H, W, K, rays=held, **geo, **dict(KW, perturb=0., occupancy=grid))[0]
                        row.update(held_out_psnr_db_rendered_through_the_grid=float(wl.psnr(npa.img2mse(rgb_g, held_target))),
                                   fraction_occupied=grid.fraction_occupied(), sigma_threshold=grid.sigma_threshold,
                                   evaluated_share=grid.last_stats["evaluated"] / grid.last_stats["total"])
                log.append(row)
            if it == args.psnr_run:
                break
            batch = wl.lego_batch(N_RAYS, seed=it).to(dev)
            with torch.no_grad():
                tgt = npa.render(H, W, K, rays=batch, **geo, **tkw)[0]
            kw = dict(KW)
            if grid is not None:
                if grid.maybe_update(nf, it) and quantile is not None and grid.n_updates == 1:
                    grid.sigma_threshold = float(grid.density.quantile(quantile))
                    grid.bits = hb.occ_mark(grid.density, 1, grid.sigma_threshold, torch.empty_like(grid.bits))
                kw["occupancy"] = grid
            rgb, _, _, extras = npa.render(H, W, K, rays=batch, **geo, **kw)
            loss = npa.img2mse(rgb, tgt) + npa.img2mse(extras["rgb0"], tgt)
            adam.zero_grad()
            loss.backward()
            adam.step()
        e1.record()
        torch.cuda.synchronize()
        runs[label] = {"wall_s_including_teacher_renders_and_evaluations": e0.elapsed_time(e1) / 1e3, "log": log}
    text = json.dumps({"precision": "fp16x3", "rays_per_step": N_RAYS, "steps": args.psnr_run, "tree": args.label, "lr": 5e-4,
                       "task": "student scene_params(seed=6) fitted to the scene of scene_params(seed=5) (the pair of bench.py --long), fresh lego_batch "
                               "every step, held-out batch of 4096 rays",
                       "runs": runs}, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
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
    ts = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.update(nf)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    result["update_128_cubed"] = {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "cells": g.n_cells,
                                  "ms_per_step_at_update_every_16": statistics.median(ts) / 16.0}
text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
