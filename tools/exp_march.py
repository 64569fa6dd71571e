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
import argparse
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
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
import workloads as wl  # noqa: E402
import nerf_pytorch_amd as npa  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("exp_march: needs the GPU (no timing without one)")
hb = npa.hip_backend
dev = torch.device("cuda", 0)
Pc, Pf = wl.scene_params()
kwn = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
nc, nf = npa.NeRF(**kwn).to(dev), npa.NeRF(**kwn).to(dev)
nc.load_state_dict(Pc)
nf.load_state_dict(Pf)
npa.set_precision("fp16x3")
LO, HI, R = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), 128
N_RAYS, N_C, N_F = 4096, 64, 128
MARCH_STEPS = (256, 512, 1024)
KW = dict(network_fn=nc, network_query_fn=None, N_samples=N_C, N_importance=N_F, network_fine=nf, perturb=1., white_bkgd=True, raw_noise_std=0.)
H = W = 800
K = wl.intrinsics(dict(H=H, W=W, focal=1111.0))
GEO = dict(chunk=32768, ndc=False, near=2., far=6., use_viewdirs=True)
rays = wl.lego_batch(N_RAYS, seed=1).to(dev)
target = torch.rand(N_RAYS, 3, generator=torch.Generator().manual_seed(2)).to(dev)
opt_two = npa.FlatAdam(list(nc.parameters()) + list(nf.parameters()), lr=0.0)
opt_one = npa.FlatAdam(list(nf.parameters()), lr=0.0)


def render(grid, mode):
    """mode: None (two networks), "grid", or the march's step count"""
    kw = dict(KW, occupancy=grid)
    if mode == "grid":
        kw["proposal"] = "grid"
    elif mode is not None:
        kw.update(proposal="march", march_steps=mode)
    return npa.render(H, W, K, rays=rays, **GEO, **kw)


def step(grid, mode):
    rgb, _, _, extras = render(grid, mode)
    loss = npa.img2mse(rgb, target)
    if mode is None:
        loss = loss + npa.img2mse(extras["rgb0"], target)
    opt = opt_two if mode is None else opt_one
    opt.zero_grad()
    loss.backward()
    opt.step()


def infer(grid, mode):
    with torch.no_grad():
        render(grid, mode)


def ball(radius):
    c = LO[0] + (torch.arange(R, dtype=torch.float64) + 0.5) * (HI[0] - LO[0]) / R
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    return npa.DensityGrid.from_mask((x * x + y * y + z * z) <= radius * radius, LO, HI, outside="skip", device=dev)


def share_of(grid):
    torch.manual_seed(0)
    infer(grid, None)
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
    for _, grid, mode in configs:
        for _ in range(3):
            fn(grid, mode)
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, grid, mode in configs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                fn(grid, mode)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / k)
    rows = {}
    for name, grid, mode in configs:
        ms = statistics.median(times[name])
        rows[name] = {"ms_median": ms, "ms_min": min(times[name]), "ms_max": max(times[name]), "rays_per_s": N_RAYS / ms * 1e3}
        timer = hb.TIMER
        hb.TIMER = hb.KernelTimer()         # a separate call with HIP events around every launch
        try:
            fn(grid, mode)
            summ = hb.TIMER.summary()
        finally:
            hb.TIMER = timer
        stats = grid.last_stats
        rows[name].update(evaluated=stats["evaluated"], total=stats["total"], evaluated_per_ray=stats["evaluated"] / N_RAYS,
                          occ_kernels_ms=sum(v["ms"] for kname, v in summ.items() if kname.startswith("occ_")),
                          field_ms=sum(v["ms"] for kname, v in summ.items() if kname.startswith(("field_", "wgrad"))))
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
    g, radius = ball_with_share(want)
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
rays_rec = wl.synthetic_rays(N_RAYS, 1).to(dev).contiguous()       # (the records render() makes of `rays`)
S = N_C + N_F
kernel = {}
for M in MARCH_STEPS:
    ts = []
    for _ in range(3):
        g.march(rays_rec, M, S)
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            g.march(rays_rec, M, S)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 100 * 1e3)
    us = statistics.median(ts)
    nbytes = (32 + 4 * S + 8) * N_RAYS
    kernel[f"M={M}"] = {"us_median": us, "us_min": min(ts), "us_max": max(ts), "rays": N_RAYS, "slots": S, "bytes_model": nbytes,
                        "gbytes_per_s_model": nbytes / us / 1e3, "rays_truncated": int(g.march(rays_rec, M, S)[2].sum())}
kernel["note"] = "host-timed back-to-back launches (allocation of the outputs included)"
result["march_kernel_128_cubed"] = kernel
text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
