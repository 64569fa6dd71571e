"""no_grad render() with an occupancy grid against the same call without one (fp16x3, 64 + 128 samples): 4096 rays and one 800 x 800
frame at chunk = 32768, hand-made ball masks whose evaluated share of sample points is about 1.0 / 0.5 / 0.25 / 0.1, and the grid
OccupancyGrid.from_network builds for the scene_params scene.  Per row: ms, rays/s, the evaluated share (last_stats), the time of the
new kernels (HIP events around nerf_occ_compact's three launches and nerf_occ_expand), read-backs of the count word per call
(calls of hb.occ_compact, each followed by the pass's one blocking .item()).

    python tools/exp_occupancy.py --out profiles/r09_exp_occupancy.json          # timing (profiler off)
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/exp_occupancy.py --trace     # a short run for the kernel table
    python tools/exp_occupancy.py --root <checkout of another commit> --label "parent commit" --out ...  # the same process layout on that tree (a tree
                                                                                 # without OccupancyGrid times the dense rows only)
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
ap.add_argument("--trace", action="store_true", help="a short untimed run (4096 rays, dense and share 0.25) for a profiler")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
import workloads as wl  # noqa: E402
import nerf_pytorch_amd as npa  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("exp_occupancy: needs the GPU (no timing without one)")
hb = npa.hip_backend
dev = torch.device("cuda", 0)
HAVE_GRID = hasattr(npa, "OccupancyGrid")
Pc, Pf = wl.scene_params()
kwn = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
nc, nf = npa.NeRF(**kwn).to(dev), npa.NeRF(**kwn).to(dev)
nc.load_state_dict(Pc)
nf.load_state_dict(Pf)
npa.set_precision("fp16x3")
LO, HI, R = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), 128
KW = dict(network_fn=nc, network_query_fn=None, N_samples=64, N_importance=128, network_fine=nf, perturb=0., white_bkgd=True, raw_noise_std=0.)
H = W = 800
K = wl.intrinsics(dict(H=H, W=W, focal=1111.0))
C2W = wl.pose_spherical(30.0, -30.0, 4.0)[:3, :4].to(dev)
rays4096 = wl.lego_batch(4096, seed=1).to(dev)


def call_batch(grid):
    kw = dict(KW, occupancy=grid) if grid is not None else KW
    return npa.render(H, W, K, chunk=32768, rays=rays4096, ndc=False, near=2., far=6., use_viewdirs=True, **kw)


def call_frame(grid):
    kw = dict(KW, occupancy=grid) if grid is not None else KW
    return npa.render(H, W, K, chunk=32768, c2w=C2W, ndc=False, near=2., far=6., use_viewdirs=True, **kw)


def ball(radius):
    c = LO[0] + (torch.arange(R, dtype=torch.float64) + 0.5) * (HI[0] - LO[0]) / R
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    return npa.OccupancyGrid.from_mask((x * x + y * y + z * z) <= radius * radius, LO, HI, outside="skip", device=dev)


def share_of(grid, call=call_batch):
    with torch.no_grad():
        call(grid)
    return grid.last_stats["evaluated"] / grid.last_stats["total"]


def ball_with_share(target):
    """bisect the radius on the 4096-ray batch (the share counts both passes; the fine depths follow the masked coarse weights)"""
    lo, hi = 0.0, 4.0
    for _ in range(14):
        mid = 0.5 * (lo + hi)
        if share_of(ball(mid)) < target:
            lo = mid
        else:
            hi = mid
    return ball(hi), hi


def time_all(configs, call, n_rays, k, reps):
    """alternate the configurations inside every repetition; HIP events around k calls each"""
    times = {name: [] for name, _ in configs}
    with torch.no_grad():
        for name, grid in configs:
            for _ in range(2):
                call(grid)
        torch.cuda.synchronize()
        for _ in range(reps):
            for name, grid in configs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(k):
                    call(grid)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / k)
    rows = {}
    for name, grid in configs:
        ms = statistics.median(times[name])
        rows[name] = {"ms_median": ms, "ms_min": min(times[name]), "ms_max": max(times[name]), "rays_per_s": n_rays / ms * 1e3}
        if grid is not None:
            # a separate pass with HIP events around the new launches.  count_readbacks_per_call counts the calls of hb.occ_compact:
            # render.py follows each with ONE blocking read of the count word M (.item()), the only host synchronisation of a pass
            readbacks = [0]
            compact, timer = hb.occ_compact, hb.TIMER

            def counted(*a, **kw):
                readbacks[0] += 1
                return compact(*a, **kw)
            hb.occ_compact, hb.TIMER = counted, hb.KernelTimer()
            try:
                with torch.no_grad():
                    call(grid)
                summ = hb.TIMER.summary()
            finally:
                hb.occ_compact, hb.TIMER = compact, timer
            rows[name].update(evaluated_share=grid.last_stats["evaluated"] / grid.last_stats["total"],
                              points=grid.last_stats["total"], count_readbacks_per_call=readbacks[0],
                              occ_kernels_ms=sum(v["ms"] for kname, v in summ.items() if kname.startswith("occ_")),
                              field_ms=sum(v["ms"] for kname, v in summ.items() if kname.startswith("field_fwd")),
                              fraction_occupied=grid.fraction_occupied())
        else:
            rows[name].update(evaluated_share=1.0, count_readbacks_per_call=0)
    return rows


def psnr(a, b):
    return float(-10.0 * torch.log10(torch.mean((a.double() - b.double()) ** 2).clamp_min(1e-300)))


if args.trace:
    g, _ = ball_with_share(0.25)
    with torch.no_grad():
        for _ in range(5):
            call_batch(None)
            call_batch(g)
    torch.cuda.synchronize()
    sys.exit(0)

result = {"precision": "fp16x3", "samples": "64 + 128", "chunk": 32768, "grid_resolution": R if HAVE_GRID else None, "tree": args.label,
          "have_grid": HAVE_GRID,
          "count_readbacks_per_call": "calls of hb.occ_compact in one render(); render.py follows each with one blocking read of the count word M, "
                                      "the only host synchronisation of a pass (counted by wrapping hb.occ_compact, not by intercepting the synchronisation)"}
configs = [("dense (no grid)", None)]
if HAVE_GRID:
    full = npa.OccupancyGrid(LO, HI, R, device=dev)
    configs.append(("grid share 1.0 (all occupied)", full))
    for target in (0.5, 0.25, 0.1):
        g, radius = ball_with_share(target)
        configs.append((f"grid share {target} (ball r = {radius:.3f}, outside skipped)", g))
    net_grid = npa.OccupancyGrid.from_network(nf, LO, HI, R, sigma_threshold=0.0, samples_per_cell=1, dilate=1)
    configs.append(("grid from_network (sigma > 0, dilate 1)", net_grid))
result["rays_4096"] = time_all(configs, call_batch, 4096, 20, args.reps)
result["frame_800x800"] = time_all(configs, call_frame, H * W, 1, args.reps)
if HAVE_GRID:
    with torch.no_grad():
        dense = call_batch(None)[0]
        got = call_batch(net_grid)[0]
        fdense = call_frame(None)[0]
        fgot = call_frame(net_grid)[0]
    result["from_network"] = {"fraction_occupied": net_grid.fraction_occupied(), "psnr_vs_dense_db_4096_rays": psnr(got, dense),
                              "psnr_vs_dense_db_frame": psnr(fgot, fdense),
                              "evaluated_share_4096_rays": result["rays_4096"]["grid from_network (sigma > 0, dilate 1)"]["evaluated_share"],
                              "evaluated_share_frame": result["frame_800x800"]["grid from_network (sigma > 0, dilate 1)"]["evaluated_share"]}
text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
