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
import sys

import grid_exp as gx

ap = gx.parser(__doc__, trace="a short untimed run (4096 rays, dense and share 0.25) for a profiler")
args = ap.parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_occupancy")
HAVE_GRID = hasattr(npa, "OccupancyGrid")
S = gx.Scene(wl, npa, dev, perturb=0.)
C2W = wl.pose_spherical(30.0, -30.0, 4.0)[:3, :4].to(dev)


def call_batch(grid):
    return S.render(**(dict(occupancy=grid) if grid is not None else {}))


def call_frame(grid):
    return S.render(c2w=C2W, **(dict(occupancy=grid) if grid is not None else {}))


def share_of(grid, call=call_batch):
    with torch.no_grad():
        call(grid)
    return gx.evaluated_share(grid)


def ball_with_share(target):
    """bisect the radius on the 4096-ray batch (the share counts both passes; the fine depths follow the masked coarse weights)"""
    return S.ball_with_share(npa.OccupancyGrid, share_of, target)


def time_all(configs, call, n_rays, k, reps):
    """alternate the configurations inside every repetition; HIP events around k calls each"""
    with torch.no_grad():
        times = gx.time_alternating([(name, lambda grid=grid: call(grid)) for name, grid in configs], k, reps, warmup=2)
    rows = {}
    for name, grid in configs:
        rows[name] = gx.row_stats(times[name], n_rays)
        if grid is not None:
            # a separate pass with HIP events around the new launches.  count_readbacks_per_call counts the calls of hb.occ_compact:
            # render.py follows each with ONE blocking read of the count word M (.item()), the only host synchronisation of a pass
            readbacks = [0]
            compact = hb.occ_compact

            def counted(*a, **kw):
                readbacks[0] += 1
                return compact(*a, **kw)
            hb.occ_compact = counted
            try:
                summ = gx.kernel_summary(hb, lambda: share_of(grid, call))
            finally:
                hb.occ_compact = compact
            rows[name].update(evaluated_share=gx.evaluated_share(grid), points=grid.last_stats["total"], count_readbacks_per_call=readbacks[0],
                              occ_kernels_ms=gx.kernel_ms(summ, "occ_"), field_ms=gx.kernel_ms(summ, "field_fwd"),
                              fraction_occupied=grid.fraction_occupied())
        else:
            rows[name].update(evaluated_share=1.0, count_readbacks_per_call=0)
    return rows


if args.trace:
    g, _ = ball_with_share(0.25)
    with torch.no_grad():
        for _ in range(5):
            call_batch(None)
            call_batch(g)
    torch.cuda.synchronize()
    sys.exit(0)

result = {"precision": "fp16x3", "samples": "64 + 128", "chunk": 32768, "grid_resolution": S.R if HAVE_GRID else None, "tree": args.label,
          "have_grid": HAVE_GRID,
          "count_readbacks_per_call": "calls of hb.occ_compact in one render(); render.py follows each with one blocking read of the count word M, "
                                      "the only host synchronisation of a pass (counted by wrapping hb.occ_compact, not by intercepting the synchronisation)"}
configs = [("dense (no grid)", None)]
if HAVE_GRID:
    full = npa.OccupancyGrid(S.LO, S.HI, S.R, device=dev)
    configs.append(("grid share 1.0 (all occupied)", full))
    for target in (0.5, 0.25, 0.1):
        g, radius = ball_with_share(target)
        configs.append((f"grid share {target} (ball r = {radius:.3f}, outside skipped)", g))
    net_grid = npa.OccupancyGrid.from_network(S.nf, S.LO, S.HI, S.R, sigma_threshold=0.0, samples_per_cell=1, dilate=1)
    configs.append(("grid from_network (sigma > 0, dilate 1)", net_grid))
result["rays_4096"] = time_all(configs, call_batch, 4096, 20, args.reps)
result["frame_800x800"] = time_all(configs, call_frame, S.H * S.W, 1, args.reps)
if HAVE_GRID:
    with torch.no_grad():
        dense = call_batch(None)[0]
        got = call_batch(net_grid)[0]
        fdense = call_frame(None)[0]
        fgot = call_frame(net_grid)[0]
    result["from_network"] = {"fraction_occupied": net_grid.fraction_occupied(), "psnr_vs_dense_db_4096_rays": gx.psnr_db(got, dense),
                              "psnr_vs_dense_db_frame": gx.psnr_db(fgot, fdense),
                              "evaluated_share_4096_rays": result["rays_4096"]["grid from_network (sigma > 0, dilate 1)"]["evaluated_share"],
                              "evaluated_share_frame": result["frame_800x800"]["grid from_network (sigma > 0, dilate 1)"]["evaluated_share"]}
gx.emit(result, args.out)
