"""Baked fields (baked.py, nerf_baked_render) of the fixture fine network on one MI355X: grids of 64^3 and 128^3 over [-2, 2]^3 from
OccupancyGrid.from_network (threshold 0, one round of dilation), sh_degree 0 / 1 / 2, n_dirs 32, step = half a cell:
  * rows, table and index bytes, the bake's time (BakedField.from_network, one run);
  * the kernel alone on the 4096-ray batch -- HIP events around back-to-back launches -- with its samples per ray;
  * a 400 x 400 and an 800 x 800 frame through render(baked=field) against the same frame through the networks with occupancy=grid,
    alternating in one run, and the PSNR of the baked frame against the network's.
The fixture scene is a fog: density nearly everywhere and colours that vary with the direction at every point.  That is the worst case
for a grid (no empty space to skip, no surface for the transmittance to end on), so the figures are a floor, not a promise.

    python tools/exp_baked.py --out profiles/r25_exp_baked.json
"""
import time

import grid_exp as gx

ap = gx.parser(__doc__)
ap.add_argument("--resolutions", type=int, nargs="+", default=[64, 128])
ap.add_argument("--frames", type=int, nargs="+", default=[400, 800])
args = ap.parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_baked")
S = gx.Scene(wl, npa, dev, perturb=0., records=True)
C2W = wl.pose_spherical(30.0, -30.0, 4.0)[:3, :4].to(dev)


def frame(side, **over):
    K = wl.intrinsics(dict(H=side, W=side, focal=1111.0 * side / S.H))
    with torch.no_grad():
        return npa.render(side, side, K, c2w=C2W, **S.GEO, **dict(S.KW, **over))


result = {"tree": args.label, "box": [S.LO[0], S.HI[0]], "precision of the network frames": "fp16x3", "n_dirs": 32, "scene": "fog (worst case)"}
for R in args.resolutions:
    grid = npa.OccupancyGrid.from_network(S.nf, S.LO, S.HI, R)
    per_grid = {"fraction_occupied": grid.fraction_occupied()}
    network = {side: frame(side, occupancy=grid)[0] for side in args.frames}
    for degree in (0, 1, 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        field = npa.BakedField.from_network(S.nf, grid, sh_degree=degree, n_dirs=32)
        torch.cuda.synchronize()
        row = {"bake_s": time.perf_counter() - t0, "rows": field.n_rows, "table_bytes": field.table.numel() * 2,
               "index_bytes": field.index.numel() * 4, "step_size": field.step_size}
        field.render_rays(S.records)
        row["samples_per_ray"] = field.last_stats["samples"] / field.last_stats["rays"]
        desc = grid._desc()
        row["kernel_us, 4096 rays"] = gx.time_launches(
            lambda: hb.baked_render(desc, field.index, field.table, degree, S.records, None, field.step_size, 1 << 14), args.reps, launches=20)
        for side in args.frames:
            ms = gx.time_alternating([("baked", lambda: frame(side, baked=field)), ("network", lambda: frame(side, occupancy=grid))], 1,
                                     args.reps, warmup=1)
            row[f"{side}x{side}"] = {"baked": gx.row_stats(ms["baked"]), "network with occupancy=": gx.row_stats(ms["network"]),
                                     "evaluated_share": gx.evaluated_share(grid), "baked_samples_per_ray": field.last_stats["samples"] / side ** 2,
                                     "psnr_db of the baked frame against the network's": gx.psnr_db(frame(side, baked=field)[0], network[side])}
        per_grid[f"sh_degree {degree}"] = row
        del field
    result[f"{R}^3"] = per_grid
gx.emit(result, args.out)
