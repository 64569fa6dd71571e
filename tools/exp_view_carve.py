"""Occupancy grids from training cameras and silhouettes (nerf_occ_view_carve) on one MI355X:
  * the kernel alone at 128^3 over [-2, 2]^3 with 25 and 100 views of 400 x 400 pixels, with and without the summed-area tables of the
    silhouettes (HIP events around 100 back-to-back launches; the tables are built beforehand), and OccupancyGrid.from_views end to end
    (upload, cumsum, the launches in chunks, the thresholding) -- next to one DensityGrid.update of the same grid, for scale;
  * the share of the cells the cameras of the lego-like workload keep: the batch's own camera above the scene (the rays of
    workloads.lego_batch start at (0, 0, 4)) and a spiral of blender poses over the upper hemisphere at radius 4, with the silhouettes
    of a ball of radius 1 (the ball masks of the other grid scripts);
  * the 4096-ray fp16x3 training step (forward, two img2mse, backward, FlatAdam.step, lr = 0) DURING THE WARM-UP of a DensityGrid: the
    grid restricted to the hull (restrict_to_views, never updated) against the all-occupied grid a DensityGrid is until warmup_steps, and
    against the step without a grid, alternating in the same run.

    python tools/exp_view_carve.py --out profiles/r19_exp_view_carve.json
"""
import grid_exp as gx

ap = gx.parser(__doc__, steps="training steps between two HIP events")
args = ap.parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_view_carve")
S = gx.Scene(wl, npa, dev, perturb=1., target=True)
occ = npa.occupancy
HV = WV = 400
KV = torch.tensor(wl.intrinsics(wl.LEGO), dtype=torch.float32)
NEAR, FAR, BALL = 2.0, 6.0, 1.0


def cameras(n):
    """the batch's camera at (0, 0, 4) and n - 1 blender poses on a spiral from 85 to 10 degrees above the plane, radius 4: [n, 3, 4]"""
    poses = [wl.pose_spherical(0.0, -90.0, 4.0)]
    for k in range(n - 1):
        poses.append(wl.pose_spherical(360.0 * k * 0.381966, -85.0 + 75.0 * k / max(n - 2, 1), 4.0))
    return torch.stack(poses)[:, :3, :4]


def silhouettes(c2w, radius=BALL):
    """bool [V, H, W] on the device: the pixel's ray passes within `radius` of the origin"""
    i, j = torch.meshgrid(torch.arange(WV, dtype=torch.float64, device=dev), torch.arange(HV, dtype=torch.float64, device=dev), indexing="xy")
    Kd = KV.double()
    dirs = torch.stack([(i - Kd[0, 2]) / Kd[0, 0], -(j - Kd[1, 2]) / Kd[1, 1], -torch.ones_like(i)], -1)
    out = []
    for pose in c2w.to(dev).double():
        d, o = (dirs[..., None, :] * pose[:, :3]).sum(-1), pose[:, 3]
        t = -(d * o).sum(-1) / (d * d).sum(-1)
        out.append(((o + d * t[..., None]).norm(dim=-1) <= radius) & (t > 0))
    return torch.stack(out)


result = {"tree": args.label, "grid_resolution": S.R, "box": [S.LO[0], S.HI[0]], "image": [HV, WV], "near_far": [NEAR, FAR],
          "silhouettes": f"ball of radius {BALL}", "margin_px": 0.5}

# ---- the kernel alone, and from_views end to end
grid = npa.OccupancyGrid(S.LO, S.HI, S.R, device=dev)
desc = grid._desc()
near_m, far_m = hb.view_planes(NEAR, FAR)
kernel, kept = {}, {}
for V in (25, 100):
    c2w = cameras(V)
    masks = silhouettes(c2w)
    cams = occ._view_inputs("exp_view_carve", c2w, HV, WV, KV, NEAR, FAR, 0.5)[0].to(dev)
    sat = occ._mask_sat(masks)
    seen = torch.empty(grid.n_cells, dtype=torch.int32, device=dev)
    words = torch.empty_like(grid.bits)
    kernel[f"{V} views, visibility only"] = gx.time_launches(
        lambda: hb.occ_view_carve(desc, grid.width, cams, HV, WV, near_m, far_m, 0.5, None, seen, None), args.reps)
    kernel[f"{V} views, with silhouettes"] = gx.time_launches(
        lambda: hb.occ_view_carve(desc, grid.width, cams, HV, WV, near_m, far_m, 0.5, sat, seen, words), args.reps)
    masks_cpu = masks.cpu()
    for name, kw in (("visibility only", {}), ("with silhouettes", dict(masks=masks_cpu))):
        build = lambda kw=kw: npa.OccupancyGrid.from_views(c2w, HV, WV, KV, NEAR, FAR, S.LO, S.HI, S.R, outside="skip", device=dev, **kw)
        ts = gx.time_alternating([("from_views", build)], 1, args.reps, warmup=1)["from_views"]
        kernel[f"{V} views, {name}: from_views end to end (masks uploaded from the host)"] = gx.row_stats(ts)
        kept[f"{V} views, {name}"] = build().fraction_occupied()
result["kernel_128_cubed_us_per_launch"] = kernel
result["kept_share_of_cells"] = kept
result["cells_whose_centre_lies_in_the_ball"] = float(gx.ball_mask(S.R, S.LO[0], S.HI[0], BALL).float().mean())
g = npa.DensityGrid(S.LO, S.HI, S.R, device=dev).update(S.nf)
result["density_update_128_cubed"] = gx.row_stats(gx.time_alternating([("update", lambda: g.update(S.nf))], 1, args.reps, warmup=0)["update"])

# ---- the training step during the warm-up
opt = S.adam(S.nc, S.nf)
c2w = cameras(100)
masks = silhouettes(c2w)
full = npa.DensityGrid(S.LO, S.HI, S.R, outside="skip", device=dev)
hull = npa.DensityGrid(S.LO, S.HI, S.R, outside="skip", device=dev).restrict_to_views(c2w, HV, WV, KV, NEAR, FAR, masks=masks)
seen_only = npa.DensityGrid(S.LO, S.HI, S.R, outside="skip", device=dev).restrict_to_views(c2w, HV, WV, KV, NEAR, FAR)
configs = [("dense (no grid)", None), ("DensityGrid in its warm-up (all occupied)", full),
           ("DensityGrid restricted to what 100 cameras see", seen_only), ("DensityGrid restricted to the hull of 100 silhouettes", hull)]


def step(grid):
    S.fit(S.render(**(dict(occupancy=grid) if grid is not None else {})), opt, rgb0=True)


times = gx.time_alternating([(name, lambda grid=grid: step(grid)) for name, grid in configs], args.steps, args.reps, warmup=3)
rows = {}
for name, grid in configs:
    rows[name] = gx.row_stats(times[name], S.N_RAYS)
    if grid is not None:
        rows[name].update(evaluated_share=gx.evaluated_share(grid), fraction_occupied=grid.fraction_occupied())
base = rows["DensityGrid in its warm-up (all occupied)"]["ms_median"]
for name in rows:
    rows[name]["speedup_vs_all_occupied"] = base / rows[name]["ms_median"]
result["train_step_4096_rays_during_warm_up"] = dict(rows, step="render() forward, two img2mse, backward, FlatAdam.step (lr = 0), fp16x3, 64 + 128 samples",
                                                     steps_per_timing=args.steps)
gx.emit(result, args.out)
