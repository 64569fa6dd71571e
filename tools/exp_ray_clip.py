"""Clipping rays to the occupied span of an occupancy grid (render_rays(clip_to_occupancy=True)) against the
same calls without it: fp16x3, 4096 rays of workloads.synthetic_rays, ball masks at 128^3 over [-2, 2]^3 with the outside skipped whose
evaluated share of sample points is about 0.25 / 0.5 (section 3.9's masks).  Three settings per mask: no clip (64 + 128 samples), clip at
N_samples = 64, clip at N_samples = ceil(64 x the mean span share of the hit rays).  Recorded:
  kernel      HIP events around nerf_occ_ray_span alone: 4096 rays, and the 20 chunks (32768 rays) of one 800 x 800 frame;
  render      no_grad render() of the 4096 rays: ms, evaluated points (last_stats), PSNR of rgb_map against the unclipped 64 + 128
              grid render of the same rays and against the render without a grid;
  train_step  render_rays through a DensityGrid holding the mask's bits + the two MSE losses + backward + FlatAdam.step (lr = 0: every
              repetition of every setting sees the same networks, so the evaluated points do not drift).

    python tools/exp_ray_clip.py --out profiles/r11_exp_ray_clip.json
    python tools/exp_ray_clip.py --root <checkout of the parent commit> --label "parent commit" --out ...   # the same process layout on
                                                                # that tree: a tree without ray_span times the "no clip" rows only
"""
import math

import grid_exp as gx

args = gx.parser(__doc__).parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_ray_clip")
HAVE_CLIP = hasattr(npa.OccupancyGrid, "ray_span")
S = gx.Scene(wl, npa, dev, perturb=0., records=True)
LO, HI, R, H, W, N_RAYS, records4096 = S.LO, S.HI, S.R, S.H, S.W, S.N_RAYS, S.records
C2W = wl.pose_spherical(30.0, -30.0, 4.0)[:3, :4].to(dev)


def render_batch(grid, n_samples=64, clip=False):
    kw = dict(N_samples=n_samples)
    if grid is not None:
        kw.update(occupancy=grid, **({"clip_to_occupancy": True} if clip else {}))
    return S.render(**kw)


def share_of(grid):
    with torch.no_grad():
        render_batch(grid)
    return gx.evaluated_share(grid)


def timed(configs, k):
    """configs: [(name, callable)]; every repetition runs each configuration once, HIP events around k calls"""
    return {name: gx.row_stats(ms) for name, ms in gx.time_alternating(configs, k, args.reps, warmup=2).items()}


result = {"precision": "fp16x3", "rays": N_RAYS, "grid_resolution": R, "tree": args.label, "have_clip": HAVE_CLIP, "masks": {}}
with torch.no_grad():
    dense = render_batch(None)[0]
frame_records = hb.make_rays(H, W, S.K, C2W, None, False, 2., 6., dev) if HAVE_CLIP else None

for target in (0.25, 0.5):
    # the radius bisected on the evaluated share of the unclipped 64 + 128 render (tools/exp_occupancy.py's masks)
    grid, radius = S.ball_with_share(npa.OccupancyGrid, share_of, target)
    row = {"ball_radius": radius, "fraction_occupied": grid.fraction_occupied()}
    settings = [("no clip, 64 + 128", 64, False)]
    if HAVE_CLIP:
        span, hit = grid.ray_span(records4096)
        share = float(((span[:, 1] - span[:, 0]) / (records4096[:, 7] - records4096[:, 6]))[hit].mean())
        n_red = max(8, math.ceil(64 * share))
        row.update(rays_hit=int(hit.sum()), mean_span_share_of_hit_rays=share, reduced_N_samples=n_red)
        settings += [("clip, 64 + 128", 64, True), (f"clip, {n_red} + 128", n_red, True)]
        # ---- the kernel alone
        desc = grid._desc()
        chunks = [frame_records[i:i + 32768].contiguous() for i in range(0, H * W, 32768)]
        kt = timed([("4096 rays", lambda: hb.occ_ray_span(desc, records4096)),
                    ("800 x 800 frame, 20 chunks of 32768 rays", lambda: [hb.occ_ray_span(desc, c) for c in chunks])], 50)
        fhit = torch.cat([hb.occ_ray_span(desc, c)[1] for c in chunks])
        kt["frame_rays_hit"] = int(fhit.sum())
        row["kernel"] = kt
    # ---- no_grad render
    with torch.no_grad():
        ref = render_batch(grid)[0]
        rows = timed([(name, (lambda n=n, c=c: render_batch(grid, n, c))) for name, n, c in settings], 20)
        for name, n, c in settings:
            out = render_batch(grid, n, c)[0]
            rows[name].update(evaluated=grid.last_stats["evaluated"], total=grid.last_stats["total"],
                              psnr_vs_unclipped_grid_render_db=gx.psnr_db(out, ref), psnr_vs_render_without_grid_db=gx.psnr_db(out, dense))
    row["render_no_grad"] = rows
    if HAVE_CLIP:
        base = rows["no clip, 64 + 128"]["ms_median"]
        row["kernel"]["share_of_unclipped_grid_render"] = row["kernel"]["4096 rays"]["ms_median"] / base
    # ---- training step (DensityGrid with the mask's bits; neither the grid nor, with lr = 0, the networks change inside the timed loop)
    if hasattr(npa, "DensityGrid"):
        dgrid = npa.DensityGrid(LO, HI, R, outside="skip", device=dev)
        dgrid.bits = grid.bits.clone()
        tc, tf = S.networks(S.Pc, S.Pf)
        opt = S.adam(tc, tf)
        target_rgb = torch.rand(N_RAYS, 3, generator=torch.Generator().manual_seed(3)).to(dev)
        stats = {}

        def step(name, n, c):
            kw = dict(N_samples=n, N_importance=128, network_fine=tf, white_bkgd=True, perturb=0., raw_noise_std=0., occupancy=dgrid)
            if c:
                kw["clip_to_occupancy"] = True
            out = npa.render_rays(records4096, tc, None, **kw)
            stats[name] = dict(dgrid.last_stats)
            opt.zero_grad()
            (npa.img2mse(out["rgb_map"], target_rgb) + npa.img2mse(out["rgb0"], target_rgb)).backward()
            opt.step()
        trows = timed([(name, (lambda name=name, n=n, c=c: step(name, n, c))) for name, n, c in settings], 5)
        for name in trows:
            trows[name].update(evaluated=stats[name]["evaluated"], total=stats[name]["total"])
        row["train_step"] = trows
    result["masks"][f"share {target}"] = row

gx.emit(result, args.out)
