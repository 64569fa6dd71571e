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
import argparse
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
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
import workloads as wl  # noqa: E402
import nerf_pytorch_amd as npa  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("exp_ray_clip: needs the GPU (no timing without one)")
hb = npa.hip_backend
dev = torch.device("cuda", 0)
HAVE_CLIP = hasattr(npa.OccupancyGrid, "ray_span")
Pc, Pf = wl.scene_params()
kwn = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
nc, nf = npa.NeRF(**kwn).to(dev), npa.NeRF(**kwn).to(dev)
nc.load_state_dict(Pc)
nf.load_state_dict(Pf)
npa.set_precision("fp16x3")
LO, HI, R = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), 128
KW = dict(network_fn=nc, network_query_fn=None, N_importance=128, network_fine=nf, perturb=0., white_bkgd=True, raw_noise_std=0.)
H = W = 800
K = wl.intrinsics(dict(H=H, W=W, focal=1111.0))
C2W = wl.pose_spherical(30.0, -30.0, 4.0)[:3, :4].to(dev)
N_RAYS = 4096
batch4096 = wl.lego_batch(N_RAYS, seed=1).to(dev)
records4096 = wl.synthetic_rays(N_RAYS, seed=1).to(dev)


def render_batch(grid, n_samples=64, clip=False):
    kw = dict(KW, N_samples=n_samples)
    if grid is not None:
        kw.update(occupancy=grid, **({"clip_to_occupancy": True} if clip else {}))
    return npa.render(H, W, K, chunk=32768, rays=batch4096, ndc=False, near=2., far=6., use_viewdirs=True, **kw)


def ball_mask(radius):
    c = LO[0] + (torch.arange(R, dtype=torch.float64) + 0.5) * (HI[0] - LO[0]) / R
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    return (x * x + y * y + z * z) <= radius * radius


def ball(radius):
    return npa.OccupancyGrid.from_mask(ball_mask(radius), LO, HI, outside="skip", device=dev)


def ball_with_share(target):
    """bisect the radius on the evaluated share of the unclipped 64 + 128 render (tools/exp_occupancy.py's masks)"""
    lo, hi = 0.0, 4.0
    for _ in range(14):
        mid = 0.5 * (lo + hi)
        g = ball(mid)
        with torch.no_grad():
            render_batch(g)
        if g.last_stats["evaluated"] / g.last_stats["total"] < target:
            lo = mid
        else:
            hi = mid
    return ball(hi), hi


def time_alternating(configs, k, reps):
    """configs: [(name, callable)]; every repetition runs each configuration once, HIP events around k calls"""
    times = {name: [] for name, _ in configs}
    for name, fn in configs:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in configs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / k)
    return {name: {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)} for name, t in times.items()}


def psnr(a, b):
    mse = float(torch.mean((a.double() - b.double()) ** 2))
    return None if mse == 0.0 else -10.0 * math.log10(mse)


result = {"precision": "fp16x3", "rays": N_RAYS, "grid_resolution": R, "tree": args.label, "have_clip": HAVE_CLIP, "masks": {}}
with torch.no_grad():
    dense = render_batch(None)[0]
frame_records = hb.make_rays(H, W, K, C2W, None, False, 2., 6., dev) if HAVE_CLIP else None

for target in (0.25, 0.5):
    grid, radius = ball_with_share(target)
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
        kt = time_alternating([("4096 rays", lambda: hb.occ_ray_span(desc, records4096)),
                               ("800 x 800 frame, 20 chunks of 32768 rays", lambda: [hb.occ_ray_span(desc, c) for c in chunks])], 50, args.reps)
        fhit = torch.cat([hb.occ_ray_span(desc, c)[1] for c in chunks])
        kt["frame_rays_hit"] = int(fhit.sum())
        row["kernel"] = kt
    # ---- no_grad render
    with torch.no_grad():
        ref = render_batch(grid)[0]
        rows = time_alternating([(name, (lambda n=n, c=c: render_batch(grid, n, c))) for name, n, c in settings], 20, args.reps)
        for name, n, c in settings:
            out = render_batch(grid, n, c)[0]
            rows[name].update(evaluated=grid.last_stats["evaluated"], total=grid.last_stats["total"],
                              psnr_vs_unclipped_grid_render_db=psnr(out, ref), psnr_vs_render_without_grid_db=psnr(out, dense))
    row["render_no_grad"] = rows
    if HAVE_CLIP:
        base = rows["no clip, 64 + 128"]["ms_median"]
        row["kernel"]["share_of_unclipped_grid_render"] = row["kernel"]["4096 rays"]["ms_median"] / base
    # ---- training step (DensityGrid with the mask's bits; neither the grid nor, with lr = 0, the networks change inside the timed loop)
    if hasattr(npa, "DensityGrid"):
        dgrid = npa.DensityGrid(LO, HI, R, outside="skip", device=dev)
        dgrid.bits = grid.bits.clone()
        tc, tf = npa.NeRF(**kwn).to(dev), npa.NeRF(**kwn).to(dev)
        tc.load_state_dict(Pc)
        tf.load_state_dict(Pf)
        opt = npa.FlatAdam(list(tc.parameters()) + list(tf.parameters()), lr=0.0)
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
        trows = time_alternating([(name, (lambda name=name, n=n, c=c: step(name, n, c))) for name, n, c in settings], 5, args.reps)
        for name in trows:
            trows[name].update(evaluated=stats[name]["evaluated"], total=stats[name]["total"])
        row["train_step"] = trows
    result["masks"][f"share {target}"] = row

text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
