"""Gradients to points, rays and camera poses through the hash-grid field (csrc/hash_input_grad.hip, HashNeRF(point_grad=True); DESIGN.md
3.28) on one MI355X: the default HashEncoding over [-1.5, 1.5]^3 (16 levels, F = 2, T = 2^19, 16 .. 512 cells), HashNeRF D = 2, W = 64,
4096-ray batches at 64 + 128 samples, white background --
  * nerf_hash_input_grad alone on the 786,432 points o + d z of the batch's rays, ray mode (with the 27 view columns) and point mode,
    beside nerf_hash_encode_fwd in the same run (host-timed back-to-back launches), and their ratio;
  * a HashNeRF training step (render() forward, two img2mse, backward, Adam at lr = 0) with and without rays that require grad,
    alternating; a pair built without the flag beside them;
  * a localisation step: the pair frozen, PoseRefinement(1), RayBatcher over the field's own frame at the true pose, render(rays=...),
    img2mse of the fine pass against the frame, backward, Adam on xi; beside it, alternating in the same run, the fused network's iNeRF step (fp16x3);
  * the pose error left after --steps localisation steps from --twist: the angle of exp(xi) and how far it moves the camera -- for the
    default encoding and for a coarse one (--coarse-levels levels up to --coarse-finest cells) --, the loss of one fixed batch along the
    line from the true pose to the twist, and its slope at the twist by autograd and by a central difference.
The field is a HashNeRF pair fitted for --fit-steps Adam steps to the fixture teacher's renders (tools/exp_hash.py): the recovery
figures are this field's on this one run.

    python tools/exp_hash_pose.py --out profiles/r34_exp_hash_pose.json
"""
import math

import grid_exp as gx

ap = gx.parser(__doc__, steps="localisation steps of the recovery run")
ap.add_argument("--fit-steps", type=int, default=300)
ap.add_argument("--hash-lr", type=float, default=1e-2)
ap.add_argument("--side", type=int, default=200, help="the frame is side x side")
ap.add_argument("--lr", type=float, default=1e-3)
ap.add_argument("--twist", type=float, nargs=6, default=[0.01, -0.015, 0.012, 0.03, -0.02, 0.025], help="the start: (omega, v)")
ap.add_argument("--theta", type=float, default=30.0)
ap.add_argument("--coarse-levels", type=int, default=8)
ap.add_argument("--coarse-finest", type=int, default=64)
ap.set_defaults(steps=200)
args = ap.parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_hash_pose")
S = gx.Scene(wl, npa, dev, perturb=0., target=True, records=True)
N_RAYS, N_C, N_F = S.N_RAYS, 64, 128
BOUND = 1.5
side = args.side
K = wl.intrinsics(dict(H=side, W=side, focal=1111.0 * side / S.H))
POSE = wl.pose_spherical(args.theta, -30.0, 4.0)[:3, :4].to(dev)[None]


def hash_pair(seed, point_grad, **grid):
    torch.manual_seed(seed)
    return [npa.HashNeRF([-BOUND] * 3, [BOUND] * 3, output_ch=5, point_grad=point_grad, **grid).to(dev) for _ in range(2)]


# ---- the entry point alone, on the points of the batch's rays at 192 sorted depths
hc, hf = hash_pair(0, True)
enc = hc.encoding
desc, P, C = enc.desc(), N_RAYS * (N_C + N_F), enc.out_dim
g = torch.Generator().manual_seed(1)
z = (2.0 + 4.0 * torch.rand(N_RAYS, N_C + N_F, generator=g)).sort(1).values.to(dev).contiguous()
pts = (S.records[:, None, 0:3] + S.records[:, None, 3:6] * z[:, :, None]).reshape(-1, 3).contiguous()
x = torch.empty(P, C, device=dev)
d_x = torch.randn(P, C + 27, generator=g).to(dev)
E = enc.embeddings.detach()
launches = {
    "nerf_hash_encode_fwd": gx.time_launches(lambda: hb.hash_encode_fwd(desc, E, x, rays=S.records, z_vals=z), args.reps, launches=20),
    "nerf_hash_input_grad, ray mode with 27 view columns": gx.time_launches(
        lambda: hb.hash_input_grad(desc, E, d_x, 0, None, S.records, z, C, 4), args.reps, launches=20),
    "nerf_hash_input_grad, ray mode without view columns": gx.time_launches(
        lambda: hb.hash_input_grad(desc, E, d_x, 0, None, S.records, z, -1, -1), args.reps, launches=20),
    "nerf_hash_input_grad, point mode": gx.time_launches(lambda: hb.hash_input_grad(desc, E, d_x, 0, pts, None, None, -1, -1), args.reps, launches=20),
}
gathered = P * enc.n_levels * 8 * 4 * enc.n_features
fwd_us = launches["nerf_hash_encode_fwd"]["us_median"]
for name, row in launches.items():
    row["gathered_bytes"] = gathered
    row["GB_per_s_host_timed"] = gathered / row["us_median"] * 1e-3
    row["over nerf_hash_encode_fwd"] = row["us_median"] / fwd_us
bytes_per_point = {"gathered rows (the forward's)": enc.n_levels * 8 * 4 * enc.n_features, "d_x, hash columns": 4 * C, "d_x, view columns (ray mode)": 4 * 27,
                   "workspace, written and read (ray mode)": 24, "depth (ray mode)": 4, "point (point mode)": 12, "d_points (point mode)": 12}
inside = float((pts.abs().amax(-1) <= BOUND).float().mean())

# ---- the training step with and without rays that require grad; a pair without the flag beside them
pc, pf = hash_pair(0, False)
adam_h = torch.optim.Adam([p for n in (hc, hf) for p in n.parameters()], lr=0.0)
adam_p = torch.optim.Adam([p for n in (pc, pf) for p in n.parameters()], lr=0.0)


def step(nets, opt, rays_grad):
    rays = S.rays.clone().requires_grad_(True) if rays_grad else S.rays
    S.fit(S.render(rays, network_fn=nets[0], network_fine=nets[1]), opt, rgb0=True)


configs = [("HashNeRF(point_grad=True), training step, rays constant", lambda: step((hc, hf), adam_h, False)),
           ("HashNeRF(point_grad=True), training step, rays require grad", lambda: step((hc, hf), adam_h, True)),
           ("HashNeRF(), training step", lambda: step((pc, pf), adam_p, False))]
times = gx.time_alternating(configs, 10, args.reps, warmup=3)
train_rows = {name: gx.row_stats(times[name], N_RAYS) for name, _ in configs}
summary = gx.kernel_summary(hb, configs[1][1])
train_rows[configs[1][0]]["hash_launches_ms_in_one_step"] = {k: v["ms"] for k, v in summary.items() if k.startswith("hash_")}

# ---- a field with structure: a pair fitted to the teacher's renders, then frozen
teacher, student, held, held_target = S.teacher_and_held_out()


def fitted_pair(**grid):
    nets = hash_pair(1, True, **grid)
    kw = dict(network_fn=nets[0], network_fine=nets[1])
    opt = torch.optim.Adam([p for n in nets for p in n.parameters()], lr=args.hash_lr)
    for i in range(args.fit_steps):
        batch = wl.lego_batch(N_RAYS, seed=2000 + i).to(dev)
        with torch.no_grad():
            want = S.render(batch, **teacher)[0]
        rgb, _, _, extras = S.render(batch, perturb=1., **kw)
        loss = npa.img2mse(rgb, want) + npa.img2mse(extras["rgb0"], want)
        opt.zero_grad()
        loss.backward()
        opt.step()
    with torch.no_grad():
        psnr = gx.psnr_db(S.render(held, **kw)[0], held_target)
        frame = npa.render(side, side, K, c2w=POSE[0], **S.GEO, **dict(S.KW, **kw))[0].reshape(1, side, side, 3).contiguous()
    for p in [p for n in nets for p in n.parameters()]:
        p.requires_grad_(False)
    return kw, psnr, npa.RayBatcher(frame, K, N_RAYS, [0], generator=torch.Generator().manual_seed(3)), nets[0].encoding.level_resolution


fit_kw, fit_psnr, batcher, _ = fitted_pair()
for p in [p for n in (S.nc, S.nf) for p in n.parameters()]:
    p.requires_grad_(False)

# ---- localisation against the field's own frame, beside the fused network's iNeRF step
with torch.no_grad():
    frame_net = npa.render(side, side, K, c2w=POSE[0], **S.GEO, **S.KW)[0].reshape(1, side, side, 3).contiguous()
batcher_net = npa.RayBatcher(frame_net, K, N_RAYS, [0], generator=torch.Generator().manual_seed(3))


def refinement(twist):
    refine = npa.PoseRefinement(1).to(dev)
    with torch.no_grad():
        refine.xi.copy_(torch.tensor([twist], device=dev))
    return refine, torch.optim.Adam(refine.parameters(), lr=args.lr)


def pose_step(refine, opt, b, kw):
    rays, rgb = b.next(refine(POSE))
    out = npa.render(side, side, K, rays=rays, **S.GEO, **dict(S.KW, **kw))
    loss = npa.img2mse(out[0], rgb)         # (the frame is the FINE pass's render: rgb0 against it would not vanish at the true pose)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss


def error_of(refine):
    """the pose error exp(xi) stands for: its angle in degrees and the distance it moves the camera"""
    T = npa.pose.se3_exp(refine.xi.detach().double().cpu())[0]
    c = torch.cat([POSE[0, :3, 3].double().cpu(), torch.ones(1, dtype=torch.float64)])
    cos = max(-1.0, min(1.0, 0.5 * (float(T[0, 0] + T[1, 1] + T[2, 2]) - 1.0)))
    return {"angle_deg": math.degrees(math.acos(cos)), "camera_moved": float((T @ c - c)[:3].norm())}


loc, net = refinement(args.twist), refinement(args.twist)
times = gx.time_alternating([("HashNeRF localisation step (pair frozen)", lambda: pose_step(*loc, batcher, fit_kw)),
                             ("fused network iNeRF step (fp16x3)", lambda: pose_step(*net, batcher_net, {}))], k=10, reps=args.reps, warmup=3)
pose_rows = {name: gx.row_stats(ms) for name, ms in times.items()}
summary = gx.kernel_summary(hb, lambda: pose_step(*loc, batcher, fit_kw))
pose_rows["HashNeRF localisation step (pair frozen)"]["hash_launches_ms_in_one_step"] = {k: v["ms"] for k, v in summary.items() if k.startswith("hash_")}


def recovery(kw, b):
    refine, opt = refinement(args.twist)
    before, losses = error_of(refine), []
    for i in range(args.steps):
        loss = pose_step(refine, opt, b, kw)
        if i % max(1, args.steps // 10) == 0 or i == args.steps - 1:
            losses.append((i, float(loss)))
    return {"before": before, "after": error_of(refine), "loss (step, img2mse)": losses}


def along_the_twist(kw, frame):
    """the loss of one fixed 4096-pixel batch at t * twist for t = 0 .. 1, and d loss / d t at t = 1 by autograd and by a central
    difference of +-2 %: whether the loss falls towards the true pose, and whether the gradient is that slope"""
    def at(t, grad=False):
        refine = npa.PoseRefinement(1).to(dev)
        with torch.no_grad():
            refine.xi.copy_(torch.tensor([args.twist], device=dev) * t)
        b = npa.RayBatcher(frame, K, N_RAYS, [0], generator=torch.Generator().manual_seed(9))
        rays, rgb = b.next(refine(POSE))
        out = npa.render(side, side, K, rays=rays, **S.GEO, **dict(S.KW, **kw))
        loss = npa.img2mse(out[0], rgb)
        if not grad:
            return float(loss)
        loss.backward()
        return float((refine.xi.grad * torch.tensor([args.twist], device=dev)).sum())
    return {"loss at t * twist": {str(t): at(t) for t in (0.0, 0.25, 0.5, 0.75, 1.0)}, "d loss / d t at t = 1, autograd": at(1.0, True),
            "d loss / d t at t = 1, central difference of +-0.02": (at(1.02) - at(0.98)) / 0.04}


recovered = {"default encoding": dict(recovery(fit_kw, batcher), resolutions=enc.level_resolution, psnr_db=fit_psnr,
                                      **along_the_twist(fit_kw, batcher.images))}
coarse_kw, coarse_psnr, coarse_batcher, coarse_res = fitted_pair(n_levels=args.coarse_levels, finest_resolution=args.coarse_finest)
recovered["coarse encoding"] = dict(recovery(coarse_kw, coarse_batcher), resolutions=coarse_res, psnr_db=coarse_psnr,
                                     **along_the_twist(coarse_kw, coarse_batcher.images))

gx.emit({"tree": args.label, "rays": N_RAYS, "samples": "64 + 128", "points": P, "one run on one machine": True,
         "encoding": {"levels": enc.n_levels, "features": enc.n_features, "log2_hashmap_size": enc.log2_hashmap_size, "rows": enc.rows_total,
                      "box": [-BOUND, BOUND], "share_of_points_inside_the_box": inside},
         "launches_alone": launches, "bytes per point by arithmetic": bytes_per_point,
         "training step, alternating (Adam at lr = 0)": train_rows,
         "field": {"fit_steps": args.fit_steps, "lr": args.hash_lr, "psnr_db on the held-out batch": fit_psnr},
         "frame": f"{side}x{side}", "pose step, alternating": pose_rows,
         "recovery": dict(recovered, twist=args.twist, lr=args.lr, steps=args.steps)}, args.out)
