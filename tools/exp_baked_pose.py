"""Gradients of the baked render to rays and camera poses (csrc/baked_rays.hip, BakedTrainer.render_rays(ray_grad=True)) on one MI355X:
the fixture of tools/exp_baked_finetune.py -- the fine network baked into a 128^3 grid over [-2, 2]^3, 4096-ray batches, white background --
and per sh_degree 0 / 1 / 2
  * the kernels of one step alone on one 4096-ray batch of a frame, host-timed back-to-back launches: nerf_baked_train_fwd,
    nerf_baked_train_bwd_samples, nerf_baked_train_bwd_rows and, where the tree has it, nerf_baked_train_bwd_rays (a tree without it --
    --root of the parent commit -- gives the first three only: the option-off comparison);
  * a localisation step: the table frozen, PoseRefinement(1), RayBatcher over the field's own frame at the true pose, ray_records,
    render_rays(ray_grad=True), img2mse, backward, Adam on xi;
  * a joint step: the same with the table trained as well (Adam on values, commit());
  * beside them, alternating in the same run, the network's iNeRF step: the two frozen fixture networks, render(rays=...) on the same
    batches, Adam on xi;
  * the pose error left after --steps localisation steps from --twist: the angle of exp(xi) and how far it moves the camera.
The scene is a fog (tools/exp_baked.py): the recovery figures are this fog's on this one run.

    python tools/exp_baked_pose.py --out profiles/r31_exp_baked_pose.json
"""
import math

import grid_exp as gx

ap = gx.parser(__doc__, steps="localisation steps of the recovery run")
ap.add_argument("--resolution", type=int, default=128)
ap.add_argument("--side", type=int, default=200, help="the frame is side x side")
ap.add_argument("--lr", type=float, default=1e-3)
ap.add_argument("--twist", type=float, nargs=6, default=[0.01, -0.015, 0.012, 0.03, -0.02, 0.025], help="the start: (omega, v)")
ap.add_argument("--theta", type=float, default=30.0)
ap.add_argument("--degrees", type=int, nargs="+", default=[0, 1, 2])
ap.set_defaults(steps=200)
args = ap.parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_baked_pose")
S = gx.Scene(wl, npa, dev, perturb=0.)
HAS = hasattr(hb, "baked_train_bwd_rays")
side = args.side
K = wl.intrinsics(dict(H=side, W=side, focal=1111.0 * side / S.H))
POSE = wl.pose_spherical(args.theta, -30.0, 4.0)[:3, :4].to(dev)[None]
NEAR, FAR = S.GEO["near"], S.GEO["far"]


def records_of(c2w):
    o, d = npa.get_rays(side, side, K, c2w)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    near, far = torch.full_like(o[:, :1], NEAR), torch.full_like(o[:, :1], FAR)
    return torch.cat([o, d, near, far, d / d.norm(dim=-1, keepdim=True)], -1).float().contiguous()


def kernel_times(trainer, rays):
    """microseconds per launch of every kernel of one step on `rays`, each alone"""
    desc, n = trainer.grid._desc(), rays.shape[0]
    g = [torch.randn(n, 3, device=dev), torch.randn(n, device=dev), torch.randn(n, device=dev)]
    counts = hb.baked_count(desc, rays, None, trainer.step_size, 1 << 14)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(counts, 0)
    total, off = int(off[-1]), off.to(torch.int32)
    fwd = lambda: hb.baked_train_fwd(desc, trainer.index, trainer.table, trainer.sh_degree, rays, None, trainer.step_size, 1 << 14, True, off, total)
    records = fwd()[3]
    samples = lambda: hb.baked_train_bwd_samples(records, off, total, trainer.step_size, True, *g)
    grads = samples()
    order, start = npa.baked.inverted_index(records[:total, 0].view(torch.int32), trainer.grid.n_cells)
    rows = lambda: hb.baked_train_bwd_rows(desc, trainer.row_node, trainer.sh_degree, rays, records, grads, order, start, total)
    out = {"samples per ray": total / n, "nerf_baked_train_fwd": gx.time_launches(fwd, args.reps),
           "nerf_baked_train_bwd_samples": gx.time_launches(samples, args.reps), "nerf_baked_train_bwd_rows": gx.time_launches(rows, args.reps)}
    if HAS:
        back = lambda: hb.baked_train_bwd_rays(desc, trainer.index, trainer.table, trainer.sh_degree, rays, records, grads, off, total)
        out["nerf_baked_train_bwd_rays"] = gx.time_launches(back, args.reps)
        out["bwd_rays / fwd"] = out["nerf_baked_train_bwd_rays"]["us_median"] / out["nerf_baked_train_fwd"]["us_median"]
        W = hb.BAKED_ROW_HALVES[trainer.sh_degree]
        out["bytes by arithmetic, bwd_rays"] = {"per sample, streamed": 80, "per sample, gathered rows (cache hits included)": 16 * W,
                                                "per ray": 64, "total streamed": 80 * total + 64 * n}
    return out


def error_of(refine):
    """the pose error exp(xi) stands for: its angle in degrees and the distance it moves the camera"""
    T = npa.pose.se3_exp(refine.xi.detach().double().cpu())[0]
    c = torch.cat([POSE[0, :3, 3].double().cpu(), torch.ones(1, dtype=torch.float64)])
    cos = max(-1.0, min(1.0, 0.5 * (float(T[0, 0] + T[1, 1] + T[2, 2]) - 1.0)))
    return {"angle_deg": math.degrees(math.acos(cos)), "camera_moved": float((T @ c - c)[:3].norm())}


def refinement(twist):
    refine = npa.PoseRefinement(1).to(dev)
    with torch.no_grad():
        refine.xi.copy_(torch.tensor([twist], device=dev))
    return refine, torch.optim.Adam(refine.parameters(), lr=args.lr)


grid = npa.OccupancyGrid.from_network(S.nf, S.LO, S.HI, args.resolution)
result = {"tree": args.label, "grid": f"{args.resolution}^3", "fraction_occupied": grid.fraction_occupied(), "frame": f"{side}x{side}",
          "batch": S.N_RAYS, "twist": args.twist, "lr": args.lr, "steps": args.steps, "scene": "fog (worst case), one run",
          "nerf_baked_train_bwd_rays": HAS}
for degree in args.degrees:
    field = npa.BakedField.from_network(S.nf, grid, sh_degree=degree, n_dirs=32)
    trainer = field.trainable()
    frame_rays = records_of(POSE[0])
    pick = torch.randperm(frame_rays.shape[0], generator=torch.Generator().manual_seed(degree))[:S.N_RAYS].to(dev)
    row = {"rows": field.n_rows, "us per launch, 4096 rays": kernel_times(trainer, frame_rays[pick].contiguous())}
    if HAS:
        with torch.no_grad():
            target = field.render_rays(frame_rays, white_bkgd=True)["rgb_map"].view(1, side, side, 3).contiguous()
        batcher = npa.RayBatcher(target, K, S.N_RAYS, [0], generator=torch.Generator().manual_seed(degree))
        for p in list(S.nc.parameters()) + list(S.nf.parameters()):
            p.requires_grad_(False)

        def baked_step(refine, opt, opt_table):
            trainer.values.requires_grad_(opt_table is not None)
            rays, rgb = batcher.next(refine(POSE))
            loss = npa.img2mse(trainer.render_rays(npa.ray_records(rays, NEAR, FAR), white_bkgd=True, ray_grad=True)["rgb_map"], rgb)
            opt.zero_grad()
            if opt_table is not None:
                opt_table.zero_grad()
            loss.backward()
            opt.step()
            if opt_table is not None:
                opt_table.step()
                trainer.commit()
            return loss

        def network_step(refine, opt):
            rays, rgb = batcher.next(refine(POSE))
            out = npa.render(side, side, K, rays=rays, **S.GEO, **S.KW)
            loss = npa.img2mse(out[0], rgb) + npa.img2mse(out[3]["rgb0"], rgb)
            opt.zero_grad()
            loss.backward()
            opt.step()

        loc, joint, net = refinement(args.twist), refinement(args.twist), refinement(args.twist)
        table_opt = torch.optim.Adam(trainer.parameters(), lr=0.0)          # (lr 0: the joint step's cost without moving the table)
        times = gx.time_alternating([("localisation step (table frozen)", lambda: baked_step(*loc, None)),
                                     ("joint step (table and pose)", lambda: baked_step(*joint, table_opt)),
                                     ("network iNeRF step (fp16x3, 64 + 128 samples)", lambda: network_step(*net))], k=10, reps=args.reps, warmup=3)
        row["ms per step, alternating"] = {name: gx.row_stats(ms) for name, ms in times.items()}
        refine, opt = refinement(args.twist)
        before, losses = error_of(refine), []
        for step in range(args.steps):
            loss = baked_step(refine, opt, None)
            if step % max(1, args.steps // 10) == 0 or step == args.steps - 1:
                losses.append((step, float(loss)))
        row["recovery"] = {"before": before, "after": error_of(refine), "loss (step, img2mse)": losses}
        trainer.values.requires_grad_(True)
    result[f"sh_degree {degree}"] = row
    del field, trainer
gx.emit(result, args.out)
