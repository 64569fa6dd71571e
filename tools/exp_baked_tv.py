"""The regularisers of a baked field's table (BakedTrainer.regularizers, csrc/baked_reg.hip) on one MI355X: the fixture fine network baked
into a grid over [-2, 2]^3 as tools/exp_baked_finetune.py bakes it, and per sh_degree 0 / 1 / 2
  * the two kernels alone on the whole table: HIP events around every launch (median of --reps launches) and host-timed back-to-back
    launches, against their bytes by arithmetic -- forward: the table in, 12 B per row out, the two index arrays in; backward: the table
    in once (the 13-row gather served by cache), the gradient out, the index arrays in -- and against --hbm-tbs, the rate the heaviest
    kernel of the library reaches (6.07 TB/s);
  * exp_baked_finetune's protocol again -- teacher frames at five poses on a circle, --steps Adam steps on random 4096-ray batches from
    four of them, the same seeds -- with lambda = 0 and with a sweep of weights on tv_sigma and tv_sh: the PSNR at the first training pose
    and at the held-out pose, before and after, and the three regularisers before and after; the time of a step with the terms.
The fixture scene is a fog (tools/exp_baked.py).  Whatever the regularisers do to the held-out PSNR, it is this fog's on this one run.

    python tools/exp_baked_tv.py --out profiles/r28_exp_baked_tv.json
"""
import statistics

import grid_exp as gx

ap = gx.parser(__doc__, steps="Adam steps per configuration")
ap.add_argument("--resolution", type=int, default=128)
ap.add_argument("--side", type=int, default=200, help="the frames are side x side")
ap.add_argument("--lr", type=float, default=0.02)
ap.add_argument("--thetas", type=float, nargs="+", default=[-90.0, -30.0, 90.0, 150.0, 30.0], help="poses on the circle; the last one is held out")
ap.add_argument("--weights", type=float, nargs="+", default=[0.0, 1e-5, 1e-4, 1e-3, 1e-2], help="the weight of tv_sigma and of tv_sh, one run each")
ap.add_argument("--hbm-tbs", type=float, default=6.07, help="the HBM rate a streaming kernel of this library reaches, TB/s")
ap.set_defaults(steps=300, reps=20)
args = ap.parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_baked_tv")
S = gx.Scene(wl, npa, dev, perturb=0.)
side = args.side
K = wl.intrinsics(dict(H=side, W=side, focal=1111.0 * side / S.H))
POSES = [wl.pose_spherical(theta, -30.0, 4.0)[:3, :4].to(dev) for theta in args.thetas]


def frame(c2w, **over):
    with torch.no_grad():
        return npa.render(side, side, K, c2w=c2w, **S.GEO, **dict(S.KW, **over))[0]


def records_of(c2w):
    """the ray records [side^2, 11] of a frame: o, d, near, far, viewdir, as render() assembles them"""
    o, d = npa.get_rays(side, side, K, c2w)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    view = d / d.norm(dim=-1, keepdim=True)
    near, far = (torch.full_like(o[:, :1], S.GEO[k]) for k in ("near", "far"))
    return torch.cat([o, d, near, far, view], -1).float().contiguous()


def kernel_times(trainer):
    """the two launches alone on the trainer's whole table"""
    desc, values, scales = trainer.grid._desc(), trainer.values.detach(), trainer.axis_scale
    g = torch.tensor([1.0, 0.5, 0.25], device=dev) / (trainer.n_rows - 1)
    fwd = lambda: hb.baked_reg_fwd(desc, trainer.index, trainer.row_node, values, trainer.sh_degree, scales, 1e-9)
    bwd = lambda: hb.baked_reg_bwd(desc, trainer.index, trainer.row_node, values, trainer.sh_degree, scales, 1e-9, g)
    out = {}
    for name, thunk in (("baked_reg_fwd_kernel", fwd), ("baked_reg_bwd_kernel", bwd)):
        thunk()
        per_launch = []
        for _ in range(args.reps):
            per_launch.append(gx.kernel_summary(hb, thunk)[name])
        nbytes = per_launch[0]["bytes"]
        us = statistics.median(v["ms"] for v in per_launch) * 1e3
        back = gx.time_launches(thunk, 5, launches=50)
        out[name] = {"us per launch, HIP events around one launch (median)": us, "us per launch, back to back": back,
                     "MB by arithmetic": nbytes / 1e6, "TB/s by arithmetic (events)": nbytes / us / 1e6,
                     "us at --hbm-tbs": nbytes / args.hbm_tbs / 1e6, "time over the time at --hbm-tbs": us / (nbytes / args.hbm_tbs / 1e6)}
    return out


def scalars(trainer):
    with torch.no_grad():
        return {k: float(v) for k, v in trainer.regularizers().items()}


grid = npa.OccupancyGrid.from_network(S.nf, S.LO, S.HI, args.resolution)
teacher = [frame(c2w, occupancy=grid) for c2w in POSES]
train_rays = torch.cat([records_of(c2w) for c2w in POSES[:-1]], 0)
train_rgb = torch.cat([t.reshape(-1, 3) for t in teacher[:-1]], 0)
result = {"tree": args.label, "grid": f"{args.resolution}^3", "fraction_occupied": grid.fraction_occupied(), "frames": f"{side}x{side}",
          "thetas (the last is held out)": args.thetas, "steps": args.steps, "lr": args.lr, "batch": S.N_RAYS, "optimizer": "torch.optim.Adam",
          "loss": "img2mse + weight * (tv_sigma + tv_sh), eps 1e-9", "hbm_tbs": args.hbm_tbs, "scene": "fog (worst case), one run"}
for degree in (0, 1, 2):
    field = npa.BakedField.from_network(S.nf, grid, sh_degree=degree, n_dirs=32)
    row = {"rows": field.n_rows, "psnr_db held out, before": gx.psnr_db(frame(POSES[-1], baked=field), teacher[-1]),
           "psnr_db first training pose, before": gx.psnr_db(frame(POSES[0], baked=field), teacher[0])}
    trainer = field.trainable()
    row["regularisers of the baked table"] = scalars(trainer)
    row["kernels alone"] = kernel_times(trainer)
    for weight in args.weights:
        trainer = field.trainable()
        opt = torch.optim.Adam(trainer.parameters(), lr=args.lr)
        pick = torch.Generator(device="cpu").manual_seed(degree)        # exp_baked_finetune's batches
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for step in range(args.steps):
            sel = torch.randint(0, train_rays.shape[0], (S.N_RAYS,), generator=pick).to(dev)
            opt.zero_grad()
            loss = npa.img2mse(trainer.render_rays(train_rays[sel], white_bkgd=True)["rgb_map"], train_rgb[sel])
            if weight > 0.0:
                reg = trainer.regularizers()
                loss = loss + weight * (reg["tv_sigma"] + reg["tv_sh"])
            loss.backward()
            opt.step()
            trainer.commit()
        e1.record()
        torch.cuda.synchronize()
        tuned = trainer.to_field()
        run = {"ms per step, whole loop": e0.elapsed_time(e1) / max(1, args.steps), "last loss": float(loss.detach()),
               "psnr_db held out, after": gx.psnr_db(frame(POSES[-1], baked=tuned), teacher[-1]),
               "psnr_db first training pose, after": gx.psnr_db(frame(POSES[0], baked=tuned), teacher[0]),
               "regularisers, after": scalars(trainer)}
        row[f"weight {weight:g}"] = run
        del trainer, tuned, opt
    base = row[f"weight {args.weights[0]:g}"]
    for weight in args.weights[1:]:
        run = row[f"weight {weight:g}"]
        for k in ("psnr_db held out, after", "psnr_db first training pose, after"):
            run[k.replace(", after", f", against weight {args.weights[0]:g}")] = run[k] - base[k]
    result[f"sh_degree {degree}"] = row
    del field
gx.emit(result, args.out)
