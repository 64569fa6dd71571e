"""Fine-tuning a baked field through its renderer (baked.BakedTrainer, csrc/baked_train.hip) on one MI355X: the fixture fine network baked
into a grid over [-2, 2]^3 (OccupancyGrid.from_network, threshold 0, one round of dilation; n_dirs 32, step = half a cell), teacher frames
rendered from the two networks under no_grad at a handful of poses on a circle, and per sh_degree 0 / 1 / 2
  * --steps Adam steps on random 4096-ray batches drawn from all poses but one, white background, img2mse against the teacher's pixels,
    commit() after every step;
  * the PSNR of the baked frame against the teacher's at the held-out pose, before and after;
  * the time of one step's stages on one such batch, HIP events around each stage alone: count, forward, sort / index (cumsum, stable
    sort, segment starts), sample backward, row backward;
  * the samples per stored row of that batch (median and maximum over the rows that got any, and over all rows): the row pass runs as
    long as its most loaded lane group.
The fixture scene is a fog (tools/exp_baked.py).  Whatever the PSNR gain is, it is this fog's on this one run.

    python tools/exp_baked_finetune.py --out profiles/r27_exp_baked_finetune.json
"""
import grid_exp as gx

ap = gx.parser(__doc__, steps="Adam steps per degree")
ap.add_argument("--resolution", type=int, default=128)
ap.add_argument("--side", type=int, default=200, help="the frames are side x side")
ap.add_argument("--lr", type=float, default=0.02)
ap.add_argument("--thetas", type=float, nargs="+", default=[-90.0, -30.0, 90.0, 150.0, 30.0], help="poses on the circle; the last one is held out")
ap.set_defaults(steps=300)
args = ap.parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_baked_finetune")
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


def stage_times(trainer, rays, reps):
    """ms per stage of one step on `rays`, each stage alone between HIP events, medians of `reps`; and the inverted index of the batch"""
    desc = trainer.grid._desc()
    n = rays.shape[0]
    g = [torch.randn(n, 3, device=dev), torch.randn(n, device=dev), torch.randn(n, device=dev)]
    state, times = {}, {}

    def count():
        state["counts"] = hb.baked_count(desc, rays, None, trainer.step_size, 1 << 14)

    def offsets():
        off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(state["counts"], 0)
        state["total"] = int(off[-1])
        state["offsets"] = off.to(torch.int32)

    def forward():
        state["records"] = hb.baked_train_fwd(desc, trainer.index, trainer.table, trainer.sh_degree, rays, None, trainer.step_size, 1 << 14, True,
                                              state["offsets"], state["total"])[3]

    def samples():
        state["grads"] = hb.baked_train_bwd_samples(state["records"], state["offsets"], state["total"], trainer.step_size, True, *g)

    def index():
        state["order"], state["start"] = npa.baked.inverted_index(state["records"][:state["total"], 0].view(torch.int32), trainer.grid.n_cells)

    def rows():
        hb.baked_train_bwd_rows(desc, trainer.row_node, trainer.sh_degree, rays, state["records"], state["grads"], state["order"], state["start"],
                                state["total"])
    for name, stage in (("count", count), ("offsets (cumsum, read back)", offsets), ("forward", forward), ("sample backward", samples),
                        ("sort / index", index), ("row backward", rows)):
        ms = []
        for _ in range(reps + 1):           # (the first call warms the stage up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            stage()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        times[name] = gx.row_stats(ms[1:])
    times["sum of the medians"] = sum(v["ms_median"] for v in times.values())
    return times, state


def samples_per_row(trainer, state):
    """per stored row the samples of its up to eight adjacent cells"""
    rx, ry, rz = trainer.grid.resolution
    start = state["start"].to(torch.int64)
    per_cell = (start[1:] - start[:-1]).view(rx, ry, rz)
    per_node = torch.zeros((rx + 1, ry + 1, rz + 1), dtype=torch.int64, device=dev)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                per_node[dx:dx + rx, dy:dy + ry, dz:dz + rz] += per_cell
    per_row = per_node.reshape(-1)[trainer.row_node[1:].to(torch.int64)].double()
    hit = per_row[per_row > 0]
    return {"samples": state["total"], "rows": int(per_row.numel()), "rows with samples": int(hit.numel()),
            "median over the rows with samples": float(hit.median()) if hit.numel() else 0.0, "median over all rows": float(per_row.median()),
            "maximum": float(per_row.max()), "mean over the rows with samples": float(hit.mean()) if hit.numel() else 0.0}


grid = npa.OccupancyGrid.from_network(S.nf, S.LO, S.HI, args.resolution)
teacher = [frame(c2w, occupancy=grid) for c2w in POSES]
train_rays = torch.cat([records_of(c2w) for c2w in POSES[:-1]], 0)
train_rgb = torch.cat([t.reshape(-1, 3) for t in teacher[:-1]], 0)
result = {"tree": args.label, "grid": f"{args.resolution}^3", "fraction_occupied": grid.fraction_occupied(), "frames": f"{side}x{side}",
          "thetas (the last is held out)": args.thetas, "steps": args.steps, "lr": args.lr, "batch": S.N_RAYS, "optimizer": "torch.optim.Adam",
          "scene": "fog (worst case), one run"}
for degree in (0, 1, 2):
    field = npa.BakedField.from_network(S.nf, grid, sh_degree=degree, n_dirs=32)
    row = {"rows": field.n_rows, "psnr_db held out, before": gx.psnr_db(frame(POSES[-1], baked=field), teacher[-1]),
           "psnr_db first training pose, before": gx.psnr_db(frame(POSES[0], baked=field), teacher[0])}
    # the records built here are render()'s: the same frame both ways
    direct = field.render_rays(records_of(POSES[-1]), white_bkgd=True)["rgb_map"].view(side, side, 3)
    row["largest difference of render(baked=) and render_rays on these records"] = float((direct - frame(POSES[-1], baked=field)).abs().max())
    trainer = field.trainable()
    opt = torch.optim.Adam(trainer.parameters(), lr=args.lr)
    pick = torch.Generator(device="cpu").manual_seed(degree)
    losses = []
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for step in range(args.steps):
        sel = torch.randint(0, train_rays.shape[0], (S.N_RAYS,), generator=pick).to(dev)
        opt.zero_grad()
        loss = npa.img2mse(trainer.render_rays(train_rays[sel], white_bkgd=True)["rgb_map"], train_rgb[sel])
        loss.backward()
        opt.step()
        trainer.commit()
        if step % max(1, args.steps // 10) == 0 or step == args.steps - 1:
            losses.append((step, float(loss)))
    e1.record()
    torch.cuda.synchronize()
    row["ms per step, whole loop (with the optimiser, commit and the batch's gather)"] = e0.elapsed_time(e1) / max(1, args.steps)
    row["loss (step, img2mse)"] = losses
    tuned = trainer.to_field()
    row["psnr_db held out, after"] = gx.psnr_db(frame(POSES[-1], baked=tuned), teacher[-1])
    row["psnr_db first training pose, after"] = gx.psnr_db(frame(POSES[0], baked=tuned), teacher[0])
    batch = train_rays[torch.randint(0, train_rays.shape[0], (S.N_RAYS,), generator=pick).to(dev)].contiguous()
    times, state = stage_times(trainer, batch, args.reps)
    row["ms per stage, 4096 rays"] = times
    row["samples per ray"] = state["total"] / S.N_RAYS
    row["samples per row"] = samples_per_row(trainer, state)
    result[f"sh_degree {degree}"] = row
    del field, trainer, tuned, opt
gx.emit(result, args.out)
