"""What render_rays(interlevel=True) costs (fp16x3, 4096 rays x (64 + 128) samples):
  - the two launches alone, nerf_interlevel_fwd and nerf_interlevel_bwd on the [4096, 64] coarse and [4096, 192] refined weights and
    depths of a rendered batch (host-timed back-to-back launches, microseconds per call), next to nerf_distortion_fwd / _bwd on the
    refined weights;
  - the TRAINING step through render() -- forward, img2mse of both images (+ 0.1 * mean interlevel with the option), backward,
    FlatAdam.step (lr = 0) -- with and without the option, on the dense path and through a DensityGrid whose ball mask is bisected
    to an evaluated share of about 0.25 (outside skipped); the configurations alternate inside every repetition.
The option off against the parent commit: bench.py alternated between the two checkouts.

    python tools/exp_interlevel.py --out profiles/r24_exp_interlevel.json
"""
import grid_exp as gx

ap = gx.parser(__doc__, steps="training steps between two HIP events")
args = ap.parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_interlevel")
S = gx.Scene(wl, npa, dev, perturb=1., target=True, records=True)
N_RAYS, nc, nf = S.N_RAYS, S.nc, S.nf
opt = S.adam(nc, nf)
LAM = 0.1


def step(grid, option):
    kw = dict(occupancy=grid) if grid is not None else {}
    rgb, _, _, extras = S.render(interlevel=option, **kw)
    loss = npa.img2mse(rgb, S.target) + npa.img2mse(extras["rgb0"], S.target)
    if option:
        loss = loss + LAM * extras["interlevel"].mean()
    opt.zero_grad()
    loss.backward()
    opt.step()


def share_of(grid):
    torch.manual_seed(0)
    with torch.no_grad():
        S.render(occupancy=grid)
    return gx.evaluated_share(grid)


# ---- the launches alone, on both passes' weights and depths of the batch
seen = []
real = hb.raw2outputs
hb.raw2outputs = lambda raw, z, *a, **k: (lambda r: (seen.append((z, r[3])), r)[1])(real(raw, z, *a, **k))
try:
    with torch.no_grad():
        out = npa.render_rays(S.records, nc, None, N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1., interlevel=True)
finally:
    hb.raw2outputs = real
(z_c, w_c), (z_f, w_f) = seen[0], seen[-1]
d_loss = torch.full((N_RAYS,), LAM / N_RAYS, device=dev)
d_wc, d_wf = torch.empty_like(w_c), torch.empty_like(w_f)
launches = {
    "nerf_interlevel_fwd": gx.time_launches(lambda: hb.interlevel(w_c, z_c, w_f, z_f), args.reps),
    "nerf_interlevel_bwd": gx.time_launches(lambda: hb.interlevel_bwd(w_c, z_c, w_f, z_f, d_loss, out=d_wc), args.reps),
    "nerf_distortion_fwd": gx.time_launches(lambda: hb.distortion(w_f, z_f, S.records, nf_stride=11, nf_offset=6), args.reps),
    "nerf_distortion_bwd": gx.time_launches(lambda: hb.distortion_bwd(w_f, z_f, S.records, d_loss, out=d_wf, nf_stride=11, nf_offset=6), args.reps),
}
read_bytes = 2 * (w_c.numel() + w_f.numel()) * 4         # 8 B per proposal point + 8 B per target point
for name, extra in (("nerf_interlevel_fwd", 4 * N_RAYS), ("nerf_interlevel_bwd", 4 * w_c.numel() + 4 * N_RAYS)):
    launches[name]["algorithmic_bytes"] = read_bytes + extra
    launches[name]["GB_per_s_host_timed"] = (read_bytes + extra) / launches[name]["us_median"] * 1e-3
positive = float((out["interlevel"] > 0).float().mean())

# ---- the training step
grid, radius = S.ball_with_share(npa.DensityGrid, share_of, 0.25)
configs = [("dense, off", None, False), ("dense, interlevel", None, True),
           (f"DensityGrid share 0.25 (ball r = {radius:.3f}), off", grid, False), (f"DensityGrid share 0.25 (ball r = {radius:.3f}), interlevel", grid, True)]
times = gx.time_alternating([(name, lambda g=g, o=o: step(g, o)) for name, g, o in configs], args.steps, args.reps, warmup=3)
rows = {name: gx.row_stats(times[name], N_RAYS) for name, _, _ in configs}
for (off, _, _), (on, _, _) in (configs[0:2], configs[2:4]):
    rows[on]["ms_over_off"] = rows[on]["ms_median"] - rows[off]["ms_median"]
gx.emit({"precision": "fp16x3", "rays": N_RAYS, "samples": "64 + 128", "tree": args.label, "lambda": LAM,
         "step": "render() forward, two img2mse (+ lambda * mean interlevel), backward, FlatAdam.step (lr = 0)", "steps_per_timing": args.steps,
         "rays_with_a_positive_loss": positive, "launches_alone_4096x(64|192)": launches, "train_step_4096_rays": rows}, args.out)
