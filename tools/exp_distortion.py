"""What render_rays(distortion=True) costs (fp16x3, 4096 rays x (64 + 128) samples):
  - the two launches alone, nerf_distortion_fwd and nerf_distortion_bwd on [4096, 192] weights of a rendered batch (host-timed
    back-to-back launches, microseconds per call), next to nerf_raw2outputs with and without the weights store;
  - the TRAINING step through render() -- forward, img2mse of both images (+ 0.1 * mean distortion with the option), backward,
    FlatAdam.step (lr = 0) -- with and without the option, on the dense path and through a DensityGrid whose ball mask is bisected
    to an evaluated share of about 0.25 (outside skipped); the configurations alternate inside every repetition.
The option off against the parent commit: tools/exp_occupancy.py and tools/exp_occupancy_train.py with --root <checkout of the parent>,
as the earlier grid changes did.

    python tools/exp_distortion.py --out profiles/r23_exp_distortion.json
"""
import grid_exp as gx

ap = gx.parser(__doc__, steps="training steps between two HIP events")
args = ap.parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_distortion")
S = gx.Scene(wl, npa, dev, perturb=1., target=True, records=True)
N_RAYS, nc, nf = S.N_RAYS, S.nc, S.nf
opt = S.adam(nc, nf)
LAM = 0.1


def step(grid, option):
    kw = dict(occupancy=grid) if grid is not None else {}
    rgb, _, _, extras = S.render(distortion=option, **kw)
    loss = npa.img2mse(rgb, S.target) + npa.img2mse(extras["rgb0"], S.target)
    if option:
        loss = loss + LAM * extras["distortion"].mean()
    opt.zero_grad()
    loss.backward()
    opt.step()


def share_of(grid):
    torch.manual_seed(0)
    with torch.no_grad():
        S.render(occupancy=grid)
    return gx.evaluated_share(grid)


# ---- the launches alone, on the refining pass's weights and depths of the batch
seen = []
real = hb.raw2outputs
hb.raw2outputs = lambda raw, z, *a, **k: (lambda r: (seen.append((raw, z, r[3])), r)[1])(real(raw, z, *a, **k))
try:
    with torch.no_grad():
        npa.render_rays(S.records, nc, None, N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1., distortion=True)
finally:
    hb.raw2outputs = real
raw, z, w = seen[-1]
d_loss = torch.full((N_RAYS,), LAM / N_RAYS, device=dev)
d_w = torch.empty_like(w)
launches = {
    "nerf_distortion_fwd": gx.time_launches(lambda: hb.distortion(w, z, S.records, nf_stride=11, nf_offset=6), args.reps),
    "nerf_distortion_bwd": gx.time_launches(lambda: hb.distortion_bwd(w, z, S.records, d_loss, out=d_w, nf_stride=11, nf_offset=6), args.reps),
    "nerf_raw2outputs": gx.time_launches(lambda: real(raw, z, S.records, 11, None, 0.0, True, want_weights=False, want_depth=False,
                                                      rays_d_offset=3), args.reps),
    "nerf_raw2outputs + weights": gx.time_launches(lambda: real(raw, z, S.records, 11, None, 0.0, True, want_weights=True, want_depth=False,
                                                                rays_d_offset=3), args.reps),
}
bytes_per_launch = 2 * w.numel() * 4
for name in ("nerf_distortion_fwd", "nerf_distortion_bwd"):
    extra = w.numel() * 4 if name.endswith("bwd") else 0
    launches[name]["algorithmic_bytes"] = bytes_per_launch + extra
    launches[name]["GB_per_s_host_timed"] = (bytes_per_launch + extra) / launches[name]["us_median"] * 1e-3

# ---- the training step
grid, radius = S.ball_with_share(npa.DensityGrid, share_of, 0.25)
configs = [("dense, off", None, False), ("dense, distortion", None, True),
           (f"DensityGrid share 0.25 (ball r = {radius:.3f}), off", grid, False), (f"DensityGrid share 0.25 (ball r = {radius:.3f}), distortion", grid, True)]
times = gx.time_alternating([(name, lambda g=g, o=o: step(g, o)) for name, g, o in configs], args.steps, args.reps, warmup=3)
rows = {name: gx.row_stats(times[name], N_RAYS) for name, _, _ in configs}
for (off, _, _), (on, _, _) in (configs[0:2], configs[2:4]):
    rows[on]["ms_over_off"] = rows[on]["ms_median"] - rows[off]["ms_median"]
gx.emit({"precision": "fp16x3", "rays": N_RAYS, "samples": "64 + 128", "tree": args.label, "lambda": LAM,
         "step": "render() forward, two img2mse (+ lambda * mean distortion), backward, FlatAdam.step (lr = 0)", "steps_per_timing": args.steps,
         "launches_alone_4096x192": launches, "train_step_4096_rays": rows}, args.out)
