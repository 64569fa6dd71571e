"""Where the time of a hash-grid field goes (4096 rays x (64 + 128) samples, the default HashEncoding over [-1.5, 1.5]^3: 16 levels, F = 2,
T = 2^19, 16 .. 512 cells; HashNeRF D = 2, W = 64):
  - nerf_hash_encode_fwd alone on the 786,432 points o + d z of the batch's rays (host-timed back-to-back launches);
  - nerf_hash_encode_bwd alone, split: the maximum + the scatter (phases = 1), and the finishing pass (phases = 2); the scatter of
    single levels of 16, 64, 128 and 512 cells;
  - the TRAINING step (render() forward, two img2mse, backward, optimizer step at lr = 0) and the no-grad render of a HashNeRF pair,
    alternating in every repetition with the same of the fused NeRF pair (fp16x3, FlatAdam); one HashNeRF step with HIP events around
    the hash launches says what share of the step they are, and events between forward, backward and optimizer step split the rest;
  - 500 Adam steps of a HashNeRF pair and of the fused pair against the fixture teacher's renders of the same batches; PSNR on a
    held-out batch every 50 steps.

    python tools/exp_hash.py --out profiles/r32_exp_hash.json
"""
import grid_exp as gx

ap = gx.parser(__doc__, steps="training steps between two HIP events")
ap.add_argument("--fit-steps", type=int, default=500)
ap.add_argument("--hash-lr", type=float, default=1e-2)
ap.add_argument("--fused-lr", type=float, default=5e-4)
args = ap.parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_hash")
S = gx.Scene(wl, npa, dev, perturb=1., target=True, records=True)
N_RAYS, N_C, N_F = S.N_RAYS, 64, 128
BOUND = 1.5


def hash_pair(seed):
    torch.manual_seed(seed)
    return [npa.HashNeRF([-BOUND] * 3, [BOUND] * 3, output_ch=5).to(dev) for _ in range(2)]


# ---- the kernels alone, on the points of the batch's rays at 192 sorted depths
hc, hf = hash_pair(0)
enc = hc.encoding
desc, P, C = enc.desc(), N_RAYS * (N_C + N_F), enc.out_dim
g = torch.Generator().manual_seed(1)
z = (2.0 + 4.0 * torch.rand(N_RAYS, N_C + N_F, generator=g)).sort(1).values.to(dev).contiguous()
x = torch.empty(P, C, device=dev)
d_out = torch.randn(P, C, generator=g).to(dev)
scratch = hb.hash_scratch(desc, dev)
grad = torch.empty_like(enc.embeddings)
E = enc.embeddings.detach()
bwd = lambda ph: hb.hash_encode_bwd(desc, d_out, rays=S.records, z_vals=z, scratch=scratch, phases=ph, d_embeddings=grad)
launches = {
    "nerf_hash_encode_fwd": gx.time_launches(lambda: hb.hash_encode_fwd(desc, E, x, rays=S.records, z_vals=z), args.reps, launches=20),
    "nerf_hash_encode_bwd, maximum + scatter": gx.time_launches(lambda: bwd(1), args.reps, launches=20),
    "nerf_hash_encode_bwd, finishing pass": gx.time_launches(lambda: bwd(2), args.reps, launches=20),
    "nerf_hash_encode_bwd": gx.time_launches(lambda: bwd(3), args.reps, launches=20),
}
adds = P * enc.n_levels * 8 * enc.n_features
launches["nerf_hash_encode_fwd"]["gathered_bytes"] = adds * 4
launches["nerf_hash_encode_fwd"]["GB_per_s_host_timed"] = adds * 4 / launches["nerf_hash_encode_fwd"]["us_median"] * 1e-3
row = launches["nerf_hash_encode_bwd, maximum + scatter"]
row["added_bytes"] = adds * 8
row["GB_per_s_host_timed"] = adds * 8 / row["us_median"] * 1e-3
# one level at a time (its own one-level encoding, same T): how the scatter's time depends on how many rows share the adds
by_level = {}
for R in (16, 64, 128, 512):
    one = npa.HashEncoding([-BOUND] * 3, [BOUND] * 3, n_levels=1, base_resolution=R, finest_resolution=R).to(dev)
    s1 = hb.hash_scratch(one.desc(), dev)
    d1, g1 = d_out[:, :one.out_dim].contiguous(), torch.empty_like(one.embeddings)
    t1 = gx.time_launches(lambda: hb.hash_encode_bwd(one.desc(), d1, rays=S.records, z_vals=z, scratch=s1, phases=1, d_embeddings=g1), args.reps,
                          launches=20)
    hb.hash_encode_bwd(one.desc(), d1, rays=S.records, z_vals=z, scratch=s1, phases=2, d_embeddings=g1)
    by_level[f"R = {R} ({'dense' if one.level_dense[0] else 'hashed'}, {one.rows_total} rows)"] = t1
inside = float(((S.records[:, None, 0:3] + S.records[:, None, 3:6] * z[:, :, None]).abs().amax(-1) <= BOUND).float().mean())

# ---- the training step and the no-grad render, HashNeRF against the fused pair
adam_h = torch.optim.Adam([p for n in (hc, hf) for p in n.parameters()], lr=0.0)
adam_f = S.adam(S.nc, S.nf)
hash_kw = dict(network_fn=hc, network_fine=hf)


def no_grad(**kw):
    with torch.no_grad():
        S.render(**kw)


configs = [("HashNeRF, training step", lambda: S.fit(S.render(**hash_kw), adam_h, rgb0=True)),
           ("fused NeRF, training step", lambda: S.fit(S.render(), adam_f, rgb0=True)),
           ("HashNeRF, no_grad render", lambda: no_grad(**hash_kw)),
           ("fused NeRF, no_grad render", lambda: no_grad())]
times = gx.time_alternating(configs, args.steps, args.reps, warmup=3)
rows = {name: gx.row_stats(times[name], N_RAYS) for name, _ in configs}


def phases_of_a_step(kw, opt, reps):
    """HIP events between the forward, the backward and the optimizer step of one training step; medians over `reps` steps, ms"""
    marks = []
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        rgb, _, _, extras = S.render(**kw)
        loss = npa.img2mse(rgb, S.target) + npa.img2mse(extras["rgb0"], S.target)
        ev[1].record()
        opt.zero_grad()
        loss.backward()
        ev[2].record()
        opt.step()
        ev[3].record()
        torch.cuda.synchronize()
        marks.append([ev[i].elapsed_time(ev[i + 1]) for i in range(3)])
    med = [sorted(m[i] for m in marks)[len(marks) // 2] for i in range(3)]
    return {"forward_ms": med[0], "backward_ms": med[1], "optimizer_ms": med[2]}


rows["HashNeRF, training step"]["phases"] = phases_of_a_step(hash_kw, adam_h, args.reps)
rows["fused NeRF, training step"]["phases"] = phases_of_a_step({}, adam_f, args.reps)
summary = gx.kernel_summary(hb, configs[0][1])
hash_ms = {k: v["ms"] for k, v in summary.items() if k.startswith("hash_")}
rows["HashNeRF, training step"]["hash_launches_ms_in_one_step"] = hash_ms
rows["HashNeRF, training step"]["hash_share_of_step"] = sum(hash_ms.values()) / rows["HashNeRF, training step"]["ms_median"]

# ---- 500 Adam steps against the teacher's renders
teacher, student, held, held_target = S.teacher_and_held_out()


def fit(nets, opt, steps):
    kw = dict(network_fn=nets[0], network_fine=nets[1])
    curve = []
    for step in range(steps + 1):
        if step % 50 == 0:
            with torch.no_grad():
                curve.append({"step": step, "psnr_db": gx.psnr_db(S.render(held, perturb=0., **kw)[0], held_target)})
        if step == steps:
            break
        batch = wl.lego_batch(N_RAYS, seed=2000 + step).to(dev)
        with torch.no_grad():
            want = S.render(batch, **teacher)[0]
        rgb, _, _, extras = S.render(batch, **kw)
        loss = npa.img2mse(rgb, want) + npa.img2mse(extras["rgb0"], want)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return curve


fit_h = hash_pair(1)
curve_h = fit(fit_h, torch.optim.Adam([p for n in fit_h for p in n.parameters()], lr=args.hash_lr, betas=(0.9, 0.999)), args.fit_steps)
fit_f = S.networks(*student)
curve_f = fit(fit_f, npa.FlatAdam([p for n in fit_f for p in n.parameters()], lr=args.fused_lr), args.fit_steps)

gx.emit({"tree": args.label, "rays": N_RAYS, "samples": "64 + 128", "points": P, "one run on one machine": True,
         "encoding": {"levels": enc.n_levels, "features": enc.n_features, "log2_hashmap_size": enc.log2_hashmap_size,
                      "resolutions": enc.level_resolution, "dense": enc.level_dense, "rows": enc.rows_total, "box": [-BOUND, BOUND],
                      "share_of_points_inside_the_box": inside},
         "network": "HashNeRF D = 2, W = 64, view directions with 4 frequencies; the fused pair: D = 8, W = 256 at fp16x3",
         "launches_alone": launches, "scatter_of_one_level_alone": by_level,
         "step": "render() forward, two img2mse, backward, optimizer step (lr = 0): torch.optim.Adam for HashNeRF, FlatAdam for the fused pair",
         "steps_per_timing": args.steps, "alternating": rows,
         "fit": {"steps": args.fit_steps, "target": "the teacher pair's render of each step's batch (perturb = 0), PSNR on a held-out batch",
                 "HashNeRF": {"lr": args.hash_lr, "optimizer": "torch.optim.Adam", "curve": curve_h},
                 "fused NeRF": {"lr": args.fused_lr, "optimizer": "FlatAdam", "curve": curve_f}}}, args.out)
