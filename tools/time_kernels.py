"""Per-launch time of the heavy kernels at BASELINE's launch sizes (4096 rays x 64 / 192 samples), HIP events around batches of
back-to-back launches on torch's current stream.  For A/B timing of two builds on ONE box (boxes differ by 2-4 %):

    NERF_HIP_LIB=/path/to/other/libnerf_hip.so python tools/time_kernels.py [--precision fp16x3] [--reps 20] [--rounds 3]

prints one JSON line: {kernel: {"coarse_ms": .., "fine_ms": ..}}.  tools/ab.sh alternates two libraries.

    --live          the sparse forms of the delta chain and the weight-gradient GEMM (nerf_field_dgrad_split_live /
                    nerf_field_wgrad_phase_live; "dgrad" includes the liveness launches).  With the default d_raw = randn no tile is
                    dead: what a dense batch pays for the list.
    --dead SHARE    zero that share of d_raw's 32-point tiles, in runs of 13 tiles (with or without --live)
                    (the dead-group experiment: a library built with tools/build_variant.sh NAME -DNERF_LIVE_GROUPS=1 or 2 in
                    NERF_HIP_LIB, and NERF_BWD_LIVE_GROUP=16 or 8 in the environment; csrc/launchers.h)
    --dead-points SHARE   zero that share of the POINTS, ray by ray: one live run of (1 - SHARE) * S samples at a random place of every
                    ray, everything else zero -- the shape of a compositing gradient; dead tiles and dead groups follow from it"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import nerf_pytorch_amd as npa  # noqa: E402
import workloads as wl  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp16x3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--only", default="")
    ap.add_argument("--live", action="store_true")
    ap.add_argument("--dead", type=float, default=0.0)
    ap.add_argument("--dead-points", default="", help="one share, or coarse,fine")
    args = ap.parse_args()
    hb = npa.hip_backend
    L = hb.lib()
    dev = torch.device("cuda", 0)
    prec = args.precision
    Pc, Pf = wl.scene_params()
    net = npa.NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True).to(dev)
    net.load_state_dict(Pf)
    packed = net.packed_params(prec)
    n = args.rays
    rays = wl.synthetic_rays(n, seed=1).to(dev)
    out = {}

    def timed(fn):
        best = None
        for _ in range(args.rounds):
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t = e0.elapsed_time(e1) / args.reps
            best = t if best is None else min(best, t)
        return round(best, 4)

    for tag, S in (("coarse", 64), ("fine", 192)):
        z = torch.sort(torch.rand(n, S, device=dev) * 4 + 2, -1)[0]
        d_raw = torch.randn(n, S, 4, device=dev) * 1e-4
        if args.dead > 0:
            T = n * S // 32
            runs = torch.rand((T + 12) // 13, device=dev) < args.dead
            d_raw.view(T, 32, 4)[runs.repeat_interleave(13)[:T]] = 0.0
        if args.dead_points:
            shares = [float(x) for x in args.dead_points.split(",")]
            share = shares[0] if tag == "coarse" or len(shares) == 1 else shares[1]
            run = max(1, round((1.0 - share) * S))
            g = torch.Generator().manual_seed(S)
            start = torch.randint(0, S - run + 1, (n, 1), generator=g)
            idx = torch.arange(S).view(1, S)
            d_raw[((idx < start) | (idx >= start + run)).to(dev)] = 0.0
        raw = torch.empty(n, S, 4, device=dev)
        act = torch.empty(max(hb.act_floats(n, S), hb.act_floats(n, S, prec)), device=dev)
        delta = torch.empty(max(L.nerf_delta_floats(n, S), hb.delta_floats(n, S, prec)), device=dev)
        partial = torch.empty(L.nerf_wgrad_partial_floats(n, S), device=dev)
        grad = torch.empty(hb.N_PARAMS, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        dp = hb.DATAPATHS[prec]
        split = dp.save_split
        flat = net.flat_params()
        if split is None:
            fwd_i = lambda: L.nerf_field_fwd(packed.data_ptr(), rays.data_ptr(), 11, z.data_ptr(), n, S, raw.data_ptr(), None, s)
            fwd_s = lambda: L.nerf_field_fwd(packed.data_ptr(), rays.data_ptr(), 11, z.data_ptr(), n, S, raw.data_ptr(), act.data_ptr(), s)
            dgrad = lambda: L.nerf_field_dgrad(packed.data_ptr(), act.data_ptr(), d_raw.data_ptr(), n, S, delta.data_ptr(), s)
        else:
            fwd_i = lambda: L.nerf_field_fwd_split(packed.data_ptr(), rays.data_ptr(), 11, z.data_ptr(), n, S, raw.data_ptr(), None, dp.fwd_split, s)
            fwd_s = lambda: L.nerf_field_fwd_split(packed.data_ptr(), rays.data_ptr(), 11, z.data_ptr(), n, S, raw.data_ptr(), act.data_ptr(), split, s)
            dgrad = lambda: L.nerf_field_dgrad_split(packed.data_ptr(), act.data_ptr(), d_raw.data_ptr(), n, S, delta.data_ptr(), split, s)
        wargs = (act.data_ptr(), delta.data_ptr(), d_raw.data_ptr(), n, S, partial.data_ptr(), grad.data_ptr(), 0, -1)
        wgemm = lambda: L.nerf_field_wgrad_phase(*wargs, 3, flat.data_ptr(), s)
        wred = lambda: L.nerf_field_wgrad_phase(*wargs, 4, flat.data_ptr(), s)
        if args.live and split is not None:
            live = torch.zeros(L.nerf_live_tiles_words(n, S), dtype=torch.int32, device=dev)
            dgrad = lambda: L.nerf_field_dgrad_split_live(packed.data_ptr(), act.data_ptr(), d_raw.data_ptr(), n, S, delta.data_ptr(), split, live.data_ptr(), s)
            wgemm = lambda: L.nerf_field_wgrad_phase_live(*wargs, 3, flat.data_ptr(), live.data_ptr(), s)
        assert fwd_s() == 0 and dgrad() == 0 and wgemm() == 0 and wred() == 0, L.nerf_last_error()
        for name, fn in (("fwd_infer", fwd_i), ("fwd_save", fwd_s), ("dgrad", dgrad), ("wgrad_gemm", wgemm), ("wgrad_reduce", wred)):
            if args.only and name not in args.only.split(","):
                continue
            out.setdefault(name, {})[tag + "_ms"] = timed(fn)
    print(json.dumps({"lib": os.environ.get("NERF_HIP_LIB", "in-tree"), "precision": prec, "live": bool(args.live), "group": os.environ.get("NERF_BWD_LIVE_GROUP", "32"), "dead": args.dead,
                      "dead_points": args.dead_points, "kernels": out}))


if __name__ == "__main__":
    main()
