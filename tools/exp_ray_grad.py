"""Cost of the gradients to the ray records (nerf_field_input_grad + the compositing's geometry adjoint) at the bench shape,
4096 rays x (64 + 128) samples, lego-like, through render(rays=(o, d)) on fp16x3 and fp32:
  (a) a training step (parameters require grad, rays do not),
  (b) the same step with the ray origins / directions requiring grad,
  (c) frozen networks, only the rays requiring grad (the iNeRF pose-refinement step).
Median wall time per step over --steps after --warmup, plus one KernelTimer pass per case (per-kernel ms, algorithmic bytes).
Writes one JSON object to stdout (and --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import torch  # noqa: E402

import nerf_pytorch_amd as npa  # noqa: E402
import workloads as wl  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    hb = npa.hip_backend
    cfg = wl.LEGO
    K = wl.intrinsics(cfg)
    Pc, Pf = wl.scene_params()
    kw = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    nc, nf = npa.NeRF(**kw).to(dev), npa.NeRF(**kw).to(dev)
    nc.load_state_dict(Pc)
    nf.load_state_dict(Pf)
    batch = wl.lego_batch(a.rays, seed=3).to(dev)
    target = torch.rand(a.rays, 3, generator=torch.Generator().manual_seed(0)).to(dev)
    rk = dict(network_fn=nc, network_fine=nf, network_query_fn=None, N_samples=64, N_importance=128, perturb=1.0, white_bkgd=True,
              raw_noise_std=0.0, use_viewdirs=True, ndc=False, near=cfg["near"], far=cfg["far"])

    def step(case):
        params_grad = case != "c"
        for m in (nc, nf):
            m.requires_grad_(params_grad)
            m.zero_grad(set_to_none=True)
        o, d = batch[0], batch[1]
        if case != "a":
            o, d = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
        rgb, _, _, ex = npa.render(cfg["H"], cfg["W"], K, chunk=32768, rays=(o, d), **rk)
        (npa.img2mse(rgb, target) + npa.img2mse(ex["rgb0"], target)).backward()

    res = {"rays": a.rays, "samples": [64, 128], "steps": a.steps, "warmup": a.warmup, "cases": {}}
    for prec in ("fp16x3", "fp32"):
        npa.set_precision(prec)
        for case in ("a", "b", "c"):
            for _ in range(a.warmup):
                step(case)
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                step(case)
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            hb.TIMER = hb.KernelTimer()
            step(case)
            kern = hb.TIMER.summary()
            hb.TIMER = None
            ig = kern.get("field_input_grad_kernel")
            floor_ms = ig["bytes"] / 6.3e9 if ig else None        # at the 6.3 TB/s the guide calls achievable
            res["cases"][f"{prec}/{case}"] = {"step_ms_median": statistics.median(ts), "step_ms_min": min(ts),
                                              "kernels_ms": {k: round(v["ms"], 4) for k, v in kern.items()},
                                              "input_grad_ms": ig["ms"] if ig else None, "input_grad_byte_floor_ms": floor_ms}
    for m in (nc, nf):
        m.requires_grad_(True)
    for prec in ("fp16x3", "fp32"):
        c = res["cases"]
        c[f"{prec}/b"]["added_over_a_ms"] = c[f"{prec}/b"]["step_ms_median"] - c[f"{prec}/a"]["step_ms_median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
