"""Cost of camera-pose refinement in the ray-batch layer, on the GPU:
  (a) the ray-batch samplers at N_rand = 4096: sample_ray_batch on one 800 x 800 view, RayBatcher.next over 100 views of 800 x 800
      (nerf_sample_ray_views);
  (b) nerf_ray_pose_grad on a 4096-ray batch: one view (views = NULL) and 100 views;
  (c) a 4096-ray fp16x3 training step (RayBatcher -> render(rays=...) -> img2mse x2 -> backward -> FlatAdam), without and with pose
      refinement (PoseRefinement + Adam on its xi), alternating step by step in the same run.
Times are host clocks around windows that end in a device synchronise: (a) and (b) per call over --reps calls, (c) per step.
--profile: a short pass over every case (no timing) for `rocprofv3 --kernel-trace --stats`, run on its own.
Writes one JSON object to stdout (and --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import nerf_pytorch_amd as npa  # noqa: E402
import workloads as wl  # noqa: E402


def per_call_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.profile:
        a.reps, a.steps, a.warmup = 20, 3, 1
    dev = torch.device("cuda", 0)
    hb = npa.hip_backend
    H = W = a.size
    V, N = a.views, a.rays
    K = np.array([[1111.0, 0, 0.5 * W], [0, 1111.0, 0.5 * H], [0, 0, 1]])
    images = torch.rand(V, H, W, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    poses = torch.stack([wl.pose_spherical(360.0 * v / V, -30.0, 4.0) for v in range(V)]).float().to(dev)
    res = {"rays": N, "views": V, "H": H, "W": W, "reps": a.reps, "steps": a.steps, "warmup": a.warmup}

    # (a) samplers
    res["sample_ray_batch_1view_us"] = per_call_us(lambda: npa.sample_ray_batch(H, W, K, poses[0, :3, :4], images[0], N), a.reps)
    batcher = npa.RayBatcher(images, K, N, list(range(V)))
    res["ray_batcher_next_us"] = per_call_us(lambda: batcher.next(poses), a.reps)
    res["sampler_bytes_per_ray"] = {"sample_ray_batch": 36 + 12, "sample_ray_views": 36 + 12 + 4 + 48}   # writes; reads (colour, view id, pose)

    # (b) pose adjoint
    _, _, pix, views = batcher.next(poses, return_pixels=True, return_views=True)
    d_rays = torch.randn(2, pix.numel(), 3, device=dev)
    d_pose1 = torch.empty(1, 3, 4, device=dev)
    d_poseV = torch.empty(V, 3, 4, device=dev)
    res["ray_pose_grad_1view_us"] = per_call_us(lambda: hb.ray_pose_grad(W, K, d_rays, pix, None, 1, d_pose1), a.reps)
    res["ray_pose_grad_views_us"] = per_call_us(lambda: hb.ray_pose_grad(W, K, d_rays, pix, views, V, d_poseV), a.reps)
    res["ray_pose_grad_bytes"] = {"1view": N * 28, "views": V * N * 32}       # d_rays + pixel (+ view id) per ray, once per block

    # (c) training step with / without refinement
    npa.set_precision("fp16x3")
    Pc, Pf = wl.scene_params()
    kw_net = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    nc, nf = npa.NeRF(**kw_net).to(dev), npa.NeRF(**kw_net).to(dev)
    nc.load_state_dict(Pc)
    nf.load_state_dict(Pf)
    opt = npa.FlatAdam(list(nc.parameters()) + list(nf.parameters()), lr=5e-4)
    refine = npa.PoseRefinement(V).to(dev)
    opt_pose = torch.optim.Adam(refine.parameters(), lr=1e-3)
    rk = dict(network_fn=nc, network_fine=nf, network_query_fn=None, N_samples=64, N_importance=128, perturb=1.0, white_bkgd=True,
              raw_noise_std=0.0, use_viewdirs=True, ndc=False, near=2.0, far=6.0, chunk=32768)

    def step(with_pose):
        batch_rays, target = batcher.next(refine(poses) if with_pose else poses)
        rgb, _, _, ex = npa.render(H, W, K, rays=batch_rays, **rk)
        opt.zero_grad()
        if with_pose:
            opt_pose.zero_grad()
        (npa.img2mse(rgb, target) + npa.img2mse(ex["rgb0"], target)).backward()
        opt.step()
        if with_pose:
            opt_pose.step()

    for _ in range(a.warmup):
        step(False)
        step(True)
    ts = {False: [], True: []}
    for _ in range(a.steps):
        for case in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(case)
            torch.cuda.synchronize()
            ts[case].append(1e3 * (time.perf_counter() - t0))
    res["step_ms_median"] = {"plain": statistics.median(ts[False]), "pose_refinement": statistics.median(ts[True])}
    res["step_ms_min"] = {"plain": min(ts[False]), "pose_refinement": min(ts[True])}
    res["refinement_added_ms"] = res["step_ms_median"]["pose_refinement"] - res["step_ms_median"]["plain"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
