"""The measuring harness the grid experiment scripts share (exp_occupancy, exp_occupancy_train, exp_ray_clip, exp_grid_proposal,
exp_early_stop, exp_march): the command line, the scene, the ball masks and their bisection, the timers, the JSON writer.  A script
keeps its closures, its configurations and the fields it adds per row.  The library comes from --root and is imported by load(), never
here: this module imports without a GPU.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch


def parser(description, steps=None, trace=None):
    """--root / --label / --out / --reps, and --steps / --trace where a help text is given; the script adds its own flags"""
    ap = argparse.ArgumentParser(description=description, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this commit", help="what --root is, for the record")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    if steps:
        ap.add_argument("--steps", type=int, default=10, help=steps)
    if trace:
        ap.add_argument("--trace", action="store_true", help=trace)
    return ap


def load(args, who):
    """import the tree under --root; returns (torch, workloads, nerf_pytorch_amd, hip_backend, device)"""
    sys.path.insert(0, os.path.abspath(args.root))
    import workloads as wl
    import nerf_pytorch_amd as npa
    if not torch.cuda.is_available():
        raise SystemExit(f"{who}: needs the GPU (no timing without one)")
    return torch, wl, npa, npa.hip_backend, torch.device("cuda", 0)


class Scene:
    """The set-up of every grid script: the two fixture networks at fp16x3, the [-2, 2]^3 box at 128^3, the 800 x 800 camera and the
    4096-ray batch.  `target`: the seed-2 colours a training step fits; `records`: the ray records render() makes of the batch."""
    LO, HI, R = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), 128
    H = W = 800
    N_RAYS = 4096
    GEO = dict(chunk=32768, ndc=False, near=2., far=6., use_viewdirs=True)
    NET = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)

    def __init__(self, wl, npa, dev, perturb, target=False, records=False):
        self.wl, self.npa, self.dev = wl, npa, dev
        self.Pc, self.Pf = wl.scene_params()
        self.nc, self.nf = self.networks(self.Pc, self.Pf)
        npa.set_precision("fp16x3")
        self.KW = dict(network_fn=self.nc, network_query_fn=None, N_samples=64, N_importance=128, network_fine=self.nf, perturb=perturb,
                       white_bkgd=True, raw_noise_std=0.)
        self.K = wl.intrinsics(dict(H=self.H, W=self.W, focal=1111.0))
        self.rays = wl.lego_batch(self.N_RAYS, seed=1).to(dev)
        if target:
            self.target = torch.rand(self.N_RAYS, 3, generator=torch.Generator().manual_seed(2)).to(dev)
        if records:
            self.records = wl.synthetic_rays(self.N_RAYS, seed=1).to(dev).contiguous()

    def networks(self, Pc, Pf):
        nc, nf = self.npa.NeRF(**self.NET).to(self.dev), self.npa.NeRF(**self.NET).to(self.dev)
        nc.load_state_dict(Pc)
        nf.load_state_dict(Pf)
        return nc, nf

    def adam(self, *nets, lr=0.0):
        return self.npa.FlatAdam([p for net in nets for p in net.parameters()], lr=lr)

    def fit(self, rendered, opt, rgb0):
        """the rest of a training step on what render() returned: img2mse against `target` (of rgb0 as well, if asked), backward, opt.step"""
        rgb, _, _, extras = rendered
        loss = self.npa.img2mse(rgb, self.target)
        if rgb0:
            loss = loss + self.npa.img2mse(extras["rgb0"], self.target)
        opt.zero_grad()
        loss.backward()
        opt.step()

    def render(self, rays=None, c2w=None, **over):
        """render() of the batch (or `rays`, or the frame at `c2w`), KW overridden by `over`"""
        where = dict(c2w=c2w) if c2w is not None else dict(rays=self.rays if rays is None else rays)
        return self.npa.render(self.H, self.W, self.K, **where, **self.GEO, **dict(self.KW, **over))

    def ball(self, grid_cls, radius):
        return grid_cls.from_mask(ball_mask(self.R, self.LO[0], self.HI[0], radius), self.LO, self.HI, outside="skip", device=self.dev)

    def ball_with_share(self, grid_cls, share_of, want):
        """the ball whose share_of(grid) is just at or above `want`, and its radius"""
        radius = bisect_radius(lambda r: share_of(self.ball(grid_cls, r)), want)
        return self.ball(grid_cls, radius), radius

    def teacher_and_held_out(self):
        """the converging pair of bench.py --long: teacher networks scene_params(seed=5) (as render() overrides), the student's start
        scene_params(seed=6), a held-out batch never trained on and the teacher's render of it"""
        Tc, Tf = self.wl.scene_params(seed=5)
        student = self.wl.scene_params(seed=6)
        tc, tf = self.networks(Tc, Tf)
        teacher = dict(network_fn=tc, network_fine=tf, perturb=0.)
        held = self.wl.lego_batch(self.N_RAYS, seed=10 ** 6).to(self.dev)
        with torch.no_grad():
            held_target = self.render(held, **teacher)[0]
        return teacher, student, held, held_target


def ball_mask(R, lo, hi, radius):
    """cells of the R^3 grid over [lo, hi]^3 whose centre lies within `radius` of the origin"""
    c = lo + (torch.arange(R, dtype=torch.float64) + 0.5) * (hi - lo) / R
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    return (x * x + y * y + z * z) <= radius * radius


def bisect_radius(share_of, want, lo=0.0, hi=4.0, iters=14):
    """the upper end of the bracket after `iters` halvings: share_of(radius) >= want there"""
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        if share_of(mid) < want:
            lo = mid
        else:
            hi = mid
    return hi


def evaluated_share(grid):
    return grid.last_stats["evaluated"] / grid.last_stats["total"]


def time_alternating(configs, k, reps, warmup):
    """configs: [(name, thunk)].  `warmup` calls of every thunk, then every repetition runs each configuration once with HIP events
    around k calls; returns {name: [ms per call, one per repetition]}"""
    times = {name: [] for name, _ in configs}
    for _, thunk in configs:
        for _ in range(warmup):
            thunk()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, thunk in configs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                thunk()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / k)
    return times


def row_stats(ms, n_rays=None):
    row = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}
    if n_rays is not None:
        row["rays_per_s"] = n_rays / row["ms_median"] * 1e3
    return row


def time_launches(thunk, reps, launches=100, warmup=3):
    """host-timed back-to-back calls: HIP events around `launches` of them, `reps` times; microseconds per call"""
    for _ in range(warmup):
        thunk()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            thunk()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / launches * 1e3)
    return {"us_median": statistics.median(ts), "us_min": min(ts), "us_max": max(ts)}


def kernel_summary(hb, thunk):
    """one call of `thunk` with HIP events around every launch (a fresh hb.KernelTimer for that call); its summary()"""
    timer = hb.TIMER
    hb.TIMER = hb.KernelTimer()
    try:
        thunk()
        return hb.TIMER.summary()
    finally:
        hb.TIMER = timer


def kernel_ms(summary, prefixes):
    return sum(v["ms"] for name, v in summary.items() if name.startswith(prefixes))


def psnr_db(a, b):
    mse = float(torch.mean((a.double() - b.double()) ** 2))
    return None if mse == 0.0 else -10.0 * math.log10(mse)


def emit(result, out):
    text = json.dumps(result, indent=1)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")
