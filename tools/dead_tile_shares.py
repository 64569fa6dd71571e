"""Dead-tile shares the device saw in the steps of the benchmark's workload ("live-tile list").

    python tools/dead_tile_shares.py [--config lego|fern] [--rays 4096] [--steps 20] [--out FILE.json]

Runs bench.py's training step (same scene parameters, ray pool, targets, optimizer) and keeps, per field backward, a device-side
copy of the two header words of the live-tile list (count, tiles); they are read back AFTER the last step -- nothing here
synchronises inside a step.  Prints one JSON line: per pass (64 = coarse, 192 = fine) the mean / min / max dead share and the share
of every launch in order (the networks train towards random targets: the shares move from step to step), and the max / mean live
share over the weight-gradient GEMM's 21 point chunks (what unequal chunks cost it).

The result also says what share of all points a backward working on tiles, on groups of 16 and on groups of 8 consecutive points
inside a tile would touch ("touched_share_*"; a group is dead when all words of its d_raw are +-0): counted from the same d_raw with
torch on the device, next to the launch, and read back with the rest.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import nerf_pytorch_amd as npa  # noqa: E402
import workloads as wl  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["lego", "fern"], default="lego")
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    hb = npa.hip_backend
    dev = torch.device("cuda", 0)
    cfg = wl.LEGO if args.config == "lego" else wl.FERN
    Pc, Pf = wl.scene_params()
    kw = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    nc, nf = npa.NeRF(**kw).to(dev), npa.NeRF(**kw).to(dev)
    nc.load_state_dict(Pc)
    nf.load_state_dict(Pf)
    opt = npa.FlatAdam(list(nc.parameters()) + list(nf.parameters()), lr=5e-4, betas=(0.9, 0.999))
    make = wl.lego_batch if args.config == "lego" else wl.fern_batch
    pool = 8
    batches = [make(args.rays, seed=i).to(dev) for i in range(pool)]
    gen = torch.Generator().manual_seed(77)
    targets = [torch.rand(args.rays, 3, generator=gen).to(dev) for _ in range(pool)]
    kwargs = dict(network_query_fn=None, perturb=1.0, N_importance=128, network_fine=nf, N_samples=64, network_fn=nc, use_viewdirs=True,
                  white_bkgd=cfg["white_bkgd"], raw_noise_std=cfg["raw_noise_std"], ndc=cfg["ndc"], lindisp=False, near=cfg["near"], far=cfg["far"])
    seen = []           # (S, P, device copy of the list up to the end of the tile numbers, live groups of 16 / of 8) per sparse field backward
    inner = hb._field_bwd

    def live_groups(d_raw, T):
        """device tensor [live 16-point groups, live 8-point groups] of d_raw (points past the launch count as zeros)"""
        bits = d_raw.reshape(-1, 4).view(torch.int32) & 0x7fffffff
        pad = torch.zeros(T * 32, 4, dtype=torch.int32, device=d_raw.device)
        pad[:bits.shape[0]] = bits
        g8 = (pad.view(T, 4, 32) != 0).any(2)
        g16 = g8[:, 0::2] | g8[:, 1::2]
        return torch.stack([g16.sum(), g8.sum()])

    def spy(L, packed, act, d_raw, grad, accumulate, precision, delta, partial, n, S, params, input_grad=None):
        out = inner(L, packed, act, d_raw, grad, accumulate, precision, delta, partial, n, S, params, input_grad)
        if hb.LAST_LIVE is not None:
            T = (n * S + 31) // 32
            seen.append((S, n * S, hb.LAST_LIVE[:4 + T].clone(), live_groups(d_raw, T)))
        return out

    hb._field_bwd = spy
    try:
        for i in range(args.steps):
            rgb, disp, acc, extras = npa.render(cfg["H"], cfg["W"], wl.intrinsics(cfg), chunk=32768, rays=batches[i % pool], verbose=False,
                                                retraw=True, **kwargs)
            opt.zero_grad()
            loss = npa.img2mse(rgb, targets[i % pool]) + npa.img2mse(extras["rgb0"], targets[i % pool])
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
    finally:
        hb._field_bwd = inner
    res = {"config": args.config, "rays": args.rays, "steps": args.steps, "precision": npa.get_precision(), "passes": {}}
    for S in sorted({s for s, _, _, _ in seen}):
        shares, imbalance, touched16, touched8 = [], [], [], []
        for s, P, words, groups in seen:
            if s != S:
                continue
            w = words.cpu()
            count, T = int(w[0]), int(w[1])
            shares.append(1.0 - count / T)
            live16, live8 = (int(x) for x in groups.cpu())
            touched16.append(live16 / (2 * T))
            touched8.append(live8 / (4 * T))
            n = max(1, min(21, (P + 255) // 256))
            ct = ((P + n - 1) // n + 31) // 32 * 32 // 32
            per_chunk = torch.bincount(w[4:4 + count].long() // ct, minlength=(T + ct - 1) // ct).double()
            imbalance.append(float(per_chunk.max() / per_chunk.mean()) if count else 1.0)
        res["passes"][str(S)] = {"launches": len(shares), "dead_share_mean": sum(shares) / len(shares), "dead_share_min": min(shares),
                                 "dead_share_max": max(shares), "chunk_max_over_mean_live": sum(imbalance) / len(imbalance),
                                 "touched_share_tiles": 1.0 - sum(shares) / len(shares),
                                 "touched_share_groups16": sum(touched16) / len(touched16), "touched_share_groups8": sum(touched8) / len(touched8),
                                 "dead_share_by_launch": [round(x, 4) for x in shares],
                                 "touched_share_groups16_by_launch": [round(x, 4) for x in touched16],
                                 "touched_share_groups8_by_launch": [round(x, 4) for x in touched8]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
