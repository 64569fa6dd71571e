"""Generate tests/golden/raygrad.npz from the REAL reference (build container only: needs the reference checkout).

The reference differentiates render() end to end with plain autograd.  This records, from the reference itself, the gradients this
package reproduces with nerf_field_input_grad / nerf_raw2outputs_bwd_geom / nerf_embed_bwd:
  (i)   d loss / d ray records of render_rays for 256 synthetic rays at 64 + 128 samples, perturb and raw_noise_std from the seeded
        torch generator (the GPU tests replay the same draws), loss = img2mse(rgb) + img2mse(rgb0);
  (ii)  d loss / d c2w of a 20 x 24 render(c2w=pose), lego-like (ndc=False, near 2, far 6, white_bkgd);
  (iii) the same, fern-like (ndc=True, near 0, far 1);
  (iv)  d/dx of Embedder.embed (10 bands) under a random upstream gradient.
Per case: the reference's value (fp32), its own fp32-vs-fp64 distance (the oracle in float64; `noise`) and the largest magnitude.
Parameters, rays and upstream gradients are regenerated from seeds, not stored.

    python tests/golden/make_golden_raygrad.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import nerf_oracle as orc  # noqa: E402
import workloads as wl  # noqa: E402

N_RAYS = 256
RAY_SEED, RAND_SEED, TARGET_SEED = 7, 123, 99
POSE_H, POSE_W, POSE_FOCAL = 20, 24, 30.0
EMBED_N = 512


def pose_case(ndc):
    """(K, c2w [3, 4], near, far, white_bkgd, target [H, W, 3]) of the pose cases"""
    K = np.array([[POSE_FOCAL, 0, 0.5 * POSE_W], [0, POSE_FOCAL, 0.5 * POSE_H], [0, 0, 1]])
    if ndc:
        c2w = torch.cat([torch.eye(3), torch.tensor([[0.1], [-0.05], [0.2]])], 1)
        near, far, white = 0.0, 1.0, False
    else:
        c2w = wl.pose_spherical(30.0, -30.0, 4.0)[:3, :4].float()
        near, far, white = 2.0, 6.0, True
    target = torch.tensor(np.random.RandomState(5 + int(ndc)).rand(POSE_H, POSE_W, 3), dtype=torch.float32)
    return K, c2w, near, far, white, target


def ray_case():
    """(rays [N, 11], target [N, 3], render_rays keyword arguments) of case (i)"""
    rays = orc.synthetic_rays(N_RAYS, seed=RAY_SEED)
    target = torch.tensor(np.random.RandomState(TARGET_SEED).rand(N_RAYS, 3), dtype=torch.float32)
    return rays, target, dict(N_samples=64, N_importance=128, perturb=1.0, raw_noise_std=1.0, white_bkgd=True)


def draw_randoms(n=N_RAYS, n_c=64, n_f=128):
    """the reference's draw order (run_nerf.py:371, :285, helpers:208, :285) on the CPU generator seeded with RAND_SEED"""
    torch.manual_seed(RAND_SEED)
    return dict(t_rand=torch.rand(n, n_c), noise_c=torch.randn(n, n_c), u=torch.rand(n, n_f), noise_f=torch.randn(n, n_c + n_f))


def embed_case():
    rs = np.random.RandomState(17)
    x = torch.tensor(rs.randn(EMBED_N, 3) * 2.0, dtype=torch.float32)
    up = torch.tensor(rs.randn(EMBED_N, 63), dtype=torch.float32)
    return x, up


def oracle_ray_grad(rays, rnd, target, Pc, Pf, kw, dtype=torch.float64):
    r = rays.to(dtype).requires_grad_(True)
    P = lambda Q: {k: v.to(dtype) for k, v in Q.items()}
    out = orc.trace_rays(r, P(Pc), P(Pf), kw["N_samples"], kw["N_importance"], perturb=kw["perturb"], white_bkgd=kw["white_bkgd"],
                         raw_noise_std=kw["raw_noise_std"], **{k: v.to(dtype) for k, v in rnd.items()})
    t = target.to(dtype)
    (orc.mse(out["rgb_map"], t) + orc.mse(out["rgb0"], t)).backward()
    return r.grad


def oracle_pose_grad(ndc, Pc, Pf, dtype=torch.float64):
    K, c2w, near, far, white, target = pose_case(ndc)
    p = c2w.to(dtype).requires_grad_(True)
    o, d = orc.pinhole_rays(POSE_H, POSE_W, K, p)
    flat = orc.assemble_render_rays(POSE_H, POSE_W, K, o, d, ndc, near, far).to(dtype)
    P = lambda Q: {k: v.to(dtype) for k, v in Q.items()}
    out = orc.trace_rays(flat, P(Pc), P(Pf), 64, 128, white_bkgd=white)
    t = target.reshape(-1, 3).to(dtype)
    (orc.mse(out["rgb_map"], t) + orc.mse(out["rgb0"], t)).backward()
    return p.grad


def oracle_embed_grad(dtype=torch.float64):
    x, up = embed_case()
    xx = x.to(dtype).requires_grad_(True)
    (orc.posenc(xx, 10) * up.to(dtype)).sum().backward()
    return xx.grad


def main():
    from pin_against_reference import load_reference, reference_networks
    run_nerf, helpers = load_reference()
    Pc, Pf = orc.scene_params()
    net_c, net_f = reference_networks(helpers, Pc), reference_networks(helpers, Pf)
    for n in (net_c, net_f):
        n.requires_grad_(False)
    embed_fn, _ = helpers.get_embedder(10, 0)
    embeddirs_fn, _ = helpers.get_embedder(4, 0)
    qfn = lambda inputs, viewdirs, network_fn: run_nerf.run_network(inputs, viewdirs, network_fn, embed_fn=embed_fn,
                                                                     embeddirs_fn=embeddirs_fn, netchunk=1024 * 64)
    rec = {}

    def put(name, ref, ref64):
        rec[name] = ref.detach().numpy()
        rec[name + "/max"] = np.float64(ref.abs().max())
        rec[name + "/noise"] = np.float64((ref.double() - ref64).abs().max())
        print(f"{name}: max {float(rec[name + '/max']):.3e}, reference fp32-vs-fp64 noise {float(rec[name + '/noise']):.3e}")

    # (i) render_rays, both passes, rays requiring grad
    rays, target, kw = ray_case()
    r = rays.clone().requires_grad_(True)
    torch.manual_seed(RAND_SEED)
    out = run_nerf.render_rays(r, network_fn=net_c, network_query_fn=qfn, network_fine=net_f, retraw=True, lindisp=False, **kw)
    (helpers.img2mse(out["rgb_map"], target) + helpers.img2mse(out["rgb0"], target)).backward()
    put("rays", r.grad, oracle_ray_grad(rays, draw_randoms(), target, Pc, Pf, kw))
    # (ii) / (iii) render(c2w=pose)
    for ndc, tag in ((False, "pose_lego"), (True, "pose_fern")):
        K, c2w, near, far, white, tgt = pose_case(ndc)
        p = c2w.clone().requires_grad_(True)
        rgb, _, _, ex = run_nerf.render(POSE_H, POSE_W, K, chunk=1024 * 32, c2w=p, ndc=ndc, near=near, far=far, use_viewdirs=True,
                                        network_fn=net_c, network_query_fn=qfn, network_fine=net_f, N_samples=64, N_importance=128,
                                        perturb=0.0, raw_noise_std=0.0, white_bkgd=white, lindisp=False, retraw=True)
        (helpers.img2mse(rgb, tgt) + helpers.img2mse(ex["rgb0"], tgt)).backward()
        put(tag, p.grad, oracle_pose_grad(ndc, Pc, Pf))
    # (iv) Embedder.embed
    x, up = embed_case()
    xg = x.clone().requires_grad_(True)
    (embed_fn(xg) * up).sum().backward()
    put("embed", xg.grad, oracle_embed_grad())
    rec["params_checksum"] = np.float64(sum(float(v.double().abs().sum()) for v in list(Pc.values()) + list(Pf.values())))
    rec["rays_checksum"] = np.float64(rays.double().abs().sum())
    path = os.path.join(HERE, "raygrad.npz")
    np.savez_compressed(path, **rec)
    print(f"-> {path} ({os.path.getsize(path)} B)")


if __name__ == "__main__":
    main()
