"""GPU (-m gpu): camera-pose gradients of the ray-batch layer (nerf_ray_pose_grad) and the device form of the reference's
use_batching mode (RayBatcher, nerf_sample_ray_views), against fp64 autograd of oracle.pinhole_rays (get_rays, pinned to the
reference), and a joint pose refinement fed by RayBatcher."""
import numpy as np
import pytest
import torch

import nerf_oracle as orc
import workloads as wl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def npa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_pytorch_amd
    return nerf_pytorch_amd


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def _K(H, W, focal):
    return np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])


def _get_rays_at(H, W, K, c2w, pix):
    """get_rays (run_nerf_helpers.py:153-162) at pixels pix = j*W + i, c2w [B, 3+, 4] (one per ray), in the reference's expressions"""
    i, j = (pix % W).float(), torch.div(pix, W, rounding_mode="floor").float()
    dirs = torch.stack([(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -torch.ones_like(i)], -1)
    rays_d = torch.sum(dirs[..., None, :] * c2w[:, :3, :3], -1)
    return torch.stack([c2w[:, :3, -1], rays_d], 0)


@pytest.mark.parametrize("precrop", [None, 0.5])
@pytest.mark.parametrize("form", ["3x4", "4x4", "table view"])
def test_sample_ray_batch_pose_gradient(npa, dev, form, precrop):
    """sample_ray_batch with a pose that requires grad: d loss / d pose (nerf_ray_pose_grad) == fp64 autograd of get_rays at the returned
    pixels; the forward outputs are bitwise those of a no-grad call with the same key."""
    H, W = 40, 56
    K = _K(H, W, 47.0)
    img = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(0)).to(dev)
    pose44 = wl.pose_spherical(37.0, -25.0, 4.0).float()
    N = 500
    if form == "table view":
        table = torch.stack([wl.pose_spherical(10.0 * v, -30.0, 4.0).float() for v in range(4)]).to(dev)
        table[2] = pose44.to(dev)
        table.requires_grad_(True)
        pose, leaf = table[2, :3, :4], table
    else:
        leaf = (pose44 if form == "4x4" else pose44[:3, :4]).clone().to(dev).requires_grad_(True)
        pose = leaf
    rays, tgt, pix = npa.sample_ray_batch(H, W, K, pose, img, N, precrop_frac=precrop, generator=torch.Generator().manual_seed(4),
                                          return_pixels=True)
    assert rays.grad_fn is not None and not tgt.requires_grad
    with torch.no_grad():
        rays_ng, tgt_ng, pix_ng = npa.sample_ray_batch(H, W, K, pose.detach(), img, N, precrop_frac=precrop,
                                                       generator=torch.Generator().manual_seed(4), return_pixels=True)
    assert torch.equal(rays, rays_ng) and torch.equal(tgt, tgt_ng) and torch.equal(pix, pix_ng)
    up = torch.randn(2, N, 3, generator=torch.Generator().manual_seed(9))
    (rays * up.to(dev)).sum().backward()
    assert leaf.grad is not None
    p64 = pose44.double().requires_grad_(True)
    pl = pix.long().cpu()
    (_get_rays_at(H, W, K, p64[None].expand(N, 4, 4), pl) * up.double()).sum().backward()
    got = leaf.grad[2] if form == "table view" else leaf.grad
    err = rel_l2(got[:3, :4], p64.grad[:3, :4])
    print(f"sample_ray_batch pose gradient ({form}, precrop {precrop}): relative L2 vs fp64 {err:.2e}")
    # measured: 1.6e-7 (no precrop) / 1.8e-7 (precrop) for every form (fp32 products, fixed-order fp32 sums over 500 rays)
    assert err <= 1e-5, err
    if form != "3x4":
        assert torch.all(got[3] == 0)
    if form == "table view":
        assert torch.all(leaf.grad[[0, 1, 3]] == 0)


def _views_scene(dev, n=8, H=24, W=20):
    images = torch.rand(n, H, W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    poses = torch.stack([wl.pose_spherical(45.0 * v, -15.0 - 4 * v, 4.0) for v in range(n)]).float().to(dev)
    return images, poses, _K(H, W, 31.0)


def test_ray_batcher_epochs(npa, dev):
    """one epoch visits every (view, pixel) of i_train exactly once, the last batch is short, the next epoch has another order, a seeded
    generator reproduces the batches bit for bit; rays == get_rays of their view's pose at their pixel, colours == the image tables'"""
    images, poses, K = _views_scene(dev)
    H, W = images.shape[1:3]
    i_train = [0, 2, 3, 5, 6]
    HW, total, N_rand = H * W, 5 * H * W, 512
    runs = []
    for _ in range(2):
        b = npa.RayBatcher(images, K, N_rand, i_train, generator=torch.Generator().manual_seed(21))
        runs.append([b.next(poses, return_pixels=True, return_views=True) for _ in range(2 * ((total + N_rand - 1) // N_rand))])
    assert (b.epoch, b.i_batch) == (2, 0)
    for x, y in zip(*runs):
        assert all(torch.equal(s, t) for s, t in zip(x, y))
    n_per = (total + N_rand - 1) // N_rand
    sizes = [t.shape[0] for _, t, _, _ in runs[0]]
    assert sizes == ([N_rand] * (n_per - 1) + [total - (n_per - 1) * N_rand]) * 2 and sizes[n_per - 1] < N_rand
    qs = []
    for e in range(2):
        ep = runs[0][e * n_per:(e + 1) * n_per]
        q = torch.cat([v.long() * HW + p.long() for _, _, p, v in ep]).cpu()
        assert torch.equal(torch.sort(q)[0], torch.arange(total))
        qs.append(q)
    assert not torch.equal(qs[0], qs[1])
    ids = torch.tensor(i_train)
    errs = []
    for rays, tgt, pix, views in runs[0][:n_per]:
        t = ids[views.long().cpu()]
        pl = pix.long().cpu()
        assert torch.equal(tgt.cpu(), images.cpu()[t, pl // W, pl % W])
        for v in torch.unique(t).tolist():
            m = t == v
            ro, rd = orc.pinhole_rays(H, W, K, poses[v].cpu())
            assert torch.equal(rays[0].cpu()[m], ro.reshape(-1, 3)[pl[m]])
            errs.append(float((rays[1].cpu()[m] - rd.reshape(-1, 3)[pl[m]]).abs().max()))
    assert max(errs) <= 2e-6, max(errs)


def test_multi_view_pose_gradient(npa, dev):
    """d loss / d poses [N, 4, 4] through RayBatcher == fp64 autograd of get_rays; views without a ray in the batch, and views outside
    i_train, get exact zeros; two runs give bit-identical gradients"""
    images, poses, K = _views_scene(dev, n=12, H=32, W=32)
    H, W = images.shape[1:3]
    i_train = list(range(0, 12, 2)) + [1, 9]
    for N_rand, seed in ((4096, 2), (5, 3)):
        grads = []
        for _ in range(2):
            b = npa.RayBatcher(images, K, N_rand, i_train, generator=torch.Generator().manual_seed(seed))
            P = poses.clone().requires_grad_(True)
            rays, _, pix, views = b.next(P, return_pixels=True, return_views=True)
            up = torch.randn(rays.shape, generator=torch.Generator().manual_seed(seed)).to(dev)
            (rays * up).sum().backward()
            grads.append(P.grad.clone())
        assert torch.equal(grads[0], grads[1])
        p64 = poses.cpu().double().requires_grad_(True)
        t = torch.tensor(i_train)[views.long().cpu()]
        (_get_rays_at(H, W, K, p64[t], pix.long().cpu()) * up.cpu().double()).sum().backward()
        err = rel_l2(grads[0], p64.grad)
        print(f"RayBatcher pose gradient, N_rand {N_rand}: relative L2 vs fp64 {err:.2e}")
        assert err <= 1e-5, err         # measured: 8.9e-8 (N_rand 4096), 1.6e-8 (N_rand 5)
        seen = set(t.tolist())
        for v in range(12):
            if v not in seen:
                assert torch.all(grads[0][v] == 0), v
        if N_rand == 5:
            assert len(seen) < len(i_train)


def test_refinement_step_through_render(npa, dev):
    """one fp32 step with trainable networks: PoseRefinement -> RayBatcher -> render(rays=batch_rays) -> img2mse -> backward gives the
    d xi of the same pixels' rays built by torch get_rays on the refined poses (the kernel's ray values substituted in the forward, so
    that only the pose adjoint differs), and bit-identical network gradients"""
    scene = wl.blender_scene(H=24, W=24, n_train=4, n_test=1)
    H, W, focal = scene["hwf"]
    K = _K(H, W, focal)
    images, poses = scene["images"].to(dev), scene["poses"].float().to(dev)
    i_train = list(scene["i_split"][0])
    Pc, Pf = wl.scene_params(0)
    kw_net = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    nc, nf = npa.NeRF(**kw_net).to(dev), npa.NeRF(**kw_net).to(dev)
    nc.load_state_dict(Pc)
    nf.load_state_dict(Pf)
    kw = dict(network_fn=nc, network_fine=nf, network_query_fn=None, N_samples=64, N_importance=128, perturb=0.0, white_bkgd=True,
              raw_noise_std=0.0, use_viewdirs=True, ndc=False, near=scene["near"], far=scene["far"], chunk=4096)
    refine = npa.PoseRefinement(len(poses)).to(dev)
    with torch.no_grad():
        refine.xi.copy_(torch.randn(len(poses), 6, generator=torch.Generator().manual_seed(5)) * 0.02)
    b = npa.RayBatcher(images, K, 1024, i_train, generator=torch.Generator().manual_seed(8))
    out = []
    for path in ("kernel", "torch"):
        for m in (nc, nf, refine):
            m.zero_grad(set_to_none=True)
        refined = refine(poses)
        if path == "kernel":
            rays, target, pix, views = b.next(refined, return_pixels=True, return_views=True)
            rays_k = rays.detach()
        else:
            t = torch.tensor(i_train, device=dev)[views.long()]
            r = _get_rays_at(H, W, K, refined[t], pix.long())
            assert float((r - rays_k).abs().max()) <= 2e-6
            rays = rays_k + (r - r.detach())
        rgb, _, _, ex = npa.render(H, W, K, rays=rays, **kw)
        (npa.img2mse(rgb, target) + npa.img2mse(ex["rgb0"], target)).backward()
        out.append((refine.xi.grad.clone(), [p.grad.clone() for m in (nc, nf) for p in m.parameters()]))
    err = rel_l2(out[0][0], out[1][0])
    print(f"d xi: kernel adjoint vs torch get_rays: relative L2 {err:.2e}")
    assert float(out[1][0].abs().sum()) > 0
    assert err <= 1e-4, err             # measured: 8.4e-7
    assert all(torch.equal(x, y) for x, y in zip(out[0][1], out[1][1]))


def _rot_err_deg(Ra, Rb):
    c = ((Ra.T @ Rb).trace() - 1.0) / 2.0
    return float(torch.rad2deg(torch.arccos(c.clamp(-1.0, 1.0))))


def test_joint_pose_recovery_fp16x3(npa, dev):
    """NeRF-- / BARF-style refinement of 6 views on fp16x3: frozen networks (workloads.scene_params(0)), 32 x 32 targets rendered at
    pose_spherical poses, each start perturbed by 2 degrees and 0.05 units about its own axis, PoseRefinement + Adam fed by RayBatcher
    (N_rand = 1024 over all six views), 360 steps, perturb = 0 and raw_noise_std = 0.  Measured worst ratios over the six views:
    rotation 17.1x, translation 16.7x (view 0); the threshold keeps about 2x of margin (the issue's floor is 4x)."""
    from nerf_pytorch_amd.pose import se3_exp
    Pc, Pf = wl.scene_params(0)
    kw_net = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    nc, nf = npa.NeRF(**kw_net).to(dev), npa.NeRF(**kw_net).to(dev)
    nc.load_state_dict(Pc)
    nf.load_state_dict(Pf)
    for m in (nc, nf):
        m.requires_grad_(False)
    H = W = 32
    V = 6
    focal = wl.LEGO["focal"] * H / wl.LEGO["H"]
    K = _K(H, W, focal)
    kw = dict(network_fn=nc, network_fine=nf, network_query_fn=None, N_samples=64, N_importance=128, perturb=0.0, white_bkgd=True,
              raw_noise_std=0.0, use_viewdirs=True, ndc=False, near=2.0, far=6.0, chunk=4096)
    # (elevation -30 degrees as in test_pose_recovery_inerf; at (340, -30) this loop stalls at 2.7x in 360 steps, so the sixth view
    # looks from -10 degrees)
    true = torch.stack([wl.pose_spherical(40.0 + 60.0 * v, -30.0 if v < 5 else -10.0, 4.0) for v in range(V)]).double()
    g = torch.Generator().manual_seed(12)
    axes = torch.nn.functional.normalize(torch.randn(V, 3, generator=g, dtype=torch.float64), dim=-1)
    shifts = torch.nn.functional.normalize(torch.randn(V, 3, generator=g, dtype=torch.float64), dim=-1)
    start = se3_exp(torch.cat([axes * np.deg2rad(2.0), shifts * 0.05], -1)) @ true
    npa.set_precision("fp16x3")
    try:
        with torch.no_grad():
            images = torch.stack([npa.render(H, W, K, c2w=true[v, :3, :4].float().to(dev), **kw)[0] for v in range(V)])
        start_d = start.float().to(dev)
        refine = npa.PoseRefinement(V).to(dev)
        opt = torch.optim.Adam(refine.parameters(), lr=2e-3)
        b = npa.RayBatcher(images, K, 1024, list(range(V)), generator=torch.Generator().manual_seed(0))
        for _ in range(360):
            rays, target = b.next(refine(start_d))
            rgb, _, _, _ = npa.render(H, W, K, rays=rays, **kw)
            loss = npa.img2mse(rgb, target)
            opt.zero_grad()
            loss.backward()
            opt.step()
        final = (se3_exp(refine.xi.detach().cpu().double()) @ start)
    finally:
        npa.set_precision("fp32")
    rr, tr = [], []
    for v in range(V):
        r0, r1 = _rot_err_deg(start[v, :3, :3], true[v, :3, :3]), _rot_err_deg(final[v, :3, :3], true[v, :3, :3])
        t0, t1 = float((start[v, :3, 3] - true[v, :3, 3]).norm()), float((final[v, :3, 3] - true[v, :3, 3]).norm())
        rr.append(r0 / max(r1, 1e-12))
        tr.append(t0 / max(t1, 1e-12))
        print(f"view {v}: rotation {r0:.3f} -> {r1:.4f} deg ({rr[-1]:.1f}x), translation {t0:.4f} -> {t1:.5f} ({tr[-1]:.1f}x)")
    print(f"epochs {b.epoch}, final loss {loss.item():.3e}; worst ratios: rotation {min(rr):.1f}x, translation {min(tr):.1f}x")
    assert min(rr) >= 8.0 and min(tr) >= 8.0, (rr, tr)
