"""Gradients to the INPUTS of render(): ray records, sample points, view directions, camera poses (nerf_field_input_grad,
nerf_raw2outputs_bwd_geom, nerf_embed_bwd).  Compared with fp64 autograd of the oracle, which differentiates the reference's
expressions end to end; the near / far columns are the one documented deviation (zero)."""
import numpy as np
import pytest
import torch

import nerf_oracle as orc
import workloads as wl
from test_gpu_parity import dev, nets, npa  # noqa: F401  (fixtures)
from test_gpu_round3 import _decode_masks

pytestmark = pytest.mark.gpu

GEO = [0, 1, 2, 3, 4, 5, 8, 9, 10]         # ray-record columns that carry a gradient (6:8 = near / far: zero by contract)
# relative L2 bounds of the point-level input gradient (fp64 reference evaluated with the kernel's own ReLU pattern)
# measured maxima over the three shapes and o / d / vd: fp32 8.6e-7, fp16x3w 1.3e-6, fp16x3 2.8e-4, bf16x3 2.8e-3
POINT_BOUND = {"fp32": 3e-6, "fp16x3w": 4e-6, "fp16x3": 6e-4, "bf16x3": 6e-3}


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def _patterns(hb, act, n_rays, S, precision):
    if precision != "fp32":
        return _decode_masks(__import__("nerf_pytorch_amd"), act, n_rays * S, n_rays, precision)
    return [(hb.saved_rows(act, n_rays, S, r) > 0).cpu() for r in [f"h{i}" for i in range(8)] + ["hv"]]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "fp16x3", "fp16x3w"])
@pytest.mark.parametrize("n_rays,S", [(3, 5), (11, 192), (48, 64)])
def test_point_level_input_grad(npa, dev, nets, precision, n_rays, S):
    """field_fwd -> field_bwd(input_grad=...) against fp64 autograd of the reference MLP with the kernel's saved ReLU pattern: d_o,
    d_d (= sum_s z_s dL/dx_s) and d_viewdir of every ray; the parameter gradient of the same call is unchanged by the input gradient."""
    nc, nf, Pc, Pf = nets
    hb = npa.hip_backend
    g = torch.Generator().manual_seed(11 * n_rays + S)
    rays = orc.synthetic_rays(n_rays, seed=S + 3)
    z = torch.sort(torch.rand(n_rays, S, generator=g) * 4.0 + 2.0, -1)[0]
    d_raw = torch.randn(n_rays, S, 4, generator=g)
    packed = nf.packed_params(precision)
    rays_d, z_d, draw_d = rays.to(dev), z.to(dev), d_raw.to(dev)
    grads = []
    for want_in in (False, True):
        _, act = hb.field_fwd(packed, rays_d, z_d, save_act=True, precision=precision)
        masks = _patterns(hb, act, n_rays, S, precision)
        grad = torch.empty(hb.N_PARAMS, device=dev)
        d_rays = torch.full((n_rays, 11), float("nan"), device=dev)
        hb.field_bwd(packed, act, draw_d, grad, accumulate=False, precision=precision, params=nf.flat_params(),
                     input_grad=(rays_d, z_d, d_rays, False) if want_in else None)
        hb.WORKSPACE.give(act)
        grads.append(grad.clone())
    assert torch.equal(grads[0], grads[1])
    P64 = {k: v.double() for k, v in Pf.items()}
    r64 = rays.double().requires_grad_(True)
    # evaluated at the kernel's own fp32 sample points (x = o + d z rounded as the forward rounds it: at 2^9 x the rounding of x alone
    # moves the encoding's phase by ~1e-4), with the exact derivative dx/do = 1, dx/dd = z
    x32 = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).double()
    pts = (x32 + (r64[:, None, 0:3] - r64[:, None, 0:3].detach()) + (r64[:, None, 3:6] - r64[:, None, 3:6].detach()) * z.double()[..., None]).reshape(-1, 3)
    dirs = r64[:, None, 8:11].expand(n_rays, S, 3).reshape(-1, 3)
    feats = torch.cat([orc.posenc(pts, 10), orc.posenc(dirs, 4)], -1)
    out, _ = orc.field_mlp_forced_relu(P64, feats, masks)
    (out * d_raw.reshape(-1, 4).double()).sum().backward()
    ref = r64.grad
    got = d_rays.cpu().double()
    assert torch.all(got[:, 6:8] == 0)
    errs = {nm: rel_l2(got[:, c], ref[:, c]) for nm, c in (("o", slice(0, 3)), ("d", slice(3, 6)), ("vd", slice(8, 11)))}
    print(f"{precision} ({n_rays}, {S}): relative L2 of d_rays vs fp64 {errs}")
    assert max(errs.values()) <= POINT_BOUND[precision], errs


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_query_points_input_grad(npa, dev, nets, precision):
    """query_points / run_network: d_pts and d_viewdirs (point mode of the input-gradient kernel)"""
    nc, nf, Pc, Pf = nets
    g = torch.Generator().manual_seed(5)
    pts = (torch.rand(700, 3, generator=g) * 2 - 1) * 1.5
    vd = torch.nn.functional.normalize(torch.randn(700, 3, generator=g), dim=-1)
    up = torch.randn(700, 4, generator=g)
    npa.set_precision(precision)
    try:
        p_, v_ = pts.to(dev).requires_grad_(True), vd.to(dev).requires_grad_(True)
        raw = npa.query_points(nf, p_, v_)
        (raw * up.to(dev)).sum().backward()
    finally:
        npa.set_precision("fp32")
    P64 = {k: v.double() for k, v in Pf.items()}
    p64, v64 = pts.double().requires_grad_(True), vd.double().requires_grad_(True)
    out = orc.field_mlp(P64, torch.cat([orc.posenc(p64, 10), orc.posenc(v64, 4)], -1))
    (out * up.double()).sum().backward()
    bound = 1e-4 if precision == "fp32" else 2e-3        # (fp32 forward vs fp64: ReLU units within rounding of zero may flip)
    assert rel_l2(p_.grad, p64.grad) <= bound
    assert rel_l2(v_.grad, v64.grad) <= bound
    assert nf.pts_linears[0].weight.grad is not None     # parameters still receive theirs


@pytest.mark.parametrize("white,noise", [(False, False), (True, True)])
def test_raw2outputs_geometry_adjoint(npa, dev, white, noise):
    n, S = 97, 70
    g = torch.Generator().manual_seed(3 + white)
    raw = torch.randn(n, S, 4, generator=g) * 3.0
    z = torch.sort(torch.rand(n, S, generator=g) * 4 + 2, -1)[0]
    d = torch.randn(n, 3, generator=g)
    nz = torch.randn(n, S, generator=g) if noise else None
    ups = [torch.randn(n, 3, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, S, generator=g),
           torch.randn(n, generator=g)]
    raw_g, z_g, d_g = (t.to(dev).requires_grad_(True) for t in (raw, z, d))
    if noise:
        torch.manual_seed(0)
    # (the package draws its own noise: inject the oracle's by calling the autograd node directly)
    from nerf_pytorch_amd.render import _Composite
    outs = _Composite.apply(raw_g, z_g, d_g, None if nz is None else nz.to(dev), 0.7 if noise else 0.0, white)
    sum(((o * u.to(dev)).sum() for o, u in zip(outs, ups))).backward()
    r64, z64, d64 = (t.double().requires_grad_(True) for t in (raw, z, d))
    ref = orc.composite(r64, z64, d64, None if nz is None else nz.double() * 0.7, white)
    sum(((o * u.double()).sum() for o, u in zip(ref, ups))).backward()
    assert rel_l2(raw_g.grad, r64.grad) <= 1e-4
    assert rel_l2(z_g.grad, z64.grad) <= 1e-4
    assert rel_l2(d_g.grad, d64.grad) <= 1e-4
    # both new outputs NULL: the plain adjoint, bit for bit
    hb = npa.hip_backend
    dr = [u.to(dev).contiguous() for u in ups]
    args = (raw.to(dev), z.to(dev), d.to(dev), 3, None if nz is None else nz.to(dev), 0.7 if noise else 0.0, white, dr[0], dr[2], dr[1])
    a = hb.raw2outputs_bwd(*args, d_weights=dr[3], d_depth=dr[4])
    b = hb.raw2outputs_bwd(*args, d_weights=dr[3], d_depth=dr[4], d_rays_d=torch.empty(n, 3, device=dev))
    assert torch.equal(a, b)


def _oracle_ray_grad(rays, Pc, Pf, rnd, target, n_c=64, n_f=128, white=True, std=0.5):
    r64 = rays.double().requires_grad_(True)
    P64c = {k: v.double() for k, v in Pc.items()}
    P64f = None if Pf is None else {k: v.double() for k, v in Pf.items()}
    out = orc.trace_rays(r64, P64c, P64f, n_c, n_f, perturb=1.0, white_bkgd=white, raw_noise_std=std,
                         **{k: v.double() for k, v in rnd.items()})
    t = target.double()
    (orc.mse(out["rgb_map"], t) + orc.mse(out["rgb0"], t)).backward()
    return r64.grad


# relative L2 of render_rays' d rays against the fp64 oracle (96 rays, jitter + density noise): fp32 is limited by the fp32 forward
# itself (ReLU units and fine depths within rounding).  Measured maxima over shared /
# separate networks: fp32 2.4e-4, fp16x3w 2.7e-4, fp16x3 2.8e-4, bf16x3 1.2e-3
RENDER_BOUND = {"fp32": 8e-4, "fp16x3w": 8e-4, "fp16x3": 8e-4, "bf16x3": 4e-3}


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "fp16x3", "fp16x3w"])
@pytest.mark.parametrize("shared", [False, True])
def test_render_rays_ray_grad(npa, dev, nets, precision, shared):
    """render_rays, both passes, rays requiring grad: d loss / d ray records against fp64 autograd of the oracle (same injected
    randoms); with the parameters requiring grad too, their gradients are bit-identical to the call whose rays do not require grad."""
    nc, nf, Pc, Pf = nets
    n = 96
    rays = orc.synthetic_rays(n, seed=21)
    rnd = orc.synthetic_randoms(n, 64, 128, seed=4)
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(9))
    kw = dict(N_samples=64, N_importance=128, network_fine=None if shared else nf, white_bkgd=True, perturb=1.0, raw_noise_std=0.5)
    rnd_d = {k: v.to(dev) for k, v in rnd.items()}
    npa.set_precision(precision)
    try:
        flat = []
        for want in (False, True):
            for m in (nc, nf):
                m.zero_grad()
            r = rays.to(dev).requires_grad_(want)
            out = npa.render_rays(r, nc, None, randoms=rnd_d, **kw)
            (npa.img2mse(out["rgb_map"], target.to(dev)) + npa.img2mse(out["rgb0"], target.to(dev))).backward()
            flat.append([nc.last_flat_grad.clone()] + ([] if shared else [nf.last_flat_grad.clone()]))
        got = r.grad
    finally:
        npa.set_precision("fp32")
    for a, b in zip(*flat):
        assert torch.equal(a, b)
    ref = _oracle_ray_grad(rays, Pc, None if shared else Pf, rnd, target)
    assert torch.all(got[:, 6:8] == 0)
    err = rel_l2(got[:, GEO], ref[:, GEO])
    print(f"render_rays {precision} shared={shared}: relative L2 of d rays vs fp64 oracle {err:.2e}")
    assert err <= RENDER_BOUND[precision], err


def _golden_gen():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_raygrad.py")
    spec = importlib.util.spec_from_file_location("_make_golden_raygrad", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, np.load(os.path.join(os.path.dirname(path), "raygrad.npz"))


# relative L2 against the REAL reference's fp32 gradients (tests/golden/raygrad.npz); the reference's own fp32-vs-fp64 distance is
# part of what is measured (its noise / max is 9.8e-4).  Measured: fp32 7.9e-4, fp16x3 and fp16x3w 2.9e-3 (the same value on both: the
# fp16 forward moves a few fine samples, not the input gradient's arithmetic, which fp16x3w carries at fp32 class), bf16x3 9.8e-3
FIXTURE_BOUND = {"fp32": 2e-3, "fp16x3w": 6e-3, "fp16x3": 6e-3, "bf16x3": 2e-2}


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "fp16x3", "fp16x3w"])
def test_render_rays_matches_reference_fixture(npa, dev, nets, precision):
    """fixture (i): d loss / d ray records of the reference's render_rays, 256 rays x (64 + 128), jitter and density noise drawn from
    the same seeded generator stream"""
    nc, nf, Pc, Pf = nets
    g, gold = _golden_gen()
    rays, target, kw = g.ray_case()
    rnd = {k: v.to(dev) for k, v in g.draw_randoms().items()}
    npa.set_precision(precision)
    try:
        r = rays.to(dev).requires_grad_(True)
        out = npa.render_rays(r, nc, None, randoms=rnd, network_fine=nf, **kw)
        (npa.img2mse(out["rgb_map"], target.to(dev)) + npa.img2mse(out["rgb0"], target.to(dev))).backward()
    finally:
        npa.set_precision("fp32")
    ref = torch.tensor(gold["rays"])
    err = rel_l2(r.grad[:, GEO], ref[:, GEO])
    print(f"render_rays {precision} vs the reference fixture: relative L2 {err:.2e} (reference noise / max "
          f"{float(gold['rays/noise']) / float(gold['rays/max']):.1e})")
    assert err <= FIXTURE_BOUND[precision], err


def _oracle_render_grad(H, W, K, o, d, ndc, near, far, white, target, Pc, Pf):
    flat = orc.assemble_render_rays(H, W, K, o, d, ndc, near, far).double()
    P64c, P64f = ({k: v.double() for k, v in P.items()} for P in (Pc, Pf))
    out = orc.trace_rays(flat, P64c, P64f, 64, 128, white_bkgd=white)
    t = target.reshape(-1, 3).double()
    (orc.mse(out["rgb_map"], t) + orc.mse(out["rgb0"], t)).backward()


@pytest.mark.parametrize("ndc", [False, True])
def test_pose_gradient_through_render(npa, dev, nets, ndc):
    """render(c2w=pose.requires_grad_()) against the REAL reference's d loss / d c2w (fixtures (ii) lego-like, (iii) fern-like NDC) and
    fp64 autograd of the oracle; render(rays=(o, d)) with o, d requiring grad against the oracle's d loss / d o, d loss / d d"""
    nc, nf, Pc, Pf = nets
    g, gold = _golden_gen()
    K, pose, near, far, white, target = g.pose_case(ndc)
    H, W = g.POSE_H, g.POSE_W
    kw = dict(network_fn=nc, network_fine=nf, network_query_fn=None, N_samples=64, N_importance=128, perturb=0.0, white_bkgd=white,
              raw_noise_std=0.0, use_viewdirs=True)
    c2w = pose.to(dev).requires_grad_(True)
    rgb, _, _, ex = npa.render(H, W, K, chunk=1024, c2w=c2w, ndc=ndc, near=near, far=far, **kw)
    (npa.img2mse(rgb, target.to(dev)) + npa.img2mse(ex["rgb0"], target.to(dev))).backward()
    ref = torch.tensor(gold["pose_fern" if ndc else "pose_lego"])
    err_ref = rel_l2(c2w.grad, ref)
    p64 = pose.double().requires_grad_(True)
    o, d = orc.pinhole_rays(H, W, K, p64)
    _oracle_render_grad(H, W, K, o, d, ndc, near, far, white, target, Pc, Pf)
    err = rel_l2(c2w.grad, p64.grad)
    print(f"pose gradient ndc={ndc}: relative L2 vs the reference fixture {err_ref:.2e}, vs fp64 oracle {err:.2e}")
    # measured: 7.8e-4 / 3.5e-4 (ndc=False), 2.2e-4 / 1.6e-4 (ndc=True) against the oracle / the reference
    assert err <= 3e-3 and err_ref <= 3e-3, (err, err_ref)
    # the same rays handed in as (o, d) tensors
    o_t, d_t = npa.get_rays(H, W, K, pose.to(dev))
    o_t, d_t = o_t.clone().requires_grad_(True), d_t.clone().requires_grad_(True)
    rgb2, _, _, ex2 = npa.render(H, W, K, chunk=1024, rays=(o_t, d_t), ndc=ndc, near=near, far=far, **kw)
    (npa.img2mse(rgb2, target.to(dev)) + npa.img2mse(ex2["rgb0"], target.to(dev))).backward()
    o64, d64 = (t.detach().cpu().double().requires_grad_(True) for t in (o_t, d_t))
    _oracle_render_grad(H, W, K, o64, d64, ndc, near, far, white, target, Pc, Pf)
    err_o, err_d = rel_l2(o_t.grad, o64.grad), rel_l2(d_t.grad, d64.grad)
    print(f"render(rays=(o, d)) ndc={ndc}: relative L2 of d_o {err_o:.2e}, d_d {err_d:.2e} vs fp64 oracle")
    assert err_o <= 3e-3 and err_d <= 3e-3, (err_o, err_d)        # measured <= 1.1e-3


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_backward_plans_give_identical_ray_grads(npa, dev, nets, monkeypatch, precision):
    """one launch, resident sub-chunks and recompute give bit-identical d_rays (per-point deltas, per-ray reduction in a fixed order).
    fp16x3 included: one launch scales its deltas by the power of two of the whole batch's max|d_raw|, a sub-chunk by its own; a power
    of two is exact unless an fp16 delta reaches the subnormal range, which does not happen here (measured: bit-identical)"""
    nc, nf, Pc, Pf = nets
    hb = npa.hip_backend
    import sys
    render_mod = sys.modules["nerf_pytorch_amd.render"]
    n = 2500
    rays = orc.synthetic_rays(n, seed=8).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(n, 64, 128, seed=6).items()}
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(1)).to(dev)

    def run():
        r = rays.clone().requires_grad_(True)
        out = npa.render_rays(r, nc, None, randoms=rnd, N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0,
                              raw_noise_std=0.5)
        (npa.img2mse(out["rgb_map"], target) + npa.img2mse(out["rgb0"], target)).backward()
        return render_mod.LAST_BACKWARD_PLAN[0], r.grad.clone()
    npa.set_precision(precision)
    try:
        plans = [run()]
        monkeypatch.setattr(hb, "SAVE_BUDGET_BYTES", 4 * hb.workspace_floats(1024, 64, 128, True, precision) + 1)
        plans.append(run())
        monkeypatch.setattr(hb, "SAVE_TOTAL_BYTES", 0)
        plans.append(run())
    finally:
        npa.set_precision("fp32")
    assert [p for p, _ in plans] == ["one launch", "resident sub-chunks", "recompute"]
    assert torch.equal(plans[1][1], plans[2][1])
    print(f"{precision}: one launch vs sub-chunks bit-identical: {torch.equal(plans[0][1], plans[1][1])}, "
          f"relative L2 {rel_l2(plans[0][1], plans[1][1]):.1e}")
    assert torch.equal(plans[0][1], plans[1][1])


def _rot_err_deg(Ra, Rb):
    c = ((Ra.T @ Rb).trace() - 1.0) / 2.0
    return float(torch.rad2deg(torch.arccos(c.clamp(-1.0, 1.0))))


def test_pose_recovery_inerf(npa, dev):
    """iNeRF-style pose refinement on fp16x3 (INTEGRATION.md recipe): frozen networks (workloads.scene_params(0)), a 32 x 32 target
    rendered at a pose_spherical pose, a start perturbed by 2 degrees and 0.05 units, 60 Adam steps on an se(3) delta with perturb = 0 and
    raw_noise_std = 0 (deterministic).  The start is exp(xi) true with |omega| = 2 degrees and |v| = 0.05 (the camera centre, 4 units
    from the origin, moves 0.16).  Measured: rotation error 2.0 -> 0.13 degrees (15.4x), translation 0.158 -> 0.0042 (37.6x); the
    thresholds keep about 2x of margin (the issue's floor is 4x)."""
    Pc, Pf = wl.scene_params(0)
    kw_net = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    nc, nf = npa.NeRF(**kw_net).to(dev), npa.NeRF(**kw_net).to(dev)
    nc.load_state_dict(Pc)
    nf.load_state_dict(Pf)
    for m in (nc, nf):
        m.requires_grad_(False)
    H = W = 32
    focal = wl.LEGO["focal"] * H / wl.LEGO["H"]
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    kw = dict(network_fn=nc, network_fine=nf, network_query_fn=None, N_samples=64, N_importance=128, perturb=0.0, white_bkgd=True,
              raw_noise_std=0.0, use_viewdirs=True, ndc=False, near=2.0, far=6.0, chunk=4096)
    true = wl.pose_spherical(40.0, -30.0, 4.0).double()

    def se3(xi):
        A = torch.zeros(4, 4, dtype=torch.float64)
        w, v = xi[:3], xi[3:]
        A = A.index_put((torch.tensor([0, 0, 1]), torch.tensor([1, 2, 2])), torch.stack([-w[2], w[1], -w[0]]))
        A = A - A.T
        A = A.index_put((torch.tensor([0, 1, 2]), torch.tensor([3, 3, 3])), v)
        return torch.linalg.matrix_exp(A)
    axis = torch.tensor([1.0, 2.0, -1.5], dtype=torch.float64)
    axis = axis / axis.norm()
    shift = torch.tensor([0.6, -0.3, 0.74], dtype=torch.float64)
    shift = shift / shift.norm()
    start = se3(torch.cat([axis * np.deg2rad(2.0), shift * 0.05])) @ true
    npa.set_precision("fp16x3")
    try:
        with torch.no_grad():
            target, _, _, ex_t = npa.render(H, W, K, c2w=true[:3, :4].float().to(dev), **kw)
        xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
        opt = torch.optim.Adam([xi], lr=2e-3)
        for _ in range(60):
            pose = (se3(xi) @ start)[:3, :4].float().to(dev)
            rgb, _, _, ex = npa.render(H, W, K, c2w=pose, **kw)
            loss = npa.img2mse(rgb, target) + npa.img2mse(ex["rgb0"], ex_t["rgb0"])
            opt.zero_grad()
            loss.backward()
            opt.step()
        final = (se3(xi) @ start).detach()
    finally:
        npa.set_precision("fp32")
    r0, r1 = _rot_err_deg(start[:3, :3], true[:3, :3]), _rot_err_deg(final[:3, :3], true[:3, :3])
    t0, t1 = float((start[:3, 3] - true[:3, 3]).norm()), float((final[:3, 3] - true[:3, 3]).norm())
    print(f"pose recovery: rotation {r0:.3f} -> {r1:.4f} deg ({r0 / max(r1, 1e-12):.1f}x), translation {t0:.4f} -> {t1:.5f} "
          f"({t0 / max(t1, 1e-12):.1f}x), final loss {loss.item():.3e}")
    assert r1 * 8.0 <= r0, (r0, r1)
    assert t1 * 16.0 <= t0, (t0, t1)


def test_frozen_networks_rays_only(npa, dev, nets):
    """frozen networks, rays requiring grad (the iNeRF step): the rays get their gradient, no weight-gradient kernel runs, .grad
    stays None and no grad-ready hook fires"""
    nc, nf, Pc, Pf = nets
    hb = npa.hip_backend
    import sys
    render_mod = sys.modules["nerf_pytorch_amd.render"]
    for m in (nc, nf):
        m.zero_grad(set_to_none=True)
        m.requires_grad_(False)
    fired = []
    render_mod.GRAD_READY_HOOKS.append(lambda m, g: fired.append(m))
    hb.TIMER = hb.KernelTimer()
    npa.set_precision("fp16x3")
    try:
        r = orc.synthetic_rays(64, seed=2).to(dev).requires_grad_(True)
        out = npa.render_rays(r, nc, None, N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True)
        (out["rgb_map"].sum() + out["rgb0"].sum()).backward()
        torch.cuda.synchronize()
        names = set(hb.TIMER.summary())
    finally:
        npa.set_precision("fp32")
        hb.TIMER = None
        render_mod.GRAD_READY_HOOKS.pop()
        for m in (nc, nf):
            m.requires_grad_(True)
    assert r.grad is not None and torch.isfinite(r.grad).all() and r.grad[:, GEO].abs().sum() > 0
    assert all(p.grad is None for m in (nc, nf) for p in m.parameters())
    assert not fired
    assert "field_input_grad_kernel" in names, names
    assert not any("wgrad" in k for k in names), names


def test_embedder_is_differentiable(npa, dev):
    """Embedder.embed's gradient (nerf_embed_bwd) against the REAL reference's (fixture (iv)) and fp64 autograd of posenc"""
    g, gold = _golden_gen()
    x, up = g.embed_case()
    emb, _ = npa.get_embedder(10)
    xg = x.to(dev).requires_grad_(True)
    (emb(xg) * up.to(dev)).sum().backward()
    err64 = rel_l2(xg.grad, g.oracle_embed_grad())
    err_ref = rel_l2(xg.grad, torch.tensor(gold["embed"]))
    print(f"embed: relative L2 vs fp64 {err64:.2e}, vs the reference fixture {err_ref:.2e}")
    assert err64 <= 3e-7 and err_ref <= 5e-7, (err64, err_ref)      # measured 5.7e-8 / 1.2e-7


def test_dense_path_refuses_ray_grad(npa, dev):
    net = npa.NeRF(D=2, W=64, input_ch=63, output_ch=5, skips=[], input_ch_views=27, use_viewdirs=True).to(dev)
    r = orc.synthetic_rays(8, seed=1).to(dev).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="DenseNeRF"):
        npa.render_rays(r, net, None, N_samples=8)
