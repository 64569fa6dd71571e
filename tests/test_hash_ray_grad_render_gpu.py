"""GPU (-m gpu): gradients to rays, points and camera poses through HashNeRF(point_grad=True) and render_rays -- d loss
/ d rays against float64 autograd of the same chain built from public pieces (HashEncoding.encode_reference, a float64 copy of the layer
stack, the oracle's compositing) on the depths the call used, by the 4 x rule; unchanged table and layer gradients; the frozen pair;
render(c2w=pose); PoseRefinement + RayBatcher; the distortion loss; mesh normals; and the refusals that stay.  33 rays, 8 + 8 samples,
the four-level pair of test_hash_render_gpu.make_pair rebuilt with the flag."""
import pytest
import torch

import nerf_oracle as orc
import workloads as wl
from test_gpu_parity import dev, npa  # noqa: F401  (fixtures)
from test_hash_cpu import FOUR
from test_hash_render_gpu import BOUND, N_C, N_F, N_RAYS, grads_of, make_pair, render_loss

pytestmark = pytest.mark.gpu

F64 = torch.float64
KINK = 2e-6         # no float64 pre-activation of the chain lies closer to its ReLU's kink (ten times fp32's error of a pre-activation of
                    # order one): fp32 and float64 take the same side of every ReLU
ARCH = dict(D=2, W=64, input_ch=8, input_ch_views=27, output_ch=4, skips=[], use_viewdirs=True)


def make_flagged_pair(npa, dev, seed=0):
    """make_pair's networks -- the same draws in the same order -- built with point_grad=True"""
    torch.manual_seed(seed)
    nets = []
    for k in range(2):
        net = npa.HashNeRF([-BOUND] * 3, [BOUND] * 3, point_grad=True, **FOUR)
        with torch.no_grad():
            net.encoding.embeddings.copy_(torch.randn(net.encoding.embeddings.shape, generator=torch.Generator().manual_seed(seed + 10 + k)))
        nets.append(net.to(dev))
    return nets


def stack(P, x, dtype):
    """the layer stack of ARCH on x [M, 35] in plain torch: (raw [M, 4], the smallest |pre-activation| in front of a ReLU)"""
    lin = torch.nn.functional.linear
    P = {k: v.to(dtype) for k, v in P.items()}
    h, closest = x[:, :8], float("inf")
    for i in range(ARCH["D"]):
        pre = lin(h, P[f"pts_linears.{i}.weight"], P[f"pts_linears.{i}.bias"])
        closest = min(closest, float(pre.detach().abs().min()))
        h = torch.relu(pre)
    alpha = lin(h, P["alpha_linear.weight"], P["alpha_linear.bias"])
    feat = lin(h, P["feature_linear.weight"], P["feature_linear.bias"])
    pre = lin(torch.cat([feat, x[:, 8:]], -1), P["views_linears.0.weight"], P["views_linears.0.bias"])
    closest = min(closest, float(pre.detach().abs().min()))
    return torch.cat([lin(torch.relu(pre), P["rgb_linear.weight"], P["rgb_linear.bias"]), alpha], -1), closest


def field(net_cpu, pts, viewdirs, dtype):
    """raw [M, 4] of a CPU copy of a HashNeRF at points [M, 3] seen along viewdirs [M, 3], in dtype; and the distance to the kinks"""
    e = net_cpu.encoding.encode_reference(pts, dtype, net_cpu.encoding.embeddings.detach().to(dtype))
    return stack({k: v.detach() for k, v in net_cpu.mlp.state_dict().items()}, torch.cat([e, orc.posenc(viewdirs, 4)], -1), dtype)


def chain_loss(nets_cpu, rays, z_c, z_f, target, dtype):
    """the loss of render_loss in dtype on the CPU, on given depths (constants): (loss, the sample points of both passes, kink distance)"""
    r = rays.to(dtype)
    loss, pts_all, closest = 0.0, [], float("inf")
    for net, z in zip(nets_cpu, (z_c, z_f)):
        zz = z.to(dtype)
        pts = r[:, None, 0:3] + r[:, None, 3:6] * zz[:, :, None]
        vd = r[:, None, 8:11].expand(pts.shape)
        raw, c = field(net, pts.reshape(-1, 3), vd.reshape(-1, 3), dtype)
        rgb = orc.composite(raw.reshape(z.shape[0], z.shape[1], 4), zz, r[:, 3:6], None, white_bkgd=True)[0]
        loss = loss + torch.mean((rgb - target.to(dtype)) ** 2)
        pts_all.append(pts.detach().reshape(-1, 3))
        closest = min(closest, c)
    return loss, pts_all, closest


def same_cells(enc, pts32, pts64):
    """fp32 and float64 locate every point in the same cell on every level, and agree on the axes outside the box"""
    for l in range(enc.n_levels):
        if not torch.equal(enc._corners(pts32, l, torch.float32)[0], enc._corners(pts64, l, F64)[0]):
            return False
    t32, t64 = (pts32 - enc._lo32) * enc._inv32, (pts64 - enc._lo32.double()) * enc._inv32.double()
    return torch.equal((t32 < 0) | (t32 > 1), (t64 < 0) | (t64 > 1))


def the_depths(npa, rays, nc, nf):
    """the depths render_rays(perturb=0) uses for these rays, through the same public pieces in the same order"""
    from nerf_pytorch_amd.render import _linspace01
    hb = npa.hip_backend
    with torch.no_grad():
        z_c = hb.sample_coarse(rays, _linspace01(N_C, rays.device), False, None)
        w = npa.raw2outputs(nc.query(rays, z_c)[..., :4], z_c, rays[:, 3:6], 0, True)[3]
        z_f = hb.sample_fine(z_c, w.contiguous(), N_F, None, _linspace01(N_F, rays.device))[0]
    return z_c, z_f


@pytest.fixture(scope="module")
def pair(npa, dev):
    return make_flagged_pair(npa, dev)


@pytest.fixture(scope="module")
def target(dev):
    return torch.rand(N_RAYS, 3, generator=torch.Generator().manual_seed(4)).to(dev)


@pytest.fixture(scope="module")
def case(npa, dev, pair, target):
    """the first ray seed for which the float64 comparison is meaningful: no sample point of either pass changes its cell between fp32
    and float64 on any level, and no ReLU of the float64 chain sits within KINK of its kink.  (rays, z_c, z_f, CPU copies of the pair)"""
    import copy
    nc, nf = pair
    cpu = [copy.deepcopy(n).cpu() for n in (nc, nf)]
    for seed in range(3, 11):
        rays = wl.synthetic_rays(N_RAYS, seed=seed).to(dev).contiguous()
        z_c, z_f = the_depths(npa, rays, nc, nf)
        r = rays.cpu()
        _, pts64, closest = chain_loss(cpu, r, z_c.cpu(), z_f.cpu(), target.cpu(), F64)
        pts32 = [(r[:, None, 0:3] + r[:, None, 3:6] * z.cpu()[:, :, None]).reshape(-1, 3) for z in (z_c, z_f)]
        ok = all(same_cells(n.encoding, a, b) for n, a, b in zip(cpu, pts32, pts64))
        inside = float(((pts32[1].abs() < BOUND).all(1)).float().mean())
        print(f"ray seed {seed}: cells agree {ok}, closest pre-activation {closest:.2e}, {inside:.2f} of the fine samples inside the box")
        if ok and closest >= KINK and inside >= 0.2:
            return rays, z_c, z_f, cpu
    pytest.fail("no ray seed in 3 .. 10 keeps every sample point in its cell between fp32 and float64")


def test_ray_gradient_against_float64_autograd_of_the_chain(npa, dev, pair, target, case):
    nc, nf = pair
    rays, z_c, z_f, cpu = case
    for n in (nc, nf):
        n.zero_grad(set_to_none=True)
    rg = rays.clone().requires_grad_(True)
    loss = render_loss(npa, rg, target, nc, nf)
    loss.backward()
    got = rg.grad.cpu()
    assert got.shape == (N_RAYS, 11) and bool(torch.isfinite(got).all())
    first = got.clone()
    rg2 = rays.clone().requires_grad_(True)
    render_loss(npa, rg2, target, nc, nf).backward()
    assert torch.equal(rg2.grad.cpu(), first)                    # no atomics: the same bits
    want = {}
    for dtype in (torch.float32, F64):
        r = rays.cpu().to(dtype).requires_grad_(True)
        l, _, _ = chain_loss(cpu, r, z_c.cpu(), z_f.cpu(), target.cpu(), dtype)
        l.backward()
        want[dtype] = r.grad.double()
        assert abs(float(l.detach()) - float(loss.detach())) <= 1e-4 * abs(float(l.detach()))           # the same depths, the same loss
    assert float(got[:, 6:8].abs().max()) == 0.0 and float(want[F64][:, 6:8].abs().max()) == 0.0      # near / far: constants
    for name, cols in (("origin", slice(0, 3)), ("direction", slice(3, 6)), ("view direction", slice(8, 11))):
        own = float((want[torch.float32][:, cols] - want[F64][:, cols]).abs().max())
        err = float((got.double()[:, cols] - want[F64][:, cols]).abs().max())
        scale = float(want[F64][:, cols].abs().max())
        print(f"d loss / d {name}: kernels {err:.3e}, the float32 chain's own {own:.3e}, largest entry {scale:.3e}")
        assert scale > 0.0 and own > 0.0 and err <= 4.0 * own


def test_table_and_layer_gradients_do_not_depend_on_the_flag(npa, dev, pair, target, case):
    nc, nf = pair
    rays = case[0]
    plain_c, plain_f = make_pair(npa, dev)
    for n in (nc, nf, plain_c, plain_f):
        n.zero_grad(set_to_none=True)
    a = render_loss(npa, rays, target, nc, nf)
    b = render_loss(npa, rays, target, plain_c, plain_f)
    assert torch.equal(a, b)
    a.backward()
    b.backward()
    flagged, plain = grads_of(nc, nf), grads_of(plain_c, plain_f)
    assert len(flagged) == len(plain) and all(torch.equal(x, y) for x, y in zip(flagged, plain))
    # ... nor on rays that require grad
    for n in (nc, nf):
        n.zero_grad(set_to_none=True)
    render_loss(npa, rays.clone().requires_grad_(True), target, nc, nf).backward()
    assert all(torch.equal(x, y) for x, y in zip(grads_of(nc, nf), plain))


def test_a_frozen_pair_fills_only_the_rays(npa, dev, target, case):
    rays = case[0]
    nc, nf = make_flagged_pair(npa, dev)
    rg = rays.clone().requires_grad_(True)
    render_loss(npa, rg, target, nc, nf).backward()
    trained = rg.grad.clone()
    for n in (nc, nf):
        n.zero_grad(set_to_none=True)
        for p in n.parameters():
            p.requires_grad_(False)
    rg = rays.clone().requires_grad_(True)
    render_loss(npa, rg, target, nc, nf).backward()
    assert all(p.grad is None for n in (nc, nf) for p in n.parameters())
    assert torch.equal(rg.grad, trained) and float(rg.grad.abs().max()) > 0.0
    # (no accumulator was ever made for the frozen tables: the maximum, the scatter and the finishing pass did not run)
    frozen = make_flagged_pair(npa, dev, seed=1)
    for n in frozen:
        for p in n.parameters():
            p.requires_grad_(False)
    rg = rays.clone().requires_grad_(True)
    render_loss(npa, rg, target, *frozen).backward()
    assert all(n.encoding._scratch == {} for n in frozen) and bool(torch.isfinite(rg.grad).all())


def _camera(dev):
    H = W = 6
    K = [[7.0, 0.0, 0.5 * W], [0.0, 7.0, 0.5 * H], [0.0, 0.0, 1.0]]
    pose = torch.tensor([[1.0, 0.0, 0.0, 0.1], [0.0, 1.0, 0.0, -0.05], [0.0, 0.0, 1.0, 4.0]], device=dev)       # looks down -z at the box
    return H, W, K, pose


def test_render_with_a_pose_that_requires_grad(npa, dev, pair):
    nc, nf = pair
    H, W, K, pose = _camera(dev)
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(6)).to(dev)
    kw = dict(network_fn=nc, network_fine=nf, network_query_fn=None, N_samples=N_C, N_importance=N_F, perturb=0., white_bkgd=True, raw_noise_std=0.)
    p1 = pose.clone().requires_grad_(True)
    rgb, _, _, extras = npa.render(H, W, K, c2w=p1, ndc=False, near=2.0, far=6.0, use_viewdirs=True, **kw)
    (npa.img2mse(rgb, target) + npa.img2mse(extras["rgb0"], target)).backward()
    # by hand: get_rays, the view directions and the records as render() assembles them, then render_rays
    p2 = pose.clone().requires_grad_(True)
    rays_o, rays_d = npa.get_rays(H, W, K, p2)
    viewdirs = (rays_d / torch.norm(rays_d, dim=-1, keepdim=True)).reshape(-1, 3).float()
    rays_o, rays_d = rays_o.reshape(-1, 3).float(), rays_d.reshape(-1, 3).float()
    near, far = 2.0 * torch.ones_like(rays_d[..., :1]), 6.0 * torch.ones_like(rays_d[..., :1])
    ret = npa.render_rays(torch.cat([rays_o, rays_d, near, far, viewdirs], -1), **kw)
    (npa.img2mse(ret["rgb_map"].reshape(H, W, 3), target) + npa.img2mse(ret["rgb0"].reshape(H, W, 3), target)).backward()
    assert p1.grad is not None and bool(torch.isfinite(p1.grad).all()) and float(p1.grad.abs().max()) > 0.0
    assert torch.equal(p1.grad, p2.grad)


def test_one_adam_step_of_pose_refinement(npa, dev, pair):
    nc, nf = pair
    H, W, K, pose = _camera(dev)
    images = torch.rand(1, H, W, 3, generator=torch.Generator().manual_seed(7)).to(dev)
    refine = npa.PoseRefinement(1).to(dev)
    opt = torch.optim.Adam(refine.parameters(), lr=1e-3)
    batcher = npa.RayBatcher(images, K, H * W, [0], generator=torch.Generator().manual_seed(8))
    batch_rays, target_s = batcher.next(refine(pose[None]))
    rgb, _, _, extras = npa.render(H, W, K, rays=batch_rays, ndc=False, near=2.0, far=6.0, use_viewdirs=True, network_fn=nc, network_fine=nf,
                                   network_query_fn=None, N_samples=N_C, N_importance=N_F, perturb=0., white_bkgd=True, raw_noise_std=0.)
    opt.zero_grad()
    (npa.img2mse(rgb, target_s) + npa.img2mse(extras["rgb0"], target_s)).backward()
    assert refine.xi.grad is not None and bool(torch.isfinite(refine.xi.grad).all()) and float(refine.xi.grad.abs().max()) > 0.0
    opt.step()
    assert bool(torch.isfinite(refine.xi).all()) and float(refine.xi.detach().abs().max()) > 0.0


def test_the_distortion_and_interlevel_losses_carry_grad_to_the_rays(npa, dev, pair, case):
    nc, nf = pair
    rays = case[0]
    rg = rays.clone().requires_grad_(True)
    ret = npa.render_rays(rg, nc, None, N_C, N_importance=N_F, network_fine=nf, perturb=0., white_bkgd=True, raw_noise_std=0., distortion=True,
                          interlevel=True)
    assert ret["distortion"].shape == (N_RAYS,) and ret["interlevel"].shape == (N_RAYS,)
    (g_d,) = torch.autograd.grad(ret["distortion"].sum(), rg, retain_graph=True)
    (g_i,) = torch.autograd.grad(ret["interlevel"].sum(), rg)
    for g in (g_d, g_i):
        assert g.shape == (N_RAYS, 11) and bool(torch.isfinite(g).all()) and float(g[:, :6].abs().max()) > 0.0


def test_mesh_normals_of_a_hash_field(npa, dev, pair):
    import copy
    nf = pair[1]
    lo, hi = (-1.31, -1.27, -1.22), (1.23, 1.33, 1.29)         # (a lattice whose nodes are no nodes of the encoding's levels)
    volume = npa.density_volume(nf, lo, hi, 9)
    assert volume.shape == (9, 9, 9) and bool(torch.isfinite(volume).all())
    cpu = copy.deepcopy(nf).cpu()
    for q in (0.5, 0.4, 0.6, 0.3, 0.7):         # the first level whose vertices keep their cells and ReLU sides between fp32 and float64
        level = float(volume.flatten().quantile(q))
        mesh = npa.mesh_from_network(nf, lo, hi, 9, level)
        v, n = mesh["vertices"], mesh["normals"]
        vc = v.cpu()
        vd = torch.tensor([0.0, 0.0, 1.0], device=dev).expand(v.shape[0], 3)
        want = {}
        for dtype in (torch.float32, F64):
            xc = vc.to(dtype).requires_grad_(True)
            raw, closest = field(cpu, xc, vd.cpu().to(dtype), dtype)
            (want[dtype],) = torch.autograd.grad(raw[:, 3].sum(), xc)
        ok = same_cells(cpu.encoding, vc, vc.double())
        print(f"level at quantile {q}: {v.shape[0]} vertices, cells agree {ok}, closest pre-activation {closest:.2e}")
        if ok and closest >= KINK and v.shape[0] > 50:
            break
    else:
        pytest.fail("no level keeps every vertex in its cell and on its side of every ReLU between fp32 and float64")
    assert n.shape == v.shape and mesh["colors"].shape == v.shape and mesh["faces"].shape[0] > 0
    length = n.norm(dim=-1)
    assert bool(((length == 0) | ((length - 1.0).abs() <= 1e-5)).all()) and float(length.max()) > 0.0
    # the gradient under the normals: the kernels' d sigma / d vertex against float64 autograd of the chain, by the 4 x rule
    x = v.clone().requires_grad_(True)
    (got,) = torch.autograd.grad(npa.query_points(nf, x, vd)[:, 3].sum(), x)
    good = torch.isfinite(got.norm(dim=-1)) & (got.norm(dim=-1) > 0)
    assert torch.equal(n, torch.where(good[:, None], -got / got.norm(dim=-1, keepdim=True), torch.zeros_like(got)))
    own = float((want[torch.float32].double() - want[F64]).abs().max())
    err = float((got.cpu().double() - want[F64]).abs().max())
    print(f"d sigma / d vertex over {v.shape[0]} vertices: kernels {err:.3e}, the float32 chain's own {own:.3e}")
    assert own > 0.0 and err <= 4.0 * own
    # vertex directions receive gradients too
    d = vd.clone().requires_grad_(True)
    (g_dir,) = torch.autograd.grad(npa.query_points(nf, v, d)[:, :3].sum(), d)
    assert bool(torch.isfinite(g_dir).all()) and float(g_dir.abs().max()) > 0.0


def test_the_refusals_that_stay(npa, dev, pair, case):
    rays = case[0]
    words = (r"gradients to rays / sample points / camera poses are implemented for the fused NeRF architecture only, not for general "
             r"\(DenseNeRF\) networks")
    rg = rays.clone().requires_grad_(True)
    plain_c, plain_f = make_pair(npa, dev)
    with pytest.raises(NotImplementedError, match=words):       # a default HashNeRF
        npa.render_rays(rg, plain_c, None, N_C, N_importance=N_F, network_fine=plain_f, perturb=0.)
    with pytest.raises(NotImplementedError, match=words):       # ... also next to a flagged one
        npa.render_rays(rg, pair[0], None, N_C, N_importance=N_F, network_fine=plain_f, perturb=0.)
    dense = npa.dense.DenseNeRF(D=2, W=64, input_ch=63, input_ch_views=27, output_ch=4, skips=[], use_viewdirs=True).to(dev)
    with pytest.raises(NotImplementedError, match=words):
        npa.render_rays(rg, dense, None, N_C, perturb=0.)
    grid = npa.OccupancyGrid([-2.0] * 3, [2.0] * 3, 8, device=dev)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match=r"occupancy= together with general \(DenseNeRF\) networks is not implemented"):
            npa.render_rays(rays, pair[0], None, N_C, N_importance=N_F, network_fine=pair[1], perturb=0., occupancy=grid)
    with pytest.raises(NotImplementedError, match="point_grad=True"):
        npa.query_points(plain_f, rays[:, :3].clone().requires_grad_(True), rays[:, 8:11])
    with pytest.raises(NotImplementedError, match="fused-kernel NeRF module is required"):
        npa.density_volume(dense, [-1.0] * 3, [1.0] * 3, 5)
