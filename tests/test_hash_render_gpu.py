"""GPU (-m gpu): HashNeRF through render_rays -- query against the chain built from public pieces (HashEncoding, the view embedder,
DenseNeRF.forward), the table gradients of a training step against table_grad_reference on that chain's d_x, the unchanged layer
gradients of a plain DenseNeRF, one Adam step through create_nerf(--i_embed 1), a checkpoint, and the refusals of the general-network
path.  33 rays, 8 + 8 samples."""
import os

import pytest
import torch

import workloads as wl
from test_gpu_parity import dev, npa  # noqa: F401  (fixtures)
from test_hash_cpu import FOUR, hash_args

pytestmark = pytest.mark.gpu

N_RAYS, N_C, N_F = 33, 8, 8
BOUND = 1.5


def make_pair(npa, dev, seed=0):
    torch.manual_seed(seed)
    nets = []
    for k in range(2):
        net = npa.HashNeRF([-BOUND] * 3, [BOUND] * 3, **FOUR)
        with torch.no_grad():       # a table large enough for the field to have structure
            net.encoding.embeddings.copy_(torch.randn(net.encoding.embeddings.shape, generator=torch.Generator().manual_seed(seed + 10 + k)))
        nets.append(net.to(dev))
    return nets


@pytest.fixture(scope="module")
def rays(dev):
    return wl.synthetic_rays(N_RAYS, seed=3).to(dev).contiguous()


@pytest.fixture(scope="module")
def target(dev):
    return torch.rand(N_RAYS, 3, generator=torch.Generator().manual_seed(4)).to(dev)


def render_loss(npa, rays, target, nc, nf, query_fn=None):
    ret = npa.render_rays(rays, nc, query_fn, N_C, N_importance=N_F, network_fine=nf, perturb=0., white_bkgd=True, raw_noise_std=0.)
    return npa.img2mse(ret["rgb_map"], target) + npa.img2mse(ret["rgb0"], target)


def grads_of(*nets):
    return [p.grad.clone() for net in nets for p in net.parameters()]


def test_query_equals_the_chain_of_public_pieces(npa, dev, rays):
    nc, _ = make_pair(npa, dev)
    z = (2.0 + 4.0 * torch.rand(N_RAYS, N_C + N_F, generator=torch.Generator().manual_seed(5))).to(dev)
    with torch.no_grad():
        got = nc.query(rays, z)
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
    dirs = rays[:, None, 8:11].expand(N_RAYS, N_C + N_F, 3).reshape(-1, 3)
    embed_views, ch = npa.get_embedder(4, 0)
    assert ch == nc.input_ch_views
    plain = npa.dense.DenseNeRF(D=2, W=64, input_ch=nc.input_ch, input_ch_views=27, output_ch=4, skips=[], use_viewdirs=True).to(dev)
    plain.load_state_dict(nc.mlp.state_dict())
    with torch.no_grad():
        want = plain(torch.cat([nc.encoding(pts), embed_views(dirs)], -1))
        hooked = nc(torch.cat([pts, embed_views(dirs)], -1))
    assert got.shape == (N_RAYS, N_C + N_F, 4)
    assert torch.equal(got.reshape(-1, 4), want) and torch.equal(hooked, want)
    assert float(got[..., 3].abs().max()) > 0.0


def test_training_step_fills_tables_and_layers_deterministically(npa, dev, rays, target):
    nc, nf = make_pair(npa, dev)
    render_loss(npa, rays, target, nc, nf).backward()
    first = grads_of(nc, nf)
    for net in (nc, nf):
        for name, p in net.named_parameters():
            assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), name
            assert float(p.grad.abs().max()) > 0.0, name
        net.zero_grad(set_to_none=True)
    render_loss(npa, rays, target, nc, nf).backward()
    assert all(torch.equal(a, b) for a, b in zip(first, grads_of(nc, nf)))

    # the chain of public pieces inside a user hook: the encoding's output becomes a leaf, so its .grad is the stack's d_x
    embed_views, _ = npa.get_embedder(4, 0)
    seen = []

    def hook(pts, viewdirs, net):
        flat = pts.reshape(-1, 3)
        dirs = viewdirs[:, None].expand(pts.shape).reshape(-1, 3)
        e = net.encoding(flat).detach().requires_grad_(True)
        seen.append((net, flat.detach(), e))
        return net.mlp(torch.cat([e, embed_views(dirs)], -1)).reshape(*pts.shape[:-1], 4)
    for net in (nc, nf):
        net.zero_grad(set_to_none=True)
    render_loss(npa, rays, target, nc, nf, hook).backward()
    assert [s[0] for s in seen] == [nc, nf]
    for (net, flat, e), table_grad in zip(seen, (first[0], first[len(list(nc.parameters()))])):
        assert net.encoding.embeddings.grad is None             # (cut off by the leaf)
        want = net.encoding.table_grad_reference(flat.cpu(), e.grad.cpu())
        assert torch.equal(table_grad.cpu(), want)
    hooked_layers = [p.grad for net in (nc, nf) for p in net.mlp.parameters()]
    ours = [g for net, gs in ((nc, first[:len(list(nc.parameters()))]), (nf, first[len(list(nc.parameters())):])) for g in gs[1:]]
    assert all(torch.equal(a, b) for a, b in zip(hooked_layers, ours))


@pytest.mark.parametrize("arch", [dict(D=2, W=64, skips=[]), dict(D=4, W=32, skips=[1])])
def test_layer_gradients_do_not_change_when_x_requires_grad(npa, dev, arch):
    """_DenseMLP's parameter gradients with and without the additional d_x, and d_x itself against float64 autograd of the same stack"""
    torch.manual_seed(1)
    net = npa.dense.DenseNeRF(input_ch=8, input_ch_views=27, output_ch=4, use_viewdirs=True, **arch).to(dev)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(65, 35, generator=g).to(dev)
    up = torch.randn(65, 4, generator=g).to(dev)
    (net(x) * up).sum().backward()
    plain = grads_of(net)
    net.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    (net(xg) * up).sum().backward()
    assert all(torch.equal(a, b) for a, b in zip(plain, grads_of(net)))
    assert xg.grad.shape == x.shape

    P = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    x64 = x.cpu().double().requires_grad_(True)
    h = x64[:, :8]
    for i in range(arch["D"]):
        h = torch.relu(torch.nn.functional.linear(h, P[f"pts_linears.{i}.weight"], P[f"pts_linears.{i}.bias"]))
        if i in arch["skips"]:
            h = torch.cat([x64[:, :8], h], -1)
    alpha = torch.nn.functional.linear(h, P["alpha_linear.weight"], P["alpha_linear.bias"])
    feat = torch.nn.functional.linear(h, P["feature_linear.weight"], P["feature_linear.bias"])
    hv = torch.relu(torch.nn.functional.linear(torch.cat([feat, x64[:, 8:]], -1), P["views_linears.0.weight"], P["views_linears.0.bias"]))
    out = torch.cat([torch.nn.functional.linear(hv, P["rgb_linear.weight"], P["rgb_linear.bias"]), alpha], -1)
    (out * up.cpu().double()).sum().backward()
    scale = float(x64.grad.abs().max())
    # fp32 GEMMs over at most 64 terms per layer, a handful of layers: 1e-5 of the largest entry leaves two decimal orders of room
    assert scale > 0.0 and float((xg.grad.cpu().double() - x64.grad).abs().max()) <= 1e-5 * scale


def test_adam_step_and_checkpoint_through_create_nerf(npa, dev, rays, target, tmp_path):
    args = hash_args(tmp_path, "--hash_bound", str(BOUND), "--white_bkgd", "--dataset_type", "blender", "--perturb", "0")
    train, test, start, grad_vars, opt = npa.create_nerf(args, device=dev)
    nc, nf = train["network_fn"], train["network_fine"]
    assert isinstance(nc, npa.HashNeRF) and type(opt) is torch.optim.Adam and start == 0
    before = [nc.encoding.embeddings.detach().clone(), nf.encoding.embeddings.detach().clone()]
    kw = {k: v for k, v in train.items() if k not in ("ndc", "use_viewdirs")}
    ret = npa.render_rays(rays, **kw)
    loss = npa.img2mse(ret["rgb_map"], target) + npa.img2mse(ret["rgb0"], target)
    opt.zero_grad()
    loss.backward()
    opt.step()
    for b, net in zip(before, (nc, nf)):
        assert not torch.equal(b, net.encoding.embeddings) and bool(torch.isfinite(net.encoding.embeddings).all())
    # the reference's checkpoint (run_nerf.py:797-804) reloads: step, both networks with their tables, the optimizer
    os.makedirs(os.path.join(str(tmp_path), "h"), exist_ok=True)
    torch.save({"global_step": 3, "network_fn_state_dict": nc.state_dict(), "network_fine_state_dict": nf.state_dict(),
                "optimizer_state_dict": opt.state_dict()}, os.path.join(str(tmp_path), "h", "000003.tar"))
    train2, _, start2, grad_vars2, opt2 = npa.create_nerf(args, device=dev)
    assert start2 == 3 and all(torch.equal(a, b) for a, b in zip(grad_vars, grad_vars2))
    assert opt2.state_dict()["state"][0]["step"] == opt.state_dict()["state"][0]["step"]
    with torch.no_grad():
        a = npa.render_rays(rays, **{k: v for k, v in test.items() if k not in ("ndc", "use_viewdirs")})["rgb_map"]
        kw2 = dict({k: v for k, v in test.items() if k not in ("ndc", "use_viewdirs")}, network_fn=train2["network_fn"],
                   network_fine=train2["network_fine"])
        b = npa.render_rays(rays, **kw2)["rgb_map"]
    assert torch.equal(a, b)


def test_the_general_network_refusals_hold_word_for_word(npa, dev, rays):
    nc, nf = make_pair(npa, dev)
    grid = npa.OccupancyGrid([-2.0] * 3, [2.0] * 3, 8, device=dev)
    kw = dict(N_importance=N_F, network_fine=nf, perturb=0.)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match=r"occupancy= together with general \(DenseNeRF\) networks is not implemented; the grid "
                                                      r"path runs the fused NeRF architecture only"):
            npa.render_rays(rays, nc, None, N_C, occupancy=grid, **kw)
    with pytest.raises(NotImplementedError, match=r"gradients to rays / sample points / camera poses are implemented for the fused NeRF "
                                                  r"architecture only, not for general \(DenseNeRF\) networks"):
        npa.render_rays(rays.clone().requires_grad_(True), nc, None, N_C, **kw)
    fused = npa.NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True).to(dev)
    with pytest.raises(NotImplementedError, match="must both be fused-kernel NeRF modules"):
        npa.render_rays(rays, nc, None, N_C, N_importance=N_F, network_fine=fused)
    with pytest.raises(ValueError, match="11 columns"):
        npa.render_rays(rays[:, :8].contiguous(), nc, None, N_C, **kw)
    # the empty batch renders, and its backward leaves exact zeros in the tables
    ret = npa.render_rays(rays[:0], nc, None, N_C, **kw)
    assert ret["rgb_map"].shape == (0, 3)
    (ret["rgb_map"].sum() + ret["rgb0"].sum()).backward()
    for net in (nc, nf):
        assert int((net.encoding.embeddings.grad != 0).sum()) == 0
