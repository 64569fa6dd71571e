"""CPU: baked fields without a GPU -- sh_basis, the packing of BakedField.from_nodes, BakedField.render_rays_reference against closed
forms, the edge rays, the stop rule, checkpoints, the guards of render_rays(baked=...) and the export of nerf_baked_render with its
argument errors."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import nerf_pytorch_amd as npa
from nerf_pytorch_amd.baked import BakedField, fibonacci_sphere, sh_basis

CPU = torch.device("cpu")
F64 = torch.float64
NAN, INF = float("nan"), float("inf")
C0 = 0.28209479177387814
NET_KW = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)


def unit_grid(res=4, mask=None):
    if mask is None:
        return npa.OccupancyGrid([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], res, device=CPU)
    return npa.OccupancyGrid.from_mask(mask, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], device=CPU)


def constant_field(sigma, colour, degree=0, res=4, mask=None, **kw):
    """constant sigma and a constant DC coefficient per channel on every node (the higher coefficients are 0)"""
    grid = unit_grid(res, mask)
    B = (degree + 1) ** 2
    nodes = torch.zeros(tuple(r + 1 for r in grid.resolution) + (1 + 3 * B,))
    nodes[..., 0] = sigma
    for c in range(3):
        nodes[..., 1 + c * B] = colour[c]
    return BakedField.from_nodes(grid, nodes, degree, **kw)


def x_ray(y=0.5, z=0.5, x0=-1.0, near=0.0, far=3.0, view=(1.0, 0.0, 0.0)):
    return [x0, y, z, 1.0, 0.0, 0.0, near, far, *view]


# ------------------------------------------------------------------------------------------------ sh_basis
def test_sh_basis_against_the_closed_forms():
    d = torch.randn(50, 3, generator=torch.Generator().manual_seed(3), dtype=F64)
    d = d / d.norm(dim=-1, keepdim=True)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    want = torch.stack([torch.full_like(x, 0.28209479177387814), -0.4886025119029199 * y, 0.4886025119029199 * z, -0.4886025119029199 * x,
                        1.0925484305920792 * x * y, -1.0925484305920792 * y * z, 0.31539156525252005 * (2 * z * z - x * x - y * y),
                        -1.0925484305920792 * x * z, 0.5462742152960396 * (x * x - y * y)], -1)
    for deg, B in ((0, 1), (1, 4), (2, 9)):
        got = sh_basis(d, deg)
        assert got.shape == (50, B) and got.dtype == F64
        assert float((got - want[:, :B]).abs().max()) <= 1e-14
    assert sh_basis(d.view(5, 10, 3), 2).shape == (5, 10, 9)
    assert sh_basis(d.float(), 1).dtype == torch.float32


def test_sh_basis_is_orthonormal_and_the_fit_matrix_inverts_it():
    Y = sh_basis(fibonacci_sphere(4096), 2)
    gram = Y.T @ Y / 4096.0
    assert float((gram - torch.eye(9, dtype=F64) / (4.0 * math.pi)).abs().max()) <= 1e-3
    fit = BakedField.sh_fit_matrix(32, 2)
    assert fit.shape == (9, 32) and fit.dtype == torch.float32
    assert float((fit.double() @ sh_basis(fibonacci_sphere(32), 2) - torch.eye(9, dtype=F64)).abs().max()) <= 1e-5
    d = fibonacci_sphere(7)
    assert float((d.norm(dim=-1) - 1.0).abs().max()) <= 1e-14
    assert float((d[:, 2] - (1.0 - (2.0 * torch.arange(7, dtype=F64) + 1.0) / 7.0)).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ packing
def test_from_nodes_packs_exactly_the_corners_of_occupied_cells():
    g = torch.Generator().manual_seed(11)
    mask = torch.rand(3, 4, 5, generator=g) < 0.3
    assert 0 < int(mask.sum()) < mask.numel()
    for degree, W in ((0, 4), (1, 16), (2, 32)):
        V = 1 + 3 * (degree + 1) ** 2
        nodes = torch.randn(4, 5, 6, V, generator=g)
        field = BakedField.from_nodes(unit_grid(mask=mask), nodes, degree)
        want = torch.zeros(4, 5, 6, dtype=torch.bool)
        for ix, iy, iz in mask.nonzero().tolist():
            want[ix:ix + 2, iy:iy + 2, iz:iz + 2] = True
        index = field.index.view(4, 5, 6)
        assert field.index.dtype == torch.int32 and field.table.dtype == torch.float16
        assert torch.equal(index > 0, want)
        M = int(want.sum())
        assert field.n_rows == M + 1 and field.table.shape == (M + 1, W)
        assert not bool(field.table[0].any()) and not bool(index[~want].any())
        assert torch.equal(index[want].long(), torch.arange(1, M + 1))             # rows in node order
        assert torch.equal(field.table[1:, :V], nodes[want].to(torch.float16))
        assert not bool(field.table[:, V:].any())
    empty = BakedField.from_nodes(unit_grid(mask=torch.zeros(3, 4, 5, dtype=torch.bool)), torch.randn(4, 5, 6, 4), 0)
    assert empty.n_rows == 1 and not bool(empty.index.any())
    full = BakedField.from_nodes(unit_grid(mask=torch.ones(3, 4, 5, dtype=torch.bool)), torch.randn(4, 5, 6, 4), 0)
    assert full.n_rows == 4 * 5 * 6 + 1 and torch.equal(full.index.long(), torch.arange(1, 121))
    with pytest.raises(ValueError, match="nodes must be"):
        BakedField.from_nodes(unit_grid(mask=mask), torch.randn(4, 5, 6, 4), 1)
    assert abs(full.step_size - 0.5 * 0.2) < 1e-7                                       # None: half the smallest cell edge


# ------------------------------------------------------------------------------------------------ the reference against closed forms
def test_constant_field_against_the_closed_forms():
    s, c = 2.0, (1.0, -2.0, 0.5)
    field = constant_field(s, c, step_size=1.0 / 8.0)
    out = field.render_rays_reference(torch.tensor([x_ray()]))
    assert int(out["n_samples"][0]) == 8 and out["rays_stopped"] == 0 and out["rgb_map"].dtype == F64
    t1 = math.exp(-s / 8.0) + 1e-10             # 1 - alpha + 1e-10 with alpha = 1 - exp(-s / 8)
    acc = 1.0 - t1 ** 8
    alpha = 1.0 - math.exp(-s / 8.0)
    # (sum_k alpha t1^k = alpha (1 - t1^8) / (1 - t1): equal to 1 - t1^8 up to the 1e-10)
    acc_exact = sum(alpha * t1 ** k for k in range(8))
    assert abs(float(out["acc_map"][0]) - acc_exact) <= 1e-14 and abs(acc_exact - acc) <= 1e-9
    for ch in range(3):
        rgb = 1.0 / (1.0 + math.exp(-C0 * float(np.float16(c[ch]))))
        assert abs(float(out["rgb_map"][0, ch]) - rgb * acc_exact) <= 1e-14
    depth = sum(alpha * t1 ** k * (1.0 + (k + 0.5) / 8.0) for k in range(8))
    assert abs(float(out["depth_map"][0]) - depth) <= 1e-14
    assert abs(float(out["disp_map"][0]) - 1.0 / (depth / acc_exact)) <= 1e-14
    white = field.render_rays_reference(torch.tensor([x_ray()]), white_bkgd=True)
    assert float((white["rgb_map"] - out["rgb_map"] - (1.0 - out["acc_map"])[:, None]).abs().max()) <= 1e-14
    assert torch.equal(white["acc_map"], out["acc_map"])
    # u moves the samples: u = 0 puts the first one on the face x = 0 (t = 0 is inside) and the ninth candidate on x = 1 (outside)
    moved = field.render_rays_reference(torch.tensor([x_ray()]), u=torch.tensor([0.0]))
    assert int(moved["n_samples"][0]) == 8
    assert abs(float(moved["depth_map"][0]) - sum(alpha * t1 ** k * (1.0 + k / 8.0) for k in range(8))) <= 1e-14
    # a ray that starts inside the box samples from near
    inside = field.render_rays_reference(torch.tensor([x_ray(x0=0.5, near=0.0, far=3.0)]))
    assert int(inside["n_samples"][0]) == 4
    assert abs(float(inside["depth_map"][0]) - sum(alpha * t1 ** k * ((k + 0.5) / 8.0) for k in range(4))) <= 1e-14
    # max_steps cuts the walk
    assert int(field.render_rays_reference(torch.tensor([x_ray()]), max_steps=11)["n_samples"][0]) == 3
    # float32: the same discrete decisions
    f32 = field.render_rays_reference(torch.tensor([x_ray()]), dtype=torch.float32)
    assert f32["rgb_map"].dtype == torch.float32 and int(f32["n_samples"][0]) == 8
    assert float((f32["rgb_map"].double() - out["rgb_map"]).abs().max()) <= 1e-6


def test_a_linear_node_field_is_reproduced_by_the_blend():
    """sigma = a + b . p on the nodes of a 4^3 grid: the trilinear blend is exact for it, so one sample of width ds at p gives
    acc = 1 - exp(-sigma(p) ds); the nodes' values are quarters and so exact in fp16"""
    grid = unit_grid(4)
    ax = torch.arange(5, dtype=F64) / 4.0
    X, Yy, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    lin = 0.5 + 1.0 * X + 2.0 * Yy + 4.0 * Z
    nodes = torch.zeros(5, 5, 5, 4)
    nodes[..., 0] = lin.float()
    assert torch.equal(nodes[..., 0].to(torch.float16).double(), lin)
    ds = 1.0 / 64.0
    field = BakedField.from_nodes(grid, nodes, 0, step_size=ds)
    g = torch.Generator().manual_seed(5)
    p = torch.rand(40, 3, generator=g)
    # one candidate per ray: along +x from p, near = 0, far = ds / 2 < the first step's successor; u = 0 samples p itself
    rays = torch.cat([p, torch.tensor([[1.0, 0.0, 0.0, 0.0, ds / 2.0, 1.0, 0.0, 0.0]]).expand(40, 8)], -1)
    out = field.render_rays_reference(rays, u=torch.zeros(40))
    assert bool((out["n_samples"] == 1).all())
    sigma = 0.5 + p.double() @ torch.tensor([1.0, 2.0, 4.0], dtype=F64)
    want = 1.0 - torch.exp(-sigma * ds)
    # t = p * 4 is exact in fp32 and f = t - floor(t) too; the blend of exact fp16 values in float64 leaves float64 rounding
    assert float((out["acc_map"] - want).abs().max()) <= 1e-14


def test_view_dependence_needs_a_degree():
    grid = unit_grid(4)
    nodes = torch.zeros(5, 5, 5, 13)
    nodes[..., 0] = 3.0
    nodes[..., 1] = 0.5                  # R: DC
    nodes[..., 1 + 3] = 2.0              # R: Y3 = -c1 x
    nodes[..., 5 + 2] = -1.0             # G: Y2 = c1 z
    deg1 = BakedField.from_nodes(grid, nodes, 1, step_size=0.125)
    fwd, back = (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0)
    rays = torch.tensor([x_ray(view=fwd), x_ray(view=back), x_ray(view=(0.0, 0.0, 1.0))])
    out = deg1.render_rays_reference(rays)
    acc = float(out["acc_map"][0])
    assert torch.equal(out["acc_map"], out["acc_map"][:1].expand(3))
    sig = lambda v: 1.0 / (1.0 + math.exp(-v))
    c1 = 0.4886025119029199
    assert abs(float(out["rgb_map"][0, 0]) - sig(0.5 * C0 - 2.0 * c1) * acc) <= 1e-14
    assert abs(float(out["rgb_map"][1, 0]) - sig(0.5 * C0 + 2.0 * c1) * acc) <= 1e-14
    assert abs(float(out["rgb_map"][2, 1]) - sig(-c1) * acc) <= 1e-14
    assert abs(float(out["rgb_map"][0, 1]) - 0.5 * acc) <= 1e-14
    assert float((out["rgb_map"][0] - out["rgb_map"][1]).abs().max()) > 0.1
    dc = constant_field(3.0, (0.5, 0.0, 0.0), step_size=0.125)
    out0 = dc.render_rays_reference(rays)
    assert torch.equal(out0["rgb_map"][0], out0["rgb_map"][1]) and torch.equal(out0["rgb_map"][0], out0["rgb_map"][2])


# ------------------------------------------------------------------------------------------------ edge rays
def edge_rays():
    """(rays [5, 11], names): rays that must give the background on the half-empty grid of edge_field()"""
    return torch.tensor([x_ray(y=1.5),                                  # misses the box
                         [NAN] + x_ray()[1:],                           # a NaN
                         x_ray(near=3.0, far=3.0),                      # near >= far
                         [-1.0, 0.5, 0.5, 0.0, 0.0, 0.0, 0.0, 3.0, 1.0, 0.0, 0.0],      # d = 0
                         x_ray(z=0.875)]), ("miss", "nan", "near >= far", "d = 0", "empty cells only")


def edge_field(**kw):
    mask = torch.ones(4, 4, 4, dtype=torch.bool)
    mask[:, :, 3] = False               # the layer z in [0.75, 1) is empty
    return constant_field(5.0, (1.0, 1.0, 1.0), mask=mask, step_size=0.125, **kw)


def test_edge_rays_return_the_background():
    rays, names = edge_rays()
    for eps in (0.0, 0.5):
        field = edge_field(stop_eps=eps)
        for white in (False, True):
            out = field.render_rays_reference(rays, white_bkgd=white)
            assert out["rays_stopped"] == 0
            for i, name in enumerate(names):
                assert int(out["n_samples"][i]) == 0, name
                assert float(out["acc_map"][i]) == 0.0 and float(out["depth_map"][i]) == 0.0, name
                assert torch.equal(out["rgb_map"][i], torch.full((3,), 1.0 if white else 0.0, dtype=F64)), name
                assert math.isnan(float(out["disp_map"][i])), name              # 0 / 0, as nerf_raw2outputs gives it
    # the same rays through the occupied layer are sampled: the grid decides, not the table
    hit = edge_field().render_rays_reference(torch.tensor([x_ray(z=0.625)]))
    assert int(hit["n_samples"][0]) == 8
    # a point outside the box is never sampled, whatever the grid says about outside
    field = edge_field()
    for outside in ("evaluate", "skip"):
        field.grid.outside = outside
        assert int(field.render_rays_reference(torch.tensor([x_ray()]))["n_samples"][0]) == 8


# ------------------------------------------------------------------------------------------------ the stop
def test_the_stop_acts_between_rounds_and_is_bounded_by_eps():
    eps = 1e-2
    grid = npa.OccupancyGrid([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], 4, device=CPU)
    nodes = torch.zeros(5, 5, 5, 4)
    nodes[..., 0] = 40.0
    nodes[..., 1:] = torch.tensor([1.0, -1.0, 0.25])
    ds = 1.0 / 200.0            # 200 candidates inside the box: four rounds; T after 64 of them is exp(-12.8) < eps
    free = BakedField.from_nodes(grid, nodes, 0, step_size=ds)
    stop = BakedField.from_nodes(grid, nodes, 0, step_size=ds, stop_eps=eps)
    rays = torch.tensor([x_ray(x0=0.0, far=2.0), x_ray(x0=0.0, far=2.0, y=0.25), x_ray(y=1.5)])
    a, b = free.render_rays_reference(rays), stop.render_rays_reference(rays)
    assert a["n_samples"].tolist() == [200, 200, 0] and a["rays_stopped"] == 0
    assert b["n_samples"].tolist() == [64, 64, 0] and b["rays_stopped"] == 2
    assert float((a["rgb_map"] - b["rgb_map"]).abs().max()) <= eps and float((a["acc_map"] - b["acc_map"]).abs().max()) <= eps
    assert float((a["acc_map"] - b["acc_map"]).abs().max()) > 0.0
    # a thin field never gets below eps: nothing stops, nothing changes
    nodes[..., 0] = 0.5
    thin_free = BakedField.from_nodes(grid, nodes, 0, step_size=ds).render_rays_reference(rays)
    thin_stop = BakedField.from_nodes(grid, nodes, 0, step_size=ds, stop_eps=eps).render_rays_reference(rays)
    assert thin_stop["rays_stopped"] == 0 and torch.equal(thin_free["rgb_map"], thin_stop["rgb_map"])
    # a ray whose only round ends below eps counts as stopped and loses nothing
    short = BakedField.from_nodes(grid, torch.full((5, 5, 5, 4), 60.0), 0, step_size=1.0 / 32.0, stop_eps=eps)
    out = short.render_rays_reference(rays[:1])
    assert out["n_samples"].tolist() == [32] and out["rays_stopped"] == 1


# ------------------------------------------------------------------------------------------------ checkpoints
def test_state_dict_round_trip(tmp_path):
    g = torch.Generator().manual_seed(2)
    mask = torch.rand(3, 4, 5, generator=g) < 0.4
    grid = npa.OccupancyGrid.from_mask(mask, [-1.0, 0.0, 1.0], [2.0, 1.0, 3.0], outside="skip", device=CPU)
    field = BakedField.from_nodes(grid, torch.randn(4, 5, 6, 13, generator=g), 1, step_size=0.07, stop_eps=1e-3)
    path = os.path.join(tmp_path, "baked.pt")
    torch.save(field.state_dict(), path)
    state = torch.load(path)
    other_grid = npa.OccupancyGrid([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], (3, 4, 5), device=CPU)
    other = BakedField.from_nodes(other_grid, torch.zeros(4, 5, 6, 13), 1)
    assert other.load_state_dict(state) is other
    assert torch.equal(other.index, field.index) and torch.equal(other.table, field.table)
    assert other.step_size == field.step_size and other.stop_eps == field.stop_eps and other.sh_degree == 1
    assert torch.equal(other.grid.bits, grid.bits) and other.grid.outside == "skip" and np.array_equal(other.grid.lo, grid.lo)
    rays = torch.tensor([[-2.0, 0.5, 2.0, 1.0, 0.01, 0.02, 0.0, 6.0, 1.0, 0.0, 0.0]])
    a, b = field.render_rays_reference(rays), other.render_rays_reference(rays)
    assert int(a["n_samples"][0]) > 0 and torch.equal(a["rgb_map"], b["rgb_map"])
    with pytest.raises(ValueError, match="sh_degree"):
        BakedField.from_nodes(other_grid, torch.zeros(4, 5, 6, 4), 0).load_state_dict(state)
    wrong = npa.OccupancyGrid([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], (3, 4, 6), device=CPU)
    with pytest.raises(ValueError, match="grid"):
        BakedField.from_nodes(wrong, torch.zeros(4, 5, 7, 13), 1).load_state_dict(state)
    assert field.to(CPU) is field


# ------------------------------------------------------------------------------------------------ guards
def test_the_parameter_is_keyword_only_and_every_guard_fires_before_a_launch(monkeypatch):
    params = inspect.signature(npa.render_rays).parameters
    names = list(params)
    assert params["baked"].kind is inspect.Parameter.KEYWORD_ONLY and params["baked"].default is None
    assert names.index("baked") > names.index("interlevel") and names[names.index("distortion") + 1] == "interlevel"
    for name in ("BakedField", "sh_basis"):
        assert name in npa.__all__ and callable(getattr(npa, name)), name
    net = npa.NeRF(**NET_KW)
    monkeypatch.setattr(npa.hip_backend, "lib", lambda: pytest.fail("a guard let a call reach the library"))
    field = constant_field(1.0, (0.0, 0.0, 0.0))
    dgrid = npa.DensityGrid([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], 4, device=CPU)
    rays = torch.tensor([x_ray()] * 4)
    refused = dict(occupancy=dict(occupancy=dgrid), clip_to_occupancy=dict(occupancy=dgrid, clip_to_occupancy=True),
                   proposal=dict(occupancy=dgrid, proposal="grid"), early_stop_eps=dict(early_stop_eps=0.1),
                   march_steps=dict(proposal="march", march_steps=16), march_stop_eps=dict(march_stop_eps=0.1),
                   march_step_size=dict(march_step_size=0.1), march_fit=dict(march_fit=1), distortion=dict(distortion=True),
                   interlevel=dict(interlevel=True), retraw=dict(retraw=True), raw_noise_std=dict(raw_noise_std=1.0),
                   randoms=dict(randoms={"u_march": torch.zeros(4)}))
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            for name, kw in refused.items():
                for nets in ((net, net), (None, None)):
                    with pytest.raises(ValueError, match=f"cannot be combined with .*{name}"):
                        npa.render_rays(rays, nets[0], None, N_samples=8, network_fine=nets[1], baked=field, **kw)
            with pytest.raises(ValueError, match="network_query_fn"):
                npa.render_rays(rays, None, lambda pts, vd, m: None, N_samples=8, baked=field)
            with pytest.raises(ValueError, match="11 columns"):
                npa.render_rays(rays[:, :8], None, None, N_samples=8, baked=field)
            with pytest.raises(ValueError, match="BakedField"):
                npa.render_rays(rays, None, None, N_samples=8, baked=dgrid)
    with pytest.raises(ValueError, match="no backward"):
        npa.render_rays(rays.clone().requires_grad_(True), None, None, N_samples=8, baked=field)
    # through the layers that forward keywords
    with pytest.raises(ValueError, match="cannot be combined with distortion"):
        npa.batchify_rays(rays, 2, network_fn=None, network_query_fn=None, N_samples=8, baked=field, distortion=True)
    K = np.array([[10.0, 0, 2.0], [0, 10.0, 2.0], [0, 0, 1]])
    with pytest.raises(ValueError, match="cannot be combined with retraw"):
        npa.render(2, 2, K, chunk=8, rays=(rays[:, 0:3], rays[:, 3:6]), ndc=False, near=0.0, far=3.0, use_viewdirs=True, network_fn=None,
                   network_query_fn=None, N_samples=8, baked=field, retraw=True)
    # the field's own parameters
    grid = unit_grid(4)
    nodes = torch.zeros(5, 5, 5, 4)
    for bad in (-1, 3, 1.0, True, "2", None):
        with pytest.raises(ValueError, match="sh_degree"):
            BakedField.from_nodes(grid, nodes, bad)
        with pytest.raises(ValueError, match="sh_degree"):
            BakedField.from_network(net, grid, sh_degree=bad)
        with pytest.raises(ValueError, match="sh_degree"):
            sh_basis(torch.zeros(1, 3), bad)
    for bad in (0.0, -0.1, NAN, INF, True, "0.1", 1e-60):
        with pytest.raises(ValueError, match="step_size"):
            BakedField.from_nodes(grid, nodes, 0, step_size=bad)
        with pytest.raises(ValueError, match="step_size"):
            BakedField.from_network(net, grid, step_size=bad)
    for bad in (-0.1, 1.0, 1.0 - 1e-12, NAN, True, "0.1", None):
        with pytest.raises(ValueError, match="stop_eps"):
            BakedField.from_nodes(grid, nodes, 0, stop_eps=bad)
        with pytest.raises(ValueError, match="stop_eps"):
            BakedField.from_network(net, grid, stop_eps=bad)
    for degree, bad in ((2, 8), (1, 3), (0, 0), (2, 16.0), (2, True)):
        with pytest.raises(ValueError, match="n_dirs"):
            BakedField.from_network(net, grid, sh_degree=degree, n_dirs=bad)
        with pytest.raises(ValueError, match="n_dirs"):
            BakedField.sh_fit_matrix(bad, degree)
    for bad in (0, -1, (1 << 24) + 1, 4.0, True):
        with pytest.raises(ValueError, match="max_steps"):
            field.render_rays_reference(rays, max_steps=bad)
        with pytest.raises(ValueError, match="max_steps"):
            field.render_rays(rays, max_steps=bad)
    with pytest.raises(npa.hip_backend.NerfHipError, match="on the GPU"):       # a CPU field renders by the reference only
        field.render_rays(rays)


# ------------------------------------------------------------------------------------------------ exports
def test_the_library_exports_and_binds_the_entry_point():
    hb = npa.hip_backend
    raw = ctypes.CDLL(npa.build.LIB_PATH)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_hip.h")) as f:
        header = f.read()
    assert hasattr(raw, "nerf_baked_render") and "nerf_baked_render" in hb.EXPORTS and "int nerf_baked_render(const NerfOccGrid* grid" in header
    assert "#define NERF_ABI_VERSION 10" in header and hb.ABI_VERSION == 10
    assert "baked.hip" in npa.build.SOURCES and "grid_device.h" in npa.build.HEADERS
    assert list(inspect.signature(hb.baked_render).parameters) == ["desc", "node_index", "table", "sh_degree", "rays", "u", "step_size",
                                                                   "max_steps", "stop_eps", "white_bkgd"]
    rows = {k: v for k, v in npa.build.resource_usage().items() if "baked_render_kernel" in k}
    assert len(rows) == 3, sorted(rows)
    for k, v in rows.items():
        assert v["scratch_bytes_per_lane"] == 0 and v.get("vgpr_spills", 0) == 0 and v.get("sgpr_spills", 0) == 0 and v["lds_bytes"] == 0, (k, v)
    L = hb.lib()
    # the limits, refused before anything is launched or read (host memory stands in for the device buffers)
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf) & ~15
    desc = hb.NerfOccGrid((ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_int * 3)(2, 2, 2), 0, ptr)

    def call(grid=True, rows=1, degree=0, stride=11, n=1, ds=0.5, M=4, eps=0.0, **null):
        a = dict(index=ptr, table=ptr, rays=ptr, rgb=ptr, disp=ptr, acc=ptr, depth=ptr, count=ptr)
        a.update(null)
        return L.nerf_baked_render(ctypes.byref(desc) if grid else None, a["index"], a["table"], rows, degree, a["rays"], stride, None, n, ds, M,
                                   eps, 0, a["rgb"], a["disp"], a["acc"], a["depth"], a["count"], None)
    err = lambda: L.nerf_last_error().decode()
    assert call(grid=False) == -1 and "null" in err()
    for name in ("index", "table", "rays", "rgb", "disp", "acc", "depth", "count"):
        assert call(**{name: None}) == -1 and "null" in err(), name
    for degree in (-1, 3):
        assert call(degree=degree) == -1 and "sh_degree" in err(), degree
    assert call(stride=10) == -1 and "11 columns" in err()
    assert call(n=-1) == -1 and "bad size" in err()
    for ds in (0.0, -0.5, NAN, INF):
        assert call(ds=ds) == -1 and "step_size" in err(), ds
    for M in (0, -4, (1 << 24) + 1):
        assert call(M=M) == -1 and "max_steps" in err(), M
    for eps in (-0.1, 1.0, 2.0, NAN):
        assert call(eps=eps) == -1 and "stop_eps" in err(), eps
    for rows_ in (0, -1):
        assert call(rows=rows_) == -1 and "n_rows" in err(), rows_
    assert call(table=ptr + 8) == -1 and "aligned" in err()
    for degree in (0, 1, 2):
        assert call(n=0, degree=degree, M=1 << 14, eps=0.5) == 0          # no rays: nothing to do
