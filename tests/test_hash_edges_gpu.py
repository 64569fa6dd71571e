"""GPU (-m gpu): the hash-grid kernels where the four-level power-of-two fixture of test_hash_gpu.py cannot see them, bit for bit against
HashEncoding.encode_reference(float32) and table_grad_reference on CPU copies -- resolutions and a box for which u R, p - i and
(x - lo) inv really round (ODD), F = 1, one level of 16 hashed rows (TINY), 32 levels (ALL_DENSE_32, MIXED_32), the default table
with row offsets beyond 2^22 (DEFAULT), lattice indices up to 2^24 (FINE); a maximum found in a later trip of the maximum kernel's
grid-stride loop; max |d_out| denormal, tiny and huge; a row that receives P M; rays + depths as the backward's point source; and the host
paths of HashNeRF that had not run (an encoding narrower than three columns, no view directions, the sliced no-grad query).
test_hash_edges_cpu.py holds the configurations and checks, without a GPU, the conditions these tests stand on."""
import pytest
import torch

import workloads as wl
from test_gpu_parity import dev, npa  # noqa: F401  (fixtures)
from test_hash_cpu import FOUR, HI, LO, four_level
from test_hash_edges_cpu import (BACKWARD_SEED, BACKWARD_SIZES, CONFIGS, MAGNITUDES, ODD_HI, ODD_LO, SATURATED_P, SATURATED_ROW, SMALL,
                                 edge_points, encoding, float64_errors, own_corner_collisions, saturated_case)
from test_hash_gpu import definition, kernel_grad

pytestmark = pytest.mark.gpu

F64 = torch.float64
CASES = SMALL + [("FINE", 2)]           # (FINE: against the fp32 definitions only -- float64 lands in other cells there)
FORWARD_SIZES = (1, 64, 257, 1000)
MAX_TRIP = 1024 * 256                   # elements one trip of hash_absmax_kernel's grid-stride loop covers (csrc/hash_encode.hip)
N_RAYS, N_DEPTHS = 33, 16


@pytest.fixture(scope="module")
def on_gpu(npa, dev):
    """(name, F) -> that configuration's encoding on the device, built once"""
    made = {}

    def get(name, F):
        if (name, F) not in made:
            made[name, F] = encoding(name, F).to(dev)
        return made[name, F]
    return get


@pytest.fixture(scope="module")
def default(npa, dev):
    """the configuration create_nerf --i_embed 1 builds: 5,262,476 rows, 42 MB of table and 84 MB of accumulator -- two tests use it"""
    return encoding("DEFAULT", 2).to(dev)


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def ints(g, *shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def grad_twice(npa, dev, enc, pts, d_out, **kw):
    """the kernel's table gradient, asserted equal over two calls that share one accumulator, which each leaves zero"""
    scratch = npa.hip_backend.hash_scratch(enc.desc(), dev)
    pts, d_out = pts.to(dev), d_out.to(dev)
    first = kernel_grad(npa, enc, pts, d_out, scratch=scratch, **kw)
    assert int(scratch[:-1].abs().max()) == 0
    second = kernel_grad(npa, enc, pts, d_out, scratch=scratch, **kw)
    assert int(scratch[:-1].abs().max()) == 0
    assert first.shape == enc.embeddings.shape and first.dtype == torch.float32 and torch.equal(second, first)
    return first.cpu()


# ------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("P", FORWARD_SIZES)
@pytest.mark.parametrize("name,F", CASES)
def test_forward_equals_the_definition_bit_for_bit(npa, dev, on_gpu, name, F, P):
    enc = on_gpu(name, F)
    pts = edge_points(enc, P, seed=P)
    want = definition(enc, pts)
    got = enc(pts.to(dev))
    assert got.shape == (P, enc.out_dim) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert torch.equal(got.detach().cpu(), want)


@pytest.mark.parametrize("name,F", [("ODD", 1), ("TINY", 4)])
def test_forward_writes_a_column_range_of_a_wider_matrix(npa, dev, on_gpu, name, F):
    enc = on_gpu(name, F)
    P, C = 257, enc.out_dim
    pts = edge_points(enc, P, seed=50).to(dev)
    wide = randn(P, 5 + C + 3, seed=3).to(dev)
    before = wide.clone()
    npa.hip_backend.hash_encode_fwd(enc.desc(), enc.embeddings.detach(), wide, 5, points=pts)
    assert torch.equal(wide[:, :5], before[:, :5]) and torch.equal(wide[:, 5 + C:], before[:, 5 + C:])
    assert torch.equal(wide[:, 5:5 + C].cpu(), definition(enc, pts))


# ------------------------------------------------------------------------------------------------ 2. backward
@pytest.mark.parametrize("P", BACKWARD_SIZES)
@pytest.mark.parametrize("name,F", CASES)
def test_backward_equals_the_fixed_point_rule_bit_for_bit_twice(npa, dev, on_gpu, name, F, P):
    enc = on_gpu(name, F)
    pts = edge_points(enc, P, seed=BACKWARD_SEED + P)
    if name == "TINY":          # 16 rows: one point adds to one row through two of its corners
        assert own_corner_collisions(enc, pts) >= 1
    d_out = randn(P, enc.out_dim, seed=P)
    want = enc.table_grad_reference(pts, d_out)
    assert float(want.abs().max()) > 0.0
    assert torch.equal(grad_twice(npa, dev, enc, pts, d_out), want)


# ------------------------------------------------------------------------------------------------ 3. the maximum, in a later trip
@pytest.mark.parametrize("name", ["DEFAULT", "MIXED_32"])
def test_the_maximum_is_found_in_a_later_trip_of_the_grid_stride_loop(npa, dev, on_gpu, request, name):
    enc = request.getfixturevalue("default") if name == "DEFAULT" else on_gpu(name, 1)
    P, C = 8200, enc.out_dim
    assert C == 32 and (P - 1) * C + C - 1 >= MAX_TRIP          # the last element is read in the loop's second trip
    pts = edge_points(enc, P, seed=60)
    d_out = randn(P, C, seed=61) * 1e-3
    d_out[P - 1, C - 1] = 50.0
    assert float(d_out.reshape(-1)[:MAX_TRIP].abs().max()) < 0.01
    want = enc.table_grad_reference(pts, d_out)
    assert torch.equal(grad_twice(npa, dev, enc, pts, d_out), want)
    if name == "DEFAULT":       # and the forward of the configuration users run, at the same points
        assert torch.equal(enc(pts.to(dev)).detach().cpu(), definition(enc, pts))


# ------------------------------------------------------------------------------------------------ 4. the magnitude of M
@pytest.mark.parametrize("s", MAGNITUDES)
def test_backward_at_a_denormal_a_tiny_and_a_huge_maximum(npa, dev, on_gpu, s):
    """max |d_out| = 3.8e-41 (a denormal: frexpf, the fp32 product w g and the conversion to double all see denormals), 3.8e-30 and
    4.9e30.  The device agrees with the definition bit for bit in all three."""
    enc = on_gpu("ODD", 2)
    pts = edge_points(enc, 1000, seed=37)
    d_out = randn(1000, enc.out_dim, seed=38) * s
    want = enc.table_grad_reference(pts, d_out)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0.0
    got = grad_twice(npa, dev, enc, pts, d_out)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ 5. a saturated row
@pytest.mark.parametrize("alternating", [False, True])
def test_a_row_that_receives_P_M(npa, dev, alternating):
    enc = four_level().to(dev)
    pts, d_out = saturated_case(alternating)
    got = grad_twice(npa, dev, enc, pts, d_out)
    assert torch.equal(got, enc.table_grad_reference(pts, d_out))
    want = 0.0 if alternating else SATURATED_P * float(torch.tensor(1.9999999))         # exact in the accumulator and in fp32
    assert got[SATURATED_ROW].tolist() == [want, want]


# ------------------------------------------------------------------------------------------------ 6. rays + depths as the point source
def test_rays_and_depths_are_the_points_in_the_backward_and_into_a_column_range(npa, dev, on_gpu):
    hb = npa.hip_backend
    enc = on_gpu("ODD", 2)
    C = enc.out_dim
    g = torch.Generator().manual_seed(8)
    rays = torch.cat([torch.randn(37, 3, generator=g) * 0.3, torch.randn(37, 3, generator=g), torch.rand(37, 5, generator=g)], 1).to(dev)
    z = (torch.rand(37, 9, generator=g) * 3.0).to(dev)
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).reshape(-1, 3).contiguous()        # a separate multiply and add
    d_out = randn(37 * 9, C, seed=9)
    want = enc.table_grad_reference(pts.cpu(), d_out)
    assert float(want.abs().max()) > 0.0
    scratch = hb.hash_scratch(enc.desc(), dev)
    from_rays = hb.hash_encode_bwd(enc.desc(), d_out.to(dev), rays=rays, z_vals=z, scratch=scratch)
    from_points = hb.hash_encode_bwd(enc.desc(), d_out.to(dev), points=pts, scratch=scratch)
    assert torch.equal(from_rays, from_points) and torch.equal(from_rays.cpu(), want) and int(scratch[:-1].abs().max()) == 0
    # the forward from rays into columns 5 .. 5 + C of a wider matrix
    wide = randn(37 * 9, 5 + C + 3, seed=3).to(dev)
    before = wide.clone()
    hb.hash_encode_fwd(enc.desc(), enc.embeddings.detach(), wide, 5, rays=rays, z_vals=z)
    assert torch.equal(wide[:, :5], before[:, :5]) and torch.equal(wide[:, 5 + C:], before[:, 5 + C:])
    assert torch.equal(wide[:, 5:5 + C].cpu(), definition(enc, pts))


# ------------------------------------------------------------------------------------------------ 7. error against float64 autograd
@pytest.mark.parametrize("name,F", [("ODD", 1), ("ODD", 2), ("ODD", 4), ("DEFAULT", 2)])
def test_backward_error_against_float64_autograd(npa, dev, on_gpu, request, name, F):
    enc = request.getfixturevalue("default") if name == "DEFAULT" else on_gpu(name, F)
    pts = edge_points(enc, 1000, seed=35)
    d_out = randn(1000, enc.out_dim, seed=36)
    got = kernel_grad(npa, enc, pts.to(dev), d_out.to(dev)).cpu()
    err, own = float64_errors(enc, pts, d_out, got)
    print(f"{name} F={F}: kernel error {err:.3e}, float32 autograd's own {own:.3e}, ratio {err / own:.2f}")
    assert own > 0.0 and err <= 4.0 * own


# ------------------------------------------------------------------------------------------------ 8. HashNeRF's host paths
@pytest.fixture(scope="module")
def rays(dev):
    return wl.synthetic_rays(N_RAYS, seed=3).to(dev).contiguous()


def seeded_net(npa, dev, seed, **kw):
    torch.manual_seed(seed)
    net = npa.HashNeRF(ODD_LO, ODD_HI, **kw)
    with torch.no_grad():
        net.encoding.embeddings.copy_(randn(*net.encoding.embeddings.shape, seed=seed + 10))
    return net.to(dev)


@pytest.mark.parametrize("case", ["narrower_than_three_columns", "no_view_directions"])
def test_query_and_its_table_gradient_equal_the_chain_of_public_pieces(npa, dev, rays, case):
    """(a) an encoding of 2 columns: _fill_views builds the view columns in a temporary and copies them behind the encoding;
    (b) use_viewdirs=False: no view columns, the density from output_linear"""
    if case == "narrower_than_three_columns":
        net = seeded_net(npa, dev, 0, n_levels=2, n_features=1, log2_hashmap_size=10, base_resolution=3, finest_resolution=37)
        assert net.input_ch == 2 and net.input_ch_views == 27
    else:
        net = seeded_net(npa, dev, 1, use_viewdirs=False, n_features=2, **CONFIGS["ODD"][2])
        assert net.input_ch == 10 and net.input_ch_views == 0
    views = net.use_viewdirs
    z = (2.0 + 4.0 * torch.rand(N_RAYS, N_DEPTHS, generator=torch.Generator().manual_seed(5))).to(dev)
    up = randn(N_RAYS, N_DEPTHS, 4, seed=6).to(dev)
    with torch.no_grad():
        got = net.query(rays, z)
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
    inside = ((pts > torch.tensor(ODD_LO, device=dev)) & (pts < torch.tensor(ODD_HI, device=dev))).all(1)
    assert 0.2 < float(inside.float().mean()) < 1.0         # points inside and outside the box
    dirs = rays[:, None, 8:11].expand(N_RAYS, N_DEPTHS, 3).reshape(-1, 3)
    embed_views, ch = npa.get_embedder(4, 0)
    assert ch == 27
    tail = [embed_views(dirs)] if views else []
    plain = npa.dense.DenseNeRF(D=2, W=64, input_ch=net.input_ch, input_ch_views=net.input_ch_views, output_ch=4, skips=[],
                                use_viewdirs=views).to(dev)
    plain.load_state_dict(net.mlp.state_dict())
    with torch.no_grad():
        want = plain(torch.cat([net.encoding(pts)] + tail, -1))
        hooked = net(torch.cat([pts] + tail, -1))
    assert got.shape == (N_RAYS, N_DEPTHS, 4)
    assert torch.equal(got.reshape(-1, 4), want) and torch.equal(hooked, want)
    assert float(got[..., 3].abs().max()) > 0.0
    # the table's gradient: the encoding's output as a leaf, so its .grad is the stack's d_x
    e = net.encoding(pts).detach().requires_grad_(True)
    (net.mlp(torch.cat([e] + tail, -1)) * up.reshape(-1, 4)).sum().backward()
    want_grad = net.encoding.table_grad_reference(pts.cpu(), e.grad.cpu())
    assert float(want_grad.abs().max()) > 0.0
    layers = [None if p.grad is None else p.grad.clone() for p in net.mlp.parameters()]        # (None: the unused view branch of (b))
    assert sum(a is not None for a in layers) >= 2 * 2 + 2
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        (net.query(rays, z) * up).sum().backward()
        assert torch.equal(net.encoding.embeddings.grad.cpu(), want_grad)
        assert all((p.grad is None) if a is None else torch.equal(a, p.grad) for a, p in zip(layers, net.mlp.parameters()))


def test_the_sliced_query_is_the_concatenation_of_its_slices(npa, dev, monkeypatch):
    """Without gradients HashNeRF.query evaluates QUERY_SLICE_POINTS points at a time.  On FOUR's box, with rays and depths on dyadic
    fractions and small integers in the table and the layers, every operation is exact: the sliced query equals the query of each
    slice alone, the unsliced one (gradients enabled) and the float64 chain, bit for bit."""
    import nerf_pytorch_amd.dense as dense
    import nerf_pytorch_amd.hashgrid as hashgrid
    assert hashgrid.QUERY_SLICE_POINTS == 1 << 20
    monkeypatch.setattr(hashgrid, "QUERY_SLICE_POINTS", 64)         # (hashgrid imported the name by value)
    n, S, per_slice = N_RAYS, N_DEPTHS, 64 // N_DEPTHS
    g = torch.Generator().manual_seed(9)
    net = npa.HashNeRF(LO, HI, D=2, W=8, input_ch_views=3, **FOUR).to(dev)
    assert (net.input_ch, net.multires_views) == (8, -1)
    table = ints(g, *net.encoding.embeddings.shape, lo=-2, hi=2)
    W = {k: ints(g, *v.shape, lo=-1, hi=1) for k, v in net.mlp.state_dict().items()}
    net.mlp.load_state_dict(W)
    with torch.no_grad():
        net.encoding.embeddings.copy_(table)
    # origins on eighths inside the box, directions in {-1, 0, 1}, depths on quarters: the points are multiples of 1/8
    lo, hi = torch.tensor(LO), torch.tensor(HI)
    origins = lo + torch.stack([ints(g, n, lo=0, hi=int(8 * (hi[a] - lo[a]))) for a in range(3)], 1) / 8.0
    rays = torch.cat([origins, ints(g, n, 3, lo=-1, hi=1), torch.zeros(n, 2), ints(g, n, 3, lo=-1, hi=1)], 1)
    z = ints(g, n, S, lo=0, hi=8) / 4.0
    rows = []
    apply = dense._DenseMLP.apply
    monkeypatch.setattr(dense._DenseMLP, "apply", lambda *a: (rows.append(a[1].shape[0]), apply(*a))[1])
    rays_d, z_d = rays.to(dev), z.to(dev)
    with torch.no_grad():
        sliced = net.query(rays_d, z_d)
        assert rows == [per_slice * S] * (n // per_slice) + [(n % per_slice) * S], rows
        del rows[:]
        alone = torch.cat([net.query(rays_d[i:i + per_slice].contiguous(), z_d[i:i + per_slice].contiguous()) for i in range(0, n, per_slice)], 0)
    assert sliced.shape == (n, S, 4) and torch.equal(sliced, alone)
    del rows[:]
    whole = net.query(rays_d, z_d)
    assert rows == [n * S] and whole.requires_grad and not sliced.requires_grad
    assert torch.equal(sliced, whole.detach())
    # the float64 chain: the definition of the encoding, then the layer stack on it and on the broadcast directions
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]
    inside = ((pts >= lo) & (pts <= hi)).all(-1)
    assert 0.2 < float(inside.float().mean()) < 1.0
    e = net.encoding.encode_reference(pts, F64, table.double())
    assert torch.equal(e, net.encoding.encode_reference(pts, torch.float32, table).double())
    W64 = {k: v.double() for k, v in W.items()}
    lin = lambda h, nm: h @ W64[nm + ".weight"].T + W64[nm + ".bias"]
    dirs = rays[:, None, 8:11].expand(n, S, 3).double()
    h = torch.relu(lin(torch.relu(lin(e, "pts_linears.0")), "pts_linears.1"))
    hv = torch.relu(lin(torch.cat([lin(h, "feature_linear"), dirs], -1), "views_linears.0"))
    ref = torch.cat([lin(hv, "rgb_linear"), lin(h, "alpha_linear")], -1)
    assert float(ref.abs().max()) > 8 and float(ref.abs().max()) * 2 ** 7 < 2 ** 24        # (weights carry at most 7 fractional bits)
    assert torch.equal(sliced.cpu().double(), ref)
