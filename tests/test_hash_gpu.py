"""GPU (-m gpu): the hash-grid kernels against HashEncoding's torch definitions, bit for bit -- nerf_hash_encode_fwd against
encode_reference(float32), nerf_hash_encode_bwd against table_grad_reference (the 64-bit fixed-point rule), twice; the column range of a
wider matrix; zero and non-finite upstream gradients; the empty batch.  The four-level configuration (two dense and two hashed
levels) at F = 2 and F = 4."""
import pytest
import torch

from test_gpu_parity import dev, npa  # noqa: F401  (fixtures)
from test_hash_cpu import FOUR, HI, LO, box_points, node_points

pytestmark = pytest.mark.gpu

F64 = torch.float64
SIZES = (0, 1, 63, 65, 1000)


def special_points(enc):
    """lattice nodes of every level, a point on each of the six faces, hi exactly, lo exactly, points outside the box"""
    lo, hi = torch.tensor(LO), torch.tensor(HI)
    inside = box_points(6, 21)
    faces = inside.clone()
    for k in range(6):
        faces[k, k // 2] = (lo, hi)[k % 2][k // 2]
    outside = torch.stack([hi + torch.tensor([0.5, 0.0, 0.0]), lo - torch.tensor([0.0, 3.0, 0.25]), hi + 1e30, lo - 7.0,
                           torch.tensor([0.0, 9.0, 1.0]), torch.tensor([-40.0, 0.25, 2.0])])
    nodes = torch.cat([node_points(enc, level)[1] for level in range(enc.n_levels)])
    return torch.cat([hi[None], faces, outside, lo[None], nodes])


def points_of(enc, P, seed):
    special = special_points(enc)
    assert special.shape[0] <= 63
    return torch.cat([special, box_points(max(P - special.shape[0], 0), seed, spread=1.15)])[:P].contiguous()


@pytest.fixture(scope="module", params=[2, 4])
def enc(request, npa, dev):
    e = npa.HashEncoding(LO, HI, n_features=request.param, **FOUR)
    with torch.no_grad():
        e.embeddings.copy_(torch.randn(e.embeddings.shape, generator=torch.Generator().manual_seed(40 + request.param)))
    return e.to(dev)


def definition(enc, pts):
    """encode_reference(float32) on the CPU: plain torch ops on CPU copies of the points and the table"""
    return enc.encode_reference(pts.cpu(), embeddings=enc.embeddings.detach().cpu())


def kernel_grad(npa, enc, pts, d_out, **kw):
    return npa.hip_backend.hash_encode_bwd(enc.desc(), d_out, points=pts, **kw)


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("P", SIZES)
def test_forward_equals_the_definition_bit_for_bit(npa, dev, enc, P):
    pts = points_of(enc, P, seed=P)
    want = definition(enc, pts)
    got = enc(pts.to(dev))
    assert got.shape == (P, enc.out_dim) and got.dtype == torch.float32
    assert torch.equal(got.detach().cpu(), want)
    if P:
        assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize("P", SIZES)
def test_forward_writes_a_column_range_of_a_wider_matrix(npa, dev, enc, P):
    hb = npa.hip_backend
    pts = points_of(enc, P, seed=100 + P).to(dev)
    C = enc.out_dim
    wide = torch.randn(P, 5 + C + 3, generator=torch.Generator().manual_seed(3)).to(dev)
    before = wide.clone()
    hb.hash_encode_fwd(enc.desc(), enc.embeddings.detach(), wide, 5, points=pts)
    assert torch.equal(wide[:, :5], before[:, :5]) and torch.equal(wide[:, 5 + C:], before[:, 5 + C:])
    assert torch.equal(wide[:, 5:5 + C].cpu(), definition(enc, pts))


def test_forward_from_rays_and_depths_equals_the_points(npa, dev, enc):
    g = torch.Generator().manual_seed(8)
    rays = torch.cat([torch.randn(37, 3, generator=g) * 0.3, torch.randn(37, 3, generator=g), torch.rand(37, 5, generator=g)], 1).to(dev)
    z = (torch.rand(37, 9, generator=g) * 3.0).to(dev)
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).reshape(-1, 3).contiguous()
    out = torch.empty(37 * 9, enc.out_dim, device=dev)
    npa.hip_backend.hash_encode_fwd(enc.desc(), enc.embeddings.detach(), out, rays=rays, z_vals=z)
    assert torch.equal(out, enc(pts).detach())
    with pytest.raises(npa.hip_backend.NerfHipError):
        npa.hip_backend.hash_encode_fwd(enc.desc(), enc.embeddings.detach(), out, points=pts, rays=rays, z_vals=z)


def test_non_finite_coordinates_do_not_fault(npa, dev, enc):
    nan, inf = float("nan"), float("inf")
    pts = torch.tensor([[nan, 0.0, 1.0], [inf, -inf, nan], [0.5, 0.5, inf], [nan, nan, nan], [0.0, 0.5, 1.0]], device=dev)
    out = enc(pts)
    torch.cuda.synchronize()
    assert torch.equal(out[4].cpu(), definition(enc, pts[4:])[0])        # (the others are unspecified)
    grad = kernel_grad(npa, enc, pts, torch.ones(5, enc.out_dim, device=dev))
    torch.cuda.synchronize()
    assert grad.shape == enc.embeddings.shape and bool(torch.isfinite(grad).all())


# ------------------------------------------------------------------------------------------------ backward
def one_cell_points(enc, n, seed):
    """n points strictly inside cell (21, 3, 30) of the finest level: eight rows take every contribution of that level"""
    R = enc.level_resolution[-1]
    u = torch.rand(n, 3, generator=torch.Generator().manual_seed(seed), dtype=F64) * 0.98 + 0.01
    lo, hi = torch.tensor(LO, dtype=F64), torch.tensor(HI, dtype=F64)
    return (lo + (torch.tensor([21.0, 3.0, 30.0], dtype=F64) + u) / R * (hi - lo)).float()


def backward_case(enc, name):
    C = enc.out_dim
    g = torch.Generator().manual_seed(77)
    if name == "random":
        return points_of(enc, 1000, seed=5), torch.randn(1000, C, generator=g)
    if name == "one_cell":
        pts = one_cell_points(enc, 4096, seed=6)
        rows, _ = enc._corners(pts, enc.n_levels - 1, torch.float32)
        assert rows.unique().numel() == 8
        return pts, torch.randn(4096, C, generator=g)
    if name == "wide_range":        # magnitudes from 1e-8 to 1e4, both signs
        mag = 10.0 ** (torch.rand(1000, C, generator=g, dtype=F64) * 12.0 - 8.0)
        mag[0, 0], mag[1, 1] = 1e-8, 1e4
        sign = torch.where(torch.rand(1000, C, generator=g) < 0.5, -1.0, 1.0)
        return points_of(enc, 1000, seed=7), (mag * sign).float()
    raise KeyError(name)


@pytest.mark.parametrize("name", ["random", "one_cell", "wide_range"])
def test_backward_equals_the_fixed_point_rule_bit_for_bit_twice(npa, dev, enc, name):
    pts, d_out = backward_case(enc, name)
    want = enc.table_grad_reference(pts, d_out)
    assert float(want.abs().max()) > 0.0
    first = kernel_grad(npa, enc, pts.to(dev), d_out.to(dev))
    second = kernel_grad(npa, enc, pts.to(dev), d_out.to(dev))
    assert first.shape == want.shape and first.dtype == torch.float32
    assert torch.equal(first.cpu(), want) and torch.equal(second, first)
    # through autograd, with the module's own accumulator reused from call to call
    for _ in range(2):
        enc.embeddings.grad = None
        (enc(pts.to(dev)) * d_out.to(dev)).sum().backward()
        assert torch.equal(enc.embeddings.grad.cpu(), want)
    assert int(enc._scratch_on(dev)[:-1].abs().max()) == 0         # the accumulator is left zero for the next call
    enc.embeddings.grad = None


def test_backward_reads_a_column_range_and_splits_into_two_phases(npa, dev, enc):
    hb = npa.hip_backend
    pts, d_out = backward_case(enc, "random")
    C = enc.out_dim
    wide = torch.randn(1000, 5 + C + 2, generator=torch.Generator().manual_seed(9))
    wide[:, 5:5 + C] = d_out
    wide[0, 0] = 1e9            # a larger value outside the range must not move the maximum
    want = enc.table_grad_reference(pts, d_out)
    scratch = hb.hash_scratch(enc.desc(), dev)
    got = hb.hash_encode_bwd(enc.desc(), wide.to(dev), 5, points=pts.to(dev), scratch=scratch)
    assert torch.equal(got.cpu(), want) and int(scratch[:-1].abs().max()) == 0
    assert hb.hash_encode_bwd(enc.desc(), wide.to(dev), 5, points=pts.to(dev), scratch=scratch, phases=1) is None
    assert int(scratch[:-1].abs().max()) > 0
    got = hb.hash_encode_bwd(enc.desc(), wide.to(dev), 5, points=pts.to(dev), scratch=scratch, phases=2)
    assert torch.equal(got.cpu(), want) and int(scratch[:-1].abs().max()) == 0


@pytest.mark.parametrize("P", SIZES)
def test_backward_at_every_size(npa, dev, enc, P):
    pts = points_of(enc, P, seed=200 + P)
    d_out = torch.randn(P, enc.out_dim, generator=torch.Generator().manual_seed(P))
    got = kernel_grad(npa, enc, pts.to(dev), d_out.to(dev))
    assert got.shape == enc.embeddings.shape
    assert torch.equal(got.cpu(), enc.table_grad_reference(pts, d_out))


def test_zero_and_non_finite_upstream_gradients(npa, dev, enc):
    pts = points_of(enc, 65, seed=11).to(dev)
    C = enc.out_dim
    scratch = npa.hip_backend.hash_scratch(enc.desc(), dev)
    zero = kernel_grad(npa, enc, pts, torch.zeros(65, C, device=dev), scratch=scratch)
    assert int((zero != 0).sum()) == 0
    d = torch.randn(65, C, generator=torch.Generator().manual_seed(12)).to(dev)
    for bad in (float("nan"), float("inf"), -float("inf")):
        d_bad = d.clone()
        d_bad[40, 3] = bad
        got = kernel_grad(npa, enc, pts, d_bad, scratch=scratch)
        torch.cuda.synchronize()
        assert bool(torch.isnan(got).all())
    # and the accumulator is clean afterwards: the next call is the definition again
    assert torch.equal(kernel_grad(npa, enc, pts, d, scratch=scratch).cpu(), enc.table_grad_reference(pts.cpu(), d.cpu()))


def test_backward_error_against_float64_autograd(npa, dev, enc):
    pts, d_out = backward_case(enc, "random")
    E64 = enc.embeddings.detach().cpu().double().requires_grad_(True)
    (enc.encode_reference(pts, F64, E64) * d_out.double()).sum().backward()
    E32 = enc.embeddings.detach().cpu().clone().requires_grad_(True)
    (enc.encode_reference(pts, torch.float32, E32) * d_out).sum().backward()
    got = kernel_grad(npa, enc, pts.to(dev), d_out.to(dev)).cpu()
    own = float((E32.grad.double() - E64.grad).abs().max())
    err = float((got.double() - E64.grad).abs().max())
    print(f"F={enc.n_features}: kernel error {err:.3e}, float32 autograd's own {own:.3e}")
    assert own > 0.0 and err <= 4.0 * own
