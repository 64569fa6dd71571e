"""GPU (-m gpu): nerf_hash_input_grad against its torch definitions.  Point mode bit for bit against
HashEncoding.point_grad_reference(float32) on CPU copies, twice, on the four-level fixture and on the edge configurations of
test_hash_edges_gpu.py -- lattice nodes, faces, lo, hi and points far outside included.  Ray mode: the per-ray fold in its written
order (lane j takes samples j, j + 64, .. ascending, then the xor butterfly 32, 16, .., 1) reproduced in torch, so columns 0:6 are held
bit for bit as well; the view columns' adjoint, whose sines and cosines come from another library, by the 4 x rule against float64."""
import pytest
import torch

from nerf_pytorch_amd.hashgrid import views_grad_reference
from test_gpu_parity import dev, npa  # noqa: F401  (fixtures)
from test_hash_cpu import FOUR, box_points, four_level
from test_hash_edges_cpu import CONFIGS, edge_points, encoding
from test_hash_gpu import SIZES, points_of

pytestmark = pytest.mark.gpu

F64 = torch.float64
CASES = [("FOUR", F) for F in (1, 2, 4)] + [(name, F) for name in ("ODD", "TINY", "ALL_DENSE_32", "MIXED_32", "DEFAULT", "FINE")
                                            for F in CONFIGS[name][3]]
RAY_COUNTS, SAMPLE_COUNTS = (1, 33), (1, 16, 64, 65, 130)       # one, two and three lane rounds, the last one partial


@pytest.fixture(scope="module")
def on_gpu(npa, dev):
    """(name, F) -> (the encoding on the CPU, its copy on the device), built once"""
    made = {}

    def get(name, F):
        if (name, F) not in made:
            cpu = four_level(F=F) if name == "FOUR" else encoding(name, F)
            gpu = npa.HashEncoding(cpu.lo, cpu.hi, n_features=F, **(FOUR if name == "FOUR" else CONFIGS[name][2]))
            gpu.load_state_dict(cpu.state_dict())
            made[name, F] = (cpu, gpu.to(dev))
        return made[name, F]
    return get


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def point_mode(npa, enc, pts, d_x, col=0):
    return npa.hip_backend.hash_input_grad(enc.desc(), enc.embeddings.detach(), d_x, col, pts, None, None, -1, -1)


# ------------------------------------------------------------------------------------------------ point mode
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("name,F", CASES)
def test_point_mode_equals_the_definition_bit_for_bit_twice(npa, dev, on_gpu, name, F, P):
    cpu, gpu = on_gpu(name, F)
    pts = points_of(cpu, P, seed=200 + P) if name == "FOUR" else edge_points(cpu, P, seed=200 + P)
    d_out = randn(P, cpu.out_dim, seed=300 + P)
    want = cpu.point_grad_reference(pts, d_out)
    first = point_mode(npa, gpu, pts.to(dev), d_out.to(dev))
    second = point_mode(npa, gpu, pts.to(dev), d_out.to(dev))
    assert first.shape == (P, 3) and first.dtype == torch.float32 and torch.equal(first, second)
    assert torch.equal(first.cpu(), want)
    if P >= 63:
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0.0
        # outside axes are exact zeros, and some are outside
        t = (pts - cpu._lo32) * cpu._inv32
        outside = (t < 0) | (t > 1)
        assert bool(outside.any()) and float(first.cpu()[outside].abs().max()) == 0.0


def test_point_mode_reads_a_column_range_of_a_wider_matrix_and_autograd_reaches_the_points(npa, dev, on_gpu):
    cpu, gpu = on_gpu("ODD", 2)
    P, C = 257, cpu.out_dim
    pts = edge_points(cpu, P, seed=77)
    wide = randn(P, 3 + C + 4, seed=78)
    want = cpu.point_grad_reference(pts, wide[:, 3:3 + C])
    assert torch.equal(point_mode(npa, gpu, pts.to(dev), wide.to(dev), col=3).cpu(), want)
    # HashEncoding(point_grad=True).forward: d loss / d points is the kernel's, the table's gradient is what it is without the flag
    flagged = npa.HashEncoding(cpu.lo, cpu.hi, n_features=2, point_grad=True, **CONFIGS["ODD"][2])
    flagged.load_state_dict(cpu.state_dict())
    flagged = flagged.to(dev)
    up = wide[:, 3:3 + C].contiguous().to(dev)
    x = pts.to(dev).requires_grad_(True)
    out = flagged(x)
    (out * up).sum().backward()
    assert torch.equal(x.grad.cpu(), want)
    (gpu(pts.to(dev)) * up).sum().backward()
    assert torch.equal(out.detach(), gpu(pts.to(dev)).detach()) and torch.equal(flagged.embeddings.grad, gpu.embeddings.grad)
    # a frozen table: only the points receive a gradient
    flagged.embeddings.grad = None
    flagged.embeddings.requires_grad_(False)
    x2 = pts.to(dev).requires_grad_(True)
    (flagged(x2) * up).sum().backward()
    assert torch.equal(x2.grad, x.grad) and flagged.embeddings.grad is None
    # without the flag the points are constants of the graph, as before
    x3 = pts.to(dev).requires_grad_(True)
    (gpu(x3) * up).sum().backward()
    assert x3.grad is None


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_a_non_finite_coordinate_leaves_every_other_row_unchanged(npa, dev, on_gpu, bad):
    cpu, gpu = on_gpu("FOUR", 2)
    pts = points_of(cpu, 200, seed=90)
    d_out = randn(200, cpu.out_dim, seed=91)
    clean = point_mode(npa, gpu, pts.to(dev), d_out.to(dev))
    for row, axis in ((0, 0), (70, 1), (199, 2)):
        dirty = pts.clone()
        dirty[row, axis] = bad
        got = point_mode(npa, gpu, dirty.to(dev), d_out.to(dev))
        keep = torch.arange(200) != row
        assert torch.equal(got.cpu()[keep], clean.cpu()[keep])
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ ray mode
def fold(values):
    """[N, S, C] -> [N, C] in the order of hash_fold_rays_kernel: lane j adds samples j, j + 64, .. in ascending order to 0, then the
    butterfly v = v + v[lane ^ d] for d = 32, 16, .., 1 (every lane ends with the same bits; lane 0's are returned)"""
    N, S, C = values.shape
    lanes = torch.zeros((N, 64, C), dtype=values.dtype)
    for first in range(0, S, 64):
        part = values[:, first:first + 64]
        lanes[:, :part.shape[1]] = lanes[:, :part.shape[1]] + part
    idx = torch.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ d]
    return lanes[:, 0]


def ray_case(cpu, N, S, seed):
    """rays whose sample points cover 1.1 x the box: origins in the box, short directions, depths in [0, 1]"""
    g = torch.Generator().manual_seed(seed)
    o = box_points(N, seed + 1, spread=0.9, lo=cpu.lo, hi=cpu.hi)
    d = torch.randn(N, 3, generator=g) * 0.4
    vd = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    rays = torch.cat([o, d, torch.zeros(N, 1), torch.ones(N, 1), vd], 1).contiguous()
    z = torch.rand(N, S, generator=g).sort(-1).values.contiguous()
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)      # (a separate multiply and add, as the kernel)
    return rays, z, pts


def ray_definition(cpu, rays, z, pts, d_x, views_col, mv, dtype):
    """[N, 11] in dtype: point_grad_reference at the fp32 sample points folded in the kernel's order, plus views_grad_reference on the
    folded view columns"""
    N, S = z.shape
    C = cpu.out_dim
    g = cpu.point_grad_reference(pts, d_x[:, :C], dtype).reshape(N, S, 3)
    out = torch.zeros((N, 11), dtype=dtype)
    out[:, 0:3] = fold(g)
    out[:, 3:6] = fold(z.to(dtype)[:, :, None] * g)
    if views_col >= 0:
        w = 3 + 6 * max(mv, 0)
        out[:, 8:11] = views_grad_reference(rays[:, 8:11], fold(d_x[:, views_col:views_col + w].to(dtype).reshape(N, S, w)), mv, dtype)
    return out


@pytest.mark.parametrize("S", SAMPLE_COUNTS)
@pytest.mark.parametrize("N", RAY_COUNTS)
def test_ray_mode_against_the_folded_definition(npa, dev, on_gpu, N, S):
    hb = npa.hip_backend
    cpu, gpu = on_gpu("FOUR", 2)
    C = cpu.out_dim
    rays, z, pts = ray_case(cpu, N, S, seed=1000 + 7 * N + S)
    # the float64 comparison stands on fp32 and float64 picking the same cells and the same outside axes at these points
    for l in range(cpu.n_levels):
        assert torch.equal(cpu._corners(pts, l, torch.float32)[0], cpu._corners(pts, l, F64)[0])
    t32, t64 = (pts - cpu._lo32) * cpu._inv32, (pts.double() - cpu._lo32.double()) * cpu._inv32.double()
    assert torch.equal((t32 < 0) | (t32 > 1), (t64 < 0) | (t64 > 1))
    d_x = randn(N * S, C + 27, seed=2000 + S)
    E = gpu.embeddings.detach()
    call = lambda vc, mv, acc=False: hb.hash_input_grad(gpu.desc(), E, d_x.to(dev), 0, None, rays.to(dev), z.to(dev), vc, mv, accumulate=acc)
    point_bits = hb.hash_input_grad(gpu.desc(), E, d_x.to(dev), 0, pts.to(dev), None, None, -1, -1).cpu()
    for vc, mv in ((-1, -1), (C, -1), (C, 4)):
        got = call(vc, mv)
        assert got.shape == (N, 11) and got.dtype == torch.float32 and torch.equal(got, call(vc, mv))       # two calls, equal bits
        got = got.cpu()
        want32 = ray_definition(cpu, rays, z, pts, d_x, vc, mv, torch.float32)
        want64 = ray_definition(cpu, rays, z, pts, d_x, vc, mv, F64)
        assert torch.equal(got[:, 0:6], want32[:, 0:6])                 # the fold has a written order: the same bits
        assert float(got[:, 6:8].abs().max()) == 0.0
        if S == 1:
            assert torch.equal(got[:, 0:3], point_bits)
        if vc < 0:
            assert float(got[:, 8:11].abs().max()) == 0.0
        elif mv < 0:
            assert torch.equal(got[:, 8:11], want32[:, 8:11])           # (no sine, no cosine: the same bits here too)
        # all columns within 4 x the float32 definition's own error of float64
        own = float((want32.double() - want64).abs().max())
        err = float((got.double() - want64).abs().max())
        print(f"N={N} S={S} views_col={vc} multires_views={mv}: kernel {err:.3e}, the float32 definition's own {own:.3e}")
        assert err <= 4.0 * own
        # accumulate: one fp32 addition per written column, columns 6:8 left alone
        start = randn(N, 11, seed=3000 + S)
        acc = call(vc, mv, start.clone().to(dev)).cpu()
        want_acc = start + got
        want_acc[:, 6:8] = start[:, 6:8]
        assert torch.equal(acc, want_acc)


def test_ray_mode_without_samples_or_rays_launches_nothing(npa, dev, on_gpu):
    hb = npa.hip_backend
    cpu, gpu = on_gpu("FOUR", 2)
    E = gpu.embeddings.detach()
    rays = torch.zeros(0, 11, device=dev)
    got = hb.hash_input_grad(gpu.desc(), E, torch.zeros(0, 35, device=dev), 0, None, rays, torch.zeros(0, 16, device=dev), 8, 4)
    assert got.shape == (0, 11)
    with pytest.raises(hb.NerfHipError):
        hb.hash_input_grad(gpu.desc(), E, torch.zeros(4, 35, device=dev), 0, torch.zeros(4, 3, device=dev), None, None, 8, 4)
    with pytest.raises(hb.NerfHipError):
        hb.hash_input_grad(gpu.desc(), E, torch.zeros(4, 35, device=dev), 0, None, torch.zeros(2, 8, device=dev), torch.zeros(2, 2, device=dev), 8, 4)
