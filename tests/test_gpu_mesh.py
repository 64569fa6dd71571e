"""GPU tests (-m gpu) of triangle meshes: nerf_iso_count / nerf_iso_emit against the definition (mesh.extract_mesh_reference) evaluated
on the CPU, bit for bit, on analytic shapes, noise, restricted noise, a lattice whose scans carry, degenerate values and an empty mesh;
then the wiring -- density_volume, mesh_from_network against the same chain written out from the public pieces, and
DensityGrid.extract_mesh."""
import numpy as np
import pytest
import torch

import nerf_pytorch_amd as npa_
from test_gpu_occupancy import BOX_HI, BOX_LO, BOX_R, bits_equal
from test_gpu_occupancy_train import positive_median_density
from test_gpu_parity import dev, nets, npa  # noqa: F401  (fixtures)
from test_mesh_cpu import SHAPES, boundary_edges, degenerate_volumes, shape_volume

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")
LO, HI = (-1.5, -1.0, -2.0), (1.5, 1.0, 2.0)
NOISE_N = (37, 21, 63)          # 48,951 nodes: 342,657 edge items = 334 blocks and 641 items; 44,640 cubes = 174 blocks and 96 cubes
RAGGED_N = (38, 21, 63)         # 45,880 cubes: the last keep word holds 24 of them
# Both scans walk their block counts in pieces of 1024 with a carry.  An edge block takes 1024 items of 7 per node, so the edge scan
# carries above 1024 * 1024 / 7 = 149,797 nodes; a cube block takes 256 cubes, so the cube scan carries above 1024 * 256 = 262,144
# cubes.  67 x 66 x 65 nodes = 287,430 nodes (1,965 edge blocks) and 66 * 65 * 64 = 274,560 cubes (1,073 cube blocks): two pieces each.
CARRY_N = (67, 66, 65)


def noise(n, seed):
    return torch.rand(n, generator=torch.Generator().manual_seed(seed))


def gyroid(n):
    ax = [torch.linspace(0.0, 4.0 * np.pi, m, dtype=torch.float64) for m in n]
    x, y, z = torch.meshgrid(*ax, indexing="ij")
    return (torch.sin(x) * torch.cos(y) + torch.sin(y) * torch.cos(z) + torch.sin(z) * torch.cos(x)).to(torch.float32)


def cases():
    """{name: (volume, level, lo, hi, keep)} on the CPU"""
    out = {name: shape_volume(name)[:1] + (0.0,) + shape_volume(name)[1:] + (None,) for name in SHAPES}
    out["noise"] = (noise(NOISE_N, 41), 0.5, LO, HI, None)
    cubes = tuple(m - 1 for m in NOISE_N)
    out["noise_keep"] = (noise(NOISE_N, 41), 0.5, LO, HI, noise(cubes, 42) < 0.5)
    cubes = tuple(m - 1 for m in RAGGED_N)
    out["noise_keep_ragged"] = (noise(RAGGED_N, 43), 0.5, LO, HI, noise(cubes, 44) < 0.5)
    out["carry"] = (gyroid(CARRY_N) + 0.2 * (noise(CARRY_N, 45) - 0.5), 0.1, LO, HI, None)
    for name, (volume, level, lo, hi) in degenerate_volumes().items():
        out[name] = (volume, level, lo, hi, None)
    return out


@pytest.fixture(scope="module")
def reference():
    """the definition on the CPU, computed once per case: {name: (volume, level, lo, hi, keep, vertices, faces)}"""
    return {name: case + npa_.extract_mesh_reference(*case) for name, case in cases().items()}


@pytest.mark.parametrize("name", list(SHAPES) + ["noise", "noise_keep", "noise_keep_ragged", "carry", "at_level", "non_finite"])
def test_the_kernels_equal_the_definition_bit_for_bit(npa, dev, reference, name):
    """torch.equal on the faces, bits_equal on the vertices.  "noise_keep" is the restricted noise volume on 37 x 21 x 63 nodes; its
    44,640 cubes fill the last keep word, so "noise_keep_ragged" (38 x 21 x 63 nodes, 24 cubes in the last word) stands beside it."""
    volume, level, lo, hi, keep, v_ref, f_ref = reference[name]
    nodes = volume.numel()
    print(f"\n{name}: {tuple(volume.shape)} nodes, V {v_ref.shape[0]}, F {f_ref.shape[0]}")
    assert f_ref.shape[0] > 0 and int(f_ref.max()) == v_ref.shape[0] - 1
    if name == "noise":         # nearly every edge crosses: about half of the 7 per node
        assert v_ref.shape[0] > 3 * nodes
    if name == "noise_keep_ragged":
        assert keep.numel() % 32 == 24 and bool(keep.reshape(-1)[-24:].any())
    if name == "carry":         # vertices in both pieces of the edge scan, triangles in both pieces of the cube scan
        assert 7 * nodes > 1024 * 1024 and keep is None and (CARRY_N[0] - 1) * (CARRY_N[1] - 1) * (CARRY_N[2] - 1) > 1024 * 256
        x = (v_ref[:, 0] - LO[0]) / (HI[0] - LO[0]) * (CARRY_N[0] - 1)
        assert int((x < 30).sum()) > 1000 and int((x > 64).sum()) > 1000
    kw = {} if keep is None else dict(keep=keep)
    v, f = npa.extract_mesh(volume.to(dev), level, lo, hi, **kw)
    assert v.is_cuda and f.is_cuda and v.dtype == torch.float32 and f.dtype == torch.int32
    assert torch.equal(f.cpu(), f_ref), int((f.cpu() != f_ref).sum()) if f.shape == f_ref.shape else (f.shape, f_ref.shape)
    assert bits_equal(v.cpu(), v_ref)
    if keep is not None:        # the same restriction as a grid of one cell per cube
        grid = npa.OccupancyGrid.from_mask(keep, lo, hi, device=dev)
        v2, f2 = npa.extract_mesh(volume.to(dev), level, lo, hi, keep=grid)
        assert torch.equal(f2, f) and bits_equal(v2, v)
    if name in ("at_level", "non_finite"):
        assert bool(torch.isfinite(v).all()) and boundary_edges(f.cpu()).numel() == 0


def test_an_empty_mesh_launches_no_emit_pass(npa, dev):
    hb = npa.hip_backend
    ball, lo, hi = shape_volume("ball")

    def traced(volume, **kw):
        timer, hb.TIMER = hb.TIMER, hb.KernelTimer()
        try:
            v, f = npa.extract_mesh(volume.to(dev), 0.0, lo, hi, **kw)
            names = {k: d["launches"] for k, d in hb.TIMER.summary().items()}
        finally:
            hb.TIMER = timer
        return v, f, names
    v, f, names = traced(ball)
    assert f.shape[0] > 0 and sorted(names) == ["iso_count (edges + scan + cubes + scan)", "iso_emit (vertices + faces)"] and set(names.values()) == {1}
    cubes = tuple(m - 1 for m in ball.shape)
    for volume, kw in ((torch.full((9, 8, 11), -1.0), {}), (torch.full((9, 8, 11), float("nan")), {}),
                       (ball, dict(keep=torch.zeros(cubes, dtype=torch.bool)))):
        v, f, names = traced(volume, **kw)
        assert names == {"iso_count (edges + scan + cubes + scan)": 1}, names
        assert v.is_cuda and f.is_cuda and tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int32


def test_density_volume_is_query_points_at_the_nodes(npa, dev, nets):
    """a lattice of 104 x 101 x 100 = 1,050,400 nodes, 1,824 more than one slice: against query_points at lo + (i, j, k) * step written out
    here, cut where density_volume cuts"""
    nf = nets[1]
    n = (104, 101, 100)
    assert npa.occupancy._SLICE_CELLS < n[0] * n[1] * n[2] < 2 * npa.occupancy._SLICE_CELLS
    got = npa.density_volume(nf, BOX_LO, BOX_HI, n)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == n
    lo = torch.tensor(np.asarray(BOX_LO, dtype=np.float32), device=dev)
    step = torch.tensor((np.asarray(BOX_HI, dtype=np.float32) - np.asarray(BOX_LO, dtype=np.float32)) / (np.asarray(n, dtype=np.float32) - np.float32(1)),
                        device=dev)
    idx = torch.stack(torch.meshgrid(*[torch.arange(m, device=dev) for m in n], indexing="ij"), -1).reshape(-1, 3).to(torch.float32)
    pts = lo + idx * step
    assert bool((pts[-1] == torch.tensor(BOX_HI, device=dev)).all())
    vd = torch.tensor([0.0, 0.0, 1.0], device=dev)
    cut = npa.occupancy._SLICE_CELLS
    with torch.no_grad():
        want = torch.cat([npa.query_points(nf, p, vd.expand(p.shape[0], 3))[:, 3] for p in (pts[:cut], pts[cut:])])
    assert bits_equal(got.reshape(-1), want) and float(got.max()) > 0
    # another view direction, an int resolution
    small = npa.density_volume(nf, BOX_LO, BOX_HI, 9, viewdir=(1.0, 0.0, 0.0))
    assert tuple(small.shape) == (9, 9, 9)


def chain_by_hand(npa, model, lo, hi, n, level, keep=None):
    """mesh_from_network written out from the public pieces"""
    volume = npa.density_volume(model, lo, hi, n)
    v, f = npa.extract_mesh(volume, level, lo, hi, keep=keep)
    vd = torch.tensor([0.0, 0.0, 1.0], device=v.device).expand(v.shape[0], 3)
    pts = v.clone().requires_grad_(True)
    (grad,) = torch.autograd.grad(npa.query_points(model, pts, vd)[:, 3].sum(), pts)
    norm = grad.norm(dim=-1, keepdim=True)
    normals = torch.where(torch.isfinite(norm) & (norm > 0), -grad / norm, torch.zeros_like(grad))
    with torch.no_grad():
        colors = torch.sigmoid(npa.query_points(model, v, -normals)[:, :3])
    return {"vertices": v, "faces": f, "normals": normals, "colors": colors}


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_mesh_from_network_is_the_chain_of_its_public_pieces(npa, dev, nets, precision):
    nf = nets[1]
    n = (33, 29, 31)
    prev = npa.get_precision()
    npa.set_precision(precision)
    try:
        volume = npa.density_volume(nf, BOX_LO, BOX_HI, n)
        level = float(volume[volume > 0].median())
        got = npa.mesh_from_network(nf, BOX_LO, BOX_HI, n, level)
        want = chain_by_hand(npa, nf, BOX_LO, BOX_HI, n, level)
        V, F = got["vertices"].shape[0], got["faces"].shape[0]
        print(f"\n{precision}: level {level:.4g}, V {V}, F {F}")
        assert F > 0 and V > 0
        assert list(got) == ["vertices", "faces", "normals", "colors"] and torch.equal(got["faces"], want["faces"])
        assert all(bits_equal(got[k], want[k]) for k in ("vertices", "normals", "colors"))
        length = got["normals"].norm(dim=-1)
        zero = (got["normals"] == 0).all(-1)
        assert bool((zero | ((length - 1).abs() < 1e-5)).all()) and int(zero.sum()) < V
        assert bool(((got["colors"] >= 0) & (got["colors"] <= 1)).all()) and tuple(got["colors"].shape) == (V, 3)
        assert all(p.grad is None for p in nf.parameters())
        # the keys on request
        assert list(npa.mesh_from_network(nf, BOX_LO, BOX_HI, n, level, normals=False, colors=False)) == ["vertices", "faces"]
        only_colors = npa.mesh_from_network(nf, BOX_LO, BOX_HI, n, level, normals=False)
        assert list(only_colors) == ["vertices", "faces", "colors"] and bits_equal(only_colors["colors"], got["colors"])
        # inside a ball of occupied cubes: a subset of the unrestricted faces (by position: the indices differ)
        cubes = tuple(m - 1 for m in n)
        centre = [torch.linspace(BOX_LO[a], BOX_HI[a], n[a], dtype=torch.float64)[:-1] + (BOX_HI[a] - BOX_LO[a]) / (2 * cubes[a]) for a in range(3)]
        ball = (centre[0][:, None, None] ** 2 + centre[1][None, :, None] ** 2 + centre[2][None, None, :] ** 2) < 1.2 ** 2
        grid = npa.OccupancyGrid.from_mask(ball, BOX_LO, BOX_HI, device=dev)
        part = npa.mesh_from_network(nf, BOX_LO, BOX_HI, n, level, occupancy=grid)
        by_hand = chain_by_hand(npa, nf, BOX_LO, BOX_HI, n, level, keep=grid)
        assert torch.equal(part["faces"], by_hand["faces"]) and all(bits_equal(part[k], by_hand[k]) for k in ("vertices", "normals", "colors"))
        rows = lambda m: {r.tobytes() for r in m["vertices"][m["faces"].to(torch.int64)].reshape(-1, 9).cpu().numpy()}
        assert 0 < part["faces"].shape[0] < F and rows(part) <= rows(got)
    finally:
        npa.set_precision(prev)


def test_density_grid_extract_mesh_is_the_mesh_of_its_own_density(npa, dev, nets):
    nf = nets[1]
    thr = positive_median_density(npa, nf, dev, BOX_R)
    g = npa.DensityGrid(BOX_LO, BOX_HI, BOX_R, device=dev, sigma_threshold=thr, dilate=1).update(nf)
    state = g.state_dict()
    bits = g.bits.clone()
    v, f = g.extract_mesh()
    half = np.float32(0.5) * g.width
    v2, f2 = npa.extract_mesh(g.density.view(g.resolution), g.sigma_threshold, g.lo + half, g.hi - half)
    assert f.shape[0] > 0 and torch.equal(f, f2) and bits_equal(v, v2)
    v3, f3 = g.extract_mesh(level=2.0 * thr)
    v4, f4 = npa.extract_mesh(g.density.view(g.resolution), 2.0 * thr, g.lo + half, g.hi - half)
    assert torch.equal(f3, f4) and bits_equal(v3, v4) and not (f3.shape == f.shape and torch.equal(f3, f))
    after = g.state_dict()
    assert torch.equal(g.bits, bits) and list(after) == list(state)
    assert all(torch.equal(after[k], state[k]) if isinstance(state[k], torch.Tensor) else after[k] == state[k] for k in state)
