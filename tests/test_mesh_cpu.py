"""CPU: triangle meshes without a GPU -- the definition (mesh.extract_mesh_reference: marching tetrahedra on the Kuhn subdivision) on
analytic shapes whose topology is known, the keep restriction, degenerate inputs, the input checks, write_ply, and the export of
nerf_iso_count / nerf_iso_emit with their refusals."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import nerf_pytorch_amd as npa

CPU = torch.device("cpu")
NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ shapes and measurements
def lattice(n, lo, hi):
    """float64 node positions [nx, ny, nz, 3] of the lattice (the fields are evaluated in double and rounded once)"""
    ax = [torch.linspace(lo[a], hi[a], n[a], dtype=torch.float64) for a in range(3)]
    return torch.stack(torch.meshgrid(*ax, indexing="ij"), -1)


def ball_field(p, r=0.8, c=(0.0, 0.0, 0.0)):
    return r - (p - torch.tensor(c, dtype=torch.float64)).norm(dim=-1)


def torus_field(p, R=0.65, a=0.25):
    return a - torch.sqrt((torch.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - R) ** 2 + p[..., 2] ** 2)


def two_balls_field(p):
    return torch.maximum(ball_field(p, 0.3, (-0.5, 0.0, 0.0)), ball_field(p, 0.3, (0.5, 0.0, 0.0)))


# name: (signed distance field, nodes, lo, hi, Euler characteristic)
SHAPES = {"ball": (ball_field, (9, 8, 11), (-1.0, -1.0, -1.2), (1.0, 1.1, 1.0), 2),
          "torus": (torus_field, (15, 14, 9), (-1.0, -1.0, -0.5), (1.0, 1.05, 0.5), 0),
          "two_balls": (two_balls_field, (13, 8, 8), (-1.0, -0.5, -0.5), (1.0, 0.5, 0.55), 4)}


def shape_volume(name):
    field, n, lo, hi, _ = SHAPES[name]
    return field(lattice(n, lo, hi)).to(torch.float32), lo, hi


def directed_edges(faces):
    """int64 [3 F] keys a * 2^32 + b of the directed edges (a, b) of the triangles"""
    f = faces.to(torch.int64)
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return (e[:, 0] << 32) | e[:, 1], (e[:, 1] << 32) | e[:, 0]


def boundary_edges(faces):
    """the directed edges (as vertex pairs [B, 2]) whose reverse does not occur; asserts no directed edge occurs twice"""
    fwd, rev = directed_edges(faces)
    assert torch.unique(fwd).numel() == fwd.numel(), "a directed edge occurs twice"
    lone = fwd[~torch.isin(fwd, rev)]
    return torch.stack([lone >> 32, lone & 0xffffffff], -1)


def signed_volume(vertices, faces):
    p = vertices.double()[faces.to(torch.int64)]
    return float((p[:, 0] * torch.cross(p[:, 1], p[:, 2], dim=-1)).sum() / 6.0)


def crossed_edges(volume, level):
    """[(class, lower node [E, 3])] of the lattice edges with exactly one endpoint inside, by class, independent of the module's tables"""
    inside = volume >= level
    nx, ny, nz = volume.shape
    out = []
    for dx, dy, dz in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)):
        f = inside[:nx - dx, :ny - dy, :nz - dz] != inside[dx:, dy:, dz:]
        out.append(((dx, dy, dz), torch.nonzero(f)))
    return out


def edges_in_id_order(volume, level):
    """(lower node int64 [E, 3], direction int64 [E, 3]) of the crossed edges in ascending 7 * node + class"""
    nx, ny, nz = volume.shape
    rows = []
    for c, (d, nodes) in enumerate(crossed_edges(volume, level)):
        ids = 7 * ((nodes[:, 0] * ny + nodes[:, 1]) * nz + nodes[:, 2]) + c
        rows.append(torch.cat([ids[:, None], nodes, torch.tensor(d).expand(nodes.shape[0], 3)], -1))
    rows = torch.cat(rows)
    rows = rows[torch.argsort(rows[:, 0])]
    return rows[:, 1:4], rows[:, 4:7]


# ------------------------------------------------------------------------------------------------ the tables
def test_the_case_table_winds_every_triangle_from_inside_to_outside():
    """ISO_TET_TRIS against integer arithmetic on the even tetrahedron (0,0,0) (1,0,0) (1,1,0) (1,1,1): every triangle uses crossing
    edges only, its normal points from the inside corners' centroid to the outside corners', and a quad's two triangles share q0 q2"""
    m = npa.mesh
    assert m.PERMS.tolist() == [[0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]]
    assert m.TET_ODD.tolist() == [False, True, True, False, False, True]
    assert m.CLASS_DIRS.tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1]]
    V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]])
    for t in range(6):      # the table's corners are the Kuhn corners, and the parity is the determinant's sign
        corners = np.array([[(q >> 2) & 1, (q >> 1) & 1, q & 1] for q in m.TET_CORNERS[t]])
        assert round(np.linalg.det((corners[1:] - corners[0]).astype(float))) == (-1 if m.TET_ODD[t] else 1)
    for mask in range(16):
        ins = [i for i in range(4) if mask >> i & 1]
        outs = [i for i in range(4) if not mask >> i & 1]
        n = int(m.TET_TRIS[mask, 0])
        assert n == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[len(ins)]
        tris = m.TET_TRIS[mask, 1:].reshape(2, 3)[:n]
        crossing = {e for e, (a, b) in enumerate(m.TET_EDGES.tolist()) if (a in ins) != (b in ins)}
        assert {int(e) for e in tris.reshape(-1)} == (crossing if n else set())
        for tri in tris:
            p = [V[m.TET_EDGES[e, 0]] + V[m.TET_EDGES[e, 1]] for e in tri]      # twice the edge midpoints
            normal = np.cross(p[1] - p[0], p[2] - p[0])
            assert normal.dot(sum(V[i] for i in outs) * len(ins) - sum(V[i] for i in ins) * len(outs)) > 0, (mask, tri)
        if n == 2:
            assert tris[0][0] == tris[1][0] and tris[0][2] == tris[1][1]


# ------------------------------------------------------------------------------------------------ analytic shapes
@pytest.mark.parametrize("name", list(SHAPES))
def test_analytic_shapes_are_closed_oriented_and_of_the_right_topology(name):
    field, n, lo, hi, euler = SHAPES[name]
    volume, lo, hi = shape_volume(name)
    v, f = npa.extract_mesh_reference(volume, 0.0, lo, hi)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.shape[1] == 3 and f.shape[1] == 3 and f.shape[0] > 0
    # closed and consistently oriented: every directed edge once, its reverse once
    assert boundary_edges(f).numel() == 0
    V, E, F = v.shape[0], 3 * f.shape[0] // 2, f.shape[0]
    assert V - E + F == euler
    nodes, dirs = edges_in_id_order(volume, 0.0)
    assert V == nodes.shape[0] and torch.unique(f).numel() == V and int(f.min()) == 0 and int(f.max()) == V - 1
    assert signed_volume(v, f) > 0
    # a vertex lies on an edge that crosses the surface: within one body diagonal of it (the fields are signed distances)
    step = (np.asarray(hi, dtype=np.float32) - np.asarray(lo, dtype=np.float32)) / (np.asarray(n, dtype=np.float32) - np.float32(1))
    assert float(field(v.double()).abs().max()) <= float(np.linalg.norm(step.astype(np.float64)))
    # ... and on that edge, by the definition's arithmetic in numpy fp32: 0 <= t <= 1 and p = p_a + t (p_b - p_a)
    vol = volume.numpy()
    a = vol[tuple(nodes.numpy().T)]
    b = vol[tuple((nodes + dirs).numpy().T)]
    t = (np.float32(0.0) - a) / (b - a)
    assert t.dtype == np.float32 and (t >= 0).all() and (t <= 1).all()
    lo32 = np.asarray(lo, dtype=np.float32)
    pa = lo32 + nodes.numpy().astype(np.float32) * step
    pb = lo32 + (nodes + dirs).numpy().astype(np.float32) * step
    want = pa + t[:, None] * (pb - pa)
    assert want.dtype == np.float32 and np.array_equal(want.view(np.int32), v.numpy().view(np.int32))


# ------------------------------------------------------------------------------------------------ keep
def test_keep_restricts_the_mesh_to_the_kept_cubes():
    volume, lo, hi = shape_volume("torus")
    nx, ny, nz = volume.shape
    v, f = npa.extract_mesh_reference(volume, 0.0, lo, hi)
    ones = torch.ones(nx - 1, ny - 1, nz - 1, dtype=torch.bool)
    for keep in (ones, npa.OccupancyGrid.from_mask(ones, lo, hi, device=CPU)):
        v1, f1 = npa.extract_mesh_reference(volume, 0.0, lo, hi, keep=keep)
        assert torch.equal(v1.view(torch.int32), v.view(torch.int32)) and torch.equal(f1, f)
    # the half space i < cut: exactly the faces of the kept cubes, in the same relative order
    cut = 6
    half = ones.clone()
    half[cut:] = False
    vh, fh = npa.extract_mesh_reference(volume, 0.0, lo, hi, keep=half)
    lo32 = np.asarray(lo, dtype=np.float32)
    step = (np.asarray(hi, dtype=np.float32) - lo32) / (np.asarray(volume.shape, dtype=np.float32) - np.float32(1))
    centroid_x = v.double()[f.to(torch.int64)][:, :, 0].mean(-1)          # a triangle lies inside its cube (no node is at the level here)
    assert not bool((volume == 0).any())
    in_kept = torch.floor((centroid_x - float(lo32[0])) / float(step[0])) < cut
    assert 0 < int(in_kept.sum()) < f.shape[0]
    assert torch.equal(vh[fh.to(torch.int64)].view(torch.int32), v[f[in_kept].to(torch.int64)].view(torch.int32))
    assert torch.unique(fh).numel() == vh.shape[0]            # no unreferenced vertex
    # boundary edges only on the cut: both ends in the plane x = lo + cut * step (an edge inside the plane has p_x = p_a,x exactly)
    lone = boundary_edges(fh)
    plane = np.float32(lo32[0] + np.float32(cut) * step[0])
    assert lone.shape[0] > 0 and bool((vh[lone.reshape(-1), 0] == float(plane)).all())
    # nothing kept: nothing emitted
    for keep in (torch.zeros_like(ones), npa.OccupancyGrid.from_mask(torch.zeros_like(ones), lo, hi, device=CPU)):
        v0, f0 = npa.extract_mesh_reference(volume, 0.0, lo, hi, keep=keep)
        assert tuple(v0.shape) == (0, 3) and tuple(f0.shape) == (0, 3) and v0.dtype == torch.float32 and f0.dtype == torch.int32


# ------------------------------------------------------------------------------------------------ degenerate inputs
def degenerate_volumes():
    """{name: (volume, level, lo, hi)}: nodes exactly at the level (an octahedron of integers); a ball with NaN, +inf and -inf nodes"""
    i = torch.arange(7, dtype=torch.float32) - 3
    octa = 2 - (i[:, None, None].abs() + i[None, :, None].abs() + i[None, None, :].abs())
    ball, lo, hi = shape_volume("ball")
    ball = ball.clone()
    ball[4, 4, 5] = NAN             # deep inside: a cavity
    ball[4, 3, 5] = INF             # inside stays inside
    ball[0, 0, 0] = -INF            # outside stays outside
    ball[3, 4, 8] = INF             # next to the surface
    ball[5, 3, 2] = -INF
    return {"at_level": (octa, 0.0, (-3.0, -3.0, -3.0), (3.0, 3.0, 3.0)), "non_finite": (ball, 0.0, lo, hi)}


def test_degenerate_inputs():
    vols = degenerate_volumes()
    volume, level, lo, hi = vols["at_level"]
    assert int((volume == level).sum()) == 18
    v, f = npa.extract_mesh_reference(volume, level, lo, hi)
    assert boundary_edges(f).numel() == 0 and signed_volume(v, f) > 0 and v.shape[0] - 3 * f.shape[0] // 2 + f.shape[0] == 2
    p = v.double()[f.to(torch.int64)]
    area = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=-1).norm(dim=-1)
    assert 0 < int((area == 0).sum()) < f.shape[0]          # zero-area triangles are kept
    volume, level, lo, hi = vols["non_finite"]
    v, f = npa.extract_mesh_reference(volume, level, lo, hi)
    assert bool(torch.isfinite(v).all()) and boundary_edges(f).numel() == 0 and f.shape[0] > 0
    assert v.shape[0] == sum(nodes.shape[0] for _, nodes in crossed_edges(volume, level))
    # a constant volume, and one of NaNs: nothing
    for fill in (1.0, -1.0, NAN):
        v, f = npa.extract_mesh_reference(torch.full((3, 4, 5), fill), 0.0, (0, 0, 0), (1, 1, 1))
        assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)
    # the smallest lattice: one corner inside cuts all seven edges at it, one triangle per tetrahedron
    for corner in ((0, 0, 0), (1, 1, 1)):
        cube = torch.full((2, 2, 2), -1.0)
        cube[corner] = 1.0
        v, f = npa.extract_mesh_reference(cube, 0.0, (0, 0, 0), (1, 2, 3))
        assert tuple(v.shape) == (7, 3) and tuple(f.shape) == (6, 3)
        p = v.double()[f.to(torch.int64)]
        normals = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=-1)
        away = p.mean(1) - torch.tensor(corner, dtype=torch.float64) * torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
        assert bool(((normals * away).sum(-1) > 0).all())
    cube = torch.tensor([1.0, -1.0]).expand(2, 2, 2).contiguous()        # inside below the plane z = 1.5
    v, f = npa.extract_mesh_reference(cube, 0.0, (0, 0, 0), (1, 2, 3))
    assert tuple(v.shape) == (9, 3) and tuple(f.shape) == (8, 3) and bool((v[:, 2] == 1.5).all())
    p = v.double()[f.to(torch.int64)]
    normals = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=-1)
    assert bool((normals[:, 2] > 0).all()) and abs(float(normals[:, 2].sum()) / 2 - 2.0) < 1e-12        # the 1 x 2 sheet, covered once


def test_input_checks():
    vol = torch.zeros(3, 3, 3)
    ok = dict(level=0.0, lo=(0, 0, 0), hi=(1, 1, 1))
    for fn in (npa.extract_mesh_reference, npa.extract_mesh):
        for bad in (torch.zeros(3, 3), torch.zeros(3, 3, 3, 1), torch.zeros(3, 3, 3, dtype=torch.int32), [[[0.0]]]):
            with pytest.raises(ValueError, match="volume"):
                fn(bad, **ok)
        for shape in ((1, 3, 3), (3, 1, 3), (3, 3, 1)):
            with pytest.raises(ValueError, match="at least 2"):
                fn(torch.zeros(shape), **ok)
        with pytest.raises(ValueError, match="2\\^31"):         # 7 * 675^3 > 2^31 (an expanded view: no memory behind it)
            fn(torch.zeros(1, 1, 1).expand(675, 675, 675), **ok)
        for lo, hi in (((0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, 1, 1)), ((0, 0, NAN), (1, 1, 1)), ((0, 0, 0), (1, INF, 1))):
            with pytest.raises(ValueError, match="lo and hi"):
                fn(vol, 0.0, lo, hi)
        for level in (NAN, INF, -INF, 1e39):
            with pytest.raises(ValueError, match="level"):
                fn(vol, level, (0, 0, 0), (1, 1, 1))
        for keep in (torch.ones(3, 3, 3, dtype=torch.bool), torch.ones(2, 2, 2), npa.OccupancyGrid((0, 0, 0), (1, 1, 1), 3, device=CPU)):
            with pytest.raises(ValueError, match="keep"):
                fn(vol, keep=keep, **ok)


def test_the_kernel_form_needs_the_gpu():
    volume, lo, hi = shape_volume("ball")
    with pytest.raises(npa.hip_backend.NerfHipError, match="GPU.*extract_mesh_reference"):
        npa.extract_mesh(volume, 0.0, lo, hi)
    grid = npa.DensityGrid((-1, -1, -1), (1, 1, 1), 4, device=CPU)
    with pytest.raises(npa.hip_backend.NerfHipError, match="GPU"):
        grid.extract_mesh()
    for fn, args in ((npa.density_volume, ((-1, -1, -1), (1, 1, 1), 4)), (npa.mesh_from_network, ((-1, -1, -1), (1, 1, 1), 4, 0.5))):
        with pytest.raises(NotImplementedError, match="fused-kernel NeRF"):
            fn(torch.nn.Linear(3, 4), *args)


# ------------------------------------------------------------------------------------------------ write_ply
def read_ply(path):
    with open(path, "rb") as f:
        data = f.read()
    head, payload = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    counts, props, element = {}, {}, None
    for line in lines[2:]:
        w = line.split()
        if w and w[0] == "element":
            element = w[1]
            counts[element], props[element] = int(w[2]), []
        elif w and w[0] == "property":
            props[element].append(" ".join(w[1:]))
    kinds = {"float": "<f4", "uchar": "u1"}
    vdt = np.dtype([(p.split()[1], kinds[p.split()[0]]) for p in props["vertex"]])
    assert props["face"] == ["list uchar int vertex_indices"]
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    nv = counts["vertex"] * vdt.itemsize
    assert len(payload) == nv + counts["face"] * fdt.itemsize
    return np.frombuffer(payload[:nv], dtype=vdt), np.frombuffer(payload[nv:], dtype=fdt)


def test_write_ply_round_trip(tmp_path):
    volume, lo, hi = shape_volume("ball")
    v, f = npa.extract_mesh_reference(volume, 0.0, lo, hi)
    g = torch.Generator().manual_seed(3)
    normals = torch.nn.functional.normalize(torch.randn(v.shape[0], 3, generator=g), dim=-1)
    colors = torch.rand(v.shape[0], 3, generator=g) * 1.2 - 0.1        # some outside [0, 1]: to8b clips
    path = str(tmp_path / "a.ply")
    npa.write_ply(path, v, f, normals, colors)
    vert, face = read_ply(path)
    assert vert.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], -1), v.numpy())
    assert np.array_equal(np.stack([vert["nx"], vert["ny"], vert["nz"]], -1), normals.numpy())
    assert np.array_equal(np.stack([vert["red"], vert["green"], vert["blue"]], -1), npa.to8b(colors.numpy()))
    assert bool((face["n"] == 3).all()) and np.array_equal(face["v"], f.numpy())
    npa.write_ply(path, v, f)
    vert, face = read_ply(path)
    assert vert.dtype.names == ("x", "y", "z") and np.array_equal(face["v"], f.numpy()) and vert.shape[0] == v.shape[0]
    npa.write_ply(path, v, f, colors=colors)
    assert read_ply(path)[0].dtype.names == ("x", "y", "z", "red", "green", "blue")
    npa.write_ply(path, v[:0], f[:0])
    vert, face = read_ply(path)
    assert vert.shape[0] == 0 and face.shape[0] == 0
    with pytest.raises(ValueError):
        npa.write_ply(path, v, f, normals[:-1])


# ------------------------------------------------------------------------------------------------ exports
def test_the_library_exports_and_binds_the_entry_points():
    hb = npa.hip_backend
    raw = ctypes.CDLL(npa.build.LIB_PATH)
    with open(os.path.join(ROOT, "include", "nerf_hip.h")) as f:
        header = f.read()
    for name, proto in (("nerf_iso_scratch_words", "size_t nerf_iso_scratch_words(int nx, int ny, int nz);"),
                        ("nerf_iso_count", "int nerf_iso_count(const float* volume, int nx, int ny, int nz, float level,"),
                        ("nerf_iso_emit", "int nerf_iso_emit(const float* volume, int nx, int ny, int nz, float level, const float lo[3], const float step[3],")):
        assert hasattr(raw, name) and name in hb.EXPORTS and proto in header, name
    assert "#define NERF_ABI_VERSION 10" in header and hb.ABI_VERSION == 10
    assert "isosurface.hip" in npa.build.SOURCES
    for name in ("extract_mesh", "extract_mesh_reference", "density_volume", "mesh_from_network", "write_ply"):
        assert name in npa.__all__ and callable(getattr(npa, name)), name
    assert list(inspect.signature(npa.extract_mesh).parameters) == ["volume", "level", "lo", "hi", "keep"]
    assert list(inspect.signature(npa.extract_mesh_reference).parameters) == ["volume", "level", "lo", "hi", "keep"]
    assert list(inspect.signature(npa.density_volume).parameters) == ["model", "lo", "hi", "resolution", "viewdir"]
    assert list(inspect.signature(npa.mesh_from_network).parameters) == ["model", "lo", "hi", "resolution", "level", "occupancy", "normals", "colors"]
    assert list(inspect.signature(npa.write_ply).parameters) == ["path", "vertices", "faces", "normals", "colors"]
    assert list(inspect.signature(npa.DensityGrid.extract_mesh).parameters) == ["self", "level"]
    assert list(inspect.signature(hb.iso_count).parameters) == ["volume", "level", "keep_words"]
    assert list(inspect.signature(hb.iso_emit).parameters) == ["volume", "level", "lo", "step", "keep_words", "scratch", "n_vertices", "n_faces"]
    L = hb.lib()
    assert L.nerf_abi_version() == 10
    # the scratch: 7 ints per node, one per 1024 edges, one per 256 cubes; 0 for a lattice the entry points refuse
    assert L.nerf_iso_scratch_words(41, 33, 29) == 7 * 39237 + (7 * 39237 + 1023) // 1024 + (40 * 32 * 28 + 255) // 256
    assert L.nerf_iso_scratch_words(2, 2, 2) == 56 + 1 + 1
    for bad in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (-2, 4, 4), (675, 675, 675), (2, 2, 1 << 30), (2 ** 31 - 1,) * 3, (46341, 46341, 2)):
        assert L.nerf_iso_scratch_words(*bad) == 0, bad
    # refused before anything is launched or read (host memory stands in for the device buffers)
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    vec = (ctypes.c_float * 3)(0.0, 0.0, 0.0)

    def count(n=(3, 3, 3), level=0.0, **null):
        a = dict(volume=ptr, keep=ptr, scratch=ptr, counts=ptr)
        a.update(null)
        return L.nerf_iso_count(a["volume"], *n, level, a["keep"], a["scratch"], a["counts"], None)

    def emit(n=(3, 3, 3), level=0.0, **null):
        a = dict(volume=ptr, lo=vec, step=vec, keep=ptr, scratch=ptr, vertices=ptr, faces=ptr)
        a.update(null)
        return L.nerf_iso_emit(a["volume"], *n, level, a["lo"], a["step"], a["keep"], a["scratch"], a["vertices"], a["faces"], None)
    for call, names in ((count, ("volume", "scratch", "counts")), (emit, ("volume", "lo", "step", "scratch", "vertices", "faces"))):
        for keep in (ptr, None):
            for name in names:
                assert call(keep=keep, **{name: None}) != 0 and "null" in L.nerf_last_error().decode(), name
            for n in ((1, 3, 3), (3, 1, 3), (3, 3, 1), (0, 3, 3), (3, -1, 3)):
                assert call(keep=keep, n=n) != 0 and "at least 2 nodes" in L.nerf_last_error().decode(), n
            for n in ((675, 675, 675), (2, 2, 1 << 29), (2 ** 31 - 1,) * 3):        # (the last: a product that leaves 64 bits)
                assert call(keep=keep, n=n) != 0 and "2^31" in L.nerf_last_error().decode(), n
            for level in (NAN, INF, -INF):
                assert call(keep=keep, level=level) != 0 and "level" in L.nerf_last_error().decode(), level
