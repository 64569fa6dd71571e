"""Triangle meshes of a density volume: what the network (or a DensityGrid) learnt, as a surface another program can open.

``extract_mesh_reference`` is the definition -- marching tetrahedra on the Kuhn subdivision of a lattice, in vectorised torch on any
device -- and ``extract_mesh`` the same mesh, bit for bit, from csrc/isosurface.hip (include/nerf_hip.h, "isosurface").  The tables of
the subdivision live in csrc/iso_tables.h; the kernels compile that file and this module parses it, so there is one copy.
``density_volume`` samples a fused NeRF at the nodes of a lattice, ``mesh_from_network`` chains the two and adds normals (the input
gradient of the density) and colours, ``write_ply`` stores the result.  World space only.
"""
import os
import re

import numpy as np
import torch

from . import hip_backend as hb
from .occupancy import _SLICE_CELLS, OccupancyGrid, _pack_bits

_FLT_MAX = float(np.finfo(np.float32).max)
_TABLES_H = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "iso_tables.h")


def _read_tables(path=_TABLES_H):
    """{name: int64 array} of the `constexpr int NAME[..]... = {...};` tables of csrc/iso_tables.h"""
    with open(path) as f:
        text = re.sub(r"//[^\n]*", "", f.read())
    out = {}
    for name, dims, body in re.findall(r"constexpr int (\w+)((?:\[\d+\])+) = (\{.*?\});", text, re.S):
        out[name] = np.array([int(v) for v in re.findall(r"-?\d+", body)], dtype=np.int64).reshape([int(v) for v in re.findall(r"\d+", dims)])
    return out


_T = _read_tables()
PERMS, CLASS_DIRS, TET_EDGES, TET_TRIS = _T["ISO_PERMS"], _T["ISO_CLASS_DIRS"], _T["ISO_TET_EDGES"], _T["ISO_TET_TRIS"]
# a cube corner is the code q = 4 dx + 2 dy + dz; the corners of tetrahedron t are 0, e_a, e_a + e_b, 7 for its permutation (a, b, c)
TET_CORNERS = np.array([[0, 4 >> p[0], (4 >> p[0]) | (4 >> p[1]), 7] for p in PERMS], dtype=np.int64)
TET_ODD = np.array([sum(p[a] > p[b] for a in range(3) for b in range(a + 1, 3)) & 1 for p in PERMS], dtype=bool)
_CLASS_OF_CODE = np.full(8, -1, dtype=np.int64)
_CLASS_OF_CODE[CLASS_DIRS @ np.array([4, 2, 1])] = np.arange(7)
# edge e of tetrahedron t: the code of its lower corner and its class
_TE_CODE = TET_CORNERS[:, TET_EDGES[:, 0]]
_TE_CLASS = _CLASS_OF_CODE[TET_CORNERS[:, TET_EDGES[:, 0]] ^ TET_CORNERS[:, TET_EDGES[:, 1]]]


def _lattice(who, volume, level, lo, hi):
    """the checked inputs every form shares: (volume fp32 contiguous, level as an fp32-exact float, lo fp32 [3], step fp32 [3])"""
    if not isinstance(volume, torch.Tensor) or volume.dim() != 3 or not volume.is_floating_point():
        raise ValueError(f"{who}: volume must be a floating-point tensor [nx, ny, nz]")
    n = tuple(int(v) for v in volume.shape)
    lo32, step32 = _lattice_step(who, lo, hi, n)
    with np.errstate(over="ignore"):
        level32 = np.float32(level)
    if isinstance(level, bool) or not np.isfinite(level32):         # (also refuses a NaN and what overflows fp32)
        raise ValueError(f"{who}: level must be a finite number, got {level!r}")
    return volume.detach().to(torch.float32).contiguous(), float(level32), lo32, step32


def _lattice_step(who, lo, hi, n):
    """(lo fp32 [3], step fp32 [3]) of a lattice of n = (nx, ny, nz) nodes from lo to hi: step = (hi - lo) / (n - 1), once, in fp32"""
    if len(n) != 3 or any(v < 2 for v in n):
        raise ValueError(f"{who}: a lattice has at least 2 nodes per axis, got {tuple(n)}")
    nodes, cubes = n[0] * n[1] * n[2], (n[0] - 1) * (n[1] - 1) * (n[2] - 1)
    if 7 * nodes >= 1 << 31 or 12 * cubes >= 1 << 31:
        raise ValueError(f"{who}: 7 * nodes and 12 * cubes must stay below 2^31 (edge ids, vertex and triangle counts are 32-bit), got {tuple(n)}")
    as3 = lambda v: np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float32)
    lo32, hi32 = as3(lo), as3(hi)
    if lo32.shape != (3,) or hi32.shape != (3,) or not (np.isfinite(lo32).all() and np.isfinite(hi32).all()):
        raise ValueError(f"{who}: lo and hi must be three finite numbers each")
    return lo32, (hi32 - lo32) / (np.asarray(n, dtype=np.float32) - np.float32(1.0))


def _keep_of(who, keep, n, device, as_words):
    """keep (an OccupancyGrid of resolution n - 1, bool [n - 1], or None) on `device`: the bit words, or the bool mask [nx-1, ny-1, nz-1]"""
    if keep is None:
        return None
    cubes = (n[0] - 1, n[1] - 1, n[2] - 1)
    if isinstance(keep, OccupancyGrid):
        if keep.resolution != cubes:
            raise ValueError(f"{who}: keep must have one cell per cube, resolution {cubes}, got {keep.resolution}")
        return keep.bits.to(device).contiguous() if as_words else keep.to_mask().to(device)
    keep = torch.as_tensor(keep)
    if keep.dtype != torch.bool or tuple(keep.shape) != cubes:
        raise ValueError(f"{who}: keep must be an OccupancyGrid or bool {cubes}, got {keep.dtype} {tuple(keep.shape)}")
    return _pack_bits(keep.to(device).reshape(-1)) if as_words else keep.to(device)


def extract_mesh_reference(volume, level, lo, hi, keep=None):
    """The triangle mesh of `volume` at `level`: (vertices fp32 [V, 3], faces int32 [F, 3]) on volume's device.  Plain torch; this is the
    definition the kernels reproduce bit for bit.

    volume [nx, ny, nz] holds values at the nodes of a lattice, node (i, j, k) at lo + (i, j, k) * step, step = (hi - lo) / (n - 1) per
    axis computed once in fp32.  n >= 2 per axis, 7 nx ny nz < 2^31 (and 12 cubes < 2^31).  A node is inside iff value >= level; a NaN is
    outside.  Where a value is interpolated it is first made finite: NaN -> -FLT_MAX, +-inf -> +-FLT_MAX.

    Marching tetrahedra on the Kuhn subdivision: cube (i, j, k) is cut into six tetrahedra, one per permutation (a, b, c) of the axes in
    the order of ISO_PERMS (csrc/iso_tables.h), with corners v0 = (0, 0, 0), v1 = e_a, v2 = e_a + e_b, v3 = (1, 1, 1).  Neighbouring cubes
    share their face diagonals, so there are no ambiguous cases: away from the lattice boundary (and from the boundary of `keep`) the
    surface is a closed, consistently oriented manifold.

    Vertices live on lattice edges.  An edge is 7 * node(lower endpoint) + class, the classes being the directions (1,0,0) (0,1,0)
    (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1); it carries a vertex iff exactly one endpoint is inside and a cube that contains it is
    emitted.  With a, b the values at the lower and upper endpoint: t = (level - a) / (b - a), p = p_a + t * (p_b - p_a) per component,
    fp32, multiply and add separate (a NaN t -- both differences overflowed -- counts as 1/2).  Vertices come in ascending edge id.

    A tetrahedron with 1 or 3 inside corners gives one triangle, with 2 a quad split (q0, q1, q2), (q0, q2, q3), from ISO_TET_TRIS; the
    normal (p1 - p0) x (p2 - p0) points from inside to outside (a solid has positive signed volume), decided by the case and the
    permutation's parity, never by floating point.  Faces come by cube index, then tetrahedron 0..5, then triangle 0..1.  Zero-area
    triangles, which arise where a node's value equals `level` (t = 0 on every edge at that node), are kept: dropping them would break
    the closedness of the index structure.

    keep: an OccupancyGrid of resolution (nx - 1, ny - 1, nz - 1) (its box is not looked at), bool [nx - 1, ny - 1, nz - 1], or None.  A
    cube whose bit is 0 emits nothing, and an edge is used only if one of the cubes sharing it (4 for an axis edge, 2 for a face
    diagonal, 1 for the body diagonal) is kept; without keep every crossed edge is used."""
    who = "extract_mesh_reference"
    vol, level, lo32, step32 = _lattice(who, volume, level, lo, hi)
    dev = vol.device
    nx, ny, nz = vol.shape
    keep_mask = _keep_of(who, keep, (nx, ny, nz), dev, as_words=False)
    ten = lambda a, dt=torch.int64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    lvl = torch.tensor(level, dtype=torch.float32, device=dev)
    inside = vol >= lvl
    fin = torch.nan_to_num(vol, nan=-_FLT_MAX, posinf=_FLT_MAX, neginf=-_FLT_MAX).reshape(-1)

    # ---- edges: flag [node, class]
    flags = torch.zeros((nx, ny, nz, 7), dtype=torch.bool, device=dev)
    if keep_mask is not None:       # cube (i, j, k) at [i + 1, j + 1, k + 1]; the rim stands for the cubes that do not exist
        padded = torch.zeros((nx + 1, ny + 1, nz + 1), dtype=torch.bool, device=dev)
        padded[1:nx, 1:ny, 1:nz] = keep_mask
    for c, (dx, dy, dz) in enumerate(CLASS_DIRS.tolist()):
        mx, my, mz = nx - dx, ny - dy, nz - dz          # the lower endpoints of this class
        f = inside[:mx, :my, :mz] != inside[dx:, dy:, dz:]
        if keep_mask is not None:
            used = torch.zeros_like(f)
            for sx in range(2 - dx):
                for sy in range(2 - dy):
                    for sz in range(2 - dz):            # the edge from node (i, j, k) lies in cube (i - sx, j - sy, k - sz)
                        used |= padded[1 - sx:1 - sx + mx, 1 - sy:1 - sy + my, 1 - sz:1 - sz + mz]
            f = f & used
        flags[:mx, :my, :mz, c] = f
    flat = flags.reshape(-1)
    prefix = torch.cumsum(flat, 0) - flat.to(torch.int64)           # the vertex index of a flagged edge
    ids = torch.nonzero(flat).reshape(-1)
    node, cls = ids // 7, ids % 7
    idx = torch.stack([node // (ny * nz), (node // nz) % ny, node % nz], -1)
    d = ten(CLASS_DIRS)[cls]
    a, b = fin[node], fin[node + (d[:, 0] * ny + d[:, 1]) * nz + d[:, 2]]
    t = (lvl - a) / (b - a)
    t = torch.where(torch.isnan(t), torch.full_like(t, 0.5), t)
    lo_t, step_t = ten(lo32, torch.float32), ten(step32, torch.float32)
    pa = lo_t + idx.to(torch.float32) * step_t
    pb = lo_t + (idx + d).to(torch.float32) * step_t
    vertices = pa + t[:, None] * (pb - pa)

    # ---- cubes: the inside mask of every tetrahedron
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    corner_in = torch.stack([inside[(q >> 2) & 1:((q >> 2) & 1) + cx, (q >> 1) & 1:((q >> 1) & 1) + cy, (q & 1):(q & 1) + cz].reshape(-1)
                             for q in range(8)], -1)
    mask = (corner_in[:, ten(TET_CORNERS)].to(torch.int32) << torch.arange(4, dtype=torch.int32, device=dev)).sum(-1)      # [cubes, 6]
    n_tri = ten(TET_TRIS[:, 0])[mask.to(torch.int64)]
    if keep_mask is not None:
        n_tri = n_tri * keep_mask.reshape(-1, 1)
    n_tri = n_tri.reshape(-1)
    sel = torch.nonzero(n_tri > 0).reshape(-1)           # (cube, tetrahedron) pairs that emit, in order
    cube, tet = sel // 6, sel % 6
    e = ten(TET_TRIS[:, 1:].reshape(16, 2, 3))[mask.reshape(-1)[sel].to(torch.int64)]     # [S, 2, 3] rows of ISO_TET_EDGES
    e = torch.where(ten(TET_ODD, torch.bool)[tet][:, None, None], e[:, :, [0, 2, 1]], e)
    tet3 = tet[:, None, None].expand_as(e)
    q, ecls = ten(_TE_CODE)[tet3, e], ten(_TE_CLASS)[tet3, e]
    node0 = ((cube // (cy * cz)) * ny + (cube // cz) % cy) * nz + cube % cz
    enode = node0[:, None, None] + (((q >> 2) & 1) * ny + ((q >> 1) & 1)) * nz + (q & 1)
    tri = prefix[7 * enode + ecls]
    valid = torch.arange(2, device=dev)[None, :] < n_tri[sel][:, None]
    faces = tri[valid].to(torch.int32)
    return vertices.reshape(-1, 3), faces.reshape(-1, 3)


def extract_mesh(volume, level, lo, hi, keep=None):
    """``extract_mesh_reference`` on the GPU (nerf_iso_count, one read-back of (V, F), nerf_iso_emit): the same vertices and faces, bit
    for bit.  An empty mesh returns after the count, without the emit launches."""
    who = "extract_mesh"
    vol, level, lo32, step32 = _lattice(who, volume, level, lo, hi)
    if not vol.is_cuda:
        # (the keep argument is still checked: a wrong call fails the same way on either device)
        _keep_of(who, keep, tuple(vol.shape), vol.device, as_words=False)
        raise hb.NerfHipError("extract_mesh: the kernels need the volume on the GPU (volume.to(device)); extract_mesh_reference is the "
                              "same mesh in plain torch on any device")
    words = _keep_of(who, keep, tuple(vol.shape), vol.device, as_words=True)
    with torch.no_grad():
        counts, scratch = hb.iso_count(vol, level, words)
        V, F = counts.tolist()          # the one read-back: it sizes the outputs
        if V == 0:
            return torch.empty((0, 3), dtype=torch.float32, device=vol.device), torch.empty((0, 3), dtype=torch.int32, device=vol.device)
        return hb.iso_emit(vol, level, lo32, step32, words, scratch, V, F)


def lattice_points(lo, hi, resolution, first, last, device):
    """fp32 [last - first, 3]: the nodes first <= n < last (n = (i ny + j) nz + k) of the lattice of `resolution` nodes from lo to hi,
    lo + (i, j, k) * step -- one multiplication, one addition --, the positions extract_mesh gives its nodes"""
    n = _res_nodes("lattice_points", resolution)
    lo32, step32 = _lattice_step("lattice_points", lo, hi, n)
    c = torch.arange(first, last, dtype=torch.int64, device=device)
    idx = torch.stack([c // (n[1] * n[2]), (c // n[2]) % n[1], c % n[2]], -1).to(torch.float32)
    return torch.as_tensor(lo32, device=device) + idx * torch.as_tensor(step32, device=device)


def _res_nodes(who, resolution):
    if isinstance(resolution, (bool, float)):
        raise ValueError(f"{who}: resolution must be an int or three ints, got {resolution!r}")
    n = (int(resolution),) * 3 if isinstance(resolution, (int, np.integer)) else tuple(int(v) for v in resolution)
    if len(n) != 3:
        raise ValueError(f"{who}: resolution must be an int or three ints, got {resolution!r}")
    return n


def density_volume(model, lo, hi, resolution, viewdir=(0.0, 0.0, 1.0)):
    """fp32 [nx, ny, nz] on the model's device: raw[:, 3] -- the density before the ReLU, what DensityGrid.update accumulates -- of a fused
    NeRF at the nodes of the lattice of `resolution` nodes (an int means cubic) from lo to hi, through query_points under no_grad in
    slices, with one fixed view direction (the density does not depend on it).  Fused NeRF modules and hashgrid.HashNeRF only."""
    from .field import NeRF
    from .hashgrid import HashNeRF
    from .render import query_points
    if not isinstance(model, (NeRF, HashNeRF)):
        raise NotImplementedError("density_volume: a fused-kernel NeRF module is required (not a DenseNeRF / other module)")
    n = _res_nodes("density_volume", resolution)
    _lattice_step("density_volume", lo, hi, n)
    dev = next(model.parameters()).device
    nodes = n[0] * n[1] * n[2]
    out = torch.empty(nodes, dtype=torch.float32, device=dev)
    vd = torch.tensor([float(v) for v in viewdir], dtype=torch.float32, device=dev)
    with torch.no_grad():
        for first in range(0, nodes, _SLICE_CELLS):
            last = min(first + _SLICE_CELLS, nodes)
            pts = lattice_points(lo, hi, n, first, last, dev)
            out[first:last] = query_points(model, pts, vd.expand(last - first, 3))[:, 3]
    return out.view(n)


def vertex_normals(model, points, viewdir=(0.0, 0.0, 1.0)):
    """fp32 [V, 3]: -grad / |grad| of query_points(model, points, viewdir)[:, 3] with respect to the points (autograd, the input-gradient
    kernel in point mode; for a hashgrid.HashNeRF, which must be built with point_grad=True, nerf_hash_input_grad): the density grows
    inwards, the normal points out.  A zero or non-finite gradient gives a zero normal."""
    from .render import query_points
    out = torch.zeros((points.shape[0], 3), dtype=torch.float32, device=points.device)
    vd = torch.tensor([float(v) for v in viewdir], dtype=torch.float32, device=points.device)
    for first in range(0, points.shape[0], _SLICE_CELLS):
        pts = points[first:first + _SLICE_CELLS].detach().to(torch.float32).clone().requires_grad_(True)
        with torch.enable_grad():
            sigma = query_points(model, pts, vd.expand(pts.shape[0], 3))[:, 3]
            (grad,) = torch.autograd.grad(sigma.sum(), pts)
        norm = grad.norm(dim=-1, keepdim=True)
        good = torch.isfinite(norm) & (norm > 0)
        out[first:first + _SLICE_CELLS] = torch.where(good, -grad / norm, torch.zeros_like(grad))
    return out


def vertex_colors(model, points, viewdirs):
    """fp32 [V, 3] in [0, 1]: sigmoid(raw[:, :3]) of the network at the points, each seen along its own view direction"""
    from .render import query_points
    out = torch.empty((points.shape[0], 3), dtype=torch.float32, device=points.device)
    with torch.no_grad():
        for first in range(0, points.shape[0], _SLICE_CELLS):
            sl = slice(first, first + _SLICE_CELLS)
            out[sl] = torch.sigmoid(query_points(model, points[sl].contiguous(), viewdirs[sl].contiguous())[:, :3])
    return out


def mesh_from_network(model, lo, hi, resolution, level, occupancy=None, normals=True, colors=True):
    """{"vertices" fp32 [V, 3], "faces" int32 [F, 3], "normals" fp32 [V, 3], "colors" fp32 [V, 3]} of a fused NeRF: ``density_volume`` on
    the lattice, ``extract_mesh`` at `level` with keep=occupancy (an OccupancyGrid of resolution - 1 cells -- from_views' hull for
    instance -- or None), ``vertex_normals`` at the vertices and ``vertex_colors`` seen along -normal (the direction a camera facing the
    surface looks in).  normals=False / colors=False leave the key out.  Exactly that chain of public pieces, nothing else."""
    volume = density_volume(model, lo, hi, resolution)
    vertices, faces = extract_mesh(volume, level, lo, hi, keep=occupancy)
    out = {"vertices": vertices, "faces": faces}
    if normals or colors:
        nrm = vertex_normals(model, vertices)
        if normals:
            out["normals"] = nrm
        if colors:
            out["colors"] = vertex_colors(model, vertices, -nrm)
    return out


def write_ply(path, vertices, faces, normals=None, colors=None):
    """Binary little-endian PLY: per vertex `float x y z`, then `float nx ny nz` with normals, then `uchar red green blue` with colors
    (floats in [0, 1] through to8b); per face `list uchar int vertex_indices`."""
    from .render import to8b
    arr = lambda t, dt: np.ascontiguousarray((t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(dt))
    v, f = arr(vertices, "<f4"), arr(faces, "<i4")
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("write_ply: vertices [V, 3] and faces [F, 3]")
    fields, props = [("xyz", "<f4", (3,))], ["float x", "float y", "float z"]
    cols = {"xyz": v}
    if normals is not None:
        fields.append(("n", "<f4", (3,)))
        props += ["float nx", "float ny", "float nz"]
        cols["n"] = arr(normals, "<f4")
    if colors is not None:
        fields.append(("rgb", "u1", (3,)))
        props += ["uchar red", "uchar green", "uchar blue"]
        cols["rgb"] = to8b(arr(colors, "<f4"))
    vert = np.empty(v.shape[0], dtype=np.dtype(fields))
    for name, col in cols.items():
        if col.shape != (v.shape[0], 3):
            raise ValueError("write_ply: normals and colors hold three values per vertex")
        vert[name] = col
    face = np.empty(f.shape[0], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    face["n"], face["v"] = 3, f
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"] + [f"property {p}" for p in props]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(vert.tobytes())
        out.write(face.tobytes())
