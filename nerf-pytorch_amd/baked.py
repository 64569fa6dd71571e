"""Baked fields: a trained network written into a sparse grid of spherical-harmonic coefficients, and rendered without the network.

``render()`` evaluates the 8x256 network at every sample point it keeps.  A ``BakedField`` evaluates it once per lattice node of an
occupancy grid instead (PlenOctrees, Yu et al. 2021; SNeRG, Hedman et al. 2021): every node that touches an occupied cell stores the
density and the coefficients of the colour logits in the real spherical harmonics of degree <= 2, and a ray is rendered by marching
the grid in world-space steps, blending the eight nodes of each kept sample's cell and compositing on the spot (csrc/baked.hip,
nerf_baked_render).  ``BakedField.render_rays_reference`` is the definition the kernel is tested against; ``render_rays(...,
baked=field)`` and ``render_kwargs_test["baked"] = field`` are the ways in.  A ``BakedField`` itself has no gradients: it is an inference
artefact.  Its trainable twin is ``BakedTrainer`` (``field.trainable()``): an fp32 master copy of the table, the same render with a
deterministic backward to the table's rows (csrc/baked_train.hip: every contribution stored once and summed per row in a fixed order, no
atomics), so the table can be fitted to images through the renderer (PlenOctrees' fine-tuning, Plenoxels) and written back with
``to_field()``.  ``BakedTrainer.regularizers()`` adds what ties a node to its neighbours: the total variation of the density and of the
colour coefficients between stored nodes and Plenoxels' Cauchy sparsity of the density, on the fp32 master, with a gradient that is a
gather (csrc/baked_reg.hip); ``regularizer_reference`` is their definition.  ``BakedTrainer.render_rays(ray_grad=True)`` also hands the
gradient to the rays (csrc/baked_rays.hip; the depths are constants), and ``ray_records`` turns ``RayBatcher``'s batches into ray records
inside the graph: a camera pose is refined against a baked field through ``PoseRefinement``.
"""
import copy
import math

import numpy as np
import torch

from . import hip_backend as hb
from .occupancy import OccupancyGrid

_SH_C0 = 0.28209479177387814
_SH_C1 = 0.4886025119029199
_SH_C2 = (1.0925484305920792, 0.31539156525252005, 0.5462742152960396)
_ROUND = 64                 # candidates per round of the kernel's walk: the unit of the stop rule
_SLICE_NODES = 1 << 20      # lattice nodes whose positions from_network builds at a time


def _check_degree(sh_degree, who):
    if isinstance(sh_degree, (bool, np.bool_)) or not isinstance(sh_degree, (int, np.integer)) or int(sh_degree) not in (0, 1, 2):
        raise ValueError(f"{who}: sh_degree must be 0, 1 or 2, got {sh_degree!r}")
    return int(sh_degree)


def _check_stop_eps(stop_eps, who):
    real = not isinstance(stop_eps, (bool, np.bool_)) and isinstance(stop_eps, (int, float, np.integer, np.floating))
    if not real or not (0.0 <= float(stop_eps) < 1.0) or not (float(np.float32(stop_eps)) < 1.0):      # (also refuses NaN)
        raise ValueError(f"{who}: stop_eps must be a real number with 0 <= stop_eps < 1, got {stop_eps!r}")
    return float(stop_eps)


def _check_step(step_size, grid, who):
    """step_size as a float; None: half the smallest cell edge of the grid"""
    if step_size is None:
        return 0.5 * float(np.min(grid.width))
    real = not isinstance(step_size, (bool, np.bool_)) and isinstance(step_size, (int, float, np.integer, np.floating))
    if real:
        try:
            with np.errstate(all="ignore"):
                real = 0.0 < float(np.float32(step_size)) < float("inf")       # (the kernel's step is fp32(step_size); also refuses NaN)
        except OverflowError:
            real = False
    if not real:
        raise ValueError(f"{who}: step_size must be None or a finite real number > 0 (as an fp32 value), got {step_size!r}")
    return float(step_size)


def _check_max_steps(max_steps, who):
    if isinstance(max_steps, (bool, np.bool_)) or not isinstance(max_steps, (int, np.integer)) or not (1 <= int(max_steps) <= 1 << 24):
        raise ValueError(f"{who}: max_steps must be an int with 1 <= max_steps <= 2^24, got {max_steps!r}")
    return int(max_steps)


def sh_basis(dirs, degree):
    """[..., B], B = (degree + 1)^2: the real spherical harmonics of degree <= `degree` (0, 1 or 2) at the unit vectors dirs [..., 3], in
    the order and with the signs of PlenOctrees / svox, in dirs' dtype:
    Y0 = c0;  Y1 = -c1 y, Y2 = c1 z, Y3 = -c1 x;  Y4 = c2 xy, Y5 = -c2 yz, Y6 = c3 (2 z^2 - x^2 - y^2), Y7 = -c2 xz, Y8 = c4 (x^2 - y^2)."""
    degree = _check_degree(degree, "sh_basis")
    if dirs.shape[-1] != 3 or not dirs.is_floating_point():
        raise ValueError("sh_basis: dirs must be a floating-point tensor [..., 3]")
    x, y, z = dirs[..., 0], dirs[..., 1], dirs[..., 2]
    out = [torch.full_like(x, _SH_C0)]
    if degree >= 1:
        out += [-_SH_C1 * y, _SH_C1 * z, -_SH_C1 * x]
    if degree >= 2:
        xx, yy, zz = x * x, y * y, z * z
        out += [_SH_C2[0] * (x * y), -_SH_C2[0] * (y * z), _SH_C2[1] * (2.0 * zz - xx - yy), -_SH_C2[0] * (x * z), _SH_C2[2] * (xx - yy)]
    return torch.stack(out, -1)


def fibonacci_sphere(n, dtype=torch.float64, device=None):
    """[n, 3] unit vectors: z_i = 1 - (2 i + 1) / n, phi_i = i pi (3 - sqrt 5), computed in float64"""
    n = int(n)
    if n < 1:
        raise ValueError("fibonacci_sphere: n >= 1")
    i = torch.arange(n, dtype=torch.float64)
    z = 1.0 - (2.0 * i + 1.0) / n
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    s = torch.sqrt(torch.clamp(1.0 - z * z, min=0.0))
    return torch.stack([s * torch.cos(phi), s * torch.sin(phi), z], -1).to(dtype=dtype, device=device)


def _render_reference(who, grid, index, table, sh_degree, step_size, stop_eps, rays, u, white_bkgd, max_steps, dtype, values,
                      ray_grad=False, geometry=None):
    """BakedField.render_rays_reference's body (its docstring is the definition), shared with BakedTrainer.render_rays_reference: `values`
    [n_rows, >= 1 + 3B] stands in for the table where it is not None, and may require grad -- everything behind the gather is ordinary
    differentiable torch.  ray_grad=True: the definition of the gradient with respect to the rays (BakedField.render_rays_reference)"""
    max_steps = _check_max_steps(max_steps, who)
    if geometry is not None and not ray_grad:
        raise ValueError(f"{who}: geometry= belongs to ray_grad=True")
    if geometry is not None and (not isinstance(geometry, torch.Tensor) or geometry.shape != rays.shape):
        raise ValueError(f"{who}: geometry must be a tensor of rays' shape")
    geo = rays if geometry is None else geometry.to(rays.device)
    r, ok, uu, dn, M, _ = OccupancyGrid._march_rays(who, geo, u, max_steps, 1)
    if rays.shape[1] < 11:
        raise ValueError(f"{who}: rays [N, >= 11] (o, d, near, far, viewdir)")
    dev = rays.device
    N = r.shape[0]
    ds32 = torch.tensor(step_size, dtype=torch.float32, device=dev)
    dz = ds32 / dn
    ok = ok & (dz[:, 0] > 0) & torch.isfinite(dz[:, 0])
    out_rgb = torch.zeros((N, 3), dtype=dtype, device=dev)
    out_acc = torch.zeros(N, dtype=dtype, device=dev)
    out_depth = torch.zeros(N, dtype=dtype, device=dev)
    n_samples = torch.zeros(N, dtype=torch.int32, device=dev)
    stopped = torch.zeros(N, dtype=torch.bool, device=dev)
    if N > 0:
        z, valid = OccupancyGrid._world_steps(r, ok, uu, dz, M)
        K = z.shape[1]
        pts = r[:, None, 0:3] + r[:, None, 3:6] * z[:, :, None]
        f32 = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=dev)
        t = (pts - f32(grid.lo)) * f32(grid.scale)
        inside, _, bit = grid._classify(pts)
        keep = valid & inside & bit
        B = (sh_degree + 1) ** 2
        index = index.to(dev).to(torch.int64)
        table = table.to(dev)
        ny, nz = grid.resolution[1] + 1, grid.resolution[2] + 1
        rows, cols = keep.nonzero(as_tuple=True)
        tk = t[rows, cols]
        cell = torch.floor(tk)
        ci = cell.to(torch.int64)
        if ray_grad:
            # the kept samples' rows of the live rays, picked before anything is computed from them: a ray that keeps nothing (a NaN
            # among its components included) gets exact zeros
            live = rays[rows]
            x = live[:, 0:3].to(dtype) + live[:, 3:6].to(dtype) * z[rows, cols].to(dtype)[:, None]
            f = (x - f32(grid.lo).to(dtype)) * f32(grid.scale).to(dtype) - cell.to(dtype)
            Yk = sh_basis(live[:, 8:11].to(dtype), sh_degree)
        else:
            f = (tk - cell).to(dtype)
            Yk = sh_basis(rays.detach()[:, 8:11].to(torch.float32).to(dtype), sh_degree)[rows]       # [S, B]
        val = torch.zeros((rows.numel(), 1 + 3 * B), dtype=dtype, device=dev)
        for c in range(8):
            ox, oy, oz = (c >> 2) & 1, (c >> 1) & 1, c & 1
            node = ((ci[:, 0] + ox) * ny + (ci[:, 1] + oy)) * nz + (ci[:, 2] + oz)
            w = (f[:, 0] if ox else 1.0 - f[:, 0]) * (f[:, 1] if oy else 1.0 - f[:, 1]) * (f[:, 2] if oz else 1.0 - f[:, 2])
            corner = table[index[node]][:, :1 + 3 * B].to(dtype) if values is None else values[index[node]][:, :1 + 3 * B].to(dtype)
            val = val + w[:, None] * corner
        sigma = torch.clamp(val[:, 0], min=0.0)
        logits = torch.zeros((rows.numel(), 3), dtype=dtype, device=dev)
        for b in range(B):
            logits = logits + val[:, 1 + b:1 + 3 * B:B] * Yk[:, b:b + 1]
        rgb_k = torch.sigmoid(logits)
        alpha_k = 1.0 - torch.exp(-sigma * ds32.to(dtype))
        alpha = torch.zeros((N, K), dtype=dtype, device=dev)
        alpha[rows, cols] = alpha_k
        step_t = 1.0 - alpha + 1e-10
        step_t = torch.where(keep, step_t, torch.ones_like(step_t))
        incl = torch.cumprod(step_t, -1)
        T = torch.cat([torch.ones((N, 1), dtype=dtype, device=dev), incl[:, :-1]], -1)
        live = keep
        if stop_eps > 0.0:         # the rounds: T at the end of round j is incl[:, 64 j + 63] (or the last column)
            ends = torch.arange(_ROUND - 1, K + _ROUND - 1, _ROUND, device=dev).clamp(max=K - 1)
            kept_in = torch.stack([keep[:, e0:e0 + _ROUND].any(-1) for e0 in range(0, K, _ROUND)], -1)
            below = (incl[:, ends] < np.float32(stop_eps).item()) & kept_in        # (a round that keeps nothing changes nothing)
            stopped = below.any(-1)
            first = torch.where(stopped, below.to(torch.uint8).argmax(-1), torch.full((N,), ends.numel(), device=dev))
            live = keep & (torch.arange(K, device=dev)[None, :] < ((first + 1) * _ROUND)[:, None])
        w = torch.where(live, alpha * T, torch.zeros_like(T))
        rgb_full = torch.zeros((N, K, 3), dtype=dtype, device=dev)
        rgb_full[rows, cols] = rgb_k
        out_rgb = (w[:, :, None] * rgb_full).sum(1)
        out_acc = w.sum(-1)
        out_depth = (w * torch.where(live, z, torch.zeros_like(z)).to(dtype)).sum(-1)       # (a candidate that is not kept may lie at inf)
        n_samples = live.sum(-1).to(torch.int32)
    if white_bkgd:
        out_rgb = out_rgb + (1.0 - out_acc)[:, None]
    ratio = out_depth / out_acc
    disp = 1.0 / torch.max(torch.full_like(ratio, 1e-10), ratio)
    return {"rgb_map": out_rgb, "disp_map": disp, "acc_map": out_acc, "depth_map": out_depth, "n_samples": n_samples,
            "rays_stopped": int(stopped.sum())}


class BakedField:
    """Density and view-dependent colour on the lattice nodes of one OccupancyGrid (or DensityGrid) of resolution (Rx, Ry, Rz).

    Storage.  The (Rx + 1)(Ry + 1)(Rz + 1) nodes are numbered as ``mesh.lattice_points`` numbers them, n = (i (Ry + 1) + j)(Rz + 1) + k.
    ``index`` (int32, one entry per node) is the node's row in ``table``, or 0; ``table`` is fp16 [M + 1, W], row 0 all zeros, serving
    every node that is not stored.  A node is stored iff one of its up to eight adjacent cells is occupied, so every corner of an
    occupied cell has a row.  With B = (sh_degree + 1)^2 a row is [sigma, R_0 .. R_{B-1}, G_0 .., B_0 ..] zero-padded to W = 4 / 16 /
    32 halves (8 / 32 / 64 bytes) for sh_degree 0 / 1 / 2: sigma is the density after the ReLU, the rest the coefficients of the
    colour LOGITS raw[..., :3] in ``sh_basis``.  ``n_rows`` = M + 1.

    ``step_size`` is the length of a march step in the scene (None: half the smallest cell edge); ``stop_eps`` > 0 ends a ray behind
    the first round of 64 candidates at whose end its transmittance is below stop_eps (0: never).
    ``last_stats`` = {"rays", "samples", "rays_stopped"} of the last ``render_rays`` call (through render_rays(baked=) /
    batchify_rays / render: summed over the chunks).  The grid's bits decide which candidates are sampled: changing them after the
    field was built leaves cells whose corners have no row, which then read zeros."""

    def __init__(self, grid, index, table, sh_degree, step_size=None, stop_eps=0.0):
        if not isinstance(grid, OccupancyGrid):
            raise ValueError("BakedField: grid must be an occupancy.OccupancyGrid or DensityGrid")
        self.grid = grid
        self.sh_degree = _check_degree(sh_degree, "BakedField")
        self.step_size = _check_step(step_size, grid, "BakedField")
        self.stop_eps = _check_stop_eps(stop_eps, "BakedField")
        self._set_storage(index, table)
        self.last_stats = None

    # ------------------------------------------------------------------ plain properties
    @property
    def n_basis(self):
        return (self.sh_degree + 1) ** 2

    @property
    def n_rows(self):
        return int(self.table.shape[0])

    @property
    def device(self):
        return self.table.device

    @property
    def node_resolution(self):
        return tuple(r + 1 for r in self.grid.resolution)

    def to(self, device):
        self.grid.to(device)
        self.index = self.index.to(device)
        self.table = self.table.to(device)
        return self

    def _set_storage(self, index, table):
        nodes = int(np.prod(self.node_resolution))
        index = torch.as_tensor(index)
        table = torch.as_tensor(table)
        W = hb.BAKED_ROW_HALVES[self.sh_degree]
        if index.dtype != torch.int32 or index.numel() != nodes:
            raise ValueError(f"BakedField: index must be int32 with one entry per lattice node ({nodes}), got {index.dtype} {tuple(index.shape)}")
        if table.dtype != torch.float16 or table.dim() != 2 or table.shape[0] < 1 or table.shape[1] != W:
            raise ValueError(f"BakedField: table must be fp16 [rows >= 1, {W}] for sh_degree {self.sh_degree}, got {table.dtype} {tuple(table.shape)}")
        if index.numel() and (int(index.min()) < 0 or int(index.max()) >= table.shape[0]):
            raise ValueError("BakedField: index must hold rows of the table")
        dev = self.grid.device
        self.index = index.reshape(-1).to(dev).contiguous()
        self.table = table.to(dev).contiguous()

    # ------------------------------------------------------------------ building
    @staticmethod
    def stored_nodes(grid):
        """bool [Rx + 1, Ry + 1, Rz + 1] on the grid's device: the nodes with at least one occupied adjacent cell (eight shifted ORs of
        the grid's mask)"""
        mask = grid.to_mask()
        rx, ry, rz = grid.resolution
        stored = torch.zeros((rx + 1, ry + 1, rz + 1), dtype=torch.bool, device=mask.device)
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    stored[dx:dx + rx, dy:dy + ry, dz:dz + rz] |= mask
        return stored

    @classmethod
    def _pack(cls, grid, stored, rows, sh_degree, step_size, stop_eps):
        """the field of `rows` fp32 [M, 1 + 3B], the values of the stored nodes in node order"""
        W = hb.BAKED_ROW_HALVES[sh_degree]
        flat = stored.reshape(-1)
        rank = torch.cumsum(flat.to(torch.int64), 0)
        index = torch.where(flat, rank, torch.zeros_like(rank)).to(torch.int32)
        table = torch.zeros((rows.shape[0] + 1, W), dtype=torch.float16, device=rows.device)
        table[1:, :rows.shape[1]] = rows.to(torch.float16)
        return cls(grid, index, table, sh_degree, step_size, stop_eps)

    @classmethod
    def from_nodes(cls, grid, nodes, sh_degree, step_size=None, stop_eps=0.0):
        """The field of explicit node values: nodes fp32 [Rx + 1, Ry + 1, Rz + 1, 1 + 3B] -- sigma, then the R, G and B coefficients --
        of which the stored nodes' rows are packed and rounded to fp16 (plain torch on the grid's device); the others are dropped."""
        sh_degree = _check_degree(sh_degree, "BakedField.from_nodes")
        if not isinstance(grid, OccupancyGrid):
            raise ValueError("BakedField.from_nodes: grid must be an occupancy.OccupancyGrid or DensityGrid")
        V = 1 + 3 * (sh_degree + 1) ** 2
        nodes = torch.as_tensor(nodes)
        want = tuple(r + 1 for r in grid.resolution) + (V,)
        if tuple(nodes.shape) != want or not nodes.is_floating_point():
            raise ValueError(f"BakedField.from_nodes: nodes must be a floating-point tensor {want}, got {tuple(nodes.shape)}")
        stored = cls.stored_nodes(grid)
        rows = nodes.detach().to(device=stored.device, dtype=torch.float32)[stored]
        return cls._pack(grid, stored, rows, sh_degree, step_size, stop_eps)

    @staticmethod
    def sh_fit_matrix(n_dirs, sh_degree):
        """fp32 [B, n_dirs]: the pseudo-inverse of sh_basis(fibonacci_sphere(n_dirs), sh_degree), computed in float64 -- the least-squares
        fit of B coefficients to values at those directions.  n_dirs >= B."""
        sh_degree = _check_degree(sh_degree, "BakedField.sh_fit_matrix")
        B = (sh_degree + 1) ** 2
        if isinstance(n_dirs, (bool, np.bool_)) or not isinstance(n_dirs, (int, np.integer)) or int(n_dirs) < B:
            raise ValueError(f"BakedField.sh_fit_matrix: n_dirs must be an int >= {B} (the basis functions of degree {sh_degree}), got {n_dirs!r}")
        return torch.linalg.pinv(sh_basis(fibonacci_sphere(int(n_dirs)), sh_degree)).to(torch.float32)

    @classmethod
    def from_network(cls, model, grid, sh_degree=2, n_dirs=32, chunk=1 << 20, step_size=None, stop_eps=0.0):
        """The field of a trained network on `grid` (on the network's device).  For the stored nodes only: the positions are
        mesh.lattice_points'; the network is evaluated through query_points under no_grad at every node from the n_dirs directions of
        fibonacci_sphere, at most `chunk` (node, direction) pairs at a time; sigma is the mean over the directions of
        relu(raw[..., 3]) (the density does not depend on the direction: the mean keeps the definition symmetric) and the colour
        coefficients are sh_fit_matrix(n_dirs, sh_degree) @ raw[..., :3].  Both sums run over the directions left to right in fp32,
        one multiplication and one addition per term, so the table does not depend on `chunk`."""
        from .mesh import lattice_points
        from .render import query_points
        sh_degree = _check_degree(sh_degree, "BakedField.from_network")
        if not isinstance(grid, OccupancyGrid):
            raise ValueError("BakedField.from_network: grid must be an occupancy.OccupancyGrid or DensityGrid")
        step_size = _check_step(step_size, grid, "BakedField.from_network")
        stop_eps = _check_stop_eps(stop_eps, "BakedField.from_network")
        fit = cls.sh_fit_matrix(n_dirs, sh_degree)
        n_dirs = int(n_dirs)
        if isinstance(chunk, (bool, np.bool_)) or not isinstance(chunk, (int, np.integer)) or int(chunk) < n_dirs:
            raise ValueError(f"BakedField.from_network: chunk must be an int >= n_dirs ({n_dirs}), got {chunk!r}")
        dev = grid.device
        B = fit.shape[0]
        fit = fit.to(dev)
        dirs = fibonacci_sphere(n_dirs, torch.float32, dev)
        stored = cls.stored_nodes(grid)
        flat = stored.reshape(-1)
        res = tuple(r + 1 for r in grid.resolution)
        per = max(1, int(chunk) // n_dirs)
        rows = []
        with torch.no_grad():
            pts = [lattice_points(grid.lo, grid.hi, res, first, min(first + _SLICE_NODES, flat.numel()), dev)[flat[first:first + _SLICE_NODES]]
                   for first in range(0, flat.numel(), _SLICE_NODES)]
            pts = torch.cat(pts, 0)
            for first in range(0, pts.shape[0], per):
                p = pts[first:first + per]
                m = p.shape[0]
                raw = query_points(model, p[:, None, :].expand(m, n_dirs, 3).reshape(-1, 3),
                                   dirs[None, :, :].expand(m, n_dirs, 3).reshape(-1, 3)).view(m, n_dirs, 4)
                sigma = torch.zeros(m, dtype=torch.float32, device=dev)
                coef = torch.zeros((m, 3, B), dtype=torch.float32, device=dev)
                for i in range(n_dirs):
                    sigma = sigma + torch.relu(raw[:, i, 3])
                    coef = coef + raw[:, i, :3, None] * fit[None, None, :, i]
                rows.append(torch.cat([(sigma / n_dirs)[:, None], coef.reshape(m, 3 * B)], -1))
        rows = torch.cat(rows, 0) if rows else torch.zeros((0, 1 + 3 * B), dtype=torch.float32, device=dev)
        return cls._pack(grid, stored, rows, sh_degree, step_size, stop_eps)

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        return {"grid": self.grid.state_dict(), "index": self.index.detach().cpu().clone(), "table": self.table.detach().cpu().clone(),
                "sh_degree": self.sh_degree, "step_size": self.step_size, "stop_eps": self.stop_eps}

    def load_state_dict(self, state):
        """Takes the state of a field of the SAME sh_degree and grid resolution (the box, the bits and the values are the state's)"""
        if int(state["sh_degree"]) != self.sh_degree:
            raise ValueError(f"BakedField.load_state_dict: the state has sh_degree {int(state['sh_degree'])}, this field {self.sh_degree}")
        res = tuple(int(v) for v in state["grid"]["resolution"])
        if res != self.grid.resolution:
            raise ValueError(f"BakedField.load_state_dict: the state's grid is {res}, this field's {self.grid.resolution}")
        step_size = _check_step(state["step_size"], self.grid, "BakedField.load_state_dict")
        stop_eps = _check_stop_eps(state["stop_eps"], "BakedField.load_state_dict")
        self.grid.load_state_dict(state["grid"])
        self._set_storage(torch.as_tensor(state["index"]).to(torch.int32), torch.as_tensor(state["table"]).to(torch.float16))
        self.step_size, self.stop_eps = step_size, stop_eps
        return self

    # ------------------------------------------------------------------ the definition
    def render_rays_reference(self, rays, u=None, white_bkgd=False, max_steps=1 << 14, dtype=torch.float64, ray_grad=False, geometry=None):
        """The definition of the baked render, in plain torch on rays' device: rays [N, >= 11] (o, d, near, far, viewdir), u fp32 [N] in
        [0, 1) or None (0.5) -> {"rgb_map" [N, 3], "disp_map", "acc_map", "depth_map" [N] in `dtype`, "n_samples" int32 [N],
        "rays_stopped" int}.  Every discrete decision is the fp32 expression of the march references; the continuous arithmetic runs in
        `dtype`.

        Geometry, fp32 (OccupancyGrid._march_rays / _world_steps): dn = the correctly rounded root of dx dx + dy dy + dz dz added left
        to right; dz = fp32(step_size) / dn; a ray is invalid when one of its first eight components is not finite, when near >= far
        or when dz is not a finite number > 0.  Candidates k = 0 .. max_steps - 1 at z_k = near + (fp32(k) + u) * dz, valid_k = z_k <
        far, p = o + d * z_k (one multiplication, one addition per axis).
        Classification (OccupancyGrid._classify): t = (p - lo) * scale in fp32, inside iff 0 <= t < R on all axes, cell floor(t);
        keep_k = valid_k and inside and the cell's bit.  A point outside the box is never sampled, whatever grid.outside says.
        Sample value, in dtype from the fp32 t: f = t - floor(t) (exact); the eight corner rows blended with the weights (wx wy) wz,
        w = f or 1 - f, corners in the order 000 001 .. 111 (x the slowest bit); sigma = max(blend, 0); logits = sum_b coefficient_b
        Y_b(viewdir) added left to right, viewdir = columns 8:11 as given; rgb = sigmoid(logits).
        Compositing over the kept samples in order of k: alpha_k = 1 - exp(-sigma_k fp32(step_size)); T_k = the exclusive product of
        1 - alpha_j + 1e-10 over the kept j < k; w_k = alpha_k T_k; rgb_map = sum w rgb (+ 1 - acc with white_bkgd), acc_map = sum w,
        depth_map = sum w z_k, disp_map = 1 / max(1e-10, depth / acc) with the NaN of 0 / 0 kept.  An invalid ray and a ray that keeps
        nothing give the background, acc = depth = 0 and n_samples = 0.
        The stop (stop_eps > 0), in units of the kernel's rounds: the candidates are taken 64 at a time; behind the first round at
        whose end the running T -- the product over everything kept so far -- is below stop_eps no further round is walked.
        "rays_stopped" counts the rays with such a round (never one with stop_eps = 0); n_samples counts what was composited.

        ray_grad=True is the definition of the GRADIENT with respect to the rays (the forward values stay those above within rounding;
        with ray_grad=False the rays are detached and the function is what it always was, bit for bit).  The depths are constants,
        as everywhere in this project: validity, z_k, valid_k, keep_k and every kept sample's cell come from `geometry` (a tensor of
        rays' shape; None: rays.detach()) by the fp32 expressions above -- nothing discrete and no depth depends on the live rays.
        The fractional coordinates come from the live rays in dtype, f = ((o + d z_k - lo) scale) - cell with z_k, lo, scale and cell
        the fp32 values cast to dtype; f may fall a rounding error outside [0, 1], the blend is then an extrapolation of the same cell
        and is continuous.  Y = sh_basis(rays[:, 8:11]) comes from the live rays as the polynomial it is: normalising the view direction
        is the caller's torch op.  Everything behind that is unchanged.  Columns 6 and 7 (near, far), any column >= 11 and u get no
        gradient; depth_map uses the constant z_k.  `geometry` exists for finite differences: without it a moved d would move z."""
        return _render_reference("BakedField.render_rays_reference", self.grid, self.index, self.table, self.sh_degree, self.step_size,
                                 self.stop_eps, rays, u, white_bkgd, max_steps, dtype, None, ray_grad, geometry)

    # ------------------------------------------------------------------ the kernel
    def render_rays(self, rays, u=None, white_bkgd=False, max_steps=1 << 14):
        """{"rgb_map" fp32 [N, 3], "disp_map", "acc_map", "depth_map" fp32 [N]} of rays [N, >= 11] on the GPU (nerf_baked_render):
        ``render_rays_reference`` within fp32 rounding, its kept samples exactly.  Runs under no_grad; the results are detached.  Sets
        ``last_stats`` = {"rays", "samples", "rays_stopped"}."""
        max_steps = _check_max_steps(max_steps, "BakedField.render_rays")
        if rays.dim() != 2 or rays.shape[1] < 11:
            raise ValueError("BakedField.render_rays: rays [N, >= 11] (o, d, near, far, viewdir)")
        with torch.no_grad():
            rays = rays.detach().to(torch.float32).contiguous()
            u = None if u is None else u.detach().to(device=rays.device, dtype=torch.float32).contiguous()
            rgb, disp, acc, depth, n_samples, stopped = hb.baked_render(self.grid._desc(), self.index, self.table, self.sh_degree, rays, u,
                                                                        self.step_size, max_steps, self.stop_eps, white_bkgd)
            n = rays.shape[0]
            self.last_stats = {"rays": n, "samples": int(n_samples.sum()) if n else 0, "rays_stopped": int(stopped.sum()) if n else 0}
        return {"rgb_map": rgb, "disp_map": disp, "acc_map": acc, "depth_map": depth}

    def trainable(self):
        """the trainable twin of this field: ``BakedTrainer(self)``"""
        return BakedTrainer(self)


# ---------------------------------------------------------------------------------------------------- fine-tuning
def inverted_index(cells, n_cells):
    """(order int32 [S], cell_start int32 [n_cells + 1]) of the cell numbers `cells` (int32 [S], one per sample record): ``order`` lists the
    samples sorted by cell with a STABLE sort -- records come ray-major and sample-minor, so the samples of a cell stand in ascending
    (ray, k) --, and the samples of cell c are order[cell_start[c] : cell_start[c + 1]].  Plain torch on cells' device: this is the
    inverted index nerf_baked_train_bwd_rows sums through, and its order is the order of that sum."""
    cells = cells.reshape(-1)
    sorted_cells, order = torch.sort(cells, stable=True)
    bounds = torch.arange(int(n_cells) + 1, dtype=sorted_cells.dtype, device=cells.device)
    cell_start = torch.searchsorted(sorted_cells, bounds)
    return order.to(torch.int32), cell_start.to(torch.int32)


def ray_records(batch_rays, near, far):
    """[N, 11] ray records (o, d, near, far, viewdir = d / |d|) of batch_rays [2, N, 3] -- origins and directions as ``RayBatcher.next``
    returns them -- in plain differentiable torch: the glue between ``PoseRefinement`` / ``RayBatcher`` and
    ``BakedTrainer.render_rays(ray_grad=True)``.  near and far are numbers; the normalisation of the view direction is part of the
    graph, so d receives the gradient of viewdir as well.

        rays, target = batcher.next(refine(poses)); out = trainer.render_rays(ray_records(rays, 2.0, 6.0), ray_grad=True)"""
    if not isinstance(batch_rays, torch.Tensor) or batch_rays.dim() != 3 or batch_rays.shape[0] != 2 or batch_rays.shape[2] != 3:
        raise ValueError("ray_records: batch_rays [2, N, 3] (origins, directions)")
    o, d = batch_rays[0], batch_rays[1]
    view = d / torch.norm(d, dim=-1, keepdim=True)
    return torch.cat([o, d, torch.full_like(o[:, :1], float(near)), torch.full_like(o[:, :1], float(far)), view], -1)


class _BakedRender(torch.autograd.Function):
    """rgb_map, acc_map, depth_map of the trainer's fp16 table with the gradient handed to ``values`` (straight-through) and, where `live`
    -- the caller's rays as they were given, or None -- is a tensor, to the rays: count, forward and, in backward, the sample pass once,
    then for ``values`` the inverted index and the row pass and for the rays the ray pass, each only where ctx.needs_input_grad asks"""

    @staticmethod
    def forward(ctx, values, live, trainer, rays, u, white_bkgd, max_steps):
        desc = trainer.grid._desc()
        counts = hb.baked_count(desc, rays, u, trainer.step_size, max_steps)
        offsets = torch.zeros(rays.shape[0] + 1, dtype=torch.int64, device=rays.device)
        offsets[1:] = torch.cumsum(counts, 0)
        total = int(offsets[-1])
        if total > hb.BAKED_MAX_SAMPLES:
            raise ValueError(f"BakedTrainer.render_rays: {total} samples in one call, at most 2^30 (render fewer rays at a time)")
        offsets = offsets.to(torch.int32)
        rgb, acc, depth, records = hb.baked_train_fwd(desc, trainer.index, trainer.table, trainer.sh_degree, rays, u, trainer.step_size,
                                                      max_steps, white_bkgd, offsets, total)
        trainer.last_stats = {"rays": int(rays.shape[0]), "samples": total}
        ctx.trainer, ctx.rays, ctx.white_bkgd, ctx.total = trainer, rays, bool(white_bkgd), total
        ctx.live = None if live is None else (live.shape, live.dtype, live.device)
        ctx.save_for_backward(records, offsets)
        return rgb, acc, depth

    @staticmethod
    def backward(ctx, g_rgb, g_acc, g_depth):
        records, offsets = ctx.saved_tensors
        trainer, total = ctx.trainer, ctx.total
        f32 = lambda g: g.detach().to(torch.float32).contiguous()
        grads = hb.baked_train_bwd_samples(records, offsets, total, trainer.step_size, ctx.white_bkgd, f32(g_rgb), f32(g_acc), f32(g_depth))
        grad = d_live = None
        if ctx.needs_input_grad[0]:
            if total > 0:
                order, cell_start = inverted_index(records[:total, 0].view(torch.int32), trainer.grid.n_cells)
            else:
                order = torch.zeros(1, dtype=torch.int32, device=records.device)
                cell_start = torch.zeros(trainer.grid.n_cells + 1, dtype=torch.int32, device=records.device)
            grad = hb.baked_train_bwd_rows(trainer.grid._desc(), trainer.row_node, trainer.sh_degree, ctx.rays, records, grads, order,
                                           cell_start, total)
        if ctx.needs_input_grad[1]:
            shape, dtype, device = ctx.live
            d_rays = hb.baked_train_bwd_rays(trainer.grid._desc(), trainer.index, trainer.table, trainer.sh_degree, ctx.rays, records, grads,
                                             offsets, total)
            d_live = torch.zeros(shape, dtype=torch.float32, device=d_rays.device)      # (the columns behind the record get none)
            d_live[:, :11] = d_rays
            d_live = d_live.to(device=device, dtype=dtype)
        return grad, d_live, None, None, None, None, None


def _check_eps(eps, who):
    real = not isinstance(eps, (bool, np.bool_)) and isinstance(eps, (int, float, np.integer, np.floating))
    if real:
        with np.errstate(all="ignore"):
            real = 0.0 < float(np.float32(eps)) < float("inf")         # (the kernels' eps is fp32(eps); also refuses NaN)
    if not real:
        raise ValueError(f"{who}: eps must be a finite real number > 0 (as an fp32 value), got {eps!r}")
    return float(eps)


def regularizer_reference(values, index, node_resolution, sh_degree, axis_scale, eps=1e-9, dtype=torch.float64):
    """The definition of the table's regularisers, in plain torch on values' device, differentiable in `values` by ordinary autograd ->
    {"tv_sigma", "tv_sh", "sparsity"}, 0-d tensors in `dtype`.

    values [n_rows, >= 1 + 3B] are the rows of a table (column 0 the density before the ReLU, columns 1 .. 3B the colour coefficients, B =
    (sh_degree + 1)^2; row 0 and further columns take no part); index (one entry per node of the (Nx, Ny, Nz) = node_resolution lattice,
    n = (i Ny + j) Nz + k) is a node's row, or 0: the node is not stored.  With s = axis_scale, three floats (BakedTrainer passes
    min(cell edge) / (cell edge along the axis)), and n + e_a the next node along axis a:
        D_a[n][c] = s_a (v[n + e_a][c] - v[n][c])   where n + e_a lies in the lattice and is stored, else 0
        t[n][c]   = sqrt(D_x^2 + D_y^2 + D_z^2 + eps)
        tv_sigma  = 1 / M       sum over the stored n of t[n][0]
        tv_sh     = 1 / (3B M)  sum over the stored n and c = 1 .. 3B of t[n][c]
        sparsity  = 1 / M       sum over the stored n of log1p(2 max(v[n][0], 0)^2)          (Plenoxels' Cauchy prior)
    M = n_rows - 1 is the number of stored nodes; with M = 0 all three are 0.  A difference to a missing neighbour is left out, not
    taken against zero: every corner of an occupied cell has a row, the render never reads a missing node, and pulling the hull towards
    0 would be wrong."""
    who = "regularizer_reference"
    sh_degree = _check_degree(sh_degree, who)
    eps = _check_eps(eps, who)
    nx, ny, nz = (int(r) for r in node_resolution)
    V = 1 + 3 * (sh_degree + 1) ** 2
    index = torch.as_tensor(index).reshape(-1).to(device=values.device, dtype=torch.int64)
    if values.dim() != 2 or values.shape[0] < 1 or values.shape[1] < V or index.numel() != nx * ny * nz:
        raise ValueError(f"{who}: values [n_rows >= 1, >= {V}] and one index entry per lattice node ({nx * ny * nz})")
    scale = [float(s) for s in axis_scale]
    if len(scale) != 3 or not all(0.0 < s < float("inf") for s in scale):
        raise ValueError(f"{who}: axis_scale must hold three finite numbers > 0, got {axis_scale!r}")
    M = int(values.shape[0]) - 1
    if M == 0:
        zero = torch.zeros((), dtype=dtype, device=values.device)
        return {"tv_sigma": zero, "tv_sh": zero.clone(), "sparsity": zero.clone()}
    stored = (index > 0).view(nx, ny, nz)
    v = values.to(dtype)[index][:, :V].view(nx, ny, nz, V)          # (a node that is not stored reads row 0 and is masked below)
    square = torch.zeros_like(v)
    for a, n in enumerate((nx, ny, nz)):
        if n < 2:
            continue
        there = stored.narrow(a, 1, n - 1)[..., None]               # the forward neighbour is stored
        d = torch.where(there, scale[a] * (v.narrow(a, 1, n - 1) - v.narrow(a, 0, n - 1)), torch.zeros((), dtype=dtype, device=v.device))
        last = list(v.shape)
        last[a] = 1
        d = torch.cat([d, torch.zeros(last, dtype=dtype, device=v.device)], a)     # the last plane has no forward neighbour
        square = square + d * d
    t = torch.sqrt(square + eps) * stored[..., None].to(dtype)
    cauchy = torch.log1p(2.0 * torch.clamp(v[..., 0], min=0.0) ** 2) * stored.to(dtype)
    return {"tv_sigma": t[..., 0].sum() / M, "tv_sh": t[..., 1:].sum() / (3 * (sh_degree + 1) ** 2 * M), "sparsity": cauchy.sum() / M}


class _BakedRegularizers(torch.autograd.Function):
    """(tv_sigma, tv_sh, sparsity) of the trainer's fp32 master: nerf_baked_reg_fwd and a float64 sum of its rows; in backward
    nerf_baked_reg_bwd with the three upstream gradients, divided by the counts, in a device buffer"""

    @staticmethod
    def forward(ctx, values, trainer, eps):
        scales = trainer.axis_scale
        terms = hb.baked_reg_fwd(trainer.grid._desc(), trainer.index, trainer.row_node, values, trainer.sh_degree, scales, eps)
        M = max(trainer.n_rows - 1, 1)
        counts = (float(M), float(3 * trainer.n_basis * M), float(M))
        sums = terms.sum(0, dtype=torch.float64)
        ctx.trainer, ctx.scales, ctx.eps, ctx.counts = trainer, scales, eps, counts
        ctx.save_for_backward(values)
        return tuple((sums[i] / counts[i]).to(torch.float32) for i in range(3))

    @staticmethod
    def backward(ctx, g_sigma, g_sh, g_sparsity):
        values, = ctx.saved_tensors
        trainer = ctx.trainer
        g = torch.stack([u.detach().to(torch.float32) / c for u, c in zip((g_sigma, g_sh, g_sparsity), ctx.counts)]).contiguous()
        grad = hb.baked_reg_bwd(trainer.grid._desc(), trainer.index, trainer.row_node, values, trainer.sh_degree, ctx.scales, ctx.eps, g)
        return grad, None, None


class BakedTrainer:
    """The trainable twin of a ``BakedField``: the table fitted to images through the renderer.

    ``values`` is an fp32 ``torch.nn.Parameter`` [n_rows, W], the master copy, initialised from the field's table; ``table`` is the fp16
    table the kernels read; ``grid``, ``index``, ``sh_degree`` and ``step_size`` are copies of the field's; ``row_node`` (int32
    [n_rows]) is the inverse of ``index``: the lattice node of every row, -1 for row 0.  The trainer shares nothing mutable with the
    field it was made from.

    ``render_rays`` renders exactly the fp16 table that inference renders and hands the gradient of that render, taken at the table's
    values, to ``values`` (straight-through); ``commit()`` after ``optimizer.step()`` rounds the master into the table again.
    Training uses stop_eps = 0: a field with stop_eps > 0 is accepted and its stop_eps is carried over to ``to_field()``, but the training
    render never stops a ray, so the set of kept samples is purely geometric -- it depends on the rays and the grid's bits, never on the
    values being trained.  The outputs are rgb_map, acc_map and depth_map; there is no disp_map (its 0 / 0 on empty rays has no useful
    gradient).  ``last_stats`` = {"rays", "samples"} of the last ``render_rays`` call.

        trainer = field.trainable()
        opt = torch.optim.Adam(trainer.parameters(), lr=1e-2)
        loss = ((trainer.render_rays(rays)["rgb_map"] - target) ** 2).mean(); loss.backward(); opt.step(); opt.zero_grad(); trainer.commit()
        field = trainer.to_field()

    ``regularizers()`` gives the total variation and the sparsity of the master, to be weighted and added to the loss."""

    def __init__(self, field):
        if not isinstance(field, BakedField):
            raise ValueError("BakedTrainer: field must be a baked.BakedField")
        self._field = BakedField(copy.deepcopy(field.grid), field.index.clone(), field.table.clone(), field.sh_degree, field.step_size,
                                 field.stop_eps)
        self.values = torch.nn.Parameter(self._field.table.to(torch.float32))
        self._set_row_node()
        self.last_stats = None

    def _set_row_node(self):
        index = self._field.index.to(torch.int64)
        row_node = torch.full((self._field.n_rows,), -1, dtype=torch.int32, device=index.device)
        stored = index > 0
        row_node[index[stored]] = torch.arange(index.numel(), dtype=torch.int32, device=index.device)[stored]
        self.row_node = row_node

    # ------------------------------------------------------------------ the field's side
    grid = property(lambda self: self._field.grid)
    index = property(lambda self: self._field.index)
    table = property(lambda self: self._field.table)
    sh_degree = property(lambda self: self._field.sh_degree)
    step_size = property(lambda self: self._field.step_size)
    stop_eps = property(lambda self: self._field.stop_eps)
    n_basis = property(lambda self: self._field.n_basis)
    n_rows = property(lambda self: self._field.n_rows)
    device = property(lambda self: self._field.device)

    def to(self, device):
        """moves everything; ``values`` becomes a new Parameter, so move the trainer before handing ``parameters()`` to an optimiser"""
        self._field.to(device)
        self.row_node = self.row_node.to(device)
        with torch.no_grad():
            self.values = torch.nn.Parameter(self.values.detach().to(device))
        return self

    def parameters(self):
        return [self.values]

    def commit(self):
        """After ``optimizer.step()``: under no_grad, zeroes row 0 and the padding columns of ``values``, clamps ``values`` to the finite
        fp16 range and rounds it into ``table``.  The master keeps its fp32 digits."""
        with torch.no_grad():
            V = 1 + 3 * self.n_basis
            self.values[0].zero_()
            self.values[:, V:].zero_()
            top = float(torch.finfo(torch.float16).max)
            self.values.clamp_(min=-top, max=top)
            self._field.table.copy_(self.values)
        return self

    def to_field(self):
        """A ``BakedField`` of the table as it stands (copies: later steps do not change it), with the stop_eps of the field the trainer
        was made from.  Its ``render_rays`` gives the bits of the trainer's forward (where no ray stops)."""
        f = self._field
        return BakedField(copy.deepcopy(f.grid), f.index.clone(), f.table.clone(), f.sh_degree, f.step_size, f.stop_eps)

    def state_dict(self):
        state = self._field.state_dict()
        state["values"] = self.values.detach().cpu().clone()
        return state

    def load_state_dict(self, state):
        """Takes the state of a trainer (or, without "values", of a field: the master is then the table) of the same sh_degree and grid
        resolution"""
        dev = self.device
        values = state.get("values")
        if values is not None and tuple(values.shape) != tuple(torch.as_tensor(state["table"]).shape):
            raise ValueError("BakedTrainer.load_state_dict: values must have the table's shape")
        self._field.load_state_dict(state)
        self._field.to(dev)
        with torch.no_grad():
            src = self._field.table if values is None else torch.as_tensor(values)
            self.values = torch.nn.Parameter(src.to(device=dev, dtype=torch.float32).clone())
        self._set_row_node()
        return self

    # ------------------------------------------------------------------ the definition
    def render_rays_reference(self, rays, u=None, white_bkgd=False, max_steps=1 << 14, dtype=torch.float64, values=None, ray_grad=False,
                              geometry=None):
        """The definition of the training render, in plain torch on rays' device: ``BakedField.render_rays_reference``'s arithmetic (one
        body, _render_reference) with stop_eps = 0 -> {"rgb_map" [N, 3], "acc_map", "depth_map" [N] in `dtype`, "n_samples" int32 [N]}.
        `values` stands in for the table: None is the fp16 table cast to `dtype`; a tensor [n_rows, W] may require grad, and the result
        is differentiable with respect to it by ordinary autograd.  The gradient the kernels produce is autograd's gradient of this
        function at the fp16 table's values.  ray_grad=True (and `geometry`): differentiable in the rays as well, by
        ``BakedField.render_rays_reference``'s definition of that gradient -- what ``render_rays(ray_grad=True)`` hands to the rays."""
        out = _render_reference("BakedTrainer.render_rays_reference", self.grid, self.index, self.table, self.sh_degree, self.step_size, 0.0,
                                rays, u, white_bkgd, max_steps, dtype, values, ray_grad, geometry)
        return {k: out[k] for k in ("rgb_map", "acc_map", "depth_map", "n_samples")}

    # ------------------------------------------------------------------ the kernels
    def render_rays(self, rays, u=None, white_bkgd=False, max_steps=1 << 14, ray_grad=False):
        """{"rgb_map" fp32 [N, 3], "acc_map", "depth_map" fp32 [N]} of rays [N, >= 11] on the GPU: nerf_baked_render's bits with stop_eps
        = 0, carrying grad to ``values`` (nerf_baked_count, nerf_baked_train_fwd; in backward nerf_baked_train_bwd_samples, a stable sort
        of the samples' cells, nerf_baked_train_bwd_rows).  Two backward calls on the same inputs give the same bits.  Under no_grad
        only the count and the forward run.

        ray_grad=False: the rays are detached, whether they require grad or not.  ray_grad=True: the same forward, bit for bit, and the
        result also carries grad to `rays` (nerf_baked_train_bwd_rays: ``render_rays_reference(ray_grad=True)``'s gradient within fp32
        rounding -- the depths are constants; columns 0:6 and 8:11 receive a gradient, near, far, further columns and u none), so a
        loss reaches camera poses through ``ray_records`` and ``PoseRefinement``.  The backward runs only what is asked for: the sample
        pass once, the sort and the row pass only if ``values`` requires grad, the ray pass only if `rays` does -- so
        ``trainer.values.requires_grad_(False)`` localises a camera against a frozen table without a sort or a row pass.  The ray pass
        reads ``table`` when backward runs: call backward before ``commit()``."""
        max_steps = _check_max_steps(max_steps, "BakedTrainer.render_rays")
        if rays.dim() != 2 or rays.shape[1] < 11:
            raise ValueError("BakedTrainer.render_rays: rays [N, >= 11] (o, d, near, far, viewdir)")
        live = rays if ray_grad else None
        rays = rays.detach().to(torch.float32).contiguous()
        u = None if u is None else u.detach().to(device=rays.device, dtype=torch.float32).contiguous()
        rgb, acc, depth = _BakedRender.apply(self.values, live, self, rays, u, bool(white_bkgd), max_steps)
        return {"rgb_map": rgb, "acc_map": acc, "depth_map": depth}

    # ------------------------------------------------------------------ regularisers
    @property
    def axis_scale(self):
        """(sx, sy, sz) = min(cell edge) / (cell edge along the axis), computed in float64: 1 on cubic cells"""
        g = self.grid
        edge = (np.asarray(g.hi, dtype=np.float64) - np.asarray(g.lo, dtype=np.float64)) / np.asarray(g.resolution, dtype=np.float64)
        return tuple(float(edge.min() / e) for e in edge)

    def regularizers_reference(self, values=None, eps=1e-9, dtype=torch.float64):
        """``regularizer_reference`` (the definition) on this trainer's index and grid; `values` None: the master"""
        values = self.values if values is None else values
        return regularizer_reference(values, self.index, self._field.node_resolution, self.sh_degree, self.axis_scale, eps, dtype)

    def regularizers(self, eps=1e-9):
        """{"tv_sigma", "tv_sh", "sparsity"}, fp32 0-d tensors on the GPU carrying grad to ``values``: ``regularizer_reference`` of the fp32
        MASTER (not of the fp16 table: the loss is a plain function of the parameter, nothing is straight-through, and a small gradient
        does not vanish in fp16 rounding) within fp32 rounding -- the total variation of the density and of the colour coefficients
        between stored neighbours and Plenoxels' Cauchy sparsity of the density (nerf_baked_reg_fwd, a float64 sum over the rows; in
        backward nerf_baked_reg_bwd, a gather without atomics: two calls give the same bits).  Under no_grad only the forward runs.

            reg = trainer.regularizers(); loss = mse + 1e-3 * reg["tv_sigma"] + 1e-4 * reg["tv_sh"] + 1e-5 * reg["sparsity"]"""
        eps = _check_eps(eps, "BakedTrainer.regularizers")
        tv_sigma, tv_sh, sparsity = _BakedRegularizers.apply(self.values, self, eps)
        return {"tv_sigma": tv_sigma, "tv_sh": tv_sh, "sparsity": sparsity}
