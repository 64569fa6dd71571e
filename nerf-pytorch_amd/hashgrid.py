"""A learned multiresolution hash-grid field: ``HashEncoding`` -- L lattices over a box, every level's rows in ONE fp32
table, gathered by nerf_hash_encode_fwd and trained through nerf_hash_encode_bwd, a scatter-add made deterministic by adding 64-bit
fixed-point integers -- and ``HashNeRF``, that encoding in front of the layer stack of dense.py, a field render_rays takes on its
general-network path.

The host computes every number a level is defined by (resolution, first row, dense or hashed) in Python float64 and integers; the
kernels and the torch definitions below (``encode_reference``, ``table_grad_reference``, ``point_grad_reference``) read the same tables.
By default no gradient reaches the points: the encoding is a function of constant positions.  ``point_grad=True`` at construction
 keeps points and rays in the graph: nerf_hash_input_grad, a gather of the forward's rows, gives d loss / d points and,
for HashNeRF.query, d loss / d ray records -- pose refinement, localisation against a trained field, surface normals.
"""
import math

import torch
import torch.nn as nn

from . import hip_backend as hb
from .dense import QUERY_SLICE_POINTS, DenseNeRF, _DenseMLP

HASH_PRIMES = (1, 2654435761, 805459861)
GRAD_BITS = 61          # |sum of a row's contributions| <= M P < 2^61 in units of 2^-q


def hash_slot(ix, iy, iz, log2_hashmap_size):
    """(ix * 1 ^ iy * 2654435761 ^ iz * 805459861) mod T in wrapping uint32 arithmetic; Python integers or int64 tensors"""
    h = ((ix * HASH_PRIMES[0]) & 0xFFFFFFFF) ^ ((iy * HASH_PRIMES[1]) & 0xFFFFFFFF) ^ ((iz * HASH_PRIMES[2]) & 0xFFFFFFFF)
    return h & ((1 << log2_hashmap_size) - 1)


def level_tables(n_levels, log2_hashmap_size, base_resolution, finest_resolution):
    """(level_resolution [L], level_offset [L + 1], level_dense [L]): R_l = floor(N_min b^l), b = exp((ln N_max - ln N_min) / (L - 1)),
    the last level N_max exactly; a level is dense iff (R + 1)^3 <= T and then owns (R + 1)^3 rows, else T; the offsets are the prefix
    sums, level_offset[L] the number of rows"""
    L, T = int(n_levels), 1 << int(log2_hashmap_size)
    n_min, n_max = int(base_resolution), int(finest_resolution)
    if not 1 <= L <= hb.HASH_MAX_LEVELS:
        raise ValueError(f"HashEncoding: n_levels must be 1 .. {hb.HASH_MAX_LEVELS}, got {n_levels}")
    if not 4 <= int(log2_hashmap_size) <= 24:
        raise ValueError(f"HashEncoding: log2_hashmap_size must be 4 .. 24, got {log2_hashmap_size}")
    if n_min < 1 or n_max < n_min or n_max > 1 << 24:
        raise ValueError(f"HashEncoding: 1 <= base_resolution <= finest_resolution <= 2^24, got {base_resolution}, {finest_resolution}")
    b = math.exp((math.log(n_max) - math.log(n_min)) / (L - 1)) if L > 1 else 1.0
    res = [int(math.floor(n_min * b ** l)) for l in range(L)]
    if L > 1:
        res[-1] = n_max
    dense = [(r + 1) ** 3 <= T for r in res]
    offset = [0]
    for r, d in zip(res, dense):
        offset.append(offset[-1] + ((r + 1) ** 3 if d else T))
    return res, offset, dense


def views_grad_reference(viewdirs, d_cols, multires_views, dtype=torch.float32):
    """the adjoint of the view columns as nerf_build_inputs writes them: d_cols [..., 3] (multires_views < 0: the identity) or
    [..., 3 + 6 Lv] = d loss / d [v, sin 2^0 v, cos 2^0 v, .., sin 2^(Lv-1) v, cos 2^(Lv-1) v] -> d loss / d v [..., 3] in `dtype`:

        g = d_cols[0:3];   for k = 0 .. Lv - 1 ascending:   a = v 2^k;   g = g + 2^k (d_sin_k cos a - d_cos_k sin a)

    every multiply, subtract and add a separate torch op in that order"""
    v, d = viewdirs.to(dtype), d_cols.to(device=viewdirs.device, dtype=dtype)
    Lv = max(int(multires_views), 0)
    if d.shape[-1] != 3 + 6 * Lv or v.shape[-1] != 3:
        raise ValueError(f"views_grad_reference: {d.shape[-1]} columns for multires_views={multires_views}")
    g = d[..., 0:3]
    for k in range(Lv):
        f = float(2 ** k)
        a = v * f
        g = g + f * (d[..., 3 + 6 * k:6 + 6 * k] * torch.cos(a) - d[..., 6 + 6 * k:9 + 6 * k] * torch.sin(a))
    return g


class _HashEncode(torch.autograd.Function):
    """x [P, width] whose columns 0 .. L F hold the encoding of the points (points [P, 3], or o + d z of rays and z_vals); `fill`
    writes the other columns first (HashNeRF: the encoded view directions).  Backward: the table's gradient from d_x's first L F
    columns, read in place through the leading dimension.  With enc.point_grad also d_points / d_rays (nerf_hash_input_grad) for the
    one that requires grad -- `views` = (first view column of x, multires_views) of the columns `fill` wrote from rays[:, 8:11] -- and
    the table's scatter only when the table requires grad."""

    @staticmethod
    def forward(ctx, embeddings, enc, points, rays, z_vals, width, fill, *views):
        P = points.shape[0] if points is not None else z_vals.numel()
        dev = embeddings.device
        x = torch.empty((P, width), dtype=torch.float32, device=dev) if width == enc.out_dim else torch.zeros((P, width), dtype=torch.float32,
                                                                                                             device=dev)
        if fill is not None:
            fill(x)
        hb.hash_encode_fwd(enc.desc(), embeddings, x, 0, points, rays, z_vals)
        ctx.enc, ctx.points, ctx.rays, ctx.z_vals = enc, points, rays, z_vals
        if enc.point_grad:
            ctx.views = views[0] if views else None
            ctx.n_extra = len(views)
            ctx.save_for_backward(embeddings)
        return x

    @staticmethod
    def backward(ctx, d_x):
        enc = ctx.enc
        d_x = d_x.to(torch.float32).contiguous()
        if enc.point_grad:
            return _HashEncode._backward_point_grad(ctx, d_x)
        grad = hb.hash_encode_bwd(enc.desc(), d_x, 0, ctx.points, ctx.rays, ctx.z_vals, scratch=enc._scratch_on(d_x.device))
        return grad, None, None, None, None, None, None

    @staticmethod
    def _backward_point_grad(ctx, d_x):
        enc = ctx.enc
        points, rays, z_vals = ctx.points, ctx.rays, ctx.z_vals
        det = lambda t: None if t is None else t.detach()
        grad = d_points = d_rays = None
        if ctx.needs_input_grad[0]:     # (a frozen table -- localisation -- launches neither the maximum, nor the scatter, nor the finish)
            grad = hb.hash_encode_bwd(enc.desc(), d_x, 0, det(points), det(rays), det(z_vals), scratch=enc._scratch_on(d_x.device))
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            embeddings, = ctx.saved_tensors
            if points is not None:
                d_points = hb.hash_input_grad(enc.desc(), embeddings.detach(), d_x, 0, det(points), None, None, -1, -1)
            else:
                views_col, multires_views = ctx.views if ctx.views is not None else (-1, -1)
                d_rec = hb.hash_input_grad(enc.desc(), embeddings.detach(), d_x, 0, None, det(rays), det(z_vals), views_col, multires_views)
                C = rays.shape[1]       # (the view direction is a record's last three columns, as nerf_build_inputs reads it)
                d_rays = d_rec if C == 11 else d_rec[:, :C].contiguous() if C < 11 else torch.cat([d_rec[:, :8], d_rec.new_zeros((rays.shape[0], C - 11)),
                                                                                                    d_rec[:, 8:]], 1)
        return (grad, None, d_points, d_rays, None, None, None) + (None,) * ctx.n_extra


class HashEncoding(nn.Module):
    """Multiresolution hash encoding over the box [lo, hi]: `n_levels` lattices from `base_resolution` to `finest_resolution` cells per
    axis in geometric steps, `n_features` floats per node, a level stored densely where its (R + 1)^3 nodes fit 2^log2_hashmap_size
    rows and hashed into that many rows where they do not.  ONE parameter, ``embeddings`` [rows_total, n_features] (fp32, uniform in
    +-1e-4): one tensor for the optimizer.  ``level_resolution`` [L], ``level_offset`` [L + 1] (the last entry is rows_total) and
    ``level_dense`` [L] are plain Python lists."""

    def __init__(self, lo, hi, n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16, finest_resolution=512, point_grad=False):
        super().__init__()
        self.point_grad = bool(point_grad)      # a plain attribute: the state_dict does not know it, __getstate__ carries it
        if int(n_features) not in (1, 2, 4):
            raise ValueError(f"HashEncoding: n_features must be 1, 2 or 4, got {n_features}")
        self.lo, self.hi = tuple(float(v) for v in lo), tuple(float(v) for v in hi)
        if len(self.lo) != 3 or len(self.hi) != 3 or not all(math.isfinite(a) and math.isfinite(b) and a < b for a, b in zip(self.lo, self.hi)):
            raise ValueError(f"HashEncoding: the box needs lo[3] < hi[3], finite; got {lo}, {hi}")
        self.n_levels, self.n_features, self.log2_hashmap_size = int(n_levels), int(n_features), int(log2_hashmap_size)
        self.base_resolution, self.finest_resolution = int(base_resolution), int(finest_resolution)
        self.level_resolution, self.level_offset, self.level_dense = level_tables(n_levels, log2_hashmap_size, base_resolution, finest_resolution)
        self.out_dim = self.n_levels * self.n_features
        # what the kernels and the references read of the box, rounded to fp32 ONCE, here
        self._lo32 = torch.tensor(self.lo, dtype=torch.float32)
        self._inv32 = torch.tensor([1.0 / (b - a) for a, b in zip(self.lo, self.hi)], dtype=torch.float64).to(torch.float32)
        self.embeddings = nn.Parameter(torch.empty(self.level_offset[-1], self.n_features, dtype=torch.float32).uniform_(-1e-4, 1e-4))
        self._desc = None
        self._scratch = {}

    def __getstate__(self):        # copy.deepcopy / pickle: the C record and the accumulators are rebuilt on first use
        return dict(self.__dict__, _desc=None, _scratch={})

    @property
    def rows_total(self):
        return self.level_offset[-1]

    def extra_repr(self):
        return (f"levels={self.n_levels}, features={self.n_features}, log2_hashmap_size={self.log2_hashmap_size}, "
                f"resolution={self.base_resolution}..{self.finest_resolution}, rows={self.rows_total}")

    def desc(self):
        """the NerfHashGrid record of include/nerf_hip.h"""
        if self._desc is None:
            d = hb.NerfHashGrid()
            d.n_levels, d.n_features, d.log2_hashmap_size, d.reserved = self.n_levels, self.n_features, self.log2_hashmap_size, 0
            for a in range(3):
                d.lo[a] = float(self._lo32[a])
                d.inv_extent[a] = float(self._inv32[a])
            for l in range(self.n_levels):
                d.level_resolution[l], d.level_dense[l], d.level_offset[l] = self.level_resolution[l], int(self.level_dense[l]), self.level_offset[l]
            d.level_offset[self.n_levels] = self.level_offset[-1]
            self._desc = d
        return self._desc

    def _scratch_on(self, device):
        """the 64-bit accumulator of this table's backward on `device`: zero between calls (the finishing pass leaves it so)"""
        key = (device.type, device.index)
        if key not in self._scratch:
            self._scratch[key] = hb.hash_scratch(self.desc(), device)
        return self._scratch[key]

    def forward(self, points):
        """[..., 3] -> [..., L F] through the kernels, with autograd to ``embeddings`` (and, with point_grad, to the points)"""
        lead = points.shape[:-1]
        pts = (points if self.point_grad else points.detach()).reshape(-1, 3).to(torch.float32).contiguous()
        out = _HashEncode.apply(self.embeddings, self, pts, None, None, self.out_dim, None)
        return out.reshape(*lead, self.out_dim)

    # ---- the definition, in plain torch ops
    def _corners(self, points, level, dtype):
        """(rows [P, 8] int64 into the table, weights [P, 8] in dtype) of the eight corners on one level, corner c = bit 0 x, bit 1 y,
        bit 2 z; separate multiplies and adds in the kernels' order"""
        R = self.level_resolution[level]
        x = points.reshape(-1, 3).to(dtype)
        lo, inv = self._lo32.to(device=x.device, dtype=dtype), self._inv32.to(device=x.device, dtype=dtype)
        u = torch.clamp((x - lo) * inv, 0.0, 1.0)
        p = u * float(R)
        i = torch.clamp(torch.floor(p).to(torch.int64), 0, R - 1)
        f = p - i.to(dtype)
        rows, weights = [], []
        for c in range(8):
            bx, by, bz = c & 1, (c >> 1) & 1, (c >> 2) & 1
            wx = f[:, 0] if bx else 1.0 - f[:, 0]
            wy = f[:, 1] if by else 1.0 - f[:, 1]
            wz = f[:, 2] if bz else 1.0 - f[:, 2]
            weights.append((wx * wy) * wz)
            ix, iy, iz = i[:, 0] + bx, i[:, 1] + by, i[:, 2] + bz
            if self.level_dense[level]:
                slot = ix + iy * (R + 1) + iz * (R + 1) ** 2
            else:
                slot = hash_slot(ix, iy, iz, self.log2_hashmap_size)
            rows.append(slot + self.level_offset[level])
        return torch.stack(rows, 1), torch.stack(weights, 1)

    def encode_reference(self, points, dtype=torch.float32, embeddings=None):
        """the encoding's definition: [..., 3] -> [..., L F] in `dtype`, differentiable with respect to `embeddings` (default: the
        module's own table)"""
        E = (self.embeddings if embeddings is None else embeddings).to(dtype)
        lead = points.shape[:-1]
        out = []
        for l in range(self.n_levels):
            rows, w = self._corners(points.to(E.device), l, dtype)
            acc = w[:, 0:1] * E[rows[:, 0]]
            for c in range(1, 8):
                acc = acc + w[:, c:c + 1] * E[rows[:, c]]
            out.append(acc)
        return torch.cat(out, 1).reshape(*lead, self.out_dim)

    def point_grad_reference(self, points, d_out, dtype=torch.float32, embeddings=None):
        """the definition of the gradient with respect to the points: [P, 3] in `dtype`, the gradient of sum(encode(points) * d_out)
        (d_out [P, L F]) with respect to `points`, in closed form.  Per level l of resolution R, with encode_reference's u, p, i, f and
        rows, every multiply, add and subtract a separate torch op in this order:

            v_c   = d_out[:, l F] * E[row_c, 0];  then for k = 1 .. F - 1:  v_c = v_c + d_out[:, l F + k] * E[row_c, k]     (c = 0 .. 7)
            df_x  = -((w_y * w_z) * v_0);  then for c = 1 .. 7:  df_x = df_x + (w_y * w_z) * v_c where bit 0 of c is set, else
                    df_x = df_x - (w_y * w_z) * v_c, with w_y = f_y where bit 1 of c is set else 1 - f_y, w_z likewise (bit 2);
                    df_y with (w_x * w_z) and bit 1, df_z with (w_x * w_y) and bit 2
            g_a   = g_a + (df_a * R) * inv_extent[a],  g_a = 0 before level 0, levels ascending; the level's term is replaced by an
                    exact 0 on an axis whose UNCLAMPED t = (x - lo) * inv_extent is < 0 or > 1

        Inside a cell the encoding is trilinear: the derivative along an axis is constant in that axis and, at a lattice plane, that of
        the cell ``_corners`` picks (right-continuous; on the upper face the last cell).  Outside the box the clamp makes the encoding
        constant in that coordinate: exactly on a face (t = 0 or 1) the derivative is the cell's, as torch.clamp's backward is inclusive
        at its bounds.  nerf_hash_input_grad in point mode is held to this function (float32) bit for bit."""
        E = (self.embeddings.detach() if embeddings is None else embeddings).to(dtype)
        x = points.reshape(-1, 3).to(device=E.device, dtype=dtype)
        d = d_out.reshape(-1, self.out_dim).to(device=E.device, dtype=dtype)
        F = self.n_features
        lo, inv = self._lo32.to(device=x.device, dtype=dtype), self._inv32.to(device=x.device, dtype=dtype)
        t = (x - lo) * inv
        outside = (t < 0.0) | (t > 1.0)
        u = torch.clamp(t, 0.0, 1.0)
        zero = torch.zeros((), dtype=dtype, device=x.device)
        g = torch.zeros_like(x)
        for l in range(self.n_levels):
            R = self.level_resolution[l]
            rows, _ = self._corners(x, l, dtype)
            p = u * float(R)
            i = torch.clamp(torch.floor(p).to(torch.int64), 0, R - 1)
            f = p - i.to(dtype)
            df = [None, None, None]
            for c in range(8):
                e = E[rows[:, c]]
                v = d[:, l * F] * e[:, 0]
                for k in range(1, F):
                    v = v + d[:, l * F + k] * e[:, k]
                w = [f[:, a] if (c >> a) & 1 else 1.0 - f[:, a] for a in range(3)]
                terms = ((w[1] * w[2]) * v, (w[0] * w[2]) * v, (w[0] * w[1]) * v)
                for a in range(3):
                    if c == 0:
                        df[a] = -terms[a]
                    else:
                        df[a] = df[a] + terms[a] if (c >> a) & 1 else df[a] - terms[a]
            contrib = torch.stack([(df[a] * float(R)) * inv[a] for a in range(3)], 1)
            g = g + torch.where(outside, zero, contrib)
        return g

    def table_grad_reference(self, points, d_out):
        """the fixed-point rule of nerf_hash_encode_bwd in torch: fp32 [rows_total, F] from d_out [P, L F]"""
        pts = points.reshape(-1, 3).to(torch.float32)
        g = d_out.reshape(-1, self.out_dim).to(device=pts.device, dtype=torch.float32)
        P, F = pts.shape[0], self.n_features
        zeros = torch.zeros((self.rows_total, F), dtype=torch.float32, device=pts.device)
        M = float(g.abs().max()) if g.numel() else 0.0
        if M == 0.0:
            return zeros
        if not math.isfinite(M):
            return torch.full_like(zeros, float("nan"))
        q = GRAD_BITS - math.frexp(M)[1] - (max(P, 1) - 1).bit_length()
        acc = torch.zeros((self.rows_total, F), dtype=torch.int64, device=pts.device)
        for l in range(self.n_levels):
            rows, w = self._corners(pts, l, torch.float32)
            gl = g[:, l * F:(l + 1) * F]
            for c in range(8):
                t = w[:, c:c + 1] * gl                      # one fp32 product
                acc.index_add_(0, rows[:, c], (t.double() * 2.0 ** q).round().long())
        return (acc.double() * 2.0 ** -q).float()


class HashNeRF(DenseNeRF):
    """One HashEncoding in front of the layer stack of dense.py: a field render_rays takes on its general-network path (it IS a
    DenseNeRF there: every refusal for general networks holds for it word for word).  The stack is a DenseNeRF of its own, ``mlp``
    (input_ch = L F), so its parameter order, its state_dict keys under ``mlp.`` and _DenseMLP see no table; the table is
    ``encoding.embeddings``.  View directions go through the existing positional encoding (input_ch_views = 3 + 6 multires_views
    columns)."""

    def __init__(self, lo, hi, D=2, W=64, input_ch_views=27, output_ch=4, skips=(), use_viewdirs=True, n_levels=16, n_features=2,
                 log2_hashmap_size=19, base_resolution=16, finest_resolution=512, point_grad=False):
        nn.Module.__init__(self)        # (not DenseNeRF's: the layers live in self.mlp, once)
        self.encoding = HashEncoding(lo, hi, n_levels, n_features, log2_hashmap_size, base_resolution, finest_resolution, point_grad=point_grad)
        if not use_viewdirs:
            input_ch_views = 0
        self.mlp = DenseNeRF(D=D, W=W, input_ch=self.encoding.out_dim, input_ch_views=input_ch_views, output_ch=output_ch, skips=list(skips),
                             use_viewdirs=use_viewdirs)
        self.D, self.W = D, W
        self.input_ch, self.input_ch_views = self.encoding.out_dim, input_ch_views
        self.output_ch = output_ch
        self.skips, self.use_viewdirs = list(skips), use_viewdirs
        self.multires_views      # (raises for a width get_embedder does not build)
        self._open_density()

    INITIAL_DENSITY = 1.0

    def _open_density(self):
        """Shift the density head's bias so that the raw density of the (nearly) zero encoding a fresh table gives is
        INITIAL_DENSITY.  A fresh table holds +-1e-4, so at the start every point sees the same hidden units and the same raw density;
        with the layers' default initialisation that constant is negative in about half of all draws, the ReLU behind it then gives no
        density anywhere, and no gradient ever reaches the table or the layers."""
        m = self.mlp
        with torch.no_grad():
            x0 = torch.zeros(1, m.input_ch)
            h = x0
            for i, lin in enumerate(m.pts_linears):
                h = torch.relu(lin(h))
                if i in m.skips:
                    h = torch.cat([x0, h], -1)
            head, row = (m.alpha_linear, 0) if m.use_viewdirs else (m.output_linear, 3)
            if row < head.bias.shape[0]:
                head.bias[row] += self.INITIAL_DENSITY - head(h)[0, row]

    @property
    def multires(self):
        raise NotImplementedError("HashNeRF: the points go through a hash encoding, not a positional one")

    @property
    def point_grad(self):
        """whether points and rays stay in the graph (the encoding's flag)"""
        return self.encoding.point_grad

    def _mlp_params(self):
        return [p for _, p in self.mlp.named_parameters()]

    def forward(self, x):
        """x [..., 3 + input_ch_views] = (raw points | encoded view directions): what run_network builds with an identity embed_fn"""
        lead = x.shape[:-1]
        x2 = x.reshape(-1, x.shape[-1]).to(torch.float32)
        if x2.shape[1] != 3 + self.input_ch_views:
            raise ValueError(f"HashNeRF.forward: {x2.shape[1]} input features for 3 point columns + input_ch_views={self.input_ch_views}")
        out = self.mlp(torch.cat([self.encoding(x2[:, :3]), x2[:, 3:]], -1))
        return out.reshape(*lead, out.shape[-1])

    def _fill_views(self, rays, z_vals, x):
        """the encoded view directions into columns input_ch .. of x, by nerf_build_inputs with the identity for the points: its three
        point columns land in front of the view columns, where the hash kernel writes afterwards"""
        if not self.use_viewdirs or x.shape[0] == 0:
            return
        n, S = z_vals.shape
        cx, cd = self.input_ch, self.input_ch_views
        tmp = x if cx >= 3 else torch.empty((x.shape[0], 3 + cd), dtype=torch.float32, device=x.device)
        at = x.data_ptr() + 4 * (cx - 3) if cx >= 3 else tmp.data_ptr()
        hb._check(hb.lib().nerf_build_inputs(hb._ptr(rays, "rays"), rays.shape[1], hb._ptr(z_vals, "z_vals"), n, S, -1, self.multires_views, 1,
                                             at, tmp.shape[1], hb._stream()), "nerf_build_inputs")
        if tmp is not x:
            x[:, cx:] = tmp[:, 3:]

    def query(self, rays, z_vals):
        """raw [N, S, 4 | output_ch] of the sample points o + d z: the hash kernel + nerf_build_inputs for the view columns, then the
        layer stack.  Without gradients ~2^20 points at a time, as DenseNeRF.query."""
        n, S = z_vals.shape
        rays_per_slice = max(1, QUERY_SLICE_POINTS // max(S, 1))
        if n > rays_per_slice and not (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            return torch.cat([self.query(rays[i:i + rays_per_slice].contiguous(), z_vals[i:i + rays_per_slice].contiguous())
                              for i in range(0, n, rays_per_slice)], 0)
        if self.use_viewdirs and rays.shape[1] < 11:
            raise ValueError("HashNeRF.query: a network with view directions needs ray records with 11 columns")
        z_c = z_vals.detach().to(torch.float32).contiguous()
        if self.point_grad and torch.is_grad_enabled() and rays.requires_grad:
            # the rays stay in the graph: the one _HashEncode node owns all of x, so its backward takes the hash columns AND the view
            # columns of _DenseMLP's d_x to d_rays in one call (depths are constants)
            rays_c = rays.to(torch.float32).contiguous()
            rays_k = rays_c.detach()
            views = (self.input_ch, self.multires_views) if self.use_viewdirs else None
            x = _HashEncode.apply(self.encoding.embeddings, self.encoding, None, rays_c, z_c, self.input_ch + self.input_ch_views,
                                  lambda m: self._fill_views(rays_k, z_c, m), views)
            out = _DenseMLP.apply(self.mlp, x, *self._mlp_params())
            return out.reshape(n, S, out.shape[-1])
        rays_c = rays.detach().to(torch.float32).contiguous()
        x = _HashEncode.apply(self.encoding.embeddings, self.encoding, None, rays_c, z_c, self.input_ch + self.input_ch_views,
                              lambda m: self._fill_views(rays_c, z_c, m))
        out = _DenseMLP.apply(self.mlp, x, *self._mlp_params())
        return out.reshape(n, S, out.shape[-1])
