"""Occupancy grids: empty-space skipping for rendering (OccupancyGrid) and for training (DensityGrid).

The reference evaluates the network at every sample point of render_rays (run_nerf.py:381-385, :397-401), the points of a trained
scene that lie in empty space included.  ``OccupancyGrid`` is one bit per cell of an axis-aligned box; handed to
``render_rays(..., occupancy=grid)`` (or put into ``render_kwargs_test["occupancy"]``) only the sample points in occupied cells go
through the network, every other sample gets ``raw = (0, 0, 0, 0)`` -- ``relu(sigma) = 0``, ``alpha = 0``, weight 0 -- and nothing
else of render_rays changes.  Device code: csrc/occupancy.hip (include/nerf_hip.h, "occupancy grid").

A static bit grid is built from a network that training is about to change.  ``DensityGrid`` is the grid that follows the network
(Instant-NGP's density grid, Mueller et al. 2022, section 5 / appendix E.2): a decayed running maximum of the density per cell,
refreshed every few steps and thresholded into the bits the renderer reads; ``render_rays(..., occupancy=density_grid)`` is
differentiable (render._RenderRaysGrid; its forward is render._grid_chain, the stages of the no-grad grid render).
"""
import math

import numpy as np
import torch

from . import hip_backend as hb

_OUTSIDE = ("evaluate", "skip")
_SLICE_CELLS = 1 << 20      # cells per evaluation slice of from_network (a multiple of 32: slices start on word boundaries)


def _res3(resolution):
    r = (resolution,) * 3 if isinstance(resolution, (int, np.integer)) else tuple(int(v) for v in resolution)
    if len(r) != 3 or any(v < 1 or v > 512 for v in r):
        raise ValueError(f"OccupancyGrid: resolution must be an int or three ints between 1 and 512, got {resolution!r}")
    return tuple(int(v) for v in r)


def _pack_bits(mask_flat):
    """bool [n_cells] -> int32 [(n_cells + 31) // 32]: cell c is bit c & 31 of word c >> 5 (the tail of the last word stays 0)"""
    n = mask_flat.numel()
    pad = (-n) % 32
    m = torch.cat([mask_flat.to(torch.int64), torch.zeros(pad, dtype=torch.int64, device=mask_flat.device)]).view(-1, 32)
    w = (m << torch.arange(32, dtype=torch.int64, device=m.device)).sum(-1)
    return torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32)


def _unpack_bits(words, n_cells):
    w = words.to(torch.int64) & 0xffffffff
    return (((w[:, None] >> torch.arange(32, dtype=torch.int64, device=w.device)) & 1).reshape(-1)[:n_cells]).bool()


def _check_eps(eps, who):
    e = float(eps)
    if not (0.0 < e < 1.0):         # (also refuses NaN)
        raise ValueError(f"{who}: early_stop_eps must satisfy 0 < eps < 1, got {eps!r}")
    return e


def _check_march_eps(eps, who):
    if isinstance(eps, bool) or not isinstance(eps, (float, np.floating)) or not (0.0 < float(eps) < 1.0):      # (also refuses NaN)
        raise ValueError(f"{who}: march_stop_eps must be a float with 0 < eps < 1, got {eps!r}")
    return float(eps)


def _check_march_step(step_size, fit, who):
    """(step_size as a float, fit as an int) of the world-space march: a finite real number > 0 and an int in 0..8, bools refused"""
    real = not isinstance(step_size, (bool, np.bool_)) and isinstance(step_size, (int, float, np.integer, np.floating))
    if real:
        try:
            with np.errstate(all="ignore"):
                real = 0.0 < float(np.float32(step_size)) < float("inf")       # (the kernel's step is fp32(step_size); also refuses NaN)
        except OverflowError:
            real = False
    if not real:
        raise ValueError(f"{who}: march_step_size must be a finite real number > 0 (as an fp32 value), got {step_size!r}")
    if isinstance(fit, (bool, np.bool_)) or not isinstance(fit, (int, np.integer)) or not (0 <= int(fit) <= 8):
        raise ValueError(f"{who}: march_fit must be an int with 0 <= march_fit <= 8, got {fit!r}")
    return float(step_size), int(fit)


def _march_inputs(who, rays, n_steps, n_slots, u):
    """(rays, u, M, S) as the march kernels take them: detached contiguous fp32 tensors (u may be None), 1 <= M <= 16384, 1 <= S <= 4096"""
    M, S = int(n_steps), int(n_slots)
    if not (1 <= M <= 16384) or not (1 <= S <= 4096):
        raise ValueError(f"{who}: 1 <= n_steps <= 16384 and 1 <= n_slots <= 4096, got {n_steps!r}, {n_slots!r}")
    return rays.detach().to(torch.float32).contiguous(), None if u is None else u.detach().to(torch.float32).contiguous(), M, S


def stop_depth_reference(z_vals, weights, eps):
    """The definition of the stop depth of render_rays(early_stop_eps=eps), in numpy (tensors of any device; fp32 [N] on z_vals' device).

    weights[r, i] are the compositing weights of the coarse depths z_vals[r, i] -- the weight i belongs to the interval [z_i, z_{i+1}]
    -- and their sum up to sample i is 1 - T, T the transmittance behind that interval.  Per ray: a = 0; a = a + weights[i] for i = 0,
    1, ... -- one fp32 addition each, strictly left to right --; i* = the first i with a >= fp32(1 - eps) (the threshold is computed in
    float64 and rounded once; a NaN weight never satisfies the comparison and poisons a: such a ray never stops);
    z_stop = z_vals[i* + 1], or +inf when there is no i* or i* is the last sample (its interval is the reference's 1e10 one: nothing
    lies behind it).  Behind z_stop the COARSE estimate of the transmittance is below eps."""
    eps = _check_eps(eps, "stop_depth_reference")
    z = np.asarray(z_vals.detach().cpu().numpy(), dtype=np.float32)
    w = np.asarray(weights.detach().cpu().numpy(), dtype=np.float32)
    if z.ndim != 2 or z.shape != w.shape:
        raise ValueError("stop_depth_reference: z_vals and weights [N, S]")
    n, S = z.shape
    out = np.full(n, np.inf, dtype=np.float32)
    if n > 0:
        with np.errstate(invalid="ignore"):         # (inf - inf among the weights: a NaN, which never crosses)
            crossed = np.cumsum(w, axis=1, dtype=np.float32) >= np.float32(hb.stop_threshold(eps))      # (sequential per row)
        first = np.argmax(crossed, axis=1)
        behind = crossed.any(axis=1) & (first + 1 < S)
        out[behind] = z[behind, first[behind] + 1]
    return torch.from_numpy(out).to(z_vals.device)


def stop_depth(z_vals, weights, eps):
    """fp32 [N] for z_vals / weights [N, S] on the GPU (nerf_occ_stop_depth): ``stop_depth_reference`` bit for bit.  A constant of the
    graph (computed without gradients from detached values)."""
    eps = _check_eps(eps, "stop_depth")
    with torch.no_grad():
        return hb.occ_stop_depth(z_vals.detach().to(torch.float32).contiguous(), weights.detach().to(torch.float32).contiguous(), eps)


_SAT_BYTES = 64 << 20       # most summed-area tables held at once by view_counts / carved (the views are fed in chunks)


def _view_inputs(who, c2w, H, W, K, near, far, margin_px, masks=None):
    """what the view tests start from: (cams fp32 [V, 16] on the CPU -- c2w row-major, fx, fy, cx, cy --, H, W, near_m, far_m, m, masks
    bool [V, H, W] or None)"""
    c2w = torch.as_tensor(c2w).detach().to(device="cpu", dtype=torch.float32)
    if c2w.dim() == 2:
        c2w = c2w[None]
    if c2w.dim() != 3 or c2w.shape[0] < 1 or c2w.shape[1] < 3 or c2w.shape[2] != 4:
        raise ValueError(f"{who}: c2w [V >= 1, 3, 4] (columns right, up, back, position)")
    V = c2w.shape[0]
    K = torch.as_tensor(K).detach().to(device="cpu", dtype=torch.float32)
    if tuple(K.shape) == (3, 3):
        K = K[None].expand(V, 3, 3)
    if tuple(K.shape) != (V, 3, 3):
        raise ValueError(f"{who}: K [3, 3] or [V, 3, 3]")
    H, W, m = int(H), int(W), float(margin_px)
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise ValueError(f"{who}: 1 <= H, W <= 16384, got {H}, {W}")
    if not (0.0 <= m < float("inf")):       # (also refuses NaN)
        raise ValueError(f"{who}: margin_px must be finite and >= 0, got {margin_px!r}")
    near_m, far_m = hb.view_planes(near, far)
    cams = torch.cat([c2w[:, :3, :].reshape(V, 12), K[:, 0, 0:1], K[:, 1, 1:2], K[:, 0, 2:3], K[:, 1, 2:3]], -1).contiguous()
    if masks is not None:
        masks = torch.as_tensor(masks)
        if masks.dtype != torch.bool or tuple(masks.shape) != (V, H, W):
            raise ValueError(f"{who}: masks must be bool [V, H, W] = {(V, H, W)}, True meaning foreground")
    return cams, H, W, near_m, far_m, m, masks


def _mask_sat(masks):
    """int32 [V, H + 1, W + 1]: sat[v, j, i] = the foreground pixels of masks[v] with row < j and column < i"""
    V, H, W = masks.shape
    sat = torch.zeros((V, H + 1, W + 1), dtype=torch.int32, device=masks.device)
    sat[:, 1:, 1:] = masks.to(torch.int32).cumsum(1, dtype=torch.int32).cumsum(2, dtype=torch.int32)
    return sat


class OccupancyGrid:
    """One bit per cell of the axis-aligned box [lo, hi] at resolution (Rx, Ry, Rz) (an int means cubic; 1..512 per axis), in the
    space of the points ``o + d z`` the network sees -- for ``ndc=True`` rays that is NDC space.

    Cell (ix, iy, iz) has linear index c = (ix Ry + iy) Rz + iz and lives in bit c & 31 of the 32-bit word c >> 5 of ``bits``.
    A point p is classified per axis by t = (p - lo) * scale in fp32 (one subtraction, one multiplication), scale = fp32(R / (hi -
    lo)) computed once in float64; it is inside iff 0 <= t < R on all axes (a NaN is outside) and then belongs to cell floor(t).
    ``occupied(pts)`` is that rule in plain torch and is the definition the kernels reproduce bit for bit.
    ``outside="evaluate"`` (default): a point outside the box is evaluated -- the grid never hides what it does not cover;
    ``outside="skip"``: it is skipped (scenes bounded by the box).  A new grid is all-occupied.
    ``last_stats`` = {"evaluated", "total"}: sample points sent through the network / of the passes, for the last render_rays (or
    batchify_rays / render: summed over its chunks) call that used this grid; with clip_to_occupancy=True also {"rays_hit", "rays"},
    with early_stop_eps also {"rays_stopped"} (rays with a finite stop depth; "evaluated" then counts what survived grid and stop).
    ``ray_span`` / ``clip_rays`` give the grid its second use: per ray the span from the first to the last occupied cell it crosses
    (``ray_span_reference`` is the definition), which render_rays(clip_to_occupancy=True) samples instead of [near, far].
    ``march`` gives it a third: the depths themselves, per ray the equal steps over [near, far] that fall in occupied cells
    (``march_reference`` is the definition) -- render_rays(proposal="march"), whose last_stats carry {"rays_truncated"} (and, with
    march_stop_eps over a DensityGrid, {"rays_stopped"}).  ``march_step`` is the march in steps of one length in the scene, with the
    step doubled per ray until its emitted steps fit the slots (``march_step_reference`` is the definition) --
    render_rays(proposal="march", march_step_size=ds, march_fit=J), whose last_stats carry {"rays_refit"} when J > 0.
    ``from_views`` builds a grid without a network, from the training cameras (and silhouettes) alone: the cells some camera sees, minus
    the cells some camera carves (``view_counts_reference`` / ``carved_reference`` are the definitions); ``restrict`` ANDs such a grid in."""

    def __init__(self, lo, hi, resolution, outside="evaluate", device=None):
        if outside not in _OUTSIDE:
            raise ValueError(f"OccupancyGrid: outside must be one of {_OUTSIDE}")
        self.resolution = _res3(resolution)
        self.outside = outside
        self._set_box(lo, hi)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.bits = _pack_bits(torch.ones(self.n_cells, dtype=torch.bool, device=device))
        self.last_stats = None

    def _set_box(self, lo, hi):
        as3 = lambda v: np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float32).reshape(3)
        self.lo, self.hi = as3(lo), as3(hi)
        if not np.all(self.hi > self.lo):       # (also refuses NaN)
            raise ValueError("OccupancyGrid: hi must exceed lo on every axis")
        r = np.asarray(self.resolution, dtype=np.float64)
        self.scale = (r / (self.hi.astype(np.float64) - self.lo.astype(np.float64))).astype(np.float32)
        self.width = ((self.hi.astype(np.float64) - self.lo.astype(np.float64)) / r).astype(np.float32)     # (a cell's edges: the view tests)

    # ------------------------------------------------------------------ plain properties
    @property
    def n_cells(self):
        return self.resolution[0] * self.resolution[1] * self.resolution[2]

    @property
    def device(self):
        return self.bits.device

    def to(self, device):
        self.bits = self.bits.to(device)
        return self

    # ------------------------------------------------------------------ masks
    @classmethod
    def from_mask(cls, mask, lo, hi, outside="evaluate", device=None):
        """grid whose cell (ix, iy, iz) is occupied iff mask[ix, iy, iz] (bool [Rx, Ry, Rz])"""
        mask = torch.as_tensor(mask)
        if mask.dim() != 3:
            raise ValueError("OccupancyGrid.from_mask: mask must be [Rx, Ry, Rz]")
        g = cls(lo, hi, tuple(mask.shape), outside, device)
        g.bits = _pack_bits(mask.to(g.device).bool().reshape(-1))
        return g

    def to_mask(self):
        return _unpack_bits(self.bits, self.n_cells).view(self.resolution)

    def fraction_occupied(self):
        return float(self.to_mask().float().mean())

    # ------------------------------------------------------------------ the definition
    def _classify(self, pts):
        """(inside bool [...], cell int64 [...] -- 0 where outside --, bit bool [...]) for pts [..., 3]: the rule of the class docstring"""
        dev = pts.device
        f = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
        t = (pts.to(torch.float32) - f(self.lo)) * f(self.scale)
        rx, ry, rz = self.resolution
        inside = ((t >= 0) & (t < f(np.asarray(self.resolution, dtype=np.float32)))).all(-1)
        i = torch.floor(torch.where(inside[..., None], t, torch.zeros_like(t))).to(torch.int64)
        c = (i[..., 0] * ry + i[..., 1]) * rz + i[..., 2]
        bits = self.bits if self.bits.device == dev else self.bits.to(dev)
        bit = ((bits[c >> 5].to(torch.int64) >> (c & 31)) & 1).bool()
        return inside, c, bit

    def occupied(self, pts):
        """bool [...] for pts [..., 3] (any device): whether a sample at that point is evaluated"""
        inside, _, bit = self._classify(pts)
        return torch.where(inside, bit, torch.full_like(bit, self.outside == "evaluate"))

    # ------------------------------------------------------------------ the occupied span of a ray
    def ray_span_reference(self, rays):
        """The definition of the occupied span, in float64 plain torch: rays [N, >= 8] (o, d, near, far; any device) ->
        (hit bool [N, 2], near_all, far_all, near_thick, far_thick), float64 [N] each.

        A ray crosses the Rx + 1 / Ry + 1 / Rz + 1 cell planes of the axes at depths t (a zero direction component crosses none);
        those inside [near, far], with near and far, cut the interval into segments: one cell each, or one stretch outside the box.
        A segment is occupied by the rule of ``occupied()`` applied to its midpoint (inside iff 0 <= g < R on all axes, cell floor(g),
        outside counts iff outside == "evaluate"), g = (o + d t - lo) * scale evaluated in float64.  ``*_all`` is the hull of the
        occupied segments of positive length, ``*_thick`` that of the occupied segments longer than 2^-9 cell, a length being measured
        in grid units along the ray's fastest axis (dt * max_a |d_a scale_a|); hit[:, 0] / hit[:, 1] say whether the all / the thick
        hull exists, and where it does not the pair is the ray's own (near, far).  A ray with a NaN or infinite component, or with
        near >= far, has no hull.  ``ray_span`` (the kernel) lies between the two hulls."""
        dev = rays.device
        if rays.shape[0] > 4096:        # (the segments of 4096 rays at 512^3 are 150 MB of float64)
            parts = [self.ray_span_reference(rays[i:i + 4096]) for i in range(0, rays.shape[0], 4096)]
            return tuple(torch.cat(p, 0) for p in zip(*parts))
        r = rays.detach()[:, :8].to(torch.float64)
        ok = torch.isfinite(r).all(-1) & (r[:, 6] < r[:, 7])
        safe = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], dtype=torch.float64, device=dev)
        r = torch.where(ok[:, None], r, safe)
        near, far = r[:, 6], r[:, 7]
        f = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), device=dev)
        res = f(self.resolution)
        go, gd = (r[:, 0:3] - f(self.lo)) * f(self.scale), r[:, 3:6] * f(self.scale)
        fastest = gd.abs().amax(-1)
        cuts = [near[:, None], far[:, None]]
        for a in range(3):
            k = torch.arange(self.resolution[a] + 1, dtype=torch.float64, device=dev)
            moves = gd[:, a] != 0
            t = (k[None, :] - go[:, a:a + 1]) / torch.where(moves, gd[:, a], torch.ones_like(near))[:, None]
            cuts.append(torch.where(moves[:, None], t, near[:, None]))
        t = torch.minimum(torch.maximum(torch.cat(cuts, -1), near[:, None]), far[:, None]).sort(-1).values
        t0, t1 = t[:, :-1], t[:, 1:]
        g = go[:, None, :] + gd[:, None, :] * (0.5 * (t0 + t1))[..., None]
        inside = ((g >= 0) & (g < res)).all(-1)
        i = torch.floor(torch.where(inside[..., None], g, torch.zeros_like(g))).to(torch.int64)
        c = (i[..., 0] * self.resolution[1] + i[..., 1]) * self.resolution[2] + i[..., 2]
        bits = self.bits if self.bits.device == dev else self.bits.to(dev)
        bit = ((bits[c >> 5].to(torch.int64) >> (c & 31)) & 1).bool()
        occ = torch.where(inside, bit, torch.full_like(bit, self.outside == "evaluate")) & ok[:, None]
        length = t1 - t0
        inf = torch.full_like(t0, float("inf"))
        out, hits = [], []
        for keep in (occ & (length > 0), occ & (length * fastest[:, None] > 2.0 ** -9)):
            h = keep.any(-1)
            hits.append(h)
            out += [torch.where(h, torch.where(keep, t0, inf).amin(-1), rays[:, 6].to(torch.float64)),
                    torch.where(h, torch.where(keep, t1, -inf).amax(-1), rays[:, 7].to(torch.float64))]
        return (torch.stack(hits, -1),) + tuple(out)

    def ray_span(self, rays):
        """(span fp32 [N, 2], hit bool [N]) for rays [N, >= 8] on the GPU (nerf_occ_ray_span): per ray the first and the last occupied
        cell it crosses inside [near, far], widened by 2^-10 cell -- every sample ``occupied()`` would keep lies in [near', far'] --
        and the ray's own (near, far), hit False, where it crosses nothing occupied.  Computed without gradients from detached values."""
        with torch.no_grad():
            span, hit = hb.occ_ray_span(self._desc(), rays.detach().to(torch.float32).contiguous())
        return span, hit.bool()

    def clip_rays(self, rays):
        """(rays', hit): the ray records with columns 6:8 (near, far) replaced by ``ray_span``'s.  Columns 0:6 and 8: keep their
        autograd history; near' / far' are constants of the graph (no gradient flows through the span, as none flows to near / far)."""
        span, hit = self.ray_span(rays)
        return torch.cat([rays[:, :6], span.to(rays.dtype), rays[:, 8:]], -1), hit

    # ------------------------------------------------------------------ ray marching
    def march_reference(self, rays, u, n_steps, n_slots):
        """The definition of the depths of render_rays(proposal="march"), in plain torch (any device): rays [N, >= 8] (o, d, near, far),
        u fp32 [N] in [0, 1) or None (0.5 for every ray) -> (z_vals fp32 [N, S], z_stop fp32 [N], truncated bool [N]), M = n_steps,
        S = n_slots.

        Candidates, k = 0 .. M - 1: t_k = (fp32(k) + u) / fp32(M) (one addition, one correctly rounded division);
        z_k = near * (1 - t_k) + far * t_k (run_nerf.py:360's expression, no contraction).  keep_k = occupied(o + d * z_k) (one multiply,
        one add per axis: run_nerf.py:381); close_k = not keep_k and k > 0 and keep_{k-1}, the first empty candidate behind an occupied
        run.  The emitted candidates are those with keep_k or close_k, in order of k, E of them: the first n = min(E, S - 1) fill
        z_vals[r, 0:n]; with E > S - 1 the ray is truncated and z_stop is the depth of emitted candidate S - 1 (the first that did not
        fit), else z_stop = far; the slots n .. S - 1 hold z_stop.  A ray whose first eight components are not all finite, or with
        near >= far, emits nothing: its row is its own far, its z_stop -inf ("stops everything"), and it is not truncated.

        A closing sample lies in an empty cell: the compaction skips it (raw = 0, alpha = 0) and it owns the gap behind its run, so an
        evaluated sample's interval z[i + 1] - z[i] reaches exactly to the next candidate and never across a gap.  Padding and
        truncation ride on z_stop: nerf_occ_compact_stop's not (z >= z_stop) drops every slot at or behind it, the last one -- the
        reference's 1e10 interval -- included.  Rows are nondecreasing: nothing is sorted."""
        r, ok, uu, _, M, S = self._march_rays("march_reference", rays, u, n_steps, n_slots)
        return self._march_walk(r, ok, *self._equal_steps(r, ok, uu, M), S)[:3]

    def march(self, rays, n_steps, n_slots, u=None):
        """(z_vals fp32 [N, n_slots], z_stop fp32 [N], truncated bool [N]) for rays [N, >= 8] on the GPU (nerf_occ_march):
        ``march_reference`` bit for bit.  Constants of the graph (computed without gradients from detached values, as the reference
        detaches z_samples)."""
        rays, u, M, S = _march_inputs("OccupancyGrid.march", rays, n_steps, n_slots, u)
        with torch.no_grad():
            z_vals, z_stop, truncated = hb.occ_march(self._desc(), rays, u, M, S)
        return z_vals, z_stop, truncated.bool()

    # ------------------------------------------------------------------ the march references: one walk, two ways to step
    @staticmethod
    def _march_rays(who, rays, u, n_steps, n_slots):
        """what every march reference starts from: (r fp32 [N, 8], ok bool [N] -- all finite and near < far --, u fp32 [N, 1],
        |d| fp32 [N, 1], M, S)"""
        M, S = int(n_steps), int(n_slots)
        if M < 1 or S < 1:
            raise ValueError(f"{who}: n_steps >= 1 and n_slots >= 1")
        if rays.dim() != 2 or rays.shape[1] < 8:
            raise ValueError(f"{who}: rays [N, >= 8] (o, d, near, far, ...)")
        dev = rays.device
        r = rays.detach()[:, :8].to(torch.float32)
        N = r.shape[0]
        ok = torch.isfinite(r).all(-1) & (r[:, 6] < r[:, 7])
        uu = torch.full((N, 1), 0.5, dtype=torch.float32, device=dev) if u is None else u.detach().to(device=dev, dtype=torch.float32).reshape(N, 1)
        d = r[:, 3:6]
        # the correctly rounded fp32 square root, taken through float64 (53 >= 2 * 24 + 2 bits: rounding twice is rounding once): a torch
        # build's own fp32 sqrt may be a vector-library routine that is an ulp off on some CPUs; the world-space step puts that ulp
        # into every depth, and an optical depth next to tau can turn a stop on it
        dn = torch.sqrt((d[:, 0:1] * d[:, 0:1] + d[:, 1:2] * d[:, 1:2] + d[:, 2:3] * d[:, 2:3]).to(torch.float64)).to(torch.float32)
        return r, ok, uu, dn, M, S

    @staticmethod
    def _equal_steps(r, ok, uu, M):
        """(z fp32 [N, M], valid bool [N, M]) of the M equal steps over [near, far]: every candidate of a valid ray counts"""
        k = torch.arange(M, dtype=torch.float32, device=r.device)[None, :]
        t = (k + uu) / torch.tensor(float(M), dtype=torch.float32, device=r.device)
        return r[:, 6:7] * (1.0 - t) + r[:, 7:8] * t, ok[:, None].expand(-1, M)

    @staticmethod
    def _world_steps(r, ok, uu, dz, M):
        """(z fp32 [N, K], valid bool [N, K]) of the steps dz [N, 1]: a candidate counts while it lies in front of far.  Candidates
        behind the last one that is valid on ANY ray are not built: they emit nothing, add nothing to an optical depth and cut nothing."""
        z = r[:, 6:7] + (torch.arange(M, dtype=torch.float32, device=r.device)[None, :] + uu) * dz
        valid = (z < r[:, 7:8]) & ok[:, None]
        cols = valid.any(0).nonzero()
        K = min(M, (int(cols.max()) + 2) if cols.numel() else 1)       # (one column more: the candidate behind the last valid one)
        return z[:, :K], valid[:, :K]

    def _march_walk(self, r, ok, z, valid, S, dn=None, tau=None):
        """the rule of the four march references, once (plain torch): (z_vals, z_stop, truncated, stopped) of the rays r [N, 8] -- ok
        [N] says which are valid -- for the candidate depths z [N, K], of which those under valid [N, K] count (a prefix of every row).
        tau None: the plain rule; else a DensityGrid's stop rule on top, with |d| = dn [N, 1]."""
        dev = r.device
        N, K = z.shape
        far = r[:, 7:8]
        pts = r[:, None, 0:3] + r[:, None, 3:6] * z[:, :, None]
        keep = self.occupied(pts) & valid
        before = torch.cat([torch.zeros_like(keep[:, :1]), keep[:, :-1]], -1)
        emit = keep | (before & ~keep & valid)
        has_cut = torch.zeros(N, dtype=torch.bool, device=dev)
        k_stop = torch.full((N,), K, dtype=torch.int64, device=dev)
        if tau is not None:
            valid_next = torch.cat([valid[:, 1:], torch.zeros_like(valid[:, :1])], -1)
            z_next = torch.where(valid_next, torch.cat([z[:, 1:], far], -1), far.expand(-1, K))
            sigma = self.proposal_sigma(pts)
            sigma = torch.where(sigma > 0, sigma, torch.zeros_like(sigma))
            c = torch.where(keep, sigma * ((z_next - z) * dn), torch.zeros_like(z))
            rounds = (K + 63) // 64         # the exclusive prefix sum in the order of the kernel's wave scan
            incl = torch.cat([c, torch.zeros((N, rounds * 64 - K), dtype=torch.float32, device=dev)], -1).view(N, rounds, 64)
            for s in (1, 2, 4, 8, 16, 32):
                incl = torch.cat([incl[..., :s], incl[..., s:] + incl[..., :-s]], -1)
            base = torch.zeros((N, rounds), dtype=torch.float32, device=dev)
            for j in range(1, rounds):
                base[:, j] = base[:, j - 1] + incl[:, j - 1, 63]
            A = (base[:, :, None] + torch.cat([torch.zeros_like(incl[..., :1]), incl[..., :-1]], -1)).view(N, rounds * 64)[:, :K]
            cut = (A >= tau) & valid                        # (a NaN never is)
            has_cut = cut.any(-1)
            k_stop = torch.where(has_cut, cut.to(torch.uint8).argmax(-1), k_stop)
            emit = emit & (torch.arange(K, device=dev)[None, :] < k_stop[:, None])
        rank = torch.cumsum(emit.to(torch.int64), -1) - 1
        truncated = emit.sum(-1) > S - 1
        stopped = has_cut & ~truncated
        first_out = emit & (rank == S - 1)          # (at most one per row)
        z_stop = torch.where(truncated, z.gather(1, first_out.to(torch.uint8).argmax(-1, keepdim=True))[:, 0], r[:, 7])
        z_stop = torch.where(stopped, z.gather(1, k_stop.clamp(max=K - 1)[:, None])[:, 0], z_stop)
        z_stop = torch.where(ok, z_stop, torch.full_like(z_stop, float("-inf")))
        z_vals = torch.where(ok, z_stop, r[:, 7])[:, None].repeat(1, S)
        rows, cols = (emit & (rank < S - 1)).nonzero(as_tuple=True)
        z_vals[rows, rank[rows, cols]] = z[rows, cols]
        return z_vals, z_stop, truncated, stopped

    def _march_step_levels(self, who, rays, u, step_size, n_steps, n_slots, fit, tau):
        """the levels of the world-space march over the shared walk: (z_vals, z_stop, truncated, level, stopped)"""
        r, ok, uu, dn, M, S = self._march_rays(who, rays, u, n_steps, n_slots)
        step_size, fit = _check_march_step(step_size, fit, who)
        dev = rays.device
        dz0 = torch.tensor(step_size, dtype=torch.float32, device=dev) / dn
        ok = ok & (dz0[:, 0] > 0) & torch.isfinite(dz0[:, 0])

        def walk(rows, dz):
            return self._march_walk(r[rows], ok[rows], *self._world_steps(r[rows], ok[rows], uu[rows], dz, M), S, dn[rows], tau)
        out = list(walk(slice(None), dz0))
        level = torch.zeros(r.shape[0], dtype=torch.int32, device=dev)
        for j in range(1, fit + 1):
            again = out[2].nonzero()[:, 0]          # the rays still truncated walk again with the step doubled
            if again.numel() == 0:
                break
            nxt = walk(again, dz0[again] * torch.tensor(float(1 << j), dtype=torch.float32, device=dev))
            for a, b in zip(out, nxt):
                a[again] = b
            level[again] = j
        return out[0], out[1], out[2], level, out[3]

    def march_step_reference(self, rays, u, step_size, n_steps, n_slots, fit=0):
        """The definition of the depths of render_rays(proposal="march", march_step_size=ds, march_fit=J), in plain torch (any device):
        rays [N, >= 8], u fp32 [N] in [0, 1) or None (0.5) -> (z_vals fp32 [N, S], z_stop fp32 [N], truncated bool [N], level int32 [N]);
        M = n_steps is the cap on candidates per ray, S = n_slots, ds = fp32(step_size) a length in the scene, J = fit.

        Per ray: dn = sqrt(dx dx + dy dy + dz dz), added left to right (march_stop_reference's expression); dz0 = ds / dn, one correctly
        rounded division.  The ray is invalid when its first eight components are not all finite, when near >= far, or when dz0 is not a
        finite number > 0 (d = 0 among them); an invalid ray emits nothing: its row is its own far, z_stop = -inf, no flag, level 0.
        Level j = 0 .. J: dz_j = dz0 * 2^j; candidates k = 0 .. M - 1 at z_k = near + (fp32(k) + u) * dz_j (one addition, one
        multiplication, one addition, not contracted); valid_k = z_k < far (z_k is nondecreasing in k: a prefix); keep_k = valid_k and
        occupied(o + d * z_k); close_k = valid_k and not keep_k and k > 0 and keep_{k-1}.  From here on everything is march_reference's
        with "k < M" read as valid_k: the emitted candidates in order of k, the first min(E, S - 1) of them fill the row, E > S - 1
        means truncated with z_stop the first candidate that did not fit, else z_stop = far; padding slots hold z_stop.
        The ray's level is the smallest j at which it is not truncated and its outputs are that level's; if no level fits, the level
        is J and the ray is truncated.  u is the same at every level.

        With |d| = 1, near = 0 and a power-of-two geometry (ds * M = far, all of them powers of two) the level-0 depths equal
        march_reference's bit for bit: (k + u) * ds and (k + u) / M * far are then the same exact scalings."""
        z, z_stop, tr, level, _ = self._march_step_levels("march_step_reference", rays, u, step_size, n_steps, n_slots, fit, None)
        return z, z_stop, tr, level

    def march_step(self, rays, step_size, n_steps, n_slots, fit=0, u=None):
        """(z_vals fp32 [N, n_slots], z_stop fp32 [N], truncated bool [N], level int32 [N]) for rays [N, >= 8] on the GPU
        (nerf_occ_march_step): ``march_step_reference`` bit for bit.  Constants of the graph (computed without gradients from detached
        values, like ``march``)."""
        rays, u, M, S = _march_inputs("OccupancyGrid.march_step", rays, n_steps, n_slots, u)
        step_size, fit = _check_march_step(step_size, fit, "OccupancyGrid.march_step")
        with torch.no_grad():
            z_vals, z_stop, truncated, level, _ = hb.occ_march_step(self._desc(), None, 0.0, rays, u, step_size, M, S, fit)
        return z_vals, z_stop, truncated.bool(), level

    # ------------------------------------------------------------------ grids from cameras and silhouettes
    _CORNERS = tuple(((k >> 2) & 1, (k >> 1) & 1, k & 1) for k in range(8))

    def _views_reference(self, who, c2w, H, W, K, near, far, margin_px, masks):
        """the rule of view_counts_reference / carved_reference, once (plain torch on c2w's device, the CPU for anything that is no
        tensor): (count int32 [n_cells], carved bool [n_cells] -- all False without masks)"""
        dev = c2w.device if isinstance(c2w, torch.Tensor) else torch.device("cpu")
        cams, H, W, near_m, far_m, m, masks = _view_inputs(who, c2w, H, W, K, near, far, margin_px, masks)
        f = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
        cams, lo, width = cams.to(dev), f(self.lo), f(self.width)
        sat = None if masks is None else _mask_sat(masks.to(dev))
        near_m, far_m, m = f(near_m), f(far_m), f(m)
        w_hi, h_hi = f(float(W - 1)) + m, f(float(H - 1)) + m
        rx, ry, rz = self.resolution
        offs = torch.tensor(self._CORNERS, dtype=torch.int64, device=dev)
        count = torch.zeros(self.n_cells, dtype=torch.int32, device=dev)
        carved = torch.zeros(self.n_cells, dtype=torch.bool, device=dev)
        for first in range(0, self.n_cells, 1 << 18):
            run = slice(first, min(first + (1 << 18), self.n_cells))
            c = torch.arange(run.start, run.stop, dtype=torch.int64, device=dev)
            idx = torch.stack([c // (ry * rz), (c // rz) % ry, c % rz], -1)
            p = lo + (idx[:, None, :] + offs[None, :, :]).to(torch.float32) * width         # [cells, 8, 3]: one multiplication, one addition
            for v in range(cams.shape[0]):
                cam = cams[v]
                d0, d1, d2 = p[..., 0] - cam[3], p[..., 1] - cam[7], p[..., 2] - cam[11]
                x = d0 * cam[0] + d1 * cam[4] + d2 * cam[8]                 # (added left to right)
                y = d0 * cam[1] + d1 * cam[5] + d2 * cam[9]
                s = -(d0 * cam[2] + d1 * cam[6] + d2 * cam[10])
                fx, fy, cx, cy = cam[12], cam[13], cam[14], cam[15]
                fxx, fyy = fx * x, fy * y
                tests = (s >= near_m, s <= far_m, fxx >= (-m - cx) * s, fxx <= (w_hi - cx) * s, -fyy >= (-m - cy) * s, -fyy <= (h_hi - cy) * s)
                unseen = torch.stack([(~t).all(-1) for t in tests], -1).any(-1)      # all eight corners fail one and the same test
                count[run] += (~unseen).to(torch.int32)
                if sat is None:
                    continue
                pi, pj = fxx / s + cx, cy - fyy / s
                ok = (s >= near_m).all(-1) & torch.isfinite(pi).all(-1) & torch.isfinite(pj).all(-1)
                i0, i1 = torch.floor(pi.amin(-1) - m), torch.ceil(pi.amax(-1) + m)
                j0, j1 = torch.floor(pj.amin(-1) - m), torch.ceil(pj.amax(-1) + m)
                ok = ok & (i0 >= 0) & (i1 <= float(W - 1)) & (j0 >= 0) & (j1 <= float(H - 1))       # else the camera abstains
                i0, i1, j0, j1 = (torch.where(ok, t, torch.zeros_like(t)).to(torch.int64) for t in (i0, i1, j0, j1))
                t = sat[v]
                n = t[j1 + 1, i1 + 1] - t[j0, i1 + 1] - t[j1 + 1, i0] + t[j0, i0]
                carved[run] |= ok & (n == 0)
        return count, carved

    def view_counts_reference(self, c2w, H, W, K, near, far, margin_px=0.5):
        """The definition of "seen by a camera", in plain torch (on c2w's device): int32 [Rx, Ry, Rz], the number of the cameras c2w
        [V, 3, 4] -- columns right, up, back, position, the convention of get_rays: pixel (i, j) looks along ((i - cx) / fx,
        -(j - cy) / fy, -1) rotated by c2w[:3, :3] -- with intrinsics K ([3, 3] or [V, 3, 3]) and H x W pixels that see each cell
        between the depths near and far.  WORLD SPACE ONLY: a grid used with ndc=True rays lives in NDC space, where a camera's frustum
        is not this one; such a grid is not supported here.

        Corner o in {0, 1}^3 of cell (ix, iy, iz) is lo + fp32(i + o) * width in fp32, one multiplication and one addition per axis,
        width = fp32((hi - lo) / R) computed once in float64 (as scale is).  In camera v, with d = p - c2w[:, 3]: x = d . c2w[:, 0],
        y = d . c2w[:, 1], s = -(d . c2w[:, 2]), each three products added left to right in fp32; s is the depth z that render() samples.
        Six inside-tests per corner, m = margin_px:
            s >= near_m        s <= far_m
            fx x >= (-m - cx) s        fx x <= ((W - 1 + m) - cx) s
            -(fy y) >= (-m - cy) s     -(fy y) <= ((H - 1 + m) - cy) s
        near_m = fp32(near (1 - 2^-10)), far_m = fp32(far (1 + 2^-10)) (computed in float64): a slack far above the rounding of a sample
        point o + d z and far below a cell.  The cell is UNSEEN by v only if all eight corners fail one and the same test.  Every test
        is a half-space and a cell is convex, so a cell whose corners all lie outside one of them has no point inside the frustum:
        the test errs only towards "seen".  They are written as inside-tests so that a NaN pose or corner fails all six: a NaN camera
        sees nothing."""
        count, _ = self._views_reference("OccupancyGrid.view_counts_reference", c2w, H, W, K, near, far, margin_px, None)
        return count.view(self.resolution)

    def carved_reference(self, c2w, H, W, K, near, far, masks, margin_px=0.5):
        """The definition of the visual hull's complement, in plain torch (on c2w's device): bool [Rx, Ry, Rz], the cells that some camera
        carves.  masks: bool [V, H, W], True meaning foreground (a silhouette: alpha > 0); the rest as ``view_counts_reference``.

        Camera v carves a cell iff all eight corners have s >= near_m, every i = fx x / s + cx and j = cy - fy y / s (IEEE division) is
        finite, the pixel rectangle i0 = floor(min i - m) .. i1 = ceil(max i + m), j0 .. j1 likewise, lies inside [0, W - 1] x
        [0, H - 1] -- otherwise the camera abstains: what it cannot see whole it does not judge -- and the rectangle holds no foreground
        pixel.  That count is read from a summed-area table, sat int32 [V, H + 1, W + 1] built with cumsum:
        sat[j1 + 1, i1 + 1] - sat[j0, i1 + 1] - sat[j1 + 1, i0] + sat[j0, i0].
        With all s > 0 the projection of the cell is the hull of its projected corners, which the rectangle contains with m pixels to
        spare: no foreground pixel's ray of camera v crosses a cell that v carves, whatever the object is."""
        if masks is None:
            raise ValueError("OccupancyGrid.carved_reference: masks bool [V, H, W] are required")
        _, carved = self._views_reference("OccupancyGrid.carved_reference", c2w, H, W, K, near, far, margin_px, masks)
        return carved.view(self.resolution)

    @staticmethod
    def _check_min_views(min_views, who):
        if isinstance(min_views, bool) or not isinstance(min_views, (int, np.integer)) or int(min_views) < 1:
            raise ValueError(f"{who}: min_views must be an int >= 1, got {min_views!r}")
        return int(min_views)

    def views_keep_reference(self, c2w, H, W, K, near, far, masks=None, min_views=1, margin_px=0.5):
        """bool [Rx, Ry, Rz]: keep = (view count >= min_views) & ~carved -- with masks None the visibility alone.  What ``from_views`` and
        ``DensityGrid.restrict_to_views`` put into a grid, by the two definitions above."""
        min_views = self._check_min_views(min_views, "OccupancyGrid.views_keep_reference")
        count, carved = self._views_reference("OccupancyGrid.views_keep_reference", c2w, H, W, K, near, far, margin_px, masks)
        return ((count >= min_views) & ~carved).view(self.resolution)

    def _views_kernel(self, who, c2w, H, W, K, near, far, margin_px, masks):
        """(seen int32 [n_cells], carved words int32 or None) on the grid's device (nerf_occ_view_carve), the views fed in chunks whose
        summed-area tables stay under _SAT_BYTES"""
        desc = self._desc()
        dev = self.device
        cams, H, W, near_m, far_m, m, masks = _view_inputs(who, c2w, H, W, K, near, far, margin_px, masks)
        V = cams.shape[0]
        chunk = V if masks is None else max(1, _SAT_BYTES // (4 * (H + 1) * (W + 1)))
        seen = torch.empty(self.n_cells, dtype=torch.int32, device=dev)
        carved = None if masks is None else torch.empty_like(self.bits)
        with torch.no_grad():
            cams = cams.to(dev)
            for v0 in range(0, V, chunk):
                sat = None if masks is None else _mask_sat(masks[v0:v0 + chunk].to(dev)).contiguous()
                hb.occ_view_carve(desc, self.width, cams[v0:v0 + chunk].contiguous(), H, W, near_m, far_m, m, sat, seen, carved, accumulate=v0 > 0)
        return seen, carved

    def view_counts(self, c2w, H, W, K, near, far, margin_px=0.5):
        """int32 [Rx, Ry, Rz] on the GPU (nerf_occ_view_carve): ``view_counts_reference`` bit for bit"""
        return self._views_kernel("OccupancyGrid.view_counts", c2w, H, W, K, near, far, margin_px, None)[0].view(self.resolution)

    def carved(self, c2w, H, W, K, near, far, masks, margin_px=0.5):
        """bool [Rx, Ry, Rz] on the GPU (nerf_occ_view_carve): ``carved_reference`` bit for bit"""
        if masks is None:
            raise ValueError("OccupancyGrid.carved: masks bool [V, H, W] are required")
        words = self._views_kernel("OccupancyGrid.carved", c2w, H, W, K, near, far, margin_px, masks)[1]
        return _unpack_bits(words, self.n_cells).view(self.resolution)

    def _views_keep_words(self, who, c2w, H, W, K, near, far, masks, min_views, margin_px, dilate):
        """the bit words of ``views_keep_reference`` on the GPU, then `dilate` rounds of the 3x3x3 OR"""
        min_views = self._check_min_views(min_views, who)
        if isinstance(dilate, bool) or int(dilate) < 0:
            raise ValueError(f"{who}: dilate >= 0")
        seen, carved = self._views_kernel(who, c2w, H, W, K, near, far, margin_px, masks)
        with torch.no_grad():
            words = hb.occ_mark(seen.to(torch.float32), 1, min_views - 0.5, torch.empty_like(self.bits))       # count > min_views - 1/2
            if carved is not None:
                words = words & ~carved
            for _ in range(int(dilate)):
                words = hb.occ_dilate(words, self.resolution)
        return words

    @classmethod
    def from_views(cls, c2w, H, W, K, near, far, lo, hi, resolution, masks=None, min_views=1, margin_px=0.5, dilate=0, outside="evaluate",
                   device=None):
        """Grid of a set of training cameras, before any network exists: cell c is occupied iff at least min_views cameras see it
        (``view_counts_reference``) and, with silhouette masks, no camera carves it (``carved_reference``: the visual hull); then `dilate`
        rounds of the 3x3x3 OR.  A cell no training camera sees is never supervised, and a cell outside the hull is empty whatever the
        network says.  The grid lives on the GPU (the cells are projected by nerf_occ_view_carve); world space only.  (A DensityGrid
        recomputes its bits on every update: there the same cells are a restriction, DensityGrid.restrict_to_views.)"""
        g = cls(lo, hi, resolution, outside, device)
        g.bits = g._views_keep_words("OccupancyGrid.from_views", c2w, H, W, K, near, far, masks, min_views, margin_px, dilate)
        return g

    def _keep_words(self, keep, who):
        """the bit words, on this grid's device, of a restriction given as a grid of the same box and resolution or as bool [Rx, Ry, Rz]"""
        if isinstance(keep, OccupancyGrid):
            if keep.resolution != self.resolution or not (np.array_equal(keep.lo, self.lo) and np.array_equal(keep.hi, self.hi)):
                raise ValueError(f"{who}: the restricting grid must have this grid's box and resolution")
            return keep.bits.to(self.device).clone()
        keep = torch.as_tensor(keep)
        if keep.dtype != torch.bool or tuple(keep.shape) != self.resolution:
            raise ValueError(f"{who}: keep must be an OccupancyGrid or bool [Rx, Ry, Rz] = {self.resolution}, got {keep.dtype} {tuple(keep.shape)}")
        return _pack_bits(keep.to(self.device).reshape(-1))

    def restrict(self, keep):
        """bits &= keep, once: keep is an OccupancyGrid of the same box and resolution (``from_views``' for instance) or bool
        [Rx, Ry, Rz].  Returns self.  (A DensityGrid remembers the restriction: DensityGrid.restrict.)"""
        if keep is None:
            raise ValueError("OccupancyGrid.restrict: a plain grid keeps no restriction that could be removed")
        self.bits = self.bits & self._keep_words(keep, "OccupancyGrid.restrict")
        return self

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        return {"lo": torch.tensor(self.lo), "hi": torch.tensor(self.hi), "resolution": torch.tensor(self.resolution, dtype=torch.int64),
                "outside": self.outside, "bits": self.bits.detach().cpu().clone()}

    def load_state_dict(self, state):
        res = _res3(tuple(int(v) for v in state["resolution"]))
        bits = torch.as_tensor(state["bits"]).to(torch.int32)
        if bits.numel() != (res[0] * res[1] * res[2] + 31) // 32:
            raise ValueError("OccupancyGrid.load_state_dict: `bits` does not match `resolution`")
        if state["outside"] not in _OUTSIDE:
            raise ValueError(f"OccupancyGrid.load_state_dict: outside must be one of {_OUTSIDE}")
        self.resolution, self.outside = res, state["outside"]
        self._set_box(state["lo"], state["hi"])
        self.bits = bits.to(self.device).contiguous().clone()
        return self

    # ------------------------------------------------------------------ building a grid from a trained network
    def cell_points(self, first, last, samples_per_cell=1, generator=None):
        """[last - first, K, 3] fp32 on the grid's device: sample 0 of every cell first <= c < last is its centre, the other K - 1 are
        uniform in the cell (drawn from `generator`)"""
        dev = self.device
        rx, ry, rz = self.resolution
        c = torch.arange(first, last, dtype=torch.int64, device=dev)
        idx = torch.stack([c // (ry * rz), (c // rz) % ry, c % rz], -1).to(torch.float64)
        K = int(samples_per_cell)
        off = torch.full((c.numel(), K, 3), 0.5, dtype=torch.float64, device=dev)
        if K > 1:
            gdev = generator.device if generator is not None else dev
            off[:, 1:] = torch.rand((c.numel(), K - 1, 3), generator=generator, device=gdev, dtype=torch.float64).to(dev)
        lo = torch.tensor(self.lo.astype(np.float64), device=dev)
        width = torch.tensor((self.hi.astype(np.float64) - self.lo.astype(np.float64)) / np.asarray(self.resolution, dtype=np.float64), device=dev)
        return (lo + (idx[:, None, :] + off) * width).to(torch.float32)

    @classmethod
    def from_network(cls, model, lo, hi, resolution, sigma_threshold=0.0, samples_per_cell=1, dilate=1, generator=None):
        """Grid of a trained network: cell c is occupied iff raw[..., 3] (the density before the ReLU) exceeds sigma_threshold at the
        cell's centre or at one of samples_per_cell - 1 uniform points in the cell; then `dilate` rounds of the 3x3x3 OR (a margin of
        one cell per round for what the point samples miss).  The network is evaluated through query_points in slices, with one fixed
        view direction (the density does not depend on it: run_nerf_helpers.py:107-108).  Pass the network that renders the final image
        (network_fine) -- or OR two grids' masks.  Fused NeRF modules only."""
        from .field import NeRF
        from .render import query_points
        if not isinstance(model, NeRF):
            raise NotImplementedError("OccupancyGrid.from_network: a fused-kernel NeRF module is required (not a DenseNeRF / other module)")
        dev = next(model.parameters()).device
        g = cls(lo, hi, resolution, device=dev)
        K = int(samples_per_cell)
        if K < 1 or dilate < 0:
            raise ValueError("OccupancyGrid.from_network: samples_per_cell >= 1 and dilate >= 0")
        bits = torch.empty_like(g.bits)
        with torch.no_grad():
            for first in range(0, g.n_cells, _SLICE_CELLS):
                last = min(first + _SLICE_CELLS, g.n_cells)
                pts = g.cell_points(first, last, K, generator).reshape(-1, 3)
                vd = torch.tensor([0.0, 0.0, 1.0], device=dev).expand(pts.shape[0], 3)
                sigma = query_points(model, pts, vd)[:, 3].contiguous()
                hb.occ_mark(sigma, K, sigma_threshold, bits[first // 32:(last + 31) // 32])
            for _ in range(int(dilate)):
                bits = hb.occ_dilate(bits, g.resolution)
        g.bits = bits
        return g

    # ------------------------------------------------------------------ what render_rays calls
    def _desc(self):
        if not self.bits.is_cuda:
            raise hb.NerfHipError("OccupancyGrid: rendering needs the grid on the GPU (grid.to(device))")
        return hb.occ_desc(self.lo, self.scale, self.resolution, self.outside == "skip", self.bits)


class DensityGrid(OccupancyGrid):
    """The grid that follows a network in training: next to ``bits`` (all ones at first) one fp32 value per cell, ``density`` [n_cells]
    (zeros at first), a decayed running maximum of raw[..., 3] (the density before the ReLU).

    ``update(model)`` visits a run of cells: density[c] = max(density[c] * decay, max_k sigma_k) with sigma_k the network's density at
    the cell's centre (and samples_per_cell - 1 uniform points in it); then, over the WHOLE grid, bits = `dilate` rounds of the 3x3x3 OR
    of (density > sigma_threshold) -- recomputed from ``density`` every time, so the dilation never accumulates.
    ``maybe_update(model, global_step)`` is the schedule of a training loop: nothing while global_step < warmup_steps (the grid stays
    all-occupied: it must not hide geometry the network has not learnt yet), afterwards an update every `update_every` steps.

    The defaults (decay 0.95, sigma_threshold 0.01, update_every 16, warmup_steps 256) are Instant-NGP's habits, not measurements made
    with these networks: the threshold in particular is in the units of the scene's density and wants a look at ``fraction_occupied()``
    -- or at ``extract_mesh()``, the surface density = sigma_threshold of the grid's own densities (mesh.py).
    ``_update_reference`` / ``_bits_reference`` are the definition of the step in plain torch, as ``occupied()`` is the classifier's.

    The densities have a second reader: render_rays(..., occupancy=grid, proposal="grid") draws its importance samples from the
    compositing weights of ``proposal_sigma`` at the coarse depths (``proposal_weights``) and evaluates one network only.
    And a third: ``march_stop`` is ``march`` that adds the densities up as it walks and stops emitting where the grid's own
    transmittance has fallen to eps (``march_stop_reference`` is the definition) -- render_rays(proposal="march", march_stop_eps=eps);
    ``march_step_stop`` is the same rule on the world-space march (``march_step_stop_reference``).

    ``restrict(keep)`` / ``restrict_to_views(cameras, silhouettes)`` cap the grid from outside: ``keep`` (bit words, None at first) is
    ANDed into the bits now and after every update, so a cell no training camera sees, or one outside the visual hull, is never
    occupied whatever density the network reports there -- and during the warm-up the grid is the hull instead of all-occupied.  A grid
    without a restriction runs exactly the launches it ran before there was one."""

    def __init__(self, lo, hi, resolution, outside="evaluate", device=None, decay=0.95, sigma_threshold=0.01, dilate=0, update_every=16,
                 warmup_steps=256):
        super().__init__(lo, hi, resolution, outside, device)
        if not (0.0 <= float(decay) <= 1.0) or int(dilate) < 0 or int(update_every) < 1 or int(warmup_steps) < 0:
            raise ValueError("DensityGrid: 0 <= decay <= 1, dilate >= 0, update_every >= 1, warmup_steps >= 0")
        self.decay, self.sigma_threshold = float(decay), float(sigma_threshold)
        self.dilate, self.update_every, self.warmup_steps = int(dilate), int(update_every), int(warmup_steps)
        self.density = torch.zeros(self.n_cells, dtype=torch.float32, device=self.bits.device)
        self.cursor = 0             # first cell of the next update's run (a multiple of 32: runs are whole words)
        self.n_updates = 0
        self.keep = None            # the restriction: int32 bit words ANDed into `bits`, or None

    def to(self, device):
        super().to(device)
        self.density = self.density.to(device)
        if self.keep is not None:
            self.keep = self.keep.to(device)
        return self

    # ------------------------------------------------------------------ the definition (plain torch, any device)
    def _update_reference(self, sigma, first, last):
        """the density step for the cells first <= c < last from sigma [(last - first) * K] (cell-major): m = max_k sigma_k, a NaN
        counting as -inf; density[c] = m if m > density[c] * decay else density[c] * decay (one fp32 multiplication, one maximum)"""
        sigma = sigma.to(device=self.density.device, dtype=torch.float32).reshape(last - first, -1)
        m = torch.where(torch.isnan(sigma), torch.full_like(sigma, float("-inf")), sigma).amax(-1)
        d = self.density[first:last] * torch.tensor(self.decay, dtype=torch.float32, device=self.density.device)
        self.density[first:last] = torch.where(m > d, m, d)

    def _density_bits_reference(self):
        """bits of the whole grid from ``density`` alone: dilate^dilate(density > sigma_threshold)"""
        mask = (self.density > torch.tensor(self.sigma_threshold, dtype=torch.float32, device=self.density.device)).view(self.resolution)
        for _ in range(self.dilate):
            mask = torch.nn.functional.max_pool3d(mask[None, None].float(), 3, 1, 1)[0, 0] > 0
        return _pack_bits(mask.reshape(-1))

    def _bits_reference(self):
        """bits of the whole grid after an update: those of ``density``, ANDed with ``keep`` where one is set"""
        bits = self._density_bits_reference()
        return bits if self.keep is None else bits & self.keep.to(bits.device)

    def _next_runs(self, fraction):
        """the cells one update visits, as [(first, last)] (two runs when the visit wraps), and the cursor moved past them: `fraction`
        of the grid's words, rounded up, from the cursor on; the first update of a grid's life visits every cell (an unvisited cell has
        density 0 and would be emptied)"""
        n_words = self.bits.numel()
        if not (0.0 < float(fraction) <= 1.0):
            raise ValueError("DensityGrid.update: 0 < fraction <= 1")
        if self.n_updates == 0:
            count = n_words
        else:
            count = min(n_words, max(1, math.ceil(float(fraction) * n_words)))
        w0 = self.cursor // 32
        runs = [(w0, min(w0 + count, n_words))]
        if w0 + count > n_words:
            runs.append((0, w0 + count - n_words))
        self.cursor = 32 * ((w0 + count) % n_words)
        self.n_updates += 1
        return [(32 * a, min(32 * b, self.n_cells)) for a, b in runs]

    # ------------------------------------------------------------------ following a network
    def update(self, model, fraction=1.0, samples_per_cell=1, generator=None):
        """one density step over `fraction` of the grid (a contiguous run of words from the cursor on, wrapping; everything on the first
        call), then the bits of the whole grid.  The network is evaluated through query_points under no_grad in slices, with one fixed
        view direction, exactly as OccupancyGrid.from_network does; fused NeRF modules only.  Returns self."""
        from .field import NeRF
        from .render import query_points
        if not isinstance(model, NeRF):
            raise NotImplementedError("DensityGrid.update: a fused-kernel NeRF module is required (not a DenseNeRF / other module)")
        if not self.bits.is_cuda:
            raise hb.NerfHipError("DensityGrid.update: the grid must be on the GPU (grid.to(device))")
        K = int(samples_per_cell)
        if K < 1:
            raise ValueError("DensityGrid.update: samples_per_cell >= 1")
        dev = self.device
        with torch.no_grad():
            for run_first, run_last in self._next_runs(fraction):
                for first in range(run_first, run_last, _SLICE_CELLS):
                    last = min(first + _SLICE_CELLS, run_last)
                    pts = self.cell_points(first, last, K, generator).reshape(-1, 3)
                    vd = torch.tensor([0.0, 0.0, 1.0], device=dev).expand(pts.shape[0], 3)
                    sigma = query_points(model, pts, vd)[:, 3].contiguous()
                    hb.occ_density_update(sigma, K, self.decay, self.density[first:last])
            bits = self._density_bits()
            if self.keep is not None:       # after thresholding and dilation: the restriction survives every update
                bits = bits & self.keep
        self.bits = bits
        return self

    def _density_bits(self):
        """``_density_bits_reference`` on the GPU: nerf_occ_mark, then `dilate` rounds of nerf_occ_dilate"""
        with torch.no_grad():
            bits = hb.occ_mark(self.density, 1, self.sigma_threshold, torch.empty_like(self.bits))
            for _ in range(self.dilate):
                bits = hb.occ_dilate(bits, self.resolution)
        return bits

    # ------------------------------------------------------------------ the restriction
    def _unrestricted_bits(self):
        """the bits this grid would hold without a restriction: all ones before its first update, afterwards those of ``density``"""
        if self.n_updates == 0:
            return _pack_bits(torch.ones(self.n_cells, dtype=torch.bool, device=self.device))
        return self._density_bits() if self.bits.is_cuda else self._density_bits_reference()

    def restrict(self, keep):
        """Cap the grid: ``keep`` -- an OccupancyGrid of the same box and resolution, or bool [Rx, Ry, Rz] -- is stored as ``self.keep``
        (int32 bit words on the grid's device) and ANDed into ``bits`` now; ``update()`` ANDs it in after thresholding and dilation
        (``_bits_reference()`` does the same), so the restriction survives every update and holds during the warm-up.  A second
        restriction replaces the first.  ``restrict(None)`` removes it: the bits are again what the grid's own state gives -- all ones
        before the first update, those of ``density`` afterwards.  Returns self."""
        return self._set_keep(None if keep is None else self._keep_words(keep, "DensityGrid.restrict"))

    def _set_keep(self, words):
        had, self.keep = self.keep is not None, words
        if had:                     # the bits without the restriction they carry
            self.bits = self._unrestricted_bits()
        if words is not None:
            self.bits = self.bits & words
        return self

    def restrict_to_views(self, c2w, H, W, K, near, far, masks=None, min_views=1, margin_px=0.5, dilate=0):
        """``restrict`` to what the training cameras see and, with silhouette masks, to their visual hull -- OccupancyGrid.from_views'
        cells for this grid's box and resolution, computed on the GPU (nerf_occ_view_carve).  Called once, before step 0: the grid path
        then skips empty space from the first step instead of after the warm-up, and ``update()`` can never turn on a cell that no
        camera supervises.  World space only.  Returns self."""
        return self._set_keep(self._views_keep_words("DensityGrid.restrict_to_views", c2w, H, W, K, near, far, masks, min_views, margin_px,
                                                     dilate))

    def maybe_update(self, model, global_step, **kw):
        """the training loop's call, once per step: False (nothing done) while global_step < warmup_steps or when global_step is no
        multiple of update_every, else update(model, **kw) and True"""
        if global_step < self.warmup_steps or global_step % self.update_every != 0:
            return False
        self.update(model, **kw)
        return True

    # ------------------------------------------------------------------ the grid's own surface
    def extract_mesh(self, level=None):
        """(vertices fp32 [V, 3], faces int32 [F, 3]): the surface density = level (default: sigma_threshold) of the grid's own ``density``,
        taken as values at the cell centres -- mesh.extract_mesh on the lattice of `resolution` nodes from lo + width / 2 to
        hi - width / 2 (fp32).  At sigma_threshold that is the boundary of what the grid path evaluates, before dilation and
        restriction.  A preview that costs no network evaluation; the grid is not changed.  Needs the grid on the GPU and at least 2
        cells per axis."""
        from .mesh import extract_mesh
        half = np.float32(0.5) * self.width
        return extract_mesh(self.density.view(self.resolution), self.sigma_threshold if level is None else level, self.lo + half,
                            self.hi - half)

    # ------------------------------------------------------------------ importance samples from the grid
    def outside_sigma(self):
        """the density of a point outside the box: sigma_threshold -- the least density the grid calls occupied -- with
        outside="evaluate", 0 with outside="skip" (``proposal_sigma``; the kernels take it as their outside_sigma argument)"""
        return self.sigma_threshold if self.outside == "evaluate" else 0.0

    def proposal_sigma(self, pts):
        """fp32 [...] for pts [..., 3] (any device): the density render_rays(proposal="grid") composites at a sample point, the
        definition nerf_occ_proposal_weights reproduces bit for bit (as ``occupied()`` is the classifier's).  The point is classified
        exactly as ``occupied()`` does; inside the box it is density[c] where the cell's bit is set and 0 where it is clear; outside
        the box (a NaN included) it is 0 with outside="skip" and fp32(sigma_threshold) with outside="evaluate" -- the least density
        the grid calls occupied, so the grid still never hides what it does not cover.  No interpolation."""
        inside, c, bit = self._classify(pts)
        density = self.density if self.density.device == pts.device else self.density.to(pts.device)
        zero = torch.zeros((), dtype=torch.float32, device=pts.device)
        out = torch.tensor(self.outside_sigma(), dtype=torch.float32, device=pts.device)
        return torch.where(inside, torch.where(bit, density[c], zero), out)

    def proposal_weights(self, rays, z_vals, want_sigma=False):
        """fp32 [N, S] for rays [N, >= 6] / z_vals [N, S] on the GPU (nerf_occ_proposal_weights): the compositing weights of the samples
        o + d z with ``proposal_sigma`` as their density -- bit for bit the weights raw2outputs gives for raw = (0, 0, 0, sigma) without
        noise.  A grid that was never updated has density 0 everywhere: every sample inside the box has a weight of exactly 0, which
        sample_pdf's 1e-5 floor turns into a uniform pdf.  Constants of the graph (computed without gradients from detached values).  want_sigma: (weights, sigma)."""
        with torch.no_grad():
            w, sigma = hb.occ_proposal_weights(self._desc(), self.density, self.outside_sigma(), rays.detach().to(torch.float32).contiguous(),
                                               z_vals.detach().to(torch.float32).contiguous(), want_sigma)
        return (w, sigma) if want_sigma else w

    # ------------------------------------------------------------------ the march that stops on the grid's own transmittance
    def march_stop_reference(self, rays, u, n_steps, n_slots, eps):
        """The definition of the depths of render_rays(proposal="march", march_stop_eps=eps), in plain torch (any device): rays
        [N, >= 8], u fp32 [N] or None -> (z_vals fp32 [N, S], z_stop fp32 [N], truncated bool [N], stopped bool [N]).

        ``march_reference`` with one more rule.  The candidates k = 0 .. M - 1, t_k, z_k, keep_k and close_k are exactly its own (an
        invalid ray keeps nothing).  Density of a candidate: sigma_k = proposal_sigma(o + d * z_k) at the same fp32 point, taken where
        sigma_k > 0, else 0 (a NaN counts as 0).  Its optical depth: c_k = sigma_k * ((z_{k+1} - z_k) * |d|) where keep_k holds and
        exactly 0 elsewhere; z_{k+1} comes from t_{k+1} = (fp32(k + 1) + u) / fp32(M) by z_k's expression and is `far` for k = M - 1;
        |d| = sqrt(dx dx + dy dy + dz dz), added left to right -- nerf_occ_proposal_weights' order of operations, no contraction: the
        interval the compositing gives an evaluated marched sample, whose next slot is always the next candidate.
        A_k is the exclusive prefix sum of c in fp32 in a FIXED order that is part of the definition: rounds of 64 candidates (k0 = 0,
        64, ...; lanes with k >= M contribute 0); inside a round the inclusive scan for d = 1, 2, 4, 8, 16, 32 in which every lane
        l >= d adds the previous step's value of lane l - d; A_k = base + incl_{l-1} (0 is added for lane 0); base starts at 0 and
        grows by incl_63 after each round.
        tau = fp32(-ln(float64(eps))); k_stop = the first k with A_k >= tau (a NaN never satisfies this: a poisoned sum never stops).
        The emitted candidates are those with (keep_k or close_k) and k < k_stop, E of them.  E > S - 1: the ray is truncated exactly
        as in march_reference and stopped = False -- the slot limit bit first.  Else, with a k_stop: z_stop = z_{k_stop}, stopped =
        True, slots E .. S - 1 hold z_stop.  Else everything is march_reference's.  Invalid rays: row = own far, z_stop = -inf, neither
        flag.

        A only grows at kept candidates, so k_stop - 1 is always a kept candidate, and its interval ends exactly at z_stop, as every
        marched sample's does.  A grid that was never updated (density == 0) never stops: z_vals, z_stop and truncated then equal
        march_reference's bit for bit."""
        r, ok, uu, dn, M, S = self._march_rays("march_stop_reference", rays, u, n_steps, n_slots)
        tau = torch.tensor(hb.march_stop_threshold(_check_march_eps(eps, "march_stop_reference")), dtype=torch.float32, device=rays.device)
        return self._march_walk(r, ok, *self._equal_steps(r, ok, uu, M), S, dn, tau)

    def march_stop(self, rays, n_steps, n_slots, eps, u=None):
        """(z_vals fp32 [N, n_slots], z_stop fp32 [N], truncated bool [N], stopped bool [N]) for rays [N, >= 8] on the GPU
        (nerf_occ_march_stop): ``march_stop_reference`` bit for bit.  Constants of the graph (computed without gradients from detached
        values, like ``march``)."""
        rays, u, M, S = _march_inputs("DensityGrid.march_stop", rays, n_steps, n_slots, u)
        eps = _check_march_eps(eps, "DensityGrid.march_stop")
        with torch.no_grad():
            z_vals, z_stop, truncated, stopped = hb.occ_march_stop(self._desc(), self.density, self.outside_sigma(), rays, u, M, S, eps)
        return z_vals, z_stop, truncated.bool(), stopped.bool()

    # ------------------------------------------------------------------ the world-space march with the stop
    def march_step_stop_reference(self, rays, u, step_size, n_steps, n_slots, eps, fit=0):
        """The definition of the depths of render_rays(proposal="march", march_step_size=ds, march_stop_eps=eps, march_fit=J), in plain
        torch (any device): ``march_step_reference``'s outputs plus stopped bool [N].

        Every level of ``march_step_reference`` also applies ``march_stop_reference``'s rule unchanged: c_k = max(sigma_k, 0) *
        ((z_{k+1} - z_k) * dn) at kept candidates, z_{k+1} = far where candidate k + 1 is not valid; the exclusive prefix sum A in the
        fixed wave order (rounds of 64, the Hillis-Steele inclusive scan over d = 1 .. 32, a running base); k_stop = the first valid k
        with A_k >= tau; emission is cut at k_stop; the slot limit bites first.  The level is the smallest at which the ray is not
        truncated, so a stop can spare a ray a doubling.  With an all-zero density the first four outputs are march_step_reference's and
        nothing stops."""
        tau = torch.tensor(hb.march_stop_threshold(_check_march_eps(eps, "march_step_stop_reference")), dtype=torch.float32, device=rays.device)
        return self._march_step_levels("march_step_stop_reference", rays, u, step_size, n_steps, n_slots, fit, tau)

    def march_step_stop(self, rays, step_size, n_steps, n_slots, eps, fit=0, u=None):
        """(z_vals fp32 [N, n_slots], z_stop fp32 [N], truncated bool [N], level int32 [N], stopped bool [N]) for rays [N, >= 8] on the
        GPU (nerf_occ_march_step with the densities): ``march_step_stop_reference`` bit for bit.  Constants of the graph."""
        rays, u, M, S = _march_inputs("DensityGrid.march_step_stop", rays, n_steps, n_slots, u)
        step_size, fit = _check_march_step(step_size, fit, "DensityGrid.march_step_stop")
        eps = _check_march_eps(eps, "DensityGrid.march_step_stop")
        with torch.no_grad():
            z_vals, z_stop, truncated, level, stopped = hb.occ_march_step(
                self._desc(), self.density, self.outside_sigma(), rays, u, step_size, M, S, fit, eps)
        return z_vals, z_stop, truncated.bool(), level, stopped.bool()

    # ------------------------------------------------------------------ checkpoints
    _SCALARS = ("decay", "sigma_threshold", "dilate", "update_every", "warmup_steps")

    def state_dict(self):
        state = super().state_dict()
        state.update(density=self.density.detach().cpu().clone(), cursor=self.cursor, n_updates=self.n_updates,
                     **{k: getattr(self, k) for k in self._SCALARS})
        if self.keep is not None:       # (a grid without a restriction keeps exactly the keys it had)
            state["keep"] = self.keep.detach().cpu().clone()
        return state

    def load_state_dict(self, state):
        missing = [k for k in ("density", "cursor", "n_updates") + self._SCALARS if k not in state]
        if missing:
            raise ValueError(f"DensityGrid.load_state_dict: not a DensityGrid state (no {missing})")
        density = torch.as_tensor(state["density"]).to(torch.float32).reshape(-1)
        res = tuple(int(v) for v in state["resolution"])
        if density.numel() != res[0] * res[1] * res[2]:
            raise ValueError("DensityGrid.load_state_dict: `density` does not match `resolution`")
        if int(state["cursor"]) % 32 or not (0 <= int(state["cursor"]) < max(density.numel(), 1)):
            raise ValueError("DensityGrid.load_state_dict: `cursor` must be a multiple of 32 inside the grid")
        keep = state.get("keep")
        if keep is not None:
            keep = torch.as_tensor(keep).to(torch.int32).reshape(-1)
            if keep.numel() != (density.numel() + 31) // 32:
                raise ValueError("DensityGrid.load_state_dict: `keep` does not match `resolution`")
        super().load_state_dict(state)
        self.keep = None if keep is None else keep.to(self.device).contiguous().clone()
        self.density = density.to(self.device).contiguous().clone()
        self.cursor, self.n_updates = int(state["cursor"]), int(state["n_updates"])
        self.decay, self.sigma_threshold = float(state["decay"]), float(state["sigma_threshold"])
        self.dilate, self.update_every, self.warmup_steps = int(state["dilate"]), int(state["update_every"]), int(state["warmup_steps"])
        return self
