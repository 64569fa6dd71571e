"""Volumetric renderer host code: the reference's hot-path call surface
(run_nerf.py:27-134, :262-418; run_nerf_helpers.py:153-239) on top of the HIP
library.  Function names, argument order, defaults and returned structures are
the reference's; the bodies enqueue fused kernels instead of ATen op chains.

Random draws (stratified jitter, density noise, CDF samples) are made here with
torch, in the reference's order and shapes, and handed to the
kernels, so a seeded run consumes the generator exactly like the reference.
"""
import dataclasses
from functools import partial

import numpy as np
import torch

from . import hip_backend as hb
from . import render_options as ro
from .field import NeRF, packed_params_pair

_LINSPACE_CACHE = {}
# The datapath a user gets without asking (round 5): the fp16 three-term split -- fp32-class products (~2^-22), the configuration
# bench.py's headline measures and the north-star gate admits at 4e-6 dB.  NERF_PRECISION=fp32 (or set_precision("fp32")) selects the
# exact-fp32 anchor; the test suite runs under it unless a test names a datapath (tests/conftest.py).
DEFAULT_PRECISION = "fp16x3"
_PRECISION = __import__("os").environ.get("NERF_PRECISION", DEFAULT_PRECISION)
if _PRECISION not in hb.PRECISIONS:
    raise ValueError(f"NERF_PRECISION={_PRECISION!r}: must be one of {hb.PRECISIONS}")


def set_precision(mode):
    """Select the field datapath (hip_backend.PRECISIONS):
      "fp16x3"    (default) every product as three fp16 MFMAs, W_hi x_hi + W_hi x_lo + W_lo x_hi with hi = fp16(v), lo = fp16(v - hi):
                  ~2^-22 per product (fp32-class), fp32 accumulation / activations / gradients; the bench headline;
      "fp32"      exact fp32 MFMA (v_mfma_f32_16x16x4_f32, bitwise an fmaf chain): the parity anchor;
      "bf16x3"    the same with bf16 parts (~2^-17 per product, 8-bit operands for the weight-gradient GEMM; fp32's exponent range:
                  the datapath for activations beyond fp16's 65504);
      "fp16_fp8c" fp16x3 for everything that needs gradients; no_grad rendering on fp16 main term + fp8 correction terms (~2^-15);
      "fp16x3w"   fp16x3 whose weight-gradient GEMM contracts TWO-WORD operands (the forward and the delta chain also save the lo
                  words): gradients of the forward's product class instead of 11-bit operands, ~1.4x the step time; forward values
                  bit-identical to fp16x3's.  The instrument that prices the default's operand storage, not a default."""
    global _PRECISION
    if mode not in hb.PRECISIONS:
        raise ValueError(f"precision must be one of {hb.PRECISIONS}")
    _PRECISION = mode


def get_precision():
    return _PRECISION


def check_range():
    """The fp16 split's range guard rail on demand (hb.RangeMonitor.report): waits for the scans in flight and returns
    {"max_activation": largest post-ReLU activation a scanned training forward saved, "warn_at": 32768, "limit": 65504, ...}.
    hip_backend.RANGE_MONITOR.every (NERF_RANGE_CHECK_EVERY, default 64) = every how many training renders a scan runs; 0 = never."""
    return hb.RANGE_MONITOR.report()


def _linspace01(n, device):
    key = (n, str(device))
    t = _LINSPACE_CACHE.get(key)
    if t is None:
        t = torch.linspace(0.0, 1.0, steps=n, dtype=torch.float32, device=device)
        _LINSPACE_CACHE[key] = t
    return t


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


# --------------------------------------------------------------------------- autograd glue
_FREED_MSG = ("nerf-pytorch_amd: the saved activations of this render were already consumed by a backward pass and "
              "freed; backward through the same graph a second time is not supported (sum the losses and call "
              "backward once)")


_STALE_MSG = ("nerf-pytorch_amd: the network parameters changed between this render's forward and its backward "
              "(optimizer.step / load_state_dict / broadcast in between); the split-bf16 backward combines activations saved "
              "by the forward with the current feature_linear / views_linears weights, so the gradient would mix two "
              "parameter states.  Call backward before updating the parameters.")


# Called as hook(model, flat_grad) from inside the backward pass the moment a network's flat gradient vector is final
# (all of its kernels are enqueued on the current stream).  parallel.GradientSync uses it to start that network's
# all-reduce while the other network's backward still runs (the coarse and fine backward are independent: the
# reference detaches z_samples, run_nerf.py:394).
GRAD_READY_HOOKS = []


def _grad_ready(model, flat_grad):
    model.last_flat_grad = flat_grad
    for hook in GRAD_READY_HOOKS:
        hook(model, flat_grad)


class _FieldQuery(torch.autograd.Function):
    """raw = field(rays, z) for explicit rays/depths; gradients w.r.t. the parameters (when they require grad) and the ray
    records (when they do: nerf_field_input_grad -- query_points' points and view directions)."""

    @staticmethod
    def forward(ctx, model, rays, z_vals, need, *params):
        prec = _PRECISION
        if prec == "fp16_fp8c" and need:        # the reduced class is an inference form; gradients: the fp16x3 datapath
            prec = "fp16x3"
        packed = model.packed_params(prec)
        raw, act = hb.field_fwd(packed, rays, z_vals, save_act=need, precision=prec,
                                guard_packed=model.packed_params("fp16x3") if prec == "fp16_fp8c" else None)
        ctx.model, ctx.packed, ctx.act, ctx.prec, ctx.saved_any = model, packed, act, prec, bool(need)
        ctx.param_state = _param_state(model)
        ctx.rays_grad = bool(ctx.needs_input_grad[1])
        ctx.wgrad = any(ctx.needs_input_grad[4:])
        if ctx.rays_grad:
            ctx.rays, ctx.z = rays.detach(), z_vals
        ctx.set_materialize_grads(False)
        return raw

    @staticmethod
    def backward(ctx, d_raw):
        model = ctx.model
        if d_raw is None or not ctx.saved_any:      # nothing requires grad: forward saved nothing on purpose
            return (None, None, None, None) + (None,) * len(_param_slices(model))
        if ctx.act is None:
            raise RuntimeError(_FREED_MSG)
        if ctx.prec != "fp32" and _param_state(model) != ctx.param_state:
            raise RuntimeError(_STALE_MSG)
        grad = torch.empty(hb.N_PARAMS, dtype=torch.float32, device=d_raw.device) if ctx.wgrad else None
        d_rays = None
        if ctx.rays_grad:
            d_rays = torch.empty((ctx.rays.shape[0], 11), dtype=torch.float32, device=d_raw.device)
        hb.field_bwd(ctx.packed, ctx.act, d_raw.contiguous(), grad, accumulate=False, precision=ctx.prec,
                     params=model.flat_params(), input_grad=None if d_rays is None else (ctx.rays, ctx.z, d_rays, False))
        hb.WORKSPACE.give(ctx.act)
        ctx.act = None      # ~10 KB per point: back to the workspace pool as soon as the gradient exists
        if grad is None:
            return (None, d_rays, None, None) + (None,) * len(_param_slices(model))
        _grad_ready(model, grad)
        return (None, d_rays, None, None) + _grad_views(model, grad)


def _param_slices(model):
    from .field import _param_table
    return _param_table()


def _param_state(model):
    """Identity of the parameter values a forward saw: storage, in-place version, fused-Adam epoch."""
    flat = model.flat_params()
    return (flat.data_ptr(), flat._version, tuple(p._version for p in model.parameters()), hb.param_epoch(flat))


def _grad_views(model, flat_grad):
    return tuple(flat_grad[off:off + int(np.prod(shape))].view(shape) for _, off, shape in _param_slices(model))


def _field_pass(cfg, rays, rnd, model_c, model_f, save):
    """One evaluation of render_rays' pipeline (run_nerf.py:351-412) on `rays`: coarse depths -> field -> composite
    [-> hierarchical depths -> field -> composite].  save=True leases workspace buffers for the saved activations
    (hb.Workspace) and returns them in the dict; everything else is small ([N,S]-sized)."""
    n_c, n_f = cfg.N_samples, cfg.N_importance
    dev = rays.device
    std, wb, prec = cfg.raw_noise_std, cfg.white_bkgd, cfg.precision
    r = {}
    guard = (lambda m: m.packed_params("fp16x3")) if prec == "fp16_fp8c" else (lambda m: None)
    r["z_c"] = hb.sample_coarse(rays, _linspace01(n_c, dev), cfg.lindisp, rnd.get("t_rand"))
    mf = model_c if (model_f is None or model_f is model_c) else model_f
    nxt = raw_f = None
    # The reduced inference class with a refining pass: hierarchical sampling divides by ~1e-5 in bins the coarse pass found empty
    # (run_nerf_helpers.py:234-236), so a 2^-15 perturbation of the coarse weights moves single fine samples by whole bins -- measured
    # on the reference's fixtures at BASELINE's batch sizes: no flipped ray, but images at 62-79 dB of the reference's instead of
    # fp16x3's 89-120 dB (tools/EXPERIMENTS.md, round 5).  The coarse pass (a quarter of the points) therefore runs on the three-term
    # products and only the refining pass (whose errors reach the image unamplified) on the reduced ones.
    prec_c = "fp16x3" if (prec == "fp16_fp8c" and n_f > 0 and hb.REDUCED_COARSE_THREE_TERM) else prec
    if n_f > 0 and mf is not model_c and prec_c == prec:
        r["packed_c"], packed_f = packed_params_pair(model_c, mf, prec)       # (both stale after an optimizer step: one pair of launches)
    else:
        r["packed_c"], packed_f = model_c.packed_params(prec_c), None
    if prec_c == "fp16_fp8c" and n_f > 0:     # the guard launch of the coarse pass also evaluates the fine pass's last sample (hb.field_fwd)
        raw_f = torch.empty((rays.shape[0], n_c + n_f, 4), dtype=torch.float32, device=dev)
        nxt = (guard(mf), raw_f)
    r["raw_c"], r["act_c"] = hb.field_fwd(r["packed_c"], rays, r["z_c"], save_act=save, precision=prec_c,
                                          guard_packed=guard(model_c) if prec_c == "fp16_fp8c" else None, next_guard=nxt)
    dist = cfg.distortion     # the last pass also hands out its weights (one more store, every other output keeps its bits)
    inter = cfg.interlevel    # likewise, and the coarse weights are kept too (render_rays refuses it without a refining pass)
    r["rgb_c"], r["disp_c"], r["acc_c"], w_c, _ = hb.raw2outputs(r["raw_c"], r["z_c"], rays, rays.shape[1], rnd.get("noise_c"), std, wb,
                                                              want_weights=n_f > 0 or dist, want_depth=False, rays_d_offset=3)
    if n_f <= 0:
        if dist:
            r["w"], r["distortion"] = w_c, hb.distortion(w_c, r["z_c"], rays, nf_stride=rays.shape[1], nf_offset=6)
        return r
    u = rnd.get("u")
    r["z_f"], r["z_std"], _ = hb.sample_fine(r["z_c"], w_c, n_f, u, None if u is not None else _linspace01(n_f, dev))
    r["packed_f"] = packed_f if packed_f is not None else mf.packed_params(prec)
    r["raw_f"], r["act_f"] = hb.field_fwd(r["packed_f"], rays, r["z_f"], save_act=save, precision=prec,
                                          guard_packed="done" if raw_f is not None else guard(mf), raw=raw_f)
    r["rgb_f"], r["disp_f"], r["acc_f"], w_f, _ = hb.raw2outputs(r["raw_f"], r["z_f"], rays, rays.shape[1], rnd.get("noise_f"), std, wb,
                                                               want_weights=dist or inter, want_depth=False, rays_d_offset=3)
    if dist:
        r["w"], r["distortion"] = w_f, hb.distortion(w_f, r["z_f"], rays, nf_stride=rays.shape[1], nf_offset=6)
    if inter:       # the coarse histogram as the proposal, the refining pass's as the target
        r["w"], r["w_c"], r["interlevel"] = w_f, w_c, hb.interlevel(w_c, r["z_c"], w_f, r["z_f"])
    return r


def _release(r):
    for k in ("act_c", "act_f"):
        hb.WORKSPACE.give(r.get(k))
        r[k] = None


# how the last training render_rays call kept its backward state: ("one launch" | "resident sub-chunks" | "recompute", rays, rays per
# sub-chunk) -- benchmarks read it to report (and refuse to mislabel) the recompute fallback
LAST_BACKWARD_PLAN = None


# ---- what _RenderRays and _RenderRaysGrid share: sub-chunking, the forward's bookkeeping, and ONE backward (_backward) over pass records.
# A pass record is a dict: z, raw, packed, act, w (the pass's compositing weights where the forward kept them; cfg.distortion /
# cfg.interlevel), on the grid path also slot, rec, m.  _grid_pass appends it; the dense node makes it from _field_pass's dict.
def _sub_chunks(n, sub):
    """n rays in sub-chunks of at most `sub`: (rays per sub-chunk, [(lo, hi)]).  More than one: equal sub-chunks, multiples of 64 rays
    (the last one takes what is left); n <= sub: `sub` as given and the one tile."""
    if n > sub:
        ceil_div = lambda a, b: -(-a // b)
        sub = min(sub, 64 * ceil_div(ceil_div(n, ceil_div(n, sub)), 64))
    return sub, [(lo, min(lo + sub, n)) for lo in range(0, n, sub)]


def _pass_records(r):
    """_field_pass's flat dict as pass records, [coarse, fine] or [only]; the last pass's weights are r["w"], the coarse ones r["w_c"]"""
    rec = lambda s, w: {"z": r["z_" + s], "raw": r["raw_" + s], "packed": r["packed_" + s], "act": r["act_" + s], "w": r.get(w)}
    return [rec("c", "w_c"), rec("f", "w")] if "z_f" in r else [rec("c", "w")]


def _give_leases(records):
    """hand the hb.WORKSPACE leases of pass records back (give ignores None: a dense record has no slot / rec, a freed one nothing)"""
    for p in records:
        for k_ in ("slot", "act", "rec"):
            hb.WORKSPACE.give(p.get(k_))
            p[k_] = None


def _resident_tiles(tiles, rays, rnd, parts):
    """the backward's tiles (lo, hi, rays, rnd, records, last) of a forward that kept every sub-chunk's records"""
    for i, ((lo, hi), records) in enumerate(zip(tiles, parts)):
        yield lo, hi, rays[lo:hi], rnd if len(tiles) == 1 else {k_: v[lo:hi] for k_, v in rnd.items()}, records, i == len(tiles) - 1


def _keep_for_backward(ctx, cfg, rays, rnd, model_c, model_f, first_param):
    """the forward's bookkeeping for _backward; the networks' parameters are the node's inputs from `first_param` on"""
    ctx.cfg, ctx.model_c, ctx.model_f = cfg, model_c, model_f
    ctx.same_net = model_f is None or model_f is model_c
    ctx.n_params_c = len(_param_slices(model_c))
    # which gradients the backward computes: the ray records' (input-gradient kernel), each network's parameters' (weight
    # gradient; a frozen network gets none: no wgrad launch, no _grad_ready, .grad stays None)
    ctx.rays_grad = bool(ctx.needs_input_grad[1])
    ctx.wgrad_c = any(ctx.needs_input_grad[first_param:first_param + ctx.n_params_c])
    ctx.wgrad_f = ctx.wgrad_c if ctx.same_net else any(ctx.needs_input_grad[first_param + ctx.n_params_c:])
    ctx.set_materialize_grads(False)
    ctx.rays, ctx.rnd = rays.detach(), rnd
    # the folded feature layer of the split datapaths' backward reads the LIVE parameters (Wf, bf, Wv) next to
    # fragments packed at forward time: remember which parameter state this forward saw
    ctx.param_state = tuple(_param_state(m) for m in (model_c, model_f) if m is not None)
    ctx.consumed = False


def _upstream(cfg, gouts, coarse_image):
    """(up_c, up_f): the upstream gradients of (rgb, disp, acc, raw, distortion, interlevel) of the coarse pass and of the fine one, None
    for a pass the call does not have.  The two losses are the trailing outputs: the distortion loss belongs to the last pass, the
    interlevel loss behind it to the coarse one.  coarse_image False (cfg.proposal: one pass, the refining one): there is no coarse image."""
    fine, inter = cfg.N_importance > 0, cfg.interlevel
    up_f = (gouts[0], gouts[1], gouts[2], gouts[3], gouts[-2 if inter else -1] if cfg.distortion else None, None)
    up_c = (gouts[4], gouts[5], gouts[6], None, None, gouts[-1] if inter else None) if fine and coarse_image else None
    if not fine:
        up_c, up_f = up_f, None
    return up_c, up_f


def _composite_adjoint(cfg, rays, p, raw, noise, up, target, rays_grad):
    """(d_raw, d_dn) of pass record p on the ray tile `rays`: the compositing backward with the losses' adjoints as its d_weights.  `up`:
    the tile's rows of the six upstream gradients (_upstream); target: the record whose (w, z) the interlevel loss fits p's weights to;
    d_dn [n, 3], the compositing's |d| term (dists = dz |d|), when the rays need a gradient and the compositing ran, else None."""
    d_rgb, d_disp, d_acc, d_raw_up, d_dist, d_inter = up
    n, dev, z = rays.shape[0], rays.device, p["z"]
    if d_rgb is None and (d_disp is not None or d_acc is not None or d_dist is not None or d_inter is not None):
        d_rgb = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    c = lambda t: t.to(torch.float32).contiguous() if t is not None else None
    if d_rgb is None:       # only `raw` itself (extras['raw'], e.g. a sigma regulariser) carries a gradient
        return c(d_raw_up), None
    d_dn = torch.empty((n, 3), dtype=torch.float32, device=dev) if rays_grad else None
    # the distortion loss reaches raw (and |d|) through the weights' adjoint: d_weights of the compositing backward
    extra = {} if d_dist is None else {"d_weights": hb.distortion_bwd(p["w"], z, rays, c(d_dist), nf_stride=rays.shape[1], nf_offset=6)}
    if d_inter is not None:     # the interlevel loss, likewise: p is the proposal, target the refining pass
        extra = {"d_weights": hb.interlevel_bwd(p["w"], z, target["w"], target["z"], c(d_inter))}
    d_raw = hb.raw2outputs_bwd(raw, z, rays, rays.shape[1], noise, cfg.raw_noise_std, cfg.white_bkgd, c(d_rgb), c(d_acc), c(d_disp),
                               rays_d_offset=3, d_rays_d=d_dn, **extra)
    if d_raw_up is not None:
        d_raw += d_raw_up
    return d_raw, d_dn


def _backward(ctx, gouts, n_lead, tiles, field_step, after_pass, release):
    """THE backward of both nodes; n_lead: the node's inputs in front of the networks' parameters.  tiles: an iterable of (lo, hi, rays, rnd, records, last), asked for one tile at a time (the dense
    node's recompute plan runs a sub-chunk's forward when its tile is asked for); field_step(record, rays, d_raw, model, grad,
    accumulate, d_rays) -> whether it wrote `grad`: the path's field backward from d_raw on; after_pass(record): the path is done with
    a pass of a tile (called for the coarse pass before the fine pass's backward, with or without an upstream gradient); release():
    nothing of the forward is needed any more.  Per tile coarse, then fine; a network's _grad_ready fires once, with the final flat
    vector, behind its last launch: after the coarse pass of the last tile -- unless the fine pass adds into the same vector --, and
    after the fine pass of the last tile."""
    if ctx.consumed:
        raise RuntimeError(_FREED_MSG)
    cfg = ctx.cfg
    none_c = (None,) * ctx.n_params_c
    none_all = (None,) * n_lead + none_c + (() if ctx.same_net else none_c)
    if not cfg.need_grad:
        return none_all
    now = tuple(_param_state(m) for m in (ctx.model_c, ctx.model_f) if m is not None)
    if cfg.precision != "fp32" and now != ctx.param_state:
        raise RuntimeError(_STALE_MSG)
    fine = cfg.N_importance > 0
    up_c, up_f = _upstream(cfg, gouts, coarse_image=cfg.proposal is None)
    has = lambda up: up is not None and any(g is not None for g in up)
    if not has(up_c) and not has(up_f):
        ctx.consumed = True
        release()
        return none_all
    dev = ctx.rays.device
    grad_c = torch.empty(hb.N_PARAMS, dtype=torch.float32, device=dev) if ctx.wgrad_c else None
    grad_f = None if (ctx.same_net or not fine or not ctx.wgrad_f) else torch.empty(hb.N_PARAMS, dtype=torch.float32, device=dev)
    wrote = {"c": False, "f": False}
    # dL/d(ray records), summed over both passes (near / far: zero -- render() builds them from Python floats)
    d_rays_all = torch.zeros((ctx.rays.shape[0], 11), dtype=torch.float32, device=dev) if ctx.rays_grad else None
    shared = ctx.same_net and fine and has(up_f)      # the fine pass adds into the coarse network's gradient
    raw_last = (ctx.saved_tensors or (None,))[0]        # one tile: the last pass's raw is an output (save_for_backward)

    def pass_grad(p, rays, noise, up, lo, hi, target, model, grad, key):
        d_rays = None if d_rays_all is None else d_rays_all[lo:hi]
        d_raw, d_dn = _composite_adjoint(cfg, rays, p, raw_last if p.get("raw") is None else p["raw"], noise,
                                         tuple(None if g is None else g[lo:hi] for g in up), target, d_rays is not None)
        if (grad is not None or d_rays is not None) and field_step(p, rays, d_raw, model, grad, wrote[key], d_rays):
            wrote[key] = True
        if d_dn is not None:
            d_rays[:, 3:6] += d_dn          # the compositing's |d| term

    for lo, hi, rays, rnd, records, last in tiles:
        if has(up_c):
            pass_grad(records[0], rays, rnd.get("noise_c"), up_c, lo, hi, records[-1], ctx.model_c, grad_c, "c")
            if last and not shared and grad_c is not None:     # final: its all-reduce may start under the fine network's backward
                _grad_ready(ctx.model_c, grad_c)
        after_pass(records[0])
        if fine and has(up_f):
            model, grad, key = (ctx.model_c, grad_c, "c") if ctx.same_net else (ctx.model_f, grad_f, "f")
            pass_grad(records[-1], rays, rnd.get("noise_f"), up_f, lo, hi, None, model, grad, key)
            if last and grad is not None:
                _grad_ready(model, grad)
        after_pass(records[-1])
    ctx.consumed = True
    release()
    lead = (None, d_rays_all) + (None,) * (n_lead - 2)
    out_c = _grad_views(ctx.model_c, grad_c) if wrote["c"] else none_c
    if ctx.same_net:
        return lead + out_c
    return lead + out_c + (_grad_views(ctx.model_f, grad_f) if wrote["f"] else none_c)


class _RenderRays(torch.autograd.Function):
    """The whole of render_rays (run_nerf.py:308-418) as one autograd node.

    Memory: the backward needs 4.8 KB of saved activations per sample point on the split datapaths (16-bit tiles; 10.7 KB of fp32
    rows on the fp32 datapath) plus as much for the deltas.  Up to hb.max_saved_rays(...) rays per call (default budget 48 GiB:
    ~22k rays at 64+128 samples on the split datapaths, ~10k on fp32, i.e. every N_rand of the BASELINE configs) they are saved by
    the forward into buffers leased from hb.WORKSPACE (persistent across steps, no per-step allocation).  Larger ray chunks (the
    reference's default chunk is 32768 rays) are rendered in equal sub-chunks.  If the saved activations of ALL sub-chunks fit
    hb.SAVE_TOTAL_BYTES (default 160 GiB of the 288 GB: the 32768-ray batch of configs[3] needs ~40 GB on the split datapaths,
    ~90 GB on fp32) every sub-chunk keeps its own lease and the backward walks them: no
    recomputation, deltas and partial sums re-use one sub-chunk-sized scratch.  Beyond that the forward runs WITHOUT
    saving and the backward re-runs it, with saving, one sub-chunk at a time (the kernels are deterministic, so the
    recomputed pass is bit-identical to the first): bounded memory for +1 inference-speed forward.

    The backward is _backward, shared with _RenderRaysGrid; the three plans are its three tile sources.  cfg.distortion: one trailing
    differentiable output, the distortion loss [N] of the last pass's weights (_field_pass), which that pass's record keeps as "w"; its
    upstream gradient enters the last pass's compositing backward as d_weights (_composite_adjoint: nerf_distortion_bwd).
    cfg.interlevel: one trailing differentiable output (behind the distortion loss), the interlevel loss [N] of the coarse pass's weights
    against the refining pass's; both records keep their "w" (the recompute plan recomputes them) and its upstream gradient enters the
    COARSE pass's compositing backward as d_weights (nerf_interlevel_bwd): it reaches model_c through the coarse pass only, and alone
    it runs no backward of the refining pass."""

    @staticmethod
    def forward(ctx, cfg, rays, rnd, model_c, model_f, *params):
        n_f = cfg.N_importance
        need = cfg.need_grad
        n = rays.shape[0]
        sub, ctx.sub_tiles = _sub_chunks(n, hb.max_saved_rays(cfg.N_samples, n_f, cfg.precision) if need else n)
        ctx.checkpoint = len(ctx.sub_tiles) > 1
        ctx.tiles = None
        if ctx.checkpoint:
            # resident sub-chunks only if they fit the budget AND what the device actually has free right now: what the driver reports
            # + the pool's idle leases LARGE ENOUGH to hold a sub-chunk's saved activations (smaller ones serve nothing) + half of
            # what torch's caching allocator holds without using (cached blocks are fragmented: only part of them can back a
            # multi-GB request).  The estimate can still be wrong: the forward below falls back to recomputation on out-of-memory.
            prec_ = cfg.precision
            lease = min(hb.act_floats(sub, cfg.N_samples, prec_), hb.act_floats(sub, cfg.N_samples + n_f, prec_) if n_f > 0 else 1 << 62)
            cached = torch.cuda.memory_reserved(rays.device) - torch.cuda.memory_allocated(rays.device)
            free_now = torch.cuda.mem_get_info(rays.device)[0] + cached // 2 + hb.WORKSPACE.idle_bytes(rays.device, lease)
            if hb.saved_bytes(sub, cfg.N_samples, n_f, prec_) * len(ctx.sub_tiles) <= min(hb.SAVE_TOTAL_BYTES, int(0.9 * free_now)):
                ctx.checkpoint = False
                ctx.tiles = ctx.sub_tiles
        global LAST_BACKWARD_PLAN
        LAST_BACKWARD_PLAN = ("recompute" if ctx.checkpoint else "resident sub-chunks" if ctx.tiles is not None else "one launch", n, sub)
        prec = cfg.precision
        dist, inter = cfg.distortion, cfg.interlevel
        if not need and not dist and not inter and hb.INFER_ONE_LAUNCH and hb.render_infer_supported(cfg.N_samples, n_f, prec):
            # no gradients: coarse depths -> network -> compositing -> hierarchical depths -> network -> compositing in ONE launch
            mf = None if (model_f is None or model_f is model_c or n_f <= 0) else model_f
            r = hb.render_rays_infer(model_c.packed_params(prec), None if mf is None else mf.packed_params(prec), rays, cfg.N_samples,
                                     n_f, cfg.lindisp, cfg.white_bkgd, cfg.raw_noise_std, prec, rnd)
        elif ctx.tiles is None:
            r = _field_pass(cfg, rays, rnd, model_c, model_f, save=need and not ctx.checkpoint)
        else:
            # every sub-chunk keeps its saved activations; the node's outputs are the concatenations (new tensors)
            parts = []
            try:
                for lo, hi in ctx.tiles:
                    parts.append(_field_pass(cfg, rays[lo:hi], {k_: v[lo:hi] for k_, v in rnd.items()}, model_c, model_f, save=True))
            except torch.cuda.OutOfMemoryError:
                # the free-memory estimate was wrong (fragmented cache, another tenant of the device): hand everything back and take
                # the recompute plan -- forward without saving, the backward re-runs it per sub-chunk (bit-identical)
                for p_ in parts:
                    _release(p_)
                parts = None
                hb.WORKSPACE.clear()
                torch.cuda.empty_cache()
                ctx.tiles, ctx.checkpoint = None, True
                LAST_BACKWARD_PLAN = ("recompute", n, sub)
            if parts is None:
                r = _field_pass(cfg, rays, rnd, model_c, model_f, save=False)
            else:
                out_keys = ("rgb_c", "disp_c", "acc_c", "raw_c") if n_f <= 0 else ("rgb_f", "disp_f", "acc_f", "raw_f", "rgb_c", "disp_c", "acc_c", "z_std")
                r = {k_: torch.cat([p_[k_] for p_ in parts], 0) for k_ in out_keys + (("distortion",) if dist else ()) + (("interlevel",) if inter else ())}
        if need and not ctx.checkpoint and hb.DATAPATHS[prec].fp16_saves:
            # the fp16 split's range guard rail: every RANGE_MONITOR.every-th training render scans what the forward saved
            # (hb.RangeMonitor; replaces run_nerf.py:414-416's DEBUG-gated NaN / Inf check)
            for r_, n_ in ([(r, n)] if ctx.tiles is None else [(p_, hi - lo) for p_, (lo, hi) in zip(parts, ctx.tiles)]):
                hb.RANGE_MONITOR.after_forward([(r_[k_], s_) for k_, s_ in (("act_c", cfg.N_samples), ("act_f", cfg.N_samples + n_f))
                                                if r_.get(k_) is not None], n_)
        # What the backward needs, WITHOUT the node's own outputs: an output carries grad_fn = this node, so keeping it
        # in ctx.__dict__ is a node -> ctx -> output -> node cycle the garbage collector cannot break (a graph dropped
        # without backward would pin its ~11 GB of saved activations for good).  The one output the backward reads,
        # `raw` of the last pass, goes through save_for_backward, which autograd knows how to hold without a cycle.
        # ctx.saved: the pass records of every tile ("w": a pass's weights under cfg.distortion / cfg.interlevel; not an output)
        ctx.saved = None
        if ctx.tiles is not None:
            ctx.saved = [_pass_records(p_) for p_ in parts]     # per-sub-chunk tensors, none is an output
        elif need and not ctx.checkpoint:
            ctx.saved = [_pass_records(r)]
            ctx.save_for_backward(ctx.saved[0][-1].pop("raw"))
        elif not need:
            _release(r)
        _keep_for_backward(ctx, cfg, rays, rnd, model_c, model_f, 5)
        tail = ((r["distortion"],) if dist else ()) + ((r["interlevel"],) if inter else ())      # trailing differentiable outputs
        if n_f <= 0:
            return (r["rgb_c"], r["disp_c"], r["acc_c"], r["raw_c"]) + tail
        ctx.mark_non_differentiable(r["z_std"])     # the reference detaches z_samples (run_nerf.py:394)
        return (r["rgb_f"], r["disp_f"], r["acc_f"], r["raw_f"], r["rgb_c"], r["disp_c"], r["acc_c"], r["z_std"]) + tail

    @staticmethod
    def backward(ctx, *gouts):
        cfg = ctx.cfg

        def recomputed():       # the recompute plan: a sub-chunk's forward runs, with saving, when _backward asks for its tile
            for lo, hi in ctx.sub_tiles:
                rays, rnd = ctx.rays[lo:hi], {k: v[lo:hi] for k, v in ctx.rnd.items()}
                yield lo, hi, rays, rnd, _pass_records(_field_pass(cfg, rays, rnd, ctx.model_c, ctx.model_f, save=True)), hi == ctx.rays.shape[0]

        def field_step(p, rays, d_raw, model, grad, accumulate, d_rays):
            hb.field_bwd(p["packed"], p["act"], d_raw, grad, accumulate, precision=cfg.precision, params=model.flat_params(),
                         input_grad=None if d_rays is None else (rays, p["z"], d_rays, True))
            return grad is not None

        def release():
            for records in ctx.saved or ():
                _give_leases(records)
            ctx.saved = None

        # (a pass's act goes back to the pool right behind that pass's backward, in front of the next pass's: a training loop finds the
        # same buffers every step)
        return _backward(ctx, gouts, 5, recomputed() if ctx.checkpoint else _resident_tiles(ctx.sub_tiles, ctx.rays, ctx.rnd, ctx.saved or ()),
                         field_step, lambda p: _give_leases([p]), release)


class _Composite(torch.autograd.Function):
    """raw2outputs with gradients w.r.t. raw, and w.r.t. z_vals / rays_d when they require grad (nerf_raw2outputs_bwd_geom)."""

    @staticmethod
    def forward(ctx, raw, z_vals, rays_d, noise, raw_noise_std, white_bkgd):
        raw, z_vals, rays_d = raw.detach(), z_vals.detach(), rays_d.detach()
        rgb, disp, acc, w, depth = hb.raw2outputs(raw, z_vals, rays_d, 3, noise, raw_noise_std, white_bkgd)
        ctx.args = (raw, z_vals, rays_d, noise, raw_noise_std, white_bkgd)
        ctx.set_materialize_grads(False)
        return rgb, disp, acc, w, depth

    @staticmethod
    def backward(ctx, d_rgb, d_disp, d_acc, d_w, d_depth):
        # all five outputs carry gradients to raw, as in the reference (a depth / weight / sparsity loss term works)
        raw, z_vals, rays_d, noise, std, wb = ctx.args
        if all(g is None for g in (d_rgb, d_disp, d_acc, d_w, d_depth)):
            return (None,) * 6
        if d_rgb is None:
            d_rgb = torch.zeros((raw.shape[0], 3), dtype=torch.float32, device=raw.device)
        c = lambda t: t.to(torch.float32).contiguous() if t is not None else None
        d_z = torch.empty_like(z_vals) if ctx.needs_input_grad[1] else None
        d_dn = torch.empty((z_vals.shape[0], 3), dtype=torch.float32, device=raw.device) if ctx.needs_input_grad[2] else None
        d_raw = hb.raw2outputs_bwd(raw, z_vals, rays_d, 3, noise, std, wb, c(d_rgb), c(d_acc), c(d_disp),
                                   d_weights=c(d_w), d_depth=c(d_depth), d_rays_d=d_dn, d_z_vals=d_z)
        return d_raw, d_z, d_dn, None, None, None


class _Distortion(torch.autograd.Function):
    """distortion_loss over nerf_distortion_fwd / _bwd: gradient to the weights only, recomputed from the inputs"""

    @staticmethod
    def forward(ctx, weights, z_vals, near_far, nf_stride):
        weights = weights.detach()
        ctx.args = (weights, z_vals, near_far, nf_stride)
        ctx.set_materialize_grads(False)
        return hb.distortion(weights, z_vals, near_far, nf_stride=nf_stride)

    @staticmethod
    def backward(ctx, d_loss):
        if d_loss is None:      # nothing upstream: no launch
            return None, None, None, None
        weights, z_vals, near_far, nf_stride = ctx.args
        return hb.distortion_bwd(weights, z_vals, near_far, d_loss.to(torch.float32).contiguous(), nf_stride=nf_stride), None, None, None


def _near_far_pair(near, far, lead, dtype, device):
    """near / far ([...] tensors or Python numbers) as two detached tensors of shape `lead`"""
    as_t = lambda v: (v.detach() if isinstance(v, torch.Tensor) else torch.as_tensor(float(v))).to(dtype=dtype, device=device)
    return as_t(near).expand(lead), as_t(far).expand(lead)


def distortion_loss(weights, z_vals, near, far):
    """The distortion loss of mip-NeRF 360 on compositing weights, per ray: [..., S] weights and depths -> [...] (two HIP launches, forward
    and adjoint; distortion_loss_reference is the definition).  With s = (z - near) / (far - near) -- 0 where far - near is not > 0: such a
    ray has loss 0 and gradient 0 --, sample i < S-1 owning [s_i, s_i+1] (mid-point m_i, length dl_i) and the last sample a zero-length
    interval at s_S-1 (its compositing distance of 1e10 is a sentinel, not a length):

        L = sum_i sum_j w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 dl_i

    ``near`` / ``far``: [...] tensors (one value per ray) or Python numbers.  Gradient to ``weights`` only: depths, near and far are
    constants of the graph, like the reference's z_samples.  THE CALLER'S CONTRACT: z_vals is non-decreasing along the last axis (what
    every path of render_rays produces); it is not checked, a check would be a host synchronisation.  1 <= S <= 4096.  Composes with
    raw2outputs, whose weights (output 3) are differentiable: distortion_loss(raw2outputs(raw, z, d)[3], z, near, far)."""
    lead, S = tuple(weights.shape[:-1]), weights.shape[-1]
    if tuple(z_vals.shape) != tuple(weights.shape):
        raise ValueError(f"distortion_loss: weights {tuple(weights.shape)} and z_vals {tuple(z_vals.shape)} differ in shape")
    w = weights.to(torch.float32).reshape(-1, S).contiguous()
    z = z_vals.detach().to(torch.float32).reshape(-1, S).contiguous()
    if isinstance(near, torch.Tensor) or isinstance(far, torch.Tensor):
        near, far = _near_far_pair(near, far, lead, torch.float32, w.device)
        near_far, stride = torch.stack([near.reshape(-1), far.reshape(-1)], -1).contiguous(), 2
    else:       # one pair for all rays
        near_far, stride = torch.tensor([float(near), float(far)], dtype=torch.float32, device=w.device), 0
    return _Distortion.apply(w, z, near_far, stride).reshape(lead)


def distortion_loss_reference(weights, z_vals, near, far):
    """THE DEFINITION distortion_loss and the render paths' "distortion" key are held to: the formulas of distortion_loss as the pairwise
    sum in plain torch, on any device, in the dtype of ``weights`` (the tests call it in float64); an [..., S, S] tensor per call.
    Differentiable w.r.t. ``weights`` by torch's autograd: dL/dw_k = 2 sum_j w_j |m_k - m_j| + 2/3 w_k dl_k.  z_vals, near and far are
    constants."""
    w = weights
    lead = tuple(w.shape[:-1])
    z = z_vals.detach().to(dtype=w.dtype, device=w.device)
    near, far = _near_far_pair(near, far, lead, w.dtype, w.device)
    span = (far - near)[..., None]
    ok = span > 0
    s = torch.where(ok, (z - near[..., None]) / torch.where(ok, span, torch.ones_like(span)), torch.zeros_like(z))
    m = torch.cat([0.5 * (s[..., :-1] + s[..., 1:]), s[..., -1:]], -1)
    dl = torch.cat([s[..., 1:] - s[..., :-1], torch.zeros_like(s[..., -1:])], -1)
    pair = (w[..., :, None] * w[..., None, :] * (m[..., :, None] - m[..., None, :]).abs()).sum((-1, -2))
    return pair + (w * w * dl).sum(-1) / 3


class _Interlevel(torch.autograd.Function):
    """interlevel_loss over nerf_interlevel_fwd / _bwd: gradient to the proposal weights only, recomputed from the inputs"""

    @staticmethod
    def forward(ctx, proposal_weights, proposal_z, weights, z_vals):
        ctx.args = (proposal_weights.detach(), proposal_z, weights, z_vals)
        ctx.set_materialize_grads(False)
        return hb.interlevel(*ctx.args)

    @staticmethod
    def backward(ctx, d_loss):
        if d_loss is None:      # nothing upstream: no launch
            return None, None, None, None
        return hb.interlevel_bwd(*ctx.args, d_loss.to(torch.float32).contiguous()), None, None, None


def interlevel_loss(proposal_weights, proposal_z, weights, z_vals):
    """The interlevel (proposal) loss of mip-NeRF 360, per ray: [..., P] proposal weights and depths, [..., S] target weights and depths
    -> [...] (two HIP launches, forward and adjoint; interlevel_loss_reference is the definition).  Sample k of either side owns the
    half-open interval from its depth to the next one, the last sample [depth_last, +inf) -- the interval whose length the compositing
    used for that sample's alpha.  Intervals overlap when their intersection has positive length, max(z_j, zp_i) < min(z_j+1, zp_i+1):
    a zero-length interval overlaps nothing, the two last intervals always overlap.  With bound_j the sum of wp_i over the proposal
    intervals overlapping target interval j:

        L = sum_j max(0, w_j - bound_j)^2 / (w_j + 1e-7)

    the penalty for every target weight the proposal histogram does not cover.  Gradient to ``proposal_weights`` ONLY: the target
    weights and both sets of depths are constants of the graph (the stop-gradient of the original).  THE CALLER'S CONTRACT: both sets of
    depths are non-decreasing along the last axis (what every path of render_rays produces); it is not checked, a check would be a
    host synchronisation.  1 <= P, S <= 4096.  Composes with raw2outputs, whose weights (output 3) are differentiable:
    interlevel_loss(raw2outputs(raw_c, z_c, d)[3], z_c, raw2outputs(raw_f, z_f, d)[3], z_f)."""
    lead, P, S = tuple(proposal_weights.shape[:-1]), proposal_weights.shape[-1], weights.shape[-1]
    if tuple(proposal_z.shape) != tuple(proposal_weights.shape) or tuple(z_vals.shape) != tuple(weights.shape) or tuple(weights.shape[:-1]) != lead:
        raise ValueError(f"interlevel_loss: proposal_weights {tuple(proposal_weights.shape)}, proposal_z {tuple(proposal_z.shape)}, weights "
                         f"{tuple(weights.shape)} and z_vals {tuple(z_vals.shape)} do not belong together")
    f = lambda t, k: t.to(torch.float32).reshape(-1, k).contiguous()
    return _Interlevel.apply(f(proposal_weights, P), f(proposal_z.detach(), P), f(weights.detach(), S), f(z_vals.detach(), S)).reshape(lead)


def interlevel_loss_reference(proposal_weights, proposal_z, weights, z_vals):
    """THE DEFINITION interlevel_loss and the render paths' "interlevel" key are held to, in plain torch, on any device, in the dtype of
    ``proposal_weights`` for the sums (the tests call it in float64): the [..., S, P] overlap mask from the comparisons of the depths as
    they are given -- no searchsorted, no prefix differences --, bound = (mask * wp).sum(-1).  Differentiable w.r.t.
    ``proposal_weights`` by torch's autograd; the target weights are detached and the depths are constants."""
    wp = proposal_weights
    w = weights.detach().to(dtype=wp.dtype, device=wp.device)
    zp, z = proposal_z.detach().to(wp.device), z_vals.detach().to(wp.device)
    if zp.dtype != z.dtype:     # (comparisons of fp32 depths are exact in any wider type)
        zp, z = zp.to(torch.promote_types(zp.dtype, z.dtype)), z.to(torch.promote_types(zp.dtype, z.dtype))
    inf = lambda t: torch.full_like(t[..., :1], float("inf"))
    z0, z1 = z[..., :, None], torch.cat([z[..., 1:], inf(z)], -1)[..., :, None]             # [..., S, 1]
    p0, p1 = zp[..., None, :], torch.cat([zp[..., 1:], inf(zp)], -1)[..., None, :]          # [..., 1, P]
    mask = torch.maximum(z0, p0) < torch.minimum(z1, p1)                                    # [..., S, P]
    bound = (mask.to(wp.dtype) * wp[..., None, :]).sum(-1)
    return ((w - bound).clamp_min(0) ** 2 / (w + 1e-7)).sum(-1)


# --------------------------------------------------------------------------- reference call surface
def query_points(model, pts, viewdirs_per_point):
    """Evaluate the field at explicit points: every point is its own ray record
    (o = pt, d = 0, z = 0  =>  o + d*z == pt exactly).  Points / view directions that require grad receive d_pts / d_viewdirs
    (the input-gradient kernel in point mode).  A hashgrid.HashNeRF goes through its own query (columns 0:4 of its output); gradients
    to its points and view directions need HashNeRF(point_grad=True)."""
    grad_on = torch.is_grad_enabled()
    in_grad = grad_on and (pts.requires_grad or viewdirs_per_point.requires_grad)
    n = pts.shape[0]
    from .hashgrid import HashNeRF
    if isinstance(model, HashNeRF):
        if in_grad and not model.point_grad:
            raise NotImplementedError("query_points: gradients to the points / view directions of a HashNeRF need a network built with "
                                      "point_grad=True (without it the positions are constants of the graph)")
        pts, vd = pts.to(torch.float32), viewdirs_per_point.to(torch.float32)
        rays = torch.cat([pts, torch.zeros((n, 5), dtype=torch.float32, device=pts.device), vd], -1)
        return model.query(rays, torch.zeros((n, 1), dtype=torch.float32, device=pts.device)).reshape(n, -1)[:, :4]
    if in_grad:
        pts = pts.to(torch.float32).contiguous()
        vd = viewdirs_per_point.to(torch.float32).contiguous()
        rays = torch.cat([pts, torch.zeros((n, 5), dtype=torch.float32, device=pts.device), vd], -1)
    else:
        pts = _f32c(pts)
        vd = _f32c(viewdirs_per_point)
        rays = torch.zeros((n, 11), dtype=torch.float32, device=pts.device)
        rays[:, 0:3] = pts
        rays[:, 8:11] = vd
    z = torch.zeros((n, 1), dtype=torch.float32, device=pts.device)
    plist = model.param_list()
    need = grad_on and (in_grad or any(p.requires_grad for p in plist))
    raw = _FieldQuery.apply(model, rays, z, need, *plist)
    return raw.reshape(n, 4)


def batchify(fn, chunk):
    """run_nerf.py:27-34."""
    if chunk is None:
        return fn

    def ret(inputs):
        return torch.cat([fn(inputs[i:i + chunk]) for i in range(0, inputs.shape[0], chunk)], 0)
    return ret


def run_network(inputs, viewdirs, fn, embed_fn, embeddirs_fn, netchunk=1024 * 64):
    """run_nerf.py:37-51.  inputs [N,S,3], viewdirs [N,3], fn a NeRF module.  The embedders are
    accepted for signature parity; encoding happens inside the fused kernel (and the
    netchunk loop disappears: the kernel tiles the points itself)."""
    from .dense import DenseNeRF
    if isinstance(fn, DenseNeRF):       # any other architecture: the reference's own composition (embed, broadcast, network)
        flat = torch.reshape(inputs, [-1, inputs.shape[-1]])
        embedded = embed_fn(flat)
        if viewdirs is not None:
            dirs = torch.reshape(viewdirs[:, None].expand(inputs.shape), [-1, inputs.shape[-1]])
            embedded = torch.cat([embedded, embeddirs_fn(dirs)], -1)
        out = batchify(fn, netchunk)(embedded)
        return torch.reshape(out, list(inputs.shape[:-1]) + [out.shape[-1]])
    if not isinstance(fn, NeRF):
        raise NotImplementedError("run_network: fn must be a nerf-pytorch_amd NeRF module")
    if viewdirs is None:
        raise ValueError("run_network: this network was built with use_viewdirs=True")
    flat = torch.reshape(inputs, [-1, inputs.shape[-1]])
    dirs = viewdirs[:, None].expand(inputs.shape)
    dirs_flat = torch.reshape(dirs, [-1, dirs.shape[-1]])
    out = query_points(fn, flat, dirs_flat)
    return torch.reshape(out, list(inputs.shape[:-1]) + [out.shape[-1]])


def raw2outputs(raw, z_vals, rays_d, raw_noise_std=0, white_bkgd=False, pytest=False):
    """run_nerf.py:262-305: (rgb_map, disp_map, acc_map, weights, depth_map)."""
    noise = None
    std = float(raw_noise_std)
    if raw_noise_std > 0.0:
        noise = torch.randn(raw[..., 3].shape, device=raw.device)
        if pytest:
            np.random.seed(0)
            noise = torch.Tensor(np.random.rand(*list(raw[..., 3].shape)) * raw_noise_std).to(raw.device)
            std = 1.0
        noise = noise.contiguous()
    raw_c = raw.to(torch.float32).contiguous()
    f32 = lambda t: t.to(torch.float32).contiguous()        # (differentiable: z_vals / rays_d receive gradients when they require them)
    return _Composite.apply(raw_c, f32(z_vals), f32(rays_d), noise, std, bool(white_bkgd))


def sample_pdf(bins, weights, N_samples, det=False, pytest=False):
    """run_nerf_helpers.py:196-239 (output is a constant: the reference detaches it, run_nerf.py:394)."""
    bins, weights = _f32c(bins), _f32c(weights)
    dev = bins.device
    lead = list(bins.shape[:-1])
    u = None
    if not det:
        u = torch.rand(lead + [N_samples], device=dev)
    if pytest:
        np.random.seed(0)
        if det:
            u = torch.Tensor(np.broadcast_to(np.linspace(0.0, 1.0, N_samples), lead + [N_samples]).copy()).to(dev)
        else:
            u = torch.Tensor(np.random.rand(*(lead + [N_samples]))).to(dev)
    b2 = bins.reshape(-1, bins.shape[-1])
    w2 = weights.reshape(-1, weights.shape[-1])
    u2 = u.reshape(-1, N_samples).contiguous() if u is not None else None
    out = hb.sample_pdf(b2, w2, N_samples, u2, None if u2 is not None else _linspace01(N_samples, dev))
    return out.reshape(lead + [N_samples])


def builtin_query_fn(fn):
    """Mark `fn` as the stock network_query_fn (run_network with the stock embedders, run_nerf.py:201-204): render_rays then takes the
    fused path, in which encoding, network and netchunk tiling happen inside one kernel.  create_nerf marks the lambda it builds."""
    fn._nerf_amd_builtin = True
    return fn


def _is_builtin_query(network_query_fn):
    return network_query_fn is None or getattr(network_query_fn, "_nerf_amd_builtin", False)


def _render_rays_hooked(rays, rnd, network_fn, network_query_fn, N_samples, n_f, network_fine, lindisp, white_bkgd, std, retraw,
                        distortion=False, interlevel=False):
    """render_rays with a USER-SUPPLIED network_query_fn (run_nerf.py:385, :401 call it for every pass): the hook sees the reference's
    arguments -- pts [N, S, 3], viewdirs [N, 3], the network module -- and whatever it returns is composited, exactly as in the
    reference (a density regulariser, a clamp, a different network call all work).  Stage by stage through the C ABI: coarse depths
    (nerf_sample_coarse), the hook (stock run_network -> nerf_field_fwd / dgrad / wgrad per point), raw2outputs with its adjoint
    (nerf_raw2outputs[_bwd]), hierarchical depths (nerf_sample_fine: sample_pdf + sort, a constant as in run_nerf.py:394)."""
    dev = rays.device
    rays_o, rays_d, viewdirs = rays[:, 0:3], rays[:, 3:6].contiguous(), rays[:, 8:11]

    def one_pass(z_vals, net, noise):
        pts = rays_o[:, None, :] + rays_d[:, None, :] * z_vals[:, :, None]       # run_nerf.py:381 / :397
        raw = network_query_fn(pts, viewdirs, net)
        return raw, _Composite.apply(raw.to(torch.float32).contiguous(), z_vals, rays_d, noise, std, bool(white_bkgd))

    z = z_c = hb.sample_coarse(rays, _linspace01(N_samples, dev), lindisp, rnd.get("t_rand"))
    raw, (rgb, disp, acc, weights, _) = one_pass(z_c, network_fn, rnd.get("noise_c"))
    w_c = weights
    ret = {}
    if n_f > 0:
        ret.update(rgb0=rgb, disp0=disp, acc0=acc)
        u = rnd.get("u")
        z, z_std, _ = hb.sample_fine(z_c, weights.detach().contiguous(), n_f, u, None if u is not None else _linspace01(n_f, dev))
        raw, (rgb, disp, acc, weights, _) = one_pass(z, network_fn if network_fine is None else network_fine, rnd.get("noise_f"))
        ret["z_std"] = z_std
    ret.update(rgb_map=rgb, disp_map=disp, acc_map=acc)
    if retraw:
        ret["raw"] = raw
    if distortion:      # of the last pass's weights (differentiable through _Composite)
        ret["distortion"] = distortion_loss(weights, z, rays[:, 6], rays[:, 7])
    if interlevel:      # the coarse pass's weights against the refining pass's (differentiable through the coarse _Composite only)
        ret["interlevel"] = interlevel_loss(w_c, z_c, weights, z)
    return ret


def _grid_pass_lease(m, P, prec):
    """floats of the save buffer of a compacted pass of m of P points: m rounded up to the next eighth of the dense size.  M moves from
    step to step in training and Workspace.take passes over a free buffer more than twice the request; with eight sizes per pass a
    steady loop finds last step's buffer (or its neighbour in size) instead of allocating 4.8 KB per point every step."""
    q = max(1, -(-P // 8))
    return hb.act_floats(q * max(1, -(-m // q)), 1, prec)


def _grid_pass(cfg, desc, rays, z_vals, model, noise, want_weights, z_stop=None, *, stats, passes=None, budget=None, keep_weights=False):
    """THE compacted pass of both grid paths: depths -> nerf_occ_compact[_stop] (classify o + d z, drop what lies at or behind z_stop,
    compact the rest into n_samples = 1 ray records) -> ONE read-back of the count M -> the field on the M records, as query_points
    evaluates points (no launch when M == 0) -> nerf_occ_expand (raw, zeros for skipped samples) -> nerf_raw2outputs.  Returns
    (raw, raw2outputs' tuple) and adds the pass to stats["evaluated" / "total"].
    passes None (no backward follows): slot and records are hb.WORKSPACE leases handed back before the compositing -- stream-ordered: the
    next lease is written by kernels enqueued after these.
    passes = the list of the current ray sub-chunk's pass records (_RenderRaysGrid.forward): the field saves its activations into a lease
    of _grid_pass_lease's size, and the record the backward reads -- z, slot, act, rec (the M records, only when the rays need a
    gradient), m, packed, raw -- is appended to `passes` BEFORE anything can fail, so that the node hands its leases back with the
    others' on an error.  budget = {"rays_grad": bool, "resident": bytes the call keeps so far, "rays": rays of the whole call} goes with
    it: beyond hb.SAVE_TOTAL_BYTES in total the pass raises.
    The compacted raw and the M zero depths live inside the pass and are plain torch allocations on both paths.
    keep_weights (cfg.distortion, the last pass; cfg.interlevel, both passes): the record also keeps the pass's compositing weights as "w" for the backward."""
    n, S = z_vals.shape
    P = n * S
    dev, prec = rays.device, cfg.precision
    p = {"z": z_vals, "slot": hb.WORKSPACE.take(P, dev), "act": None, "rec": None, "m": 0}
    if passes is not None:
        passes.append(p)
    rec_ws = hb.WORKSPACE.take(11 * P, dev)
    try:
        slot, records, count = hb.occ_compact(desc, rays, z_vals, p["slot"], rec_ws, z_stop)
        m = p["m"] = int(count.item())      # the field launch needs M on the host
        raw = torch.empty((n, S, 4), dtype=torch.float32, device=dev)
        raw_c = torch.empty((max(m, 1), 1, 4), dtype=torch.float32, device=dev)
        if m > 0:
            if passes is not None:
                lease = _grid_pass_lease(m, P, prec)
                budget["resident"] += 4 * (lease + P + (11 * m if budget["rays_grad"] else 0))
                if budget["resident"] > hb.SAVE_TOTAL_BYTES:
                    raise RuntimeError(f"render_rays(occupancy=DensityGrid): the saved activations of this call's {budget['rays']} rays exceed "
                                       f"hip_backend.SAVE_TOTAL_BYTES = {hb.SAVE_TOTAL_BYTES} bytes (NERF_SAVE_TOTAL_GB); the grid path "
                                       "has no recompute plan: render fewer rays per call (chunk=) or raise the budget")
                p["act"] = hb.WORKSPACE.take(lease, dev)
            p["packed"] = model.packed_params(prec)
            hb.field_fwd(p["packed"], records[:m], torch.zeros((m, 1), dtype=torch.float32, device=dev), save_act=passes is not None,
                         precision=prec, raw=raw_c[:m], act=p["act"])
            if passes is not None and budget["rays_grad"]:
                p["rec"] = hb.WORKSPACE.take(11 * m, dev)
                p["rec"][:11 * m].copy_(records[:m].reshape(-1))
        hb.occ_expand(slot, raw_c, raw)
    finally:
        hb.WORKSPACE.give(rec_ws)
        if passes is None:
            hb.WORKSPACE.give(p["slot"])
    p["raw"] = raw
    stats["evaluated"] += m
    stats["total"] += P
    outs = hb.raw2outputs(raw, z_vals, rays, rays.shape[1], noise, cfg.raw_noise_std, cfg.white_bkgd, want_weights=want_weights,
                          want_depth=False, rays_d_offset=3)
    if keep_weights:
        p["w"] = outs[3]
    return raw, outs


def _grid_chain(cfg, desc, grid, rays, rnd, model_c, model_f, run_pass):
    """THE stages of a grid render on one ray chunk or sub-chunk -- _render_rays_hooked's chain with device code where the hook sits --
    with run_pass(rays, z_vals, model, noise, want_weights, z_stop) = _grid_pass bound to the caller's cfg, desc and bookkeeping.
    Everything option-dependent is read from cfg, which render_rays fills once for both paths:
      cfg.march_steps (proposal="march"): the depths are the grid's own (nerf_occ_march: march_steps candidates, N_samples slots) and
        the chunk is ONE pass of model_c on them, compacted with the march's stop depth (the caller hands the evaluated network as
        model_c, N_importance = 0 and the pass's noise as noise_c); with cfg.march_stop_eps the depths are nerf_occ_march_stop's, the
        march that also stops on the DensityGrid's own transmittance -- nothing else of the chunk changes (cfg.march_step_size: below);
      else coarse depths (nerf_sample_coarse) and their weights: cfg.proposal ("grid") takes the grid's own
        (DensityGrid.proposal_weights: one launch, no network, no read-back; the evaluated network is model_c), otherwise a pass of
        model_c, which is the whole chunk when N_importance = 0;
      cfg.early_stop_eps: the coarse weights give one stop depth per ray (nerf_occ_stop_depth), with which the refining pass compacts;
      nerf_sample_fine, and the refining pass on model_f (model_c without one).
    One host synchronisation per pass and none of its own.  Returns the output tuple (rgb, disp, acc, raw[, rgb0, disp0, acc0][, z_std][, distortion][, interlevel])
    and the device counters (stopped rays, truncated rays, refit rays; None without the option), which the caller reads back after its
    passes.  cfg.march_step_size (with cfg.march_fit): the march's depths are nerf_occ_march_step's -- steps of one length in the
    scene, march_steps the cap on candidates, the step doubled per ray until it fits the slots -- and nothing else of the chunk changes."""
    n_c, n_f = cfg.N_samples, cfg.N_importance
    dev = rays.device
    # cfg.distortion: the LAST pass hands out and keeps its weights, and the chain's tuple ends with their distortion loss on the depths
    # the pass was given and the near / far of `rays` (the clipped ones under clip_to_occupancy)
    # cfg.interlevel (two passes, no proposal: render_rays refuses the rest): BOTH passes hand out and keep their weights, and the tuple
    # ends with the interlevel loss of the coarse pass's weights against the refining pass's (skipped and stopped samples: weight 0)
    dist, inter = cfg.distortion, cfg.interlevel
    last_kw = {"keep_weights": True} if dist or inter else {}
    loss_of = lambda w, z: (hb.distortion(w, z, rays, nf_stride=rays.shape[1], nf_offset=6),) if dist else ()
    if cfg.march_steps is not None:
        n_stopped = n_refit = None
        if cfg.march_step_size is not None:      # world-space steps, march_steps is the cap: one kernel for both forms
            dens = cfg.march_stop_eps is not None
            z_m, z_stop, truncated, level, stopped = hb.occ_march_step(
                desc, grid.density if dens else None, grid.outside_sigma() if dens else 0.0, rays, rnd.get("u_march"),
                cfg.march_step_size, cfg.march_steps, n_c, cfg.march_fit, cfg.march_stop_eps)
            if dens:
                n_stopped = stopped.sum()
            if cfg.march_fit > 0:
                n_refit = (level > 0).sum()
        elif cfg.march_stop_eps is not None:
            z_m, z_stop, truncated, stopped = hb.occ_march_stop(desc, grid.density, grid.outside_sigma(), rays, rnd.get("u_march"),
                                                                cfg.march_steps, n_c, cfg.march_stop_eps)
            n_stopped = stopped.sum()
        else:
            z_m, z_stop, truncated = hb.occ_march(desc, rays, rnd.get("u_march"), cfg.march_steps, n_c)
        n_truncated = truncated.sum()
        raw, (rgb, disp, acc, w_m, _) = run_pass(rays, z_m, model_c, rnd.get("noise_c"), dist, z_stop, **last_kw)
        return (rgb, disp, acc, raw) + loss_of(w_m, z_m), n_stopped, n_truncated, n_refit
    z_c = hb.sample_coarse(rays, _linspace01(n_c, dev), cfg.lindisp, rnd.get("t_rand"))
    coarse = ()
    if cfg.proposal is not None:
        w_c = grid.proposal_weights(rays, z_c)
    else:
        raw_c, (rgb_c, disp_c, acc_c, w_c, _) = run_pass(rays, z_c, model_c, rnd.get("noise_c"), n_f > 0 or dist, None,
                                                         **(({"keep_weights": True} if inter else {}) if n_f > 0 else last_kw))
        if n_f <= 0:
            return (rgb_c, disp_c, acc_c, raw_c) + loss_of(w_c, z_c), None, None, None
        coarse = (rgb_c, disp_c, acc_c)
    z_stop = n_stopped = None
    if cfg.early_stop_eps is not None:
        z_stop = hb.occ_stop_depth(z_c, w_c, cfg.early_stop_eps)
        n_stopped = torch.isfinite(z_stop).sum()
    u = rnd.get("u")
    z_f, z_std, _ = hb.sample_fine(z_c, w_c, n_f, u, None if u is not None else _linspace01(n_f, dev))
    raw_f, (rgb_f, disp_f, acc_f, w_f, _) = run_pass(rays, z_f, model_c if model_f is None else model_f, rnd.get("noise_f"), dist or inter,
                                                     z_stop, **last_kw)
    return ((rgb_f, disp_f, acc_f, raw_f) + coarse + (z_std,) + loss_of(w_f, z_f) + ((hb.interlevel(w_c, z_c, w_f, z_f),) if inter else ()),
            n_stopped, None, None)


def _grid_stats(grid, stats, n_stopped, n_truncated, n_refit=None):
    """grid.last_stats of one call: the passes' counts and the chain's device counters (None without the option), read back here -- after
    the passes, which synchronised anyway -- once per call (a march with a stop or a fit has several counters: one stacked read-back)"""
    counters = [(k_, v) for k_, v in (("rays_stopped", n_stopped), ("rays_truncated", n_truncated), ("rays_refit", n_refit)) if v is not None]
    if len(counters) == 1:
        stats[counters[0][0]] = int(counters[0][1].item())
    elif counters:
        for (k_, _), v in zip(counters, torch.stack([v for _, v in counters]).tolist()):
            stats[k_] = int(v)
    grid.last_stats = stats


def _render_rays_occupancy(cfg, rays, rnd, model_c, model_f, grid):
    """render_rays without gradients through an occupancy grid (occupancy.OccupancyGrid): _grid_chain once over the whole chunk, nothing
    kept.  One host synchronisation per pass: two per call with N_importance > 0, one under a proposal or without a refining pass.
    Returns the chain's output tuple."""
    desc = grid._desc()
    stats = {"evaluated": 0, "total": 0}
    outs, *counters = _grid_chain(cfg, desc, grid, rays, rnd, model_c, model_f, partial(_grid_pass, cfg, desc, stats=stats))
    _grid_stats(grid, stats, *counters)
    return outs


class _RenderRaysGrid(torch.autograd.Function):
    """render_rays through an occupancy.DensityGrid WITH gradients, as one autograd node with _RenderRays' backward (_backward: one
    _grad_ready per network with the final flat vector, a shared network accumulated in the kernel, no weight-gradient launch for a
    frozen network, the stale-parameter and freed-graph checks; no saved output in ctx).

    Forward: _grid_chain -- the stages of the no-grad grid render -- per ray sub-chunk, every pass a saving _grid_pass.  Backward, per
    pass: _composite_adjoint (nerf_raw2outputs_bwd) -> this node's field_step: nerf_occ_gather (d_raw of the M points) -> delta chain /
    weight gradient on the M records, the input gradient in point mode when the rays need one -> nerf_occ_fold_rays (per-point [M, 11]
    -> per-ray [N, 11]); then the compositing's |d| term.  A skipped sample has raw = 0 and no gradient: what a network_query_fn that
    evaluates only the occupied points computes.

    Kept from forward to backward, per pass: slot (4 B per sample point), the saved activations of M points (leased at
    _grid_pass_lease's size), z, raw, and the M records (44 B each) only when the rays need a gradient -- hb.WORKSPACE leases, given
    back by the backward or freed with a dropped graph.  Calls above hb.max_saved_rays(...) rays run in equal ray sub-chunks, every
    one resident with leases of its own M; beyond hb.SAVE_TOTAL_BYTES in total the call raises (no recompute plan on this path).

    The options of _grid_chain as the backward sees them.  cfg.proposal ("grid"): the coarse weights are a constant of the graph,
    nothing saved, and the node has ONE pass, the refining one on model_c; outputs (rgb, disp, acc, raw, z_std).  cfg.early_stop_eps:
    z_stop is a constant of the graph, computed per sub-chunk; a stopped sample has slot -1 like a skipped one -- raw = 0, no gradient
    -- so nothing beyond slot is kept for it and the backward is unchanged.  cfg.march_steps: depths and stop depth are constants of
    the graph, computed per sub-chunk; with N_importance = 0 the backward is the coarse-only one; outputs (rgb, disp, acc, raw) --
    cfg.march_stop_eps, cfg.march_step_size and cfg.march_fit change which kernel computes those constants and nothing of the
    backward.  cfg.distortion, cfg.interlevel (the two-pass form only): the trailing outputs and their adjoints are _RenderRays'; the
    d_weights enter the compositing backward in front of nerf_occ_gather."""

    @staticmethod
    def forward(ctx, cfg, rays, rnd, model_c, model_f, grid, *params):
        n_c, n_f = cfg.N_samples, cfg.N_importance
        prec = cfg.precision
        n = rays.shape[0]
        desc = grid._desc()
        sub, tiles = _sub_chunks(n, hb.max_saved_rays(n_c, n_f, prec))
        global LAST_BACKWARD_PLAN
        LAST_BACKWARD_PLAN = ("resident sub-chunks" if len(tiles) > 1 else "one launch", n, min(n, sub))
        stats = {"evaluated": 0, "total": 0}
        budget = {"rays_grad": bool(ctx.needs_input_grad[1]), "resident": 0, "rays": n}
        n_stopped, n_truncated, n_refit = [], [], []
        parts, outs = [], []
        try:
            for lo, hi in tiles:
                rnd_t = rnd if len(tiles) == 1 else {k_: v[lo:hi] for k_, v in rnd.items()}
                parts.append([])
                out, stopped, truncated, refit = _grid_chain(cfg, desc, grid, rays[lo:hi], rnd_t, model_c, model_f,
                                                             partial(_grid_pass, cfg, desc, stats=stats, passes=parts[-1], budget=budget))
                outs.append(out)
                n_stopped += [] if stopped is None else [stopped]
                n_truncated += [] if truncated is None else [truncated]
                n_refit += [] if refit is None else [refit]
        except BaseException:
            for passes in parts:
                _give_leases(passes)
            raise
        _grid_stats(grid, stats, torch.stack(n_stopped).sum() if n_stopped else None, torch.stack(n_truncated).sum() if n_truncated else None,
                    torch.stack(n_refit).sum() if n_refit else None)
        if hb.DATAPATHS[prec].fp16_saves:       # the fp16 split's range guard rail sees the compacted passes' saved activations
            for passes in parts:
                acts = [(p["act"], 1) for p in passes if p["act"] is not None]
                if acts:
                    hb.RANGE_MONITOR.after_forward(acts, [p["m"] for p in passes if p["act"] is not None])
        if len(tiles) == 1:
            out = outs[0]
            # `raw` of the last pass is an output of this node: held through save_for_backward, never in ctx (_RenderRays.forward)
            ctx.save_for_backward(parts[0][-1].pop("raw"))
        else:
            out = tuple(torch.cat([o[i] for o in outs], 0) for i in range(len(outs[0])))       # new tensors: the per-tile ones are no outputs
        ctx.tiles, ctx.parts = tiles, parts
        _keep_for_backward(ctx, cfg, rays, rnd, model_c, model_f, 6)
        if n_f > 0:     # z_std (in front of the trailing losses if there are any): the reference detaches z_samples (run_nerf.py:394)
            ctx.mark_non_differentiable(out[-1 - int(cfg.distortion) - int(cfg.interlevel)])
        return tuple(out)

    @staticmethod
    def backward(ctx, *gouts):
        prec = ctx.cfg.precision

        def field_step(p, rays, d_raw, model, grad, accumulate, d_rays):
            m, z, dev = p["m"], p["z"], rays.device
            if m == 0:         # no point of this pass was evaluated: no field launch, zero gradient from it
                if grad is not None and not accumulate:
                    grad.zero_()
                return grad is not None
            slot = p["slot"][:z.numel()].view(torch.int32)
            d_raw_c = hb.occ_gather(slot, d_raw, torch.empty((m, 1, 4), dtype=torch.float32, device=dev))
            d_rec = rec = None
            if d_rays is not None:
                rec = p["rec"][:11 * m].view(m, 11)
                d_rec = torch.empty((m, 11), dtype=torch.float32, device=dev)
            hb.field_bwd(p["packed"], p["act"], d_raw_c, grad, accumulate, precision=prec, params=model.flat_params(),
                         input_grad=None if d_rec is None else (rec, torch.zeros((m, 1), dtype=torch.float32, device=dev), d_rec, False))
            if d_rec is not None:
                hb.occ_fold_rays(slot, z, d_rec, d_rays, accumulate=True)
            return grad is not None

        def release():
            for passes in ctx.parts:
                _give_leases(passes)
            ctx.parts = None

        return _backward(ctx, gouts, 6, _resident_tiles(ctx.tiles, ctx.rays, ctx.rnd, ctx.parts), field_step, lambda p: None, release)


def _render_rays_baked(ray_batch, baked, network_query_fn, perturb, white_bkgd, pytest, given):
    """render_rays(baked=field): the guards (`given`: render_rays' option arguments as they came), the one draw, the field's own launch"""
    from .baked import BakedField
    bad = ro.options_set(**given)
    if not isinstance(baked, BakedField):
        raise ValueError(f"render_rays: baked must be None or a baked.BakedField, got {type(baked).__name__}")
    if bad:
        raise ValueError(f"render_rays: baked= renders from the baked field alone and cannot be combined with {', '.join(bad)}")
    if not _is_builtin_query(network_query_fn):
        raise ValueError("render_rays: baked= together with a user network_query_fn: there is no network to query")
    if ray_batch.dim() != 2 or ray_batch.shape[-1] < 11:
        raise ValueError("render_rays: baked= needs ray records of 11 columns (o, d, near, far, viewdir: render(use_viewdirs=True))")
    if torch.is_grad_enabled() and ray_batch.requires_grad:
        raise ValueError("render_rays: baked= has no backward: rays that require grad are refused (render under torch.no_grad() or detach them)")
    n = ray_batch.shape[0]
    u = None
    if perturb > 0.:
        u = torch.rand(n, device=ray_batch.device)
        if pytest:
            np.random.seed(0)
            u = torch.Tensor(np.random.rand(n)).to(ray_batch.device)
    return baked.render_rays(ray_batch, u=u, white_bkgd=bool(white_bkgd))


def render_rays(ray_batch, network_fn, network_query_fn, N_samples, retraw=False, lindisp=False, perturb=0.,
                N_importance=0, network_fine=None, white_bkgd=False, raw_noise_std=0., verbose=False, pytest=False,
                *, randoms=None, occupancy=None, clip_to_occupancy=False, proposal=None, early_stop_eps=None, march_steps=None,
                march_stop_eps=None, march_step_size=None, march_fit=0, distortion=False, interlevel=False, baked=None):
    """run_nerf.py:308-418.  Same arguments, same returned dict.

    ``network_query_fn``: None or the function create_nerf built (builtin_query_fn) -> the fused path; ANY other callable is called
    for every pass with (pts, viewdirs, network) like the reference does (_render_rays_hooked).  ``verbose`` is accepted and prints
    nothing (run_nerf.py:414-416's DEBUG-gated NaN check: see render.check_range()); the reference's ``netchunk`` has no counterpart
    (the kernels tile the points themselves).

    ``randoms`` (keyword-only, not in the reference) injects the random tensors
    {t_rand [N,N_samples], noise_c [N,N_samples], u [N,N_importance], noise_f [N,N_samples+N_importance]}
    instead of drawing them: the explicit form of the reference's ``pytest=`` hook.

    ``occupancy`` (keyword-only, not in the reference): an occupancy.OccupancyGrid -- sample points in empty cells are not sent
    through the network and get raw = 0 (_grid_chain / _grid_pass).  Fused NeRF networks only: a grid together with a DenseNeRF or a
    user network_query_fn raises NotImplementedError.  With a needed gradient (grad mode on and parameters or rays that require grad)
    an occupancy.DensityGrid renders differentiably w.r.t. both networks' parameters and the ray records (_RenderRaysGrid: skipped
    samples get no gradient); a plain OccupancyGrid raises NotImplementedError there.  None: nothing changes.

    ``clip_to_occupancy`` (keyword-only, not in the reference; needs ``occupancy``): True replaces (near, far) of every ray by the
    span of the occupied cells it crosses (occupancy.clip_rays: nerf_occ_ray_span) before the coarse depths are drawn, so all
    N_samples of them land where the grid lets the network be evaluated; a ray that crosses nothing occupied keeps its interval.
    The call equals render_rays(occupancy.clip_rays(ray_batch)[0], ..., occupancy=occupancy) bit for bit, gradients included (near' /
    far' are constants of the graph); last_stats additionally carries "rays_hit" and "rays".  False: nothing changes.

    ``proposal`` (keyword-only, not in the reference; needs an occupancy.DensityGrid as ``occupancy`` and N_importance > 0): "grid"
    draws the importance samples from the grid instead of a coarse network.  The coarse depths are drawn as always (after
    clip_to_occupancy if that is on); their weights are the compositing weights of the grid's own density per cell
    (DensityGrid.proposal_sigma is the definition, nerf_occ_proposal_weights the kernel: no network, no interpolation);
    nerf_sample_fine turns them into the sorted N_samples + N_importance depths, and ONE network -- network_fine if given, else
    network_fn -- is evaluated on those through the compacted grid pass, with gradients to its parameters and the ray records as
    without the option.  The other network is never touched: no launch, no gradient (.grad stays None), no _grad_ready.  The dict
    holds rgb_map, disp_map, acc_map, z_std (and raw with retraw) and NO rgb0 / disp0 / acc0: there is no coarse image (the reference's
    train() guards its coarse loss with ``if 'rgb0' in extras``).  last_stats counts the one pass: total = N * (N_samples +
    N_importance).  Random draws: t_rand, u, noise_f in that order; noise_c is not drawn and is ignored in ``randoms`` -- the generator
    stream therefore differs from the two-network render's, by design.  Before the grid's first update its densities are 0 and all
    bits are set: the weights of the samples inside the box are exactly 0 (beyond a box with outside="evaluate" they carry
    sigma_threshold), sample_pdf's 1e-5 floor makes the pdf uniform, and the network sees the stratified plus uniformly drawn depths
    -- nothing is hidden during the warm-up.  None: nothing changes.

    ``early_stop_eps`` (keyword-only, not in the reference; a float with 0 < eps < 1; needs ``occupancy`` and N_importance > 0): early
    ray termination for the refining pass.  The coarse pass -- untouched -- has just returned its compositing weights (the coarse
    network's, or the grid's under proposal="grid"); their running sum up to sample i is 1 - T, so one launch (nerf_occ_stop_depth;
    occupancy.stop_depth_reference is the definition) finds per ray the coarse depth z_stop behind which that estimate of the
    transmittance is below eps, and the refining pass's compaction (nerf_occ_compact_stop) drops every sample with z >= z_stop next to
    the ones in empty cells: raw = 0, no network evaluation, no gradient, no saved activations.  Order inside a call: coarse depths
    (after clip_to_occupancy) -> coarse weights -> z_stop -> nerf_sample_fine as before -> the refining pass.  rgb0 / disp0 / acc0, z_std
    and the random draws are those of the call without the option.  AN APPROXIMATION: what is dropped from the refined image is the
    REFINING pass's own transmittance at z_stop, which is close to eps where the two passes agree but is not bounded by it (a coarse
    network that sees a surface the fine one does not cuts visible geometry) -- hence opt-in.  z_stop is a constant of the graph.
    last_stats additionally carries "rays_stopped" (rays with a finite z_stop); "evaluated" counts what survived grid and stop.
    None: nothing changes -- same launches, same bits, same draws.

    ``proposal="march"`` with ``march_steps=M`` (keyword-only, not in the reference; needs ``occupancy``, a plain OccupancyGrid under
    no_grad or a DensityGrid with gradients): grid ray marching.  The depths are no longer the reference's thinned out: every ray is
    walked in M equal steps over [near, far] (after clip_to_occupancy if that is on: the steps then span the occupied hull) and only
    the steps in occupied cells, plus one closing step behind every occupied run, are written into S = N_samples + max(N_importance, 0)
    slots (occupancy.OccupancyGrid.march_reference is the definition, nerf_occ_march the kernel; no coarse pass, no sample_pdf, no
    sort).  ONE network -- network_fine if given, else network_fn -- is evaluated on them through the compacted grid pass; the closing
    steps lie in empty cells and get raw = 0, so a sample's interval never reaches across a gap; the padding behind the last emitted
    step, and whatever did not fit into S slots, is dropped by the compaction's stop depth.  The other network is never touched: no
    launch, .grad stays None, no _grad_ready.  The dict holds rgb_map, disp_map, acc_map (and raw [N, S, 4] with retraw): no rgb0 /
    disp0 / acc0 and no z_std.  Random draws: with perturb > 0 one offset per ray, u_march [N] (all steps of a ray move together; 0.5
    without), then with raw_noise_std > 0 noise_f [N, S] -- these are the ``randoms`` keys; t_rand, u and noise_c are neither drawn nor
    read.  last_stats = {"evaluated", "total" = N * S, "rays_truncated"} (rays whose emitted steps did not fit: raise N_samples +
    N_importance, or lower march_steps).  1 <= march_steps <= 16384, S <= 4096; lindisp and early_stop_eps (there are no coarse weights to
    stop on) are refused.  ``march_steps`` without proposal="march" is refused.

    ``march_stop_eps`` (keyword-only, not in the reference; a float with 0 < eps < 1; needs proposal="march" and an
    occupancy.DensityGrid as ``occupancy``): the march's own termination rule.  The marcher adds up the grid's densities as it walks --
    per kept step sigma * (the step's interval) * |d|, the optical depth the compositing would give that sample if the network
    answered what the grid holds -- and once the grid's own transmittance exp(-sum) has fallen to eps the ray stops emitting: no slot,
    no field evaluation, no saved activation, no gradient (occupancy.DensityGrid.march_stop_reference is the definition,
    nerf_occ_march_stop the kernel, which replaces nerf_occ_march in the call).  The slots a stop frees go to nobody; a ray that would
    have been truncated behind its stop no longer is.  The single compacted pass with the march's z_stop, the backward (depths and
    z_stop are constants of the graph), the draws (u_march, then noise_f) and the output keys are those of the march without the
    option.  AN APPROXIMATION: what is dropped from the image is the NETWORK's own transmittance behind the stop.  The grid's
    densities are a decayed running maximum per cell, so they overestimate and the grid stops early rather than late: the dropped
    transmittance is close to eps where grid and network agree, but it is not bounded by eps (a cell whose maximum came from a thin
    structure stops rays that pass beside it) -- hence opt-in.  A grid that was never updated has density 0 and stops nothing.
    last_stats additionally carries "rays_stopped" (a truncated ray does not count: the slot limit bit first).  Refused: the option
    without proposal="march", a value that is not a float in (0, 1) (bools included), a plain OccupancyGrid (it has no densities).
    None: nothing changes -- same launches, same bits, same draws.

    ``march_step_size`` (keyword-only, not in the reference; a finite real number > 0; needs proposal="march") with ``march_fit``
    (keyword-only; an int in 0..8, default 0): the march in steps of ONE LENGTH IN THE SCENE, fitted per ray to the slots.  Without it
    a ray's step is (far - near) / march_steps in depth: its length in the scene changes with |d| (rays_d is not normalised), with near
    / far and with clip_to_occupancy.  With march_step_size=ds every ray steps ds along its direction -- dz = ds / |d| in depth, from
    near + u dz on, while z < far -- and march_steps, still required, is the cap on candidates per ray; "half a cell of a 128^3 grid"
    is said once.  march_fit=J lets a ray whose emitted steps do not fit its S slots walk again with the step doubled, up to J times:
    the slot limit then coarsens a ray instead of cutting off what lies behind its first cells; a ray that fits at no level keeps level
    J's depths and stays truncated (occupancy.OccupancyGrid.march_step_reference is the definition, with march_stop_eps
    DensityGrid.march_step_stop_reference -- every level applies the stop rule, so a stop can spare a doubling; nerf_occ_march_step is
    the kernel of both and replaces nerf_occ_march / nerf_occ_march_stop in the call).  A ray with d = 0 has no step and emits nothing.
    Nothing else of the call changes: the single compacted pass with the march's z_stop, the backward (depths and z_stop are constants
    of the graph), the draws (u_march, then noise_f), the output keys, clip_to_occupancy before the march.  last_stats additionally
    carries "rays_refit" (rays whose step was doubled at least once) when march_fit > 0.  Refused: either option without
    proposal="march", a step that is not a finite real number > 0 or a fit that is not an int in 0..8 (bools included), march_fit > 0
    without march_step_size; lindisp stays NotImplementedError.  None / 0: nothing changes -- same launches, same bits, same draws.

    ``distortion`` (keyword-only, not in the reference; a bool): True adds one key, "distortion" [N] fp32, last in the dict: the
    distortion loss (distortion_loss; distortion_loss_reference is the definition) of the compositing weights of the pass whose image
    is rgb_map -- the refining pass, or the only one with N_importance = 0, under a proposal or under the march -- computed from
    exactly the weights the compositing used (noise included), that pass's depths and the near / far of the ray records the pass
    saw.  Under clip_to_occupancy those are the clipped ones: the identity render_rays(occupancy.clip_rays(rays)[0], ...) holds for
    this key too, and THE LOSS'S SCALE THEN FOLLOWS THE CLIPPED SPAN (depths are normalised by far' - near' per ray).  A skipped,
    stopped or padded sample of the grid paths has raw = 0, weight 0, and contributes nothing.  There is no loss on the coarse or the
    proposal weights and no gradient to depths, near or far; gradients reach parameters and ray records through the weights, by the
    compositing's and the field's existing adjoints (nerf_distortion_bwd -> d_weights of nerf_raw2outputs_bwd), on every path and in
    all backward plans.  render() delivers it as extras["distortion"] with the rays' leading shape:
    loss = img_loss + lam * extras["distortion"].mean().  Cost: the last pass's compositing also stores its weights (the same kernel,
    every other output keeps its bits), one launch for the loss, and one for its adjoint when the key carries a gradient; the fused
    node keeps the weights (N * S * 4 bytes) for its backward.  A call WITHOUT a needed gradient takes the staged passes with the
    option, not the one-launch inference kernel, which has no weights to give.  False: nothing changes -- same launches, same bits,
    same draws.

    ``interlevel`` (keyword-only, not in the reference; a bool; needs N_importance > 0 and a coarse pass): True adds one key,
    "interlevel" [N] fp32, last in the dict (behind "distortion" when both are on): the interlevel loss of mip-NeRF 360
    (interlevel_loss; interlevel_loss_reference is the definition) with the COARSE pass's compositing weights on the coarse depths as
    the proposal histogram and the refining pass's weights on its depths as the target -- both exactly the weights the compositing
    used, noise included.  It penalises every refining weight that exceeds what the coarse histogram holds over the same span, and so
    trains network_fn for what its weights are used for: telling nerf_sample_fine where to draw.  The target is a constant of the
    graph: the upstream gradient enters the coarse pass's compositing backward as d_weights (nerf_interlevel_bwd -> nerf_raw2outputs_bwd)
    and reaches network_fn, and the ray records when they require grad, by the existing adjoints; network_fine gets nothing from it
    (a loss of this key alone leaves its .grad None and runs no backward of the refining pass), and a network that serves both passes
    gets it through the coarse pass only.  There is no gradient to depths.  Supported on the fused node in all backward plans (it keeps
    both passes' weights, N * (2 N_samples + N_importance) * 4 bytes; the recompute plan recomputes them), through a DensityGrid in
    its two-pass form, also with clip_to_occupancy and early_stop_eps (skipped and stopped samples have weight 0 and contribute
    nothing), with a user network_query_fn and with general (DenseNeRF) networks (interlevel_loss on _Composite's weights).  A call
    WITHOUT a needed gradient takes the staged passes, as with ``distortion``.  render() delivers it as extras["interlevel"] with the
    rays' leading shape.  Refused with ValueError: N_importance = 0, proposal="grid" (a grid is not trained by gradients),
    proposal="march" (there is no coarse pass), a value that is not a bool.  False: nothing changes -- same launches, same bits, same
    draws.

    ``baked`` (keyword-only, not in the reference): a baked.BakedField -- the rays are rendered from the field's grid of densities and
    spherical-harmonic colours by one launch (nerf_baked_render; BakedField.render_rays_reference is the definition) and NO network is
    touched: network_fn and network_fine may be None, N_samples / N_importance / lindisp are not read (the field marches in its own
    step_size).  perturb > 0 draws one offset per ray with one torch.rand(N) (all steps of a ray move together; 0.5 without);
    white_bkgd is honoured.  The dict holds exactly rgb_map, disp_map, acc_map and depth_map; the field's last_stats = {"rays",
    "samples", "rays_stopped"}.  Inference only: refused with ValueError, before anything reaches the library, together with
    occupancy, clip_to_occupancy, proposal, early_stop_eps, the march options, distortion, interlevel, retraw, randoms,
    raw_noise_std > 0, a user network_query_fn, and -- in grad mode -- rays that require grad (there is no backward).  Clipping stays
    possible by hand: baked.grid.clip_rays(rays)[0].  None: nothing changes -- same launches, same bits, same draws."""
    given = dict(N_samples=N_samples, retraw=retraw, lindisp=lindisp, perturb=perturb, N_importance=N_importance, white_bkgd=white_bkgd,
                 raw_noise_std=raw_noise_std, pytest=pytest, randoms=randoms, occupancy=occupancy, clip_to_occupancy=clip_to_occupancy,
                 proposal=proposal, early_stop_eps=early_stop_eps, march_steps=march_steps, march_stop_eps=march_stop_eps,
                 march_step_size=march_step_size, march_fit=march_fit, distortion=distortion, interlevel=interlevel)
    if baked is not None:       # (in front of every check: whatever else is wrong with the call, the field refuses the options it was given)
        return _render_rays_baked(ray_batch, baked, network_query_fn, perturb, white_bkgd, pytest, given)
    opt = ro.ray_options(**given)
    from .dense import DenseNeRF, render_rays_dense
    nets = [network_fn] + ([network_fine] if network_fine is not None else [])
    dense = all(isinstance(m, DenseNeRF) for m in nets)         # architectures outside the fused kernels: layer by layer (dense.py)
    if not dense and not all(isinstance(m, NeRF) for m in nets):
        raise NotImplementedError("render_rays: network_fn / network_fine must both be fused-kernel NeRF modules (D=8, W=256, 10 / 4 "
                                  "frequencies, view directions) or both general ones (nerf_pytorch_amd.NeRF builds either)")
    if not dense and ray_batch.shape[-1] <= 8:
        raise ValueError("render_rays: these networks use view directions; the ray records need 11 columns (render(use_viewdirs=True))")
    rays_grad = torch.is_grad_enabled() and ray_batch.requires_grad
    # (general networks: only a call whose networks are all HashNeRF(point_grad=True) takes rays in the graph -- hashgrid.HashNeRF.query)
    if rays_grad and dense and not all(getattr(m, "point_grad", False) for m in nets):
        raise NotImplementedError("render_rays: gradients to rays / sample points / camera poses are implemented for the fused "
                                  "NeRF architecture only, not for general (DenseNeRF) networks")
    # rays that require grad stay in the graph (d loss / d ray records: nerf_field_input_grad + the compositing's |d| term)
    rays = ray_batch.to(torch.float32).contiguous()
    if not rays_grad:
        rays = rays.detach()
    n, dev, n_f = rays.shape[0], rays.device, opt.N_importance
    builtin = _is_builtin_query(network_query_fn)
    # THE cfg of the call; its path says which noise scale the kernels apply and whether a backward can follow
    cfg_of = partial(ro.RenderCfg.of, opt, precision=_PRECISION, grid=occupancy is not None)
    wants_grad = lambda params: torch.is_grad_enabled() and (rays_grad or any(p.requires_grad for p in params))
    if n == 0 and dense and occupancy is None and builtin:
        # general networks: the dense path's own order, outputs attached to the networks (dense._render_no_rays)
        cfg = cfg_of(raw_noise_std=0., need_grad=wants_grad(p for m in nets for p in m.parameters()))
        return ro.result_dict(opt, render_rays_dense(cfg, rays, {}, network_fn, network_fine if n_f > 0 else None), coarse_first=True)
    if n == 0:      # empty batch: the reference returns empty tensors of the right trailing shapes
        if occupancy is not None:       # nothing was evaluated; the grid is validated as on the staged path
            occupancy._desc()
            occupancy.last_stats = dict.fromkeys(("evaluated", "total") + opt.stats_keys, 0)
        return ro.result_dict(opt, opt.empty_outputs(dev), coarse_first=False)
    rnd, std = ro.draw_randoms(opt, n, dev)
    if occupancy is not None:
        if not builtin:
            raise NotImplementedError("render_rays: occupancy= together with a user network_query_fn is not implemented (mask inside the "
                                      "hook with occupancy.occupied(pts) instead)")
        if dense:
            raise NotImplementedError("render_rays: occupancy= together with general (DenseNeRF) networks is not implemented; the grid "
                                      "path runs the fused NeRF architecture only")
        evaluated = nets[-1:] if opt.one_pass else nets        # (one pass: network_fine if given, else network_fn)
        grid_grad = wants_grad(p for m in evaluated for p in m.parameters())
        if grid_grad and not isinstance(occupancy, ro.DensityGrid):
            raise NotImplementedError("render_rays: a plain OccupancyGrid together with a needed gradient (grad mode on and parameters or "
                                      "rays that require grad) is not implemented: a static grid would hide what the network has not "
                                      "learnt yet.  Render under torch.no_grad(), or train through an occupancy.DensityGrid (the grid "
                                      "that follows the network: maybe_update every step)")
        cfg = cfg_of(raw_noise_std=std, need_grad=grid_grad)        # what _grid_chain reads, once for both paths
        if opt.march:       # ONE pass over all the slots: what the two paths below run as a coarse-only call on the march's depths
            cfg = dataclasses.replace(cfg, N_samples=opt.slots, N_importance=0)
            rnd = {k_: v for k_, v in (("u_march", rnd.get("u_march")), ("noise_c", rnd.get("noise_f"))) if v is not None}
        n_hit = None
        if clip_to_occupancy:       # (after the guards: a refused call launches nothing; the draws above do not depend on near / far)
            rays, hit = occupancy.clip_rays(rays)
            n_hit = hit.sum()       # read back after the passes, which synchronise anyway
        if opt.one_pass:        # one network, handed on as model_c
            model_c, model_f = evaluated[0], None
        else:
            same = n_f <= 0 or network_fine is None or network_fine is network_fn
            model_c, model_f = network_fn, None if same else network_fine
        if grid_grad:
            params = model_c.param_list() + ([] if model_f is None else model_f.param_list())
            outs = _RenderRaysGrid.apply(cfg, rays, rnd, model_c, model_f, occupancy, *params)
        else:
            outs = _render_rays_occupancy(cfg, rays, rnd, model_c, model_f, occupancy)
        if n_hit is not None:
            occupancy.last_stats = dict(occupancy.last_stats, rays_hit=int(n_hit.item()), rays=n)
        return ro.result_dict(opt, outs, coarse_first=True)
    if not builtin:
        return _render_rays_hooked(rays, rnd, network_fn, network_query_fn, opt.N_samples, n_f, network_fine if n_f > 0 else None,
                                   opt.lindisp, opt.white_bkgd, std, opt.retraw, opt.distortion, opt.interlevel)
    if dense:
        cfg = cfg_of(raw_noise_std=std, need_grad=wants_grad(p for m in nets for p in m.parameters()))
        return ro.result_dict(opt, render_rays_dense(cfg, rays, rnd, network_fn, network_fine if n_f > 0 else None), coarse_first=True)
    params = network_fn.param_list()
    same = network_fine is None or network_fine is network_fn
    if n_f > 0 and not same:
        params = params + network_fine.param_list()
    # activations are saved only when a backward can follow (Function.forward itself always runs in no-grad mode)
    cfg = cfg_of(raw_noise_std=std, need_grad=wants_grad(params))
    outs = _RenderRays.apply(cfg, rays, rnd, network_fn, None if (same or n_f <= 0) else network_fine, *params)
    return ro.result_dict(opt, outs, coarse_first=False)


def batchify_rays(rays_flat, chunk=1024 * 32, **kwargs):
    """run_nerf.py:54-66.  Injected ``randoms`` (one row per ray) are sliced with the rays, so a chunked call consumes
    the same draws as an unchunked one.  An ``occupancy`` grid's last_stats are summed over the chunks: "evaluated", "total" and the keys
    the call's options add, which render_options._stats_keys names once for render_rays and for this function
    (unchecked_stats_keys: the keywords are forwarded as given, nothing is validated here); so are a ``baked`` field's."""
    all_ret = {}
    randoms = kwargs.pop("randoms", None)
    occ = kwargs.get("occupancy")
    occ_stats = dict.fromkeys(("evaluated", "total") + ro.unchecked_stats_keys(kwargs), 0)
    if randoms is not None:
        for k, v in randoms.items():
            if v.shape[0] != rays_flat.shape[0]:
                raise ValueError(f"randoms[{k!r}] has {v.shape[0]} rows for {rays_flat.shape[0]} rays")
    baked = kwargs.get("baked")
    baked_stats = dict.fromkeys(("rays", "samples", "rays_stopped"), 0)
    for i in range(0, rays_flat.shape[0], chunk):
        if randoms is not None:
            kwargs["randoms"] = {k: v[i:i + chunk] for k, v in randoms.items()}
        ret = render_rays(rays_flat[i:i + chunk], **kwargs)
        if occ is not None and occ.last_stats is not None:
            occ_stats = {k: occ_stats[k] + occ.last_stats[k] for k in occ_stats}
        if baked is not None:
            baked_stats = {k: baked_stats[k] + baked.last_stats[k] for k in baked_stats}
        for k in ret:
            all_ret.setdefault(k, []).append(ret[k])
    if occ is not None:
        occ.last_stats = occ_stats
    if baked is not None:
        baked.last_stats = baked_stats
    return {k: (v[0] if len(v) == 1 else torch.cat(v, 0)) for k, v in all_ret.items()}


# ---- ray geometry: per-ray (not per-sample) work, stays PyTorch behind render()
def get_rays(H, W, K, c2w):
    """run_nerf_helpers.py:153-162."""
    dev = c2w.device if isinstance(c2w, torch.Tensor) else None
    i, j = torch.meshgrid(torch.linspace(0, W - 1, W, device=dev), torch.linspace(0, H - 1, H, device=dev), indexing='ij')
    i = i.t()
    j = j.t()
    dirs = torch.stack([(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -torch.ones_like(i)], -1)
    rays_d = torch.sum(dirs[..., None, :] * c2w[:3, :3], -1)
    rays_o = c2w[:3, -1].expand(rays_d.shape)
    return rays_o, rays_d


def get_rays_np(H, W, K, c2w):
    """run_nerf_helpers.py:165-172."""
    i, j = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing='xy')
    dirs = np.stack([(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -np.ones_like(i)], -1)
    rays_d = np.sum(dirs[..., np.newaxis, :] * c2w[:3, :3], -1)
    rays_o = np.broadcast_to(c2w[:3, -1], np.shape(rays_d))
    return rays_o, rays_d


def ndc_rays(H, W, focal, near, rays_o, rays_d):
    """run_nerf_helpers.py:175-192."""
    t = -(near + rays_o[..., 2]) / rays_d[..., 2]
    rays_o = rays_o + t[..., None] * rays_d
    o0 = -1. / (W / (2. * focal)) * rays_o[..., 0] / rays_o[..., 2]
    o1 = -1. / (H / (2. * focal)) * rays_o[..., 1] / rays_o[..., 2]
    o2 = 1. + 2. * near / rays_o[..., 2]
    d0 = -1. / (W / (2. * focal)) * (rays_d[..., 0] / rays_d[..., 2] - rays_o[..., 0] / rays_o[..., 2])
    d1 = -1. / (H / (2. * focal)) * (rays_d[..., 1] / rays_d[..., 2] - rays_o[..., 1] / rays_o[..., 2])
    d2 = -2. * near / rays_o[..., 2]
    return torch.stack([o0, o1, o2], -1), torch.stack([d0, d1, d2], -1)


def render(H, W, K, chunk=1024 * 32, rays=None, c2w=None, ndc=True, near=0., far=1., use_viewdirs=False,
           c2w_staticcam=None, **kwargs):
    """run_nerf.py:69-134: [rgb_map, disp_map, acc_map, extras].  With c2w the ray records are built by one HIP
    launch (get_rays + view directions + ndc_rays + near / far: SURVEY 8 f-2), no [H,W,3] intermediates."""
    # (use_viewdirs=False: the 11-column ray records are built all the same; networks without view directions ignore columns 8-10)
    req = lambda t: isinstance(t, torch.Tensor) and t.requires_grad
    geo_grad = torch.is_grad_enabled() and (req(c2w) or req(c2w_staticcam) or (rays is not None and any(req(t) for t in rays)))
    if geo_grad and c2w is not None:
        # a pose that requires grad: the reference's own torch ops (get_rays, normalise, ndc_rays) carry d loss / d c2w
        rays = get_rays(H, W, K, c2w)
        c2w = None
    if c2w is not None:
        net = kwargs.get("network_fn")
        if net is None and kwargs.get("baked") is not None:     # no network: the rays are built where the baked field lives
            dev = kwargs["baked"].device
        else:
            dev = next(net.parameters()).device if net is not None else (c2w.device if isinstance(c2w, torch.Tensor) else None)
        rays = hb.make_rays(H, W, K, c2w, c2w_staticcam, ndc, near, far, dev)
        sh = (H, W, 3)
    elif (not geo_grad and c2w_staticcam is None and isinstance(rays[0], torch.Tensor) and rays[0].is_cuda
          and isinstance(near, (int, float)) and isinstance(far, (int, float))):
        # one launch: view directions + NDC warp + near / far columns -> [N, 11] records (run_nerf.py:100-123)
        rays_o, rays_d = rays
        sh = rays_d.shape
        rays = hb.assemble_rays(_f32c(rays_o).reshape(-1, 3), _f32c(rays_d).reshape(-1, 3), ndc, H, W, K[0][0], near, far)
    else:
        rays_o, rays_d = rays
        viewdirs = rays_d
        if c2w_staticcam is not None:       # run_nerf.py:103-105
            rays_o, rays_d = get_rays(H, W, K, c2w_staticcam)
        viewdirs = viewdirs / torch.norm(viewdirs, dim=-1, keepdim=True)
        viewdirs = torch.reshape(viewdirs, [-1, 3]).float()
        sh = rays_d.shape
        if ndc:
            rays_o, rays_d = ndc_rays(H, W, K[0][0], 1., rays_o, rays_d)
        rays_o = torch.reshape(rays_o, [-1, 3]).float()
        rays_d = torch.reshape(rays_d, [-1, 3]).float()
        near, far = near * torch.ones_like(rays_d[..., :1]), far * torch.ones_like(rays_d[..., :1])
        rays = torch.cat([rays_o, rays_d, near, far, viewdirs], -1)
    all_ret = batchify_rays(rays, chunk, **kwargs)
    for k in all_ret:
        k_sh = list(sh[:-1]) + list(all_ret[k].shape[1:])
        all_ret[k] = torch.reshape(all_ret[k], k_sh)
    k_extract = ['rgb_map', 'disp_map', 'acc_map']
    ret_list = [all_ret[k] for k in k_extract]
    ret_dict = {k: all_ret[k] for k in all_ret if k not in k_extract}
    return ret_list + [ret_dict]


to8b = lambda x: (255 * np.clip(x, 0, 1)).astype(np.uint8)
_MSE_SCRATCH = {}


class _Img2Mse(torch.autograd.Function):
    """run_nerf_helpers.py:11 on the device in one launch (+ one for the gradient) instead of sub / pow / mean and their three
    backward kernels: the loss of run_nerf.py:765-772 is evaluated twice per step."""

    @staticmethod
    def forward(ctx, x, y):
        xc, yc = x.contiguous(), y.contiguous()
        key = (str(x.device), hb._stream())         # (per stream: the kernel's ticket word must not be shared by concurrent launches)
        if key not in _MSE_SCRATCH:
            _MSE_SCRATCH[key] = torch.zeros(hb.lib().nerf_mse_scratch_floats(), dtype=torch.float32, device=x.device)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        hb._check(hb.lib().nerf_mse_fwd(xc.data_ptr(), yc.data_ptr(), xc.numel(), _MSE_SCRATCH[key].data_ptr(), out.data_ptr(), hb._stream()),
                  "nerf_mse_fwd")
        ctx.save_for_backward(xc, yc)
        return out

    @staticmethod
    def backward(ctx, g):
        xc, yc = ctx.saved_tensors
        dx = torch.empty_like(xc)
        hb._check(hb.lib().nerf_mse_bwd(xc.data_ptr(), yc.data_ptr(), xc.numel(), g.to(torch.float32).contiguous().data_ptr(), dx.data_ptr(),
                                        hb._stream()), "nerf_mse_bwd")
        return dx, (-dx if ctx.needs_input_grad[1] else None)


def img2mse(x, y):
    """run_nerf_helpers.py:11.  fp32 tensors of one shape on the GPU: one HIP launch; anything else (CPU tensors, broadcasting,
    other dtypes): the reference's expression."""
    if (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.is_cuda and y.is_cuda and x.dtype == torch.float32
            and y.dtype == torch.float32 and x.shape == y.shape and x.numel() > 0):
        return _Img2Mse.apply(x, y)
    return torch.mean((x - y) ** 2)


_LOG10 = {}


def mse2psnr(x):
    """run_nerf_helpers.py:12, same arithmetic and result shape ([1]); log(10) lives on x's device once instead of being uploaded at
    every call (a pageable host-to-device copy per step would make the host wait for the stream in the train() loop)"""
    t = _LOG10.get(x.device)
    if t is None:
        t = _LOG10[x.device] = torch.log(torch.tensor([10.])).to(x.device)
    return -10. * torch.log(x) / t


def _write_png(path, rgb8):
    """Minimal PNG writer (imageio is not a dependency of the hot path)."""
    import struct
    import zlib
    h, w, c = rgb8.shape
    rows = b"".join(b"\x00" + rgb8[y].tobytes() for y in range(h))

    def chunk(tag, data):
        body = tag + data
        return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body) & 0xffffffff)
    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 6, 0, 0, 0))
    png += chunk(b"IDAT", zlib.compress(rows, 6)) + chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(png)


class _FrameSink:
    """Output side of render_path.  The reference blocks on `.cpu().numpy()` and encodes every frame on
    the rendering thread (run_nerf.py:155-169).  Here frame i's device->host copies go to pinned memory asynchronously,
    `to8b` runs on the device, and the PNG of frame i-1 is encoded by a worker thread while frame i+1 renders; the
    returned arrays and files are the same."""

    def __init__(self, savedir=None, workers=2):
        self.savedir = savedir
        self.rgbs, self.disps, self.jobs = [], [], []
        self.pending = None
        self.pool = None
        if savedir is not None:
            from concurrent.futures import ThreadPoolExecutor
            self.pool = ThreadPoolExecutor(max_workers=workers)

    @staticmethod
    def _to_host(t):
        if not t.is_cuda:
            return t.detach().clone()
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t.detach(), non_blocking=True)
        return h

    def push(self, index, rgb, disp):
        rgb8 = None
        if self.savedir is not None:
            rgb8 = self._to_host((255 * rgb.detach().clamp(0, 1)).to(torch.uint8))      # to8b (helpers:11) on the device
        entry = (index, self._to_host(rgb), self._to_host(disp), rgb8)
        event = None
        if rgb.is_cuda:
            event = torch.cuda.Event()
            event.record()
        self._finish()                      # the previous frame: its copies had a whole frame time to land
        self.pending = (entry, event)

    def _finish(self):
        if self.pending is None:
            return
        (index, rgb, disp, rgb8), event = self.pending
        self.pending = None
        if event is not None:
            event.synchronize()
        self.rgbs.append(rgb.numpy())
        self.disps.append(disp.numpy())
        if rgb8 is not None:
            import os
            path = os.path.join(self.savedir, '{:03d}.png'.format(index))
            self.jobs.append(self.pool.submit(_write_png, path, rgb8.numpy()))

    def close(self):
        self._finish()
        for j in self.jobs:
            j.result()                      # re-raises an encoder / IO error
        if self.pool is not None:
            self.pool.shutdown()
        return np.stack(self.rgbs, 0), np.stack(self.disps, 0)


def render_path(render_poses, hwf, K, chunk, render_kwargs, gt_imgs=None, savedir=None, render_factor=0):
    """run_nerf.py:137-175: (rgbs[F,H,W,3], disps[F,H,W]) as numpy."""
    import os
    H, W, focal = hwf
    if render_factor != 0:
        H = H // render_factor
        W = W // render_factor
        focal = focal / render_factor
    sink = _FrameSink(savedir)
    for i, c2w in enumerate(render_poses):
        rgb, disp, acc, _ = render(H, W, K, chunk=chunk, c2w=c2w[:3, :4], **render_kwargs)
        sink.push(i, rgb, disp)
    return sink.close()

