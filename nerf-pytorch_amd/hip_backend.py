"""ctypes binding of libnerf_hip.so (C ABI: include/nerf_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every function
below hands raw device pointers of fp32 CUDA(ROCm) tensors to the library and
enqueues HIP kernels on ``torch.cuda.current_stream()``.

There is no fallback: if the library is missing or a call fails, this raises.
"""
import ctypes
import os
from typing import NamedTuple, Optional

import torch  # import torch BEFORE loading the library: one HIP runtime per process (torch's bundled one)

from . import build as _build

_c_float_p = ctypes.c_void_p
_LIB = None
ABI_VERSION = 10       # NERF_ABI_VERSION of include/nerf_hip.h this binding was written against


class NerfHipError(RuntimeError):
    pass


def _declare(lib):
    i, l, f, p, sz = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    sig = {
        "nerf_abi_version": (i, []),
        "nerf_last_error": (ctypes.c_char_p, []),
        "nerf_param_count": (i, []),
        "nerf_param_offset": (i, [i, ctypes.POINTER(i), ctypes.POINTER(i)]),
        "nerf_packed_floats": (i, []),
        "nerf_pack_params": (i, [p, p, p]),
        "nerf_debug_pack_table": (i, [p]),
        "nerf_embed": (i, [p, l, i, p, p]),
        "nerf_sample_coarse": (i, [p, i, i, p, i, i, p, p, p]),
        "nerf_sample_ray_batch": (i, [i, i, p, p, i, p, i, i, i, i, i, ctypes.c_uint, ctypes.c_uint, p, p, p, p]),
        "nerf_make_rays": (i, [i, i, p, p, p, i, f, f, p, i, p]),
        "nerf_assemble_rays": (i, [p, p, l, i, i, i, f, f, f, p, i, p]),
        "nerf_buffer_layout": (i, [p, ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(i)]),
        "nerf_debug_layout": (i, [i, i, i, i, ctypes.POINTER(ctypes.c_longlong)]),
        "nerf_act_floats": (sz, [i, i]),
        "nerf_workspace_floats": (sz, [i, i, i, i]),
        "nerf_pack_params_split_pair": (i, [p, p, p, p, i, i, p]),
        "nerf_act_floats_dp": (sz, [i, i, i]),
        "nerf_delta_floats_dp": (sz, [i, i, i]),
        "nerf_workspace_floats_dp": (sz, [i, i, i, i, i]),
        "nerf_field_fwd": (i, [p, p, i, p, i, i, p, p, p]),
        "nerf_raw2outputs": (i, [p, p, p, i, i, i, p, f, i, p, p, p, p, p, p]),
        "nerf_raw2outputs_bwd": (i, [p, p, p, i, i, i, p, f, i, p, p, p, p, p, p, p]),
        "nerf_sample_fine": (i, [p, p, i, i, i, p, p, p, p, p, p]),
        "nerf_distortion_fwd": (i, [p, p, p, i, i, i, p, p]),
        "nerf_distortion_bwd": (i, [p, p, p, i, i, i, p, p, i, p]),
        "nerf_interlevel_fwd": (i, [p, p, i, p, p, i, i, p, p]),
        "nerf_interlevel_bwd": (i, [p, p, i, p, p, i, i, p, p, i, p]),
        "nerf_sample_pdf": (i, [p, p, i, i, i, p, p, p, p]),
        "nerf_delta_floats": (sz, [i, i]),
        "nerf_wgrad_partial_floats": (sz, [i, i]),
        "nerf_field_bwd": (i, [p, p, p, i, i, p, p, p, i, p]),
        "nerf_field_dgrad": (i, [p, p, p, i, i, p, p]),
        "nerf_field_wgrad": (i, [p, p, p, i, i, p, p, i, p]),
        "nerf_packed3_floats": (i, []),
        "nerf_debug_pack3_table": (i, [p]),
        "nerf_field_wgrad_phase": (i, [p, p, p, i, i, p, p, i, i, i, p, p]),
        "nerf_pack_params_split": (i, [p, p, i, i, p]),
        "nerf_field_fwd_split": (i, [p, p, i, p, i, i, p, p, i, p]),
        "nerf_field_dgrad_split": (i, [p, p, p, i, i, p, i, p]),
        "nerf_field_fwd_last_sample": (i, [p, p, i, p, i, i, p, p, p, i, p]),
        "nerf_debug_pack16_table": (i, [p]),
        "nerf_adam_step": (i, [p, p, p, p, i, f, f, f, f, i, p]),
        "nerf_render_workspace_floats": (sz, [p, i, i]),
        "nerf_render_rays_fwd": (i, [p, p, p, p, i, i, p, p, p, p, p, p, p, p, p, p, p, p, p, i, p]),
        "nerf_render_rays_bwd": (i, [p, p, p, p, p, p, i, i, p, p, p, p, p, p, p, p, p, p, p, p, p, i, p]),
        "nerf_render_infer_supported": (i, [p]),
        "nerf_mse_scratch_floats": (i, []),
        "nerf_mse_fwd": (i, [p, p, l, p, p, p]),
        "nerf_mse_bwd": (i, [p, p, l, p, p, p]),
        "nerf_build_inputs": (i, [p, i, p, i, i, i, i, i, p, i, p]),
        "nerf_dense_fwd": (i, [p, i, i, p, i, p, p, i, i, l, i, i, p]),
        "nerf_dense_dgrad": (i, [p, i, i, p, i, p, i, i, l, i, p, i, p]),
        "nerf_dense_wgrad_scratch_floats": (sz, [l, i]),
        "nerf_dense_wgrad": (i, [p, i, i, p, i, i, l, p, i, p, p, i, p]),
        "nerf_render_rays_infer": (i, [p, p, p, p, i, i, p, p, p, p, p, p, p, p, p, p, p, p, p, p]),
        "nerf_range_scan": (i, [p, i, i, p, p]),
        "nerf_field_input_grad": (i, [p, p, p, i, p, i, i, p, i, p]),
        "nerf_raw2outputs_bwd_geom": (i, [p, p, p, i, i, i, p, f, i, p, p, p, p, p, p, p, p, p]),
        "nerf_embed_bwd": (i, [p, l, i, p, p, i, p]),
        "nerf_sample_ray_views": (i, [i, i, p, p, i, i, p, l, i, p, l, i, l, ctypes.c_uint, ctypes.c_uint, p, p, p, p, p]),
        "nerf_ray_pose_grad": (i, [i, p, p, i, p, p, i, p, i, p]),
        "nerf_occ_scratch_words": (sz, [l]),
        "nerf_occ_compact": (i, [p, p, i, p, i, i, p, p, p, p, p]),
        "nerf_occ_expand": (i, [p, p, l, p, p]),
        "nerf_occ_mark": (i, [p, l, i, f, p, p]),
        "nerf_occ_dilate": (i, [p, i, i, i, p, p]),
        "nerf_occ_gather": (i, [p, p, l, p, p]),
        "nerf_occ_fold_rays": (i, [p, p, p, i, i, p, i, p]),
        "nerf_occ_density_update": (i, [p, l, i, f, p, p]),
        "nerf_occ_ray_span": (i, [p, p, i, i, p, p, p]),
        "nerf_occ_proposal_weights": (i, [p, p, f, p, i, p, i, i, p, p, p]),
        "nerf_occ_stop_depth": (i, [p, p, i, i, f, p, p]),
        "nerf_occ_compact_stop": (i, [p, p, i, p, p, i, i, p, p, p, p, p]),
        "nerf_occ_march": (i, [p, p, i, p, i, i, i, p, p, p, p]),
        "nerf_occ_march_stop": (i, [p, p, f, p, i, p, i, i, i, f, p, p, p, p, p]),
        "nerf_occ_march_step": (i, [p, p, f, p, i, p, i, f, i, i, i, f, p, p, p, p, p, p]),
        "nerf_occ_view_carve": (i, [p, p, p, i, i, i, f, f, f, p, i, p, p, p]),
        "nerf_iso_scratch_words": (sz, [i, i, i]),
        "nerf_iso_count": (i, [p, i, i, i, f, p, p, p, p]),
        "nerf_iso_emit": (i, [p, i, i, i, f, p, p, p, p, p, p, p]),
        "nerf_baked_render": (i, [p, p, p, i, i, p, i, p, i, f, i, f, i, p, p, p, p, p, p]),
        "nerf_baked_count": (i, [p, p, i, p, i, f, i, p, p]),
        "nerf_baked_train_fwd": (i, [p, p, p, i, i, p, i, p, i, f, i, i, p, i, p, p, p, p, p]),
        "nerf_baked_train_bwd_samples": (i, [p, p, i, i, f, i, p, p, p, p, p]),
        "nerf_baked_train_bwd_rows": (i, [p, p, i, i, p, i, i, p, p, p, p, i, p, p]),
        "nerf_baked_train_bwd_rays": (i, [p, p, p, i, i, p, i, i, p, p, p, i, p, p]),
        "nerf_baked_reg_fwd": (i, [p, p, p, p, i, i, f, f, f, f, p, p]),
        "nerf_baked_reg_bwd": (i, [p, p, p, p, i, i, f, f, f, f, p, p, p]),
        "nerf_hash_scratch_words": (sz, [p]),
        "nerf_hash_encode_fwd": (i, [p, p, p, p, i, p, i, l, p, i, p]),
        "nerf_hash_encode_bwd": (i, [p, p, p, i, p, i, l, p, i, p, p, i, p]),
        "nerf_hash_input_grad_workspace_floats": (sz, [l]),
        "nerf_hash_input_grad": (i, [p, p, p, p, i, p, i, l, p, i, i, i, p, p, p, i, p]),
        "nerf_live_tiles_words": (sz, [i, i]),
        "nerf_bwd_skip_dead": (i, []),
        "nerf_field_dgrad_split_live": (i, [p, p, p, i, i, p, i, p, p]),
        "nerf_field_wgrad_phase_live": (i, [p, p, p, i, i, p, p, i, i, i, p, p, p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)      # AttributeError here = header / library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    return sig


EXPORTS = ["nerf_abi_version", "nerf_last_error", "nerf_param_count", "nerf_param_offset", "nerf_packed_floats",
           "nerf_pack_params", "nerf_debug_pack_table", "nerf_embed", "nerf_make_rays", "nerf_assemble_rays", "nerf_sample_coarse", "nerf_sample_ray_batch", "nerf_buffer_layout", "nerf_debug_layout", "nerf_act_floats", "nerf_workspace_floats", "nerf_field_fwd",
           "nerf_raw2outputs", "nerf_raw2outputs_bwd", "nerf_sample_fine", "nerf_sample_pdf", "nerf_delta_floats", "nerf_pack_params_split_pair", "nerf_act_floats_dp", "nerf_delta_floats_dp", "nerf_workspace_floats_dp",
           "nerf_wgrad_partial_floats", "nerf_field_bwd", "nerf_field_dgrad", "nerf_field_wgrad",
           "nerf_packed3_floats", "nerf_debug_pack3_table",
           "nerf_field_wgrad_phase", "nerf_debug_pack16_table",
           "nerf_pack_params_split", "nerf_field_fwd_split", "nerf_field_dgrad_split", "nerf_field_fwd_last_sample",
           "nerf_adam_step",
           "nerf_render_workspace_floats", "nerf_render_rays_fwd", "nerf_render_rays_bwd", "nerf_render_infer_supported",
           "nerf_render_rays_infer", "nerf_mse_scratch_floats", "nerf_mse_fwd", "nerf_mse_bwd", "nerf_build_inputs", "nerf_dense_fwd", "nerf_dense_dgrad", "nerf_dense_wgrad_scratch_floats",
           "nerf_dense_wgrad", "nerf_range_scan", "nerf_field_input_grad", "nerf_raw2outputs_bwd_geom", "nerf_embed_bwd",
           "nerf_sample_ray_views", "nerf_ray_pose_grad",
           "nerf_occ_scratch_words", "nerf_occ_compact", "nerf_occ_expand", "nerf_occ_mark", "nerf_occ_dilate",
           "nerf_occ_gather", "nerf_occ_fold_rays", "nerf_occ_density_update", "nerf_occ_ray_span", "nerf_occ_proposal_weights",
           "nerf_occ_stop_depth", "nerf_occ_compact_stop", "nerf_occ_march", "nerf_occ_march_stop", "nerf_occ_march_step",
           "nerf_occ_view_carve",
           "nerf_iso_scratch_words", "nerf_iso_count", "nerf_iso_emit", "nerf_baked_render",
           "nerf_baked_count", "nerf_baked_train_fwd", "nerf_baked_train_bwd_samples", "nerf_baked_train_bwd_rows",
           "nerf_baked_train_bwd_rays",
           "nerf_baked_reg_fwd", "nerf_baked_reg_bwd",
           "nerf_hash_scratch_words", "nerf_hash_encode_fwd", "nerf_hash_encode_bwd",
           "nerf_hash_input_grad_workspace_floats", "nerf_hash_input_grad",
           "nerf_live_tiles_words", "nerf_bwd_skip_dead", "nerf_field_dgrad_split_live", "nerf_field_wgrad_phase_live",
           "nerf_distortion_fwd", "nerf_distortion_bwd", "nerf_interlevel_fwd", "nerf_interlevel_bwd"]


def lib():
    """Load (once) and return the shared library.  Raises if it has not been built."""
    global _LIB
    if _LIB is None:
        # (NERF_HIP_LIB: another build of the same ABI -- kernel A/B timing on one box, tools/time_kernels.py)
        path = os.environ.get("NERF_HIP_LIB") or _build.LIB_PATH
        if not os.path.exists(path):
            raise NerfHipError(
                f"{path} not found: build it with `python __graft_entry__.py build` (hipcc --offload-arch=gfx950). "
                "There is no PyTorch fallback for the render hot path.")
        _LIB = ctypes.CDLL(path)
        _declare(_LIB)
        if _LIB.nerf_abi_version() != ABI_VERSION:
            raise NerfHipError("libnerf_hip.so ABI version mismatch")
    return _LIB


def _check(rc, name):
    if rc != 0:
        raise NerfHipError(f"{name} failed (code {rc}): {lib().nerf_last_error().decode()}")


def _ptr(t, name="tensor", optional=False):
    if t is None:
        if optional:
            return None
        raise NerfHipError(f"{name} is required")
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise NerfHipError(f"{name} must be a contiguous fp32 tensor on the GPU "
                           f"(got {type(t).__name__} {getattr(t, 'dtype', None)} {getattr(t, 'device', None)})")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """Optional HIP-event bracketing of the heavy launches (bench.py).  Events are recorded on torch's
    current stream, which is the stream the kernels are enqueued on.  `work` = algorithmic FLOPs."""

    def __init__(self):
        self.records = []       # (name, start_event, end_event, algorithmic flops, algorithmic HBM bytes)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1, fl, by in self.records:
            d = out.setdefault(name, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += fl
            d["bytes"] += by
        return out


TIMER = None        # set to a KernelTimer() to enable


class _timed:
    def __init__(self, name, flops, nbytes=0.0):
        self.name, self.flops, self.nbytes = name, flops, nbytes

    def __enter__(self):
        if TIMER is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if TIMER is not None:
            self.e1.record()
            TIMER.records.append((self.name, self.e0, self.e1, self.flops, self.nbytes))


FLOP_FWD_PER_POINT = 2 * 593408
FLOP_DGRAD_PER_POINT = 2 * 557696
FLOP_WGRAD_PER_POINT = 2 * 593408
FLOP_WGRAD_BIG_PER_POINT = 2 * 8 * 256 * 256            # the eight full-width jobs
# algorithmic HBM bytes per point (SURVEY §8d / DESIGN.md §2): what a launch must move once
BYTES_ACT_PER_POINT = 4 * (9 * 256 + 128 + 64 + 32) + 32 * 9 + 16  # saved activations + encodings + ReLU bitmasks (256 bits x 9 layers) + raw
BYTES_DELTA_PER_POINT = 4 * (9 * 256 + 128)             # deltas written by dgrad
BYTES_WGRAD_BIG_PER_POINT = 4 * 8 * (256 + 256)         # each full-width job reads its delta and its input once
BYTES_WGRAD_SMALL_PER_POINT = 4 * (2 * (256 + 64) + (4 + 256) + (128 + 256) + (128 + 32) + (4 + 128))
# split datapaths: feature_linear is folded into the view branch (csrc/nerf_common.h): one 256x256 layer
# less is EXECUTED in each of the three kernels, `feature` and its delta are neither written nor re-read
FOLD_MAC = 256 * 256
FLOP_FWD3_PER_POINT = 2 * (593408 - FOLD_MAC)
FLOP_DGRAD3_PER_POINT = 2 * (557696 - FOLD_MAC)
FLOP_WGRAD3_PER_POINT = 2 * (593408 - FOLD_MAC)
BYTES_ACT3_PER_POINT = BYTES_ACT_PER_POINT - 4 * 256
BYTES_DELTA3_PER_POINT = BYTES_DELTA_PER_POINT - 4 * 256
BYTES_ACT3_BF16_PER_POINT = 2 * (8 * 256 + 128 + 64) + 32 * 9 + 16  # bf16 rows + encodings, ReLU bitmasks, raw
BYTES_DELTA3_BF16_PER_POINT = 2 * (8 * 256 + 128 + 4)
BYTES_ACT3_LO_PER_POINT = 2 * (8 * 256 + 128 + 64)        # "fp16x3w": the lo words of the saved rows and of the xyz encoding
# 12 jobs on 16-bit operands (round 5: the alpha head's row rides on the (delta_hv, h7) job -- h7 is not re-read for it): 9,808 B per
# point (PMC: 9.83 KB)
BYTES_WGRAD_MIXED_PER_POINT = 0.5 * (BYTES_WGRAD_BIG_PER_POINT + BYTES_WGRAD_SMALL_PER_POINT - 4 * (256 + 256)) - 2 * 256


N_PARAMS = 595844


def param_table():
    """[(name, offset, shape)] of the flat parameter vector, from the library itself."""
    L = lib()
    names = []
    for i in range(8):
        names += [f"pts_linears.{i}.weight", f"pts_linears.{i}.bias"]
    names += ["views_linears.0.weight", "views_linears.0.bias", "feature_linear.weight", "feature_linear.bias",
              "alpha_linear.weight", "alpha_linear.bias", "rgb_linear.weight", "rgb_linear.bias"]
    out = []
    for idx, nm in enumerate(names):
        r, c = ctypes.c_int(), ctypes.c_int()
        off = L.nerf_param_offset(idx, ctypes.byref(r), ctypes.byref(c))
        shape = (r.value, c.value) if nm.endswith("weight") else (r.value,)
        out.append((nm, off, shape))
    return out


def pack_table():
    """Host-side gather table of the fragment repack (numpy int32, -1 = zero padding)."""
    import numpy as np
    L = lib()
    tab = np.empty(L.nerf_packed_floats(), dtype=np.int32)
    _check(L.nerf_debug_pack_table(tab.ctypes.data_as(ctypes.c_void_p)), "nerf_debug_pack_table")
    return tab


# "fp16x3" / "bf16x3": the three-term split W x = W_hi x_hi + W_hi x_lo + W_lo x_hi with fp16 / bf16 parts (csrc/split_types.h) on the
# weight-ring kernels; the operands of the weight-gradient GEMM are the stored hi words (11 / 8 significant bits).
# "fp16x3" (round 4) = the same three-term split with IEEE-half parts (csrc/split_types.h): ~2^-22 per product instead of 2^-17
# and 11-bit instead of 8-bit operands for the weight-gradient GEMM, at the bf16 MFMA count; needs |activations| < 65520.
# "fp16_fp8c" (round 4, INFERENCE class): no_grad rendering with every product of the 256-wide layers as fp16 main term + two fp8
# correction terms (csrc/field_ring8.h: ~2^-15 per product, 2 instead of 3 MFMA-equivalents; every ray's last sample re-evaluated
# with the three-term fp16 products); anything that needs gradients runs the fp16x3 datapath unchanged.  Never the bench headline.
# "fp16x3w" (round 6): fp16x3 with TWO-WORD operands in the weight-gradient GEMM -- the forward and the delta chain save the lo words
# next to the hi words and the GEMM contracts d_hi X_hi + d_hi X_lo + d_lo X_hi (the forward's product class, ~2^-22, instead of 11-bit
# operands) at twice the saved bytes and three times the GEMM's MFMAs.  Forward values are bit-identical to fp16x3's.  Not the default:
# it is the instrument that prices the one-word operand storage (profiles/r06_*).
class Datapath(NamedTuple):
    """One precision name in every vocabulary of the C ABI (the table at the top of include/nerf_hip.h) and of the timer.  None = the
    datapath has no such form: the fp32 entry points carry no code, the reduced inference class saves and trains nothing."""
    family: int                     # layout family of nerf_*_floats_dp / nerf_debug_layout: 0 fp32 rows, 1 16-bit tiles, 2 hi + lo tiles
    fwd_split: Optional[int]        # `split` of nerf_field_fwd_split without a save buffer
    save_split: Optional[int]       # ... with one, and of nerf_field_dgrad_split[_live]
    pack_of: str                    # whose fragment repack its kernels read: that datapath's ...
    pack_streams: int               # ... `streams` and
    pack_split: Optional[int]       # ... `split` of nerf_pack_params_split[_pair]
    cfg: Optional[int]              # NerfRenderCfg.precision
    wgrad: Optional[int]            # `datapath` of nerf_field_wgrad_phase[_live] (the binding itself passes -1, "as recorded")
    elem16: Optional[torch.dtype]   # element type of the saved rows and deltas
    fwd_label: str                  # KernelTimer labels: the forward without ...
    save_label: Optional[str]       # ... and with saving,
    dgrad_label: Optional[str]      # the delta chain,
    gemm_label: Optional[str]       # the streaming weight-gradient GEMM
    bytes_save: float = 0.0         # algorithmic HBM bytes per point: a saving forward,
    bytes_dgrad: float = 0.0        # the delta chain,
    bytes_gemm: float = 0.0         # the GEMM

    @property
    def fp16_saves(self):
        """saves fp16 rows and deltas: the datapaths the RangeMonitor watches"""
        return self.save_split is not None and self.elem16 is torch.float16


PACK_ALL_STREAMS = 1 | 4        # the 16-point forward stream and the transposed streams of the delta chain
DATAPATHS = {
    "fp32": Datapath(0, None, None, "fp32", 0, None, 0, 0, None, "field_fwd_kernel", "field_fwd_kernel<save>", "field_dgrad_kernel", None,
                     BYTES_ACT_PER_POINT, BYTES_DELTA_PER_POINT),
    "fp16x3": Datapath(1, 1, 1, "fp16x3", PACK_ALL_STREAMS, 1, 3, 5, torch.float16, "field_fwd16r_kernel<fp16>", "field_fwd16r_kernel<fp16, save>",
                       "field_dgrad3r_kernel<fp16>", "wgrad1_kernel<fp16>", BYTES_ACT3_BF16_PER_POINT, BYTES_DELTA3_BF16_PER_POINT, BYTES_WGRAD_MIXED_PER_POINT),
    "bf16x3": Datapath(1, 0, 0, "bf16x3", PACK_ALL_STREAMS, 0, 1, 4, torch.bfloat16, "field_fwd16r_kernel", "field_fwd16r_kernel<save bf16>",
                       "field_dgrad3r_kernel<bf16 out>", "wgrad1_kernel", BYTES_ACT3_BF16_PER_POINT, BYTES_DELTA3_BF16_PER_POINT, BYTES_WGRAD_MIXED_PER_POINT),
    # the reduced inference stream (fp16 main + fp8 correction fragments) in the 16-point forward stream's slot; 3 = last sample left out
    "fp16_fp8c": Datapath(1, 3, None, "fp16_fp8c", 1, 2, None, None, torch.float16, "field_fwd16r_kernel<fp16 + fp8c>", None, None, None),
    # (5: two-word saves; the inference forward and the repack are fp16x3's)
    "fp16x3w": Datapath(2, 1, 5, "fp16x3", PACK_ALL_STREAMS, 1, 5, 6, torch.float16, "field_fwd16r_kernel<fp16>", "field_fwd16r_kernel<fp16, save hi+lo>",
                        "field_dgrad3r_kernel<fp16, hi+lo>", "wgrad1_kernel<fp16, 3 terms>", BYTES_ACT3_BF16_PER_POINT + BYTES_ACT3_LO_PER_POINT,
                        2 * BYTES_DELTA3_BF16_PER_POINT, 2 * BYTES_WGRAD_MIXED_PER_POINT),
}
PRECISIONS = tuple(DATAPATHS)
SPLIT = tuple(p for p, d in DATAPATHS.items() if d.family)     # datapaths on the three-term-split kernels (folded feature layer, tiled saves)
PACK_OF = {p: d.pack_of for p, d in DATAPATHS.items() if d.pack_of != p}    # datapaths that read another datapath's fragment repack


def _datapath(precision):
    if precision not in DATAPATHS:
        raise ValueError(f"precision must be one of {PRECISIONS}")
    return DATAPATHS[precision]


def pack_table3():
    """Host-side gather table of the TRANSPOSED (hi, lo) fragment streams of the delta chain (the first region of the packed3 buffer:
    W'^T | feature_linear^T | L7^T .. L1^T): per 16-bit element 2*canonical_index + is_lo, -1 = padding."""
    import numpy as np
    L = lib()
    # packed3 = transposed (hi, lo) streams | fp32 small parameters | 16-point forward stream (P16F) | derived W', b'
    n16 = 2 * (L.nerf_packed3_floats() - (L.nerf_packed_floats() - _small_offset()) - P16F_WORDS - N_DERIVED)
    tab = np.empty(n16, dtype=np.int32)
    _check(L.nerf_debug_pack3_table(tab.ctypes.data_as(ctypes.c_void_p)), "nerf_debug_pack3_table")
    return tab


P16F_WORDS = 593920        # csrc/nerf_common.h: words of the 16-point forward stream
N_DERIVED = 128 * 256 + 128  # csrc/nerf_common.h: W' = Wv[:, :256] Wf and b' (folded feature layer), appended to packed3;
#                              in the pack tables they are "canonical" indices N_PARAMS + k*256 + j, N_PARAMS + 32768 + k


def pack_table16():
    """Host-side gather table of the 16-point inference stream: per 16-bit element 2*canonical_index + is_lo, -1 = padding."""
    import numpy as np
    tab = np.empty(2 * P16F_WORDS, dtype=np.int32)
    _check(lib().nerf_debug_pack16_table(tab.ctypes.data_as(ctypes.c_void_p)), "nerf_debug_pack16_table")
    return tab


def _small_offset():
    # SM_BIAS of csrc/nerf_common.h = first word after the fp32 forward + backward weight streams
    return 593408 + 557056


def pack_params(flat, out=None, precision="fp32"):
    L = lib()
    dp = DATAPATHS.get(precision, DATAPATHS["fp32"])
    split = dp.pack_split is not None       # the (hi, lo) fragments of the split's type, in the streams its kernels read
    if out is None:
        out = torch.empty(L.nerf_packed3_floats() if split else L.nerf_packed_floats(), dtype=torch.float32, device=flat.device)
    if split:
        _check(L.nerf_pack_params_split(_ptr(flat, "params"), _ptr(out, "packed"), dp.pack_streams, dp.pack_split, _stream()), "nerf_pack_params_split")
    else:
        _check(L.nerf_pack_params(_ptr(flat, "params"), _ptr(out, "packed"), _stream()), "nerf_pack_params")
    return out


def pack_params_pair(flat_a, flat_b, precision):
    """the (hi, lo) fragment repack of two networks in the two launches one takes (nerf_pack_params_split_pair; fp16x3 / bf16x3)"""
    L = lib()
    dp = DATAPATHS[precision]
    if dp.pack_streams != PACK_ALL_STREAMS:
        raise NerfHipError(f"pack_params_pair: {precision!r} has no paired repack")
    out_a = torch.empty(L.nerf_packed3_floats(), dtype=torch.float32, device=flat_a.device)
    out_b = torch.empty(L.nerf_packed3_floats(), dtype=torch.float32, device=flat_a.device)
    _check(L.nerf_pack_params_split_pair(_ptr(flat_a, "params"), _ptr(out_a, "packed"), _ptr(flat_b, "params"), _ptr(out_b, "packed"), dp.pack_streams, dp.pack_split,
                                         _stream()), "nerf_pack_params_split_pair")
    return out_a, out_b


def embed(x, n_freqs):
    x = x.contiguous()
    out = torch.empty(x.shape[:-1] + (3 + 6 * n_freqs,), dtype=torch.float32, device=x.device)
    n = x.numel() // 3
    _check(lib().nerf_embed(_ptr(x, "x"), n, n_freqs, _ptr(out), _stream()), "nerf_embed")
    return out


def sample_coarse(rays, t_vals, lindisp, t_rand):
    n, stride = rays.shape
    S = t_vals.numel()
    z = torch.empty((n, S), dtype=torch.float32, device=rays.device)
    _check(lib().nerf_sample_coarse(_ptr(rays, "rays"), stride, n, _ptr(t_vals, "t_vals"), S, int(bool(lindisp)),
                                    _ptr(t_rand, "t_rand", True), _ptr(z), _stream()), "nerf_sample_coarse")
    return z


def make_rays(H, W, K, c2w, c2w_staticcam, ndc, near, far, device):
    """[H*W, 11] ray records of render(c2w=...) in one launch (get_rays + viewdirs + ndc_rays + near/far)."""
    import numpy as np

    def host(m, shape):
        if m is None:
            return None
        if isinstance(m, torch.Tensor):
            m = m.detach().cpu().numpy()
        return np.ascontiguousarray(np.asarray(m, dtype=np.float32)[:shape[0], :shape[1]])
    Kh, ph, sh = host(K, (3, 3)), host(c2w, (3, 4)), host(c2w_staticcam, (3, 4))
    rays = torch.empty((H * W, 11), dtype=torch.float32, device=device)
    as_p = lambda arr: None if arr is None else arr.ctypes.data_as(ctypes.c_void_p)
    _check(lib().nerf_make_rays(int(H), int(W), as_p(Kh), as_p(ph), as_p(sh), int(bool(ndc)), float(near), float(far),
                                _ptr(rays), 11, _stream()), "nerf_make_rays")
    return rays


def assemble_rays(rays_o, rays_d, ndc, H, W, focal, near, far):
    """[N, 11] ray records of render(rays=(rays_o, rays_d), ...) in one launch (view directions + ndc_rays + near / far)."""
    n = rays_o.numel() // 3
    rays = torch.empty((n, 11), dtype=torch.float32, device=rays_o.device)
    _check(lib().nerf_assemble_rays(_ptr(rays_o, "rays_o"), _ptr(rays_d, "rays_d"), n, int(bool(ndc)), int(H), int(W),
                                    float(focal), float(near), float(far), _ptr(rays), 11, _stream()), "nerf_assemble_rays")
    return rays


def sample_ray_batch(H, W, K, pose, image, n_rand, window, key, want_pixels=False):
    """nerf_sample_ray_batch: n_rand distinct pixels of `image` inside window = (h0, w0, nh, nw), their rays and colours in one launch.
    pose: device tensor holding c2w[:3,:4] (a view into a [N,4,4] pose table is fine); key: two 32-bit words."""
    import numpy as np
    Kh = np.ascontiguousarray(np.asarray(K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else K, dtype=np.float32)[:3, :3])
    if not (isinstance(pose, torch.Tensor) and pose.is_cuda and pose.dtype == torch.float32 and pose.dim() == 2 and pose.shape[0] >= 3
            and pose.shape[1] >= 4 and pose.stride(1) == 1):
        raise NerfHipError("sample_ray_batch: pose must be a float32 [3+, 4] device tensor with contiguous rows")
    dev = image.device
    rays = torch.empty((2, n_rand, 3), dtype=torch.float32, device=dev)
    target = torch.empty((n_rand, 3), dtype=torch.float32, device=dev)
    pix = torch.empty((n_rand,), dtype=torch.int32, device=dev) if want_pixels else None
    h0, w0, nh, nw = (int(v) for v in window)
    _check(lib().nerf_sample_ray_batch(int(H), int(W), Kh.ctypes.data_as(ctypes.c_void_p), pose.data_ptr(), int(pose.stride(0)),
                                       _ptr(image, "image"), h0, w0, nh, nw, int(n_rand), int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff,
                                       _ptr(rays), _ptr(target), pix.data_ptr() if pix is not None else None, _stream()),
           "nerf_sample_ray_batch")
    return (rays, target, pix) if want_pixels else (rays, target)


def _host_K(K):
    import numpy as np
    return np.ascontiguousarray(np.asarray(K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else K, dtype=np.float32)[:3, :3])


def _iptr(t, name, optional=False):
    if t is None and optional:
        return None
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise NerfHipError(f"{name} must be a contiguous int32 tensor on the GPU")
    return t.data_ptr()


def sample_ray_views(H, W, K, view_ids, poses, images, n_rand, batch, key, want_pixels=False, want_views=False):
    """nerf_sample_ray_views: batch `batch` (B = min(n_rand, V*H*W - batch*n_rand) rays) of the epoch keyed by `key` over the
    (view, pixel) space of view_ids (device int32 [V], indices into poses [N, 3+, 4] and images [N, H, W, 3]).
    Returns (batch_rays [2, B, 3], target [B, 3], pixels [B] or None, views [B] or None)."""
    Kh = _host_K(K)
    if not (isinstance(poses, torch.Tensor) and poses.is_cuda and poses.dtype == torch.float32 and poses.dim() == 3 and poses.shape[1] >= 3
            and poses.shape[2] >= 4 and poses.stride(2) == 1):
        raise NerfHipError("sample_ray_views: poses must be a float32 [N, 3+, 4] device tensor with contiguous rows")
    if not (isinstance(images, torch.Tensor) and images.is_cuda and images.dtype == torch.float32 and images.dim() == 4
            and tuple(images.shape[1:]) == (H, W, 3) and images.shape[0] == poses.shape[0] and images[0].is_contiguous()):
        raise NerfHipError("sample_ray_views: images must be a float32 [N, H, W, 3] device tensor with contiguous views, N = len(poses)")
    V = view_ids.numel()
    total = V * H * W
    n_out = min(int(n_rand), total - int(batch) * int(n_rand))
    if n_out <= 0:
        raise NerfHipError("sample_ray_views: batch lies past the end of the epoch")
    dev = images.device
    rays = torch.empty((2, n_out, 3), dtype=torch.float32, device=dev)
    target = torch.empty((n_out, 3), dtype=torch.float32, device=dev)
    pix = torch.empty((n_out,), dtype=torch.int32, device=dev) if want_pixels else None
    vw = torch.empty((n_out,), dtype=torch.int32, device=dev) if want_views else None
    _check(lib().nerf_sample_ray_views(int(H), int(W), Kh.ctypes.data_as(ctypes.c_void_p), _iptr(view_ids, "view_ids"), V, poses.shape[0],
                                       poses.data_ptr(), int(poses.stride(0)), int(poses.stride(1)), images.data_ptr(),
                                       int(images.stride(0)), int(n_rand), int(batch), int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff,
                                       _ptr(rays), _ptr(target), None if pix is None else pix.data_ptr(), None if vw is None else vw.data_ptr(),
                                       _stream()), "nerf_sample_ray_views")
    return rays, target, pix, vw


def ray_pose_grad(W, K, d_rays, pixels, views, n_views, d_pose=None, accumulate=False):
    """nerf_ray_pose_grad: d_pose [n_views, 3, 4] (+)= d loss / d c2w[:3, :4] of each view from d_rays [2, B, 3] (views None: one view)."""
    Kh = _host_K(K)
    d_rays = d_rays.contiguous()
    n = d_rays.shape[1]
    if not (d_rays.dim() == 3 and d_rays.shape[0] == 2 and d_rays.shape[2] == 3 and pixels.numel() == n
            and (views is None or views.numel() == n)):
        raise NerfHipError("ray_pose_grad: d_rays must be [2, B, 3], pixels (and views) [B]")
    if d_pose is None:
        d_pose = torch.empty((n_views, 3, 4), dtype=torch.float32, device=d_rays.device)
    elif d_pose.numel() != 12 * n_views:
        raise NerfHipError("ray_pose_grad: d_pose must be [n_views, 3, 4]")
    _check(lib().nerf_ray_pose_grad(int(W), Kh.ctypes.data_as(ctypes.c_void_p), _ptr(d_rays, "d_rays"), n, _iptr(pixels, "pixels"),
                                    _iptr(views, "views", optional=True), int(n_views), _ptr(d_pose, "d_pose"), int(bool(accumulate)),
                                    _stream()), "nerf_ray_pose_grad")
    return d_pose


def act_floats(n_rays, n_samples, precision=None):
    """floats of a save buffer: for `precision`'s layout (fp32 rows: 10.6 KB / point; split datapaths' 16-bit tiles: 4.8 KB / point), or,
    without a precision, the larger of the two (a buffer any datapath may write)"""
    if precision is None:
        return lib().nerf_act_floats(int(n_rays), int(n_samples))
    return lib().nerf_act_floats_dp(int(n_rays), int(n_samples), _datapath(precision).family)


def delta_floats(n_rays, n_samples, precision=None):
    """floats of the delta scratch of one backward pass (see act_floats)"""
    if precision is None:
        return lib().nerf_delta_floats(int(n_rays), int(n_samples))
    return lib().nerf_delta_floats_dp(int(n_rays), int(n_samples), _datapath(precision).family)


class Workspace:
    """Caller-owned, persistent scratch of the backward path (the library allocates nothing and keeps no
    pointer).  The saved activations of a forward live from the forward to its backward; the deltas and the per-chunk
    partial gradients live inside one field_bwd call.  Buffers are LEASED from this pool (take) and handed back (give):
    a training loop of fixed shape re-uses the same device buffers every step -- same pointers, no allocation -- and a
    forward whose backward is still pending simply keeps its lease (a second forward leases another buffer).  A lease
    that is never returned (graph dropped without backward) is an ordinary tensor and is freed with its owner."""
    MAX_FREE = 16

    def __init__(self):
        self._free = {}

    def take(self, n_floats, device):
        free = self._free.setdefault(str(device), [])
        best = None
        for i, t in enumerate(free):
            # best fit; among equally sized buffers the lowest address, so that the choice does not depend on the order
            # in which earlier leases came back
            if t.numel() >= n_floats and (best is None or (t.numel(), t.data_ptr()) < (free[best].numel(), free[best].data_ptr())):
                best = i
        if best is not None and free[best].numel() <= 2 * n_floats + (1 << 20):
            return free.pop(best)
        return torch.empty(max(int(n_floats), 1), dtype=torch.float32, device=device)

    def give(self, t):
        if t is None:
            return
        free = self._free.setdefault(str(t.device), [])
        if any(f.data_ptr() == t.data_ptr() for f in free):
            return
        free.append(t)
        if len(free) > self.MAX_FREE:       # (list.remove would compare tensors elementwise)
            free.pop(min(range(len(free)), key=lambda i: free[i].numel()))

    def idle_bytes(self, device, at_least_floats=0):
        """bytes of the idle leases on `device` that a take() of at_least_floats can re-use instead of allocating (a lease smaller than
        the request serves nothing; take() also passes over leases more than twice the request)"""
        return 4 * sum(t.numel() for t in self._free.get(str(device), []) if t.numel() >= at_least_floats)

    def clear(self):
        self._free.clear()


WORKSPACE = Workspace()
SAVE_BUDGET_BYTES = int(float(os.environ.get("NERF_SAVE_BUDGET_GB", "48")) * (1 << 30))
# what ONE render_rays call may keep alive for its backward in total (a ray chunk above SAVE_BUDGET_BYTES is rendered in
# sub-chunks that each keep their own saved activations, as long as all of them fit here: 160 of the 288 GB of an MI355X)
SAVE_TOTAL_BYTES = int(float(os.environ.get("NERF_SAVE_TOTAL_GB", "160")) * (1 << 30))


def workspace_floats(n_rays, n_coarse, n_fine, training=True, precision=None):
    """nerf_workspace_floats[_dp](): floats of scratch one training render_rays call needs (saved activations of both
    passes + deltas + partial gradients of the larger pass) on `precision`'s layouts (None: the larger of the two); 0 for inference."""
    if precision is None:
        return lib().nerf_workspace_floats(int(n_rays), int(n_coarse), int(n_fine), int(bool(training)))
    return lib().nerf_workspace_floats_dp(int(n_rays), int(n_coarse), int(n_fine), int(bool(training)), _datapath(precision).family)


def max_saved_rays(n_coarse, n_fine, precision=None):
    """Largest ray count whose backward scratch fits SAVE_BUDGET_BYTES (multiple of 1024, at least 1024): larger ray
    chunks are back-propagated in sub-chunks of this size (render._RenderRays).  64 + 128 samples under the default 48 GiB:
    10,240 rays on fp32 rows, 21,504 on the split datapaths' 16-bit tiles."""
    per_1024 = 4 * workspace_floats(1024, n_coarse, n_fine, True, precision)
    return max(1, SAVE_BUDGET_BYTES // max(per_1024, 1)) * 1024


def saved_bytes(n_rays, n_coarse, n_fine, precision=None):
    """bytes of saved activations (both passes) a training render_rays call over n_rays keeps until its backward"""
    return 4 * (act_floats(n_rays, n_coarse, precision) + (act_floats(n_rays, n_coarse + n_fine, precision) if n_fine > 0 else 0))


class NerfRenderCfg(ctypes.Structure):
    """include/nerf_hip.h NerfRenderCfg (render_rays in one call)"""
    _fields_ = [("n_coarse", ctypes.c_int), ("n_fine", ctypes.c_int), ("lindisp", ctypes.c_int), ("white_bkgd", ctypes.c_int),
                ("raw_noise_std", ctypes.c_float), ("precision", ctypes.c_int), ("reserved", ctypes.c_int)]


ACT_LAYOUTS = {0: "fp32 rows", 1: "tile32 fp32", 2: "tile32 bf16", 3: "tile16 fp32", 4: "tile16 bf16", 5: "tile16 fp16", 6: "tile16 fp16 hi + lo"}


def buffer_layout(buf):
    """What the library recorded for a scratch buffer it wrote (nerf_buffer_layout): (kind, is_delta, n_rays, n_samples),
    kind -1 = unknown.  act kinds: ACT_LAYOUTS; delta kinds: 0 fp32 rows, 1 / 2 tiles fp32 / bf16."""
    d, n, s_ = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    kind = lib().nerf_buffer_layout(buf.data_ptr(), ctypes.byref(d), ctypes.byref(n), ctypes.byref(s_))
    return kind, bool(d.value), n.value, s_.value


def _row16(f):
    """csrc/nerf_common.h row16(): row of feature f inside a 16-point tile (numpy / torch integer arrays or ints)."""
    return (f & ~15) + 8 * ((f >> 3) & 1) + 2 * (f & 3) + ((f >> 2) & 1)


def _row16h(f):
    """csrc/nerf_common.h row16h(): row of feature f inside a 16-point tile of bf16 rows."""
    return (f & ~15) + 8 * ((f >> 1) & 1) + 2 * ((f >> 2) & 3) + (f & 1)


_REGIONS = {**{"h%d" % i: (i, 256) for i in range(8)}, "feat": (8, 256), "hv": (9, 128)}


def buffer_regions(n_rays, n_samples, split, is_delta=False):
    """nerf_debug_layout: region offsets (floats) of a save / delta buffer for n_rays x n_samples points; split = the split
    datapaths' tiles of 16-bit elements (False: the fp32 datapath's point-major rows; 2: the two-word layout, whose "lo" entry is the
    offset of the mirror that holds the lo words)."""
    out = (ctypes.c_longlong * 16)()
    _check(lib().nerf_debug_layout(int(n_rays), int(n_samples), int(split), int(bool(is_delta)), out), "nerf_debug_layout")
    keys = [f"h{i}" for i in range(8)] + ["feat", "hv"] + (["graw", "scale"] if is_delta else ["enc", "dir", "dir_pt", "mask"])
    reg = {k: int(out[i]) for i, k in enumerate(keys)}
    reg["total"] = int(out[14])
    reg["lo"] = int(out[15]) if int(split) == 2 else 0
    return reg


def _tile32(flat16, Pa, F, P):
    """32-point feature-major tiles of 16-bit elements -> point-major [P, F] fp32"""
    return flat16[:Pa * F].float().view(Pa // 32, F, 32).permute(0, 2, 1).reshape(Pa, F)[:P]


def saved_rows(buf, n_rays, n_samples, region, precision="fp32", part="hi"):
    """Debug / test view of one region of a save buffer as a point-major [P, F] fp32 tensor.  region: "h0".."h7", "hv", "enc", and
    on the fp32 datapath "feat" (the split datapaths fold feature_linear into the view branch and never write it).  fp32 datapath:
    point-major fp32 rows; split datapaths: 16-bit elements (fp16 / bf16 by `precision`), the 256- / 128-wide rows in 16-point tiles
    with the row16h row order, the encoding in 32-point feature-major tiles (csrc/nerf_common.h)."""
    split = precision in SPLIT
    P = n_rays * n_samples
    reg = buffer_regions(n_rays, n_samples, DATAPATHS[precision].family)
    F = 64 if region == "enc" else _REGIONS[region][1]
    off = reg[region] + (reg["lo"] if part == "lo" else 0)      # part="lo" ("fp16x3w" only): the remainders T(v - hi)
    if part == "lo" and not reg["lo"]:
        raise NerfHipError("saved_rows(part='lo'): only the two-word layout (\"fp16x3w\") holds lo words")
    if not split:
        return buf[off:off + P * F].view(P, F)
    Pa = (P + 31) // 32 * 32
    flat = buf[off:off + (Pa * F + 1) // 2].view(DATAPATHS[precision].elem16)
    if region == "enc":
        return _tile32(flat, Pa, F, P)
    rows = flat[:Pa * F].float().view(Pa // 16, F, 16).permute(0, 2, 1).reshape(Pa, F)[:P]      # [P, row]
    return rows[:, _row16h(torch.arange(F, device=rows.device))]                              # feature f sits at row16h(f)


def saved_dir(buf, n_rays, n_samples, precision="fp32"):
    """the per-ray direction encoding a saving forward wrote: [n_rays, 32] fp32 (27 used)"""
    off = buffer_regions(n_rays, n_samples, DATAPATHS[precision].family)["dir"]
    return buf[off:off + n_rays * 32].view(n_rays, 32)


def saved_masks(buf, n_rays, n_samples, precision="fp32"):
    """the ReLU bitmask words of a save buffer as int32 [9, P, 8] (layers 0..7 + view branch; 256 bits per point and layer, in the
    lane order of the datapath's kernels: csrc/nerf_common.h)"""
    P = n_rays * n_samples
    off = buffer_regions(n_rays, n_samples, DATAPATHS[precision].family)["mask"]
    return buf[off:off + 9 * P * 8].view(torch.int32).view(9, P, 8)


def relu_patterns(buf, n_rays, n_samples, precision="fp16x3"):
    """Debug / test view: the ReLU patterns a split datapath's forward saved (and its delta chain applies), as 9 boolean tensors
    [P, width] on the buffer's device -- trunk layers 0..7 (256 wide) and the view branch (128).  Word (layer, p, half), bit i <->
    feature 32*(i>>4) + d32row(i&15, half) (csrc/nerf_common.h).  A checker that forces THIS pattern onto an fp64 autograd of the
    reference network measures the backward's arithmetic alone (ReLU units within rounding of zero legitimately take either side)."""
    if precision not in SPLIT:
        raise NerfHipError("relu_patterns: the split datapaths' bitmask order")
    P = n_rays * n_samples
    words = saved_masks(buf, n_rays, n_samples, precision).view(9, P, 2, 4)
    dev = buf.device
    i = torch.arange(128, device=dev)
    shifts = torch.arange(32, device=dev)
    out = []
    for layer in range(9):
        width = 256 if layer < 8 else 128
        m = torch.zeros(P, width, dtype=torch.bool, device=dev)
        for half in range(2):
            feat = 32 * (i >> 4) + ((i & 15) & 3) + 8 * ((i & 15) >> 2) + 4 * half
            bits = ((words[layer, :, half, :, None] >> shifts) & 1).reshape(P, 128).bool()
            n = width // 2
            m[:, feat[:n]] = bits[:, :n]
        out.append(m)
    return out


def delta_rows(buf, n_rays, n_samples, region, precision="fp32", part="hi"):
    """Debug / test view of one region of a delta buffer as point-major [P, F] fp32: "h0".."h7", "hv", "feat" (fp32 datapath only),
    "graw" (split datapaths: the tiled 4-wide copy of the scaled d_raw)."""
    split = precision in SPLIT
    P = n_rays * n_samples
    reg = buffer_regions(n_rays, n_samples, DATAPATHS[precision].family, is_delta=True)
    F = 4 if region == "graw" else _REGIONS[region][1]
    off = reg[region] + (reg["lo"] if part == "lo" else 0)
    if part == "lo" and not reg["lo"]:
        raise NerfHipError("delta_rows(part='lo'): only the two-word layout (\"fp16x3w\") holds lo words")
    if not split:
        return buf[off:off + P * F].view(P, F)
    Pa = (P + 31) // 32 * 32
    flat = buf[off:off + (Pa * F + 1) // 2].view(DATAPATHS[precision].elem16)
    return _tile32(flat, Pa, F, P)


def delta_scale_word(buf, n_rays, n_samples):
    """fp16 split: the bit pattern of the launch's max|d_raw| the dgrad left in its delta buffer (int32 scalar tensor)"""
    off = buffer_regions(n_rays, n_samples, 1, is_delta=True)["scale"]       # (the same word in the one- and the two-word layout)
    return buf[off:off + 1].view(torch.int32)


# render_rays without gradients as ONE launch on the split datapaths (csrc/render_fused.hip; bit-identical to the
# chain of launches and as fast or faster for every ray count measured).  NERF_INFER_ONE_LAUNCH=0 keeps the chain:
# sample_coarse -> field forward -> composite -> sample_fine -> field forward -> composite
INFER_ONE_LAUNCH = os.environ.get("NERF_INFER_ONE_LAUNCH", "1") != "0"
# the reduced inference class ("fp16_fp8c") evaluates the COARSE pass of a coarse + fine rendering on the three-term fp16 products
# (render._field_pass); NERF_REDUCED_COARSE=reduced keeps round 4's all-reduced chain (with its two-pass last-sample guard)
REDUCED_COARSE_THREE_TERM = os.environ.get("NERF_REDUCED_COARSE", "fp16x3") != "reduced"


def render_cfg(n_coarse, n_fine, lindisp, white_bkgd, raw_noise_std, precision):
    if precision == "fp16_fp8c":
        raise NerfHipError("render_cfg: the one-call entry points run the fp32 / bf16x3 / fp16x3 datapaths; the reduced inference class "
                           "\"fp16_fp8c\" is a chain of launches with its last-sample guard in between (render._field_pass)")
    return NerfRenderCfg(int(n_coarse), int(n_fine), int(bool(lindisp)), int(bool(white_bkgd)), float(raw_noise_std),
                         DATAPATHS[precision].cfg, 1)


def render_infer_supported(n_coarse, n_fine, precision):
    """whether nerf_render_rays_infer takes these sample counts on this datapath"""
    if precision in ("fp32", "fp16_fp8c"):      # (the reduced class runs the chain of launches: its last-sample guard sits between them)
        return False
    cfg = render_cfg(n_coarse, n_fine, 0, 0, 0.0, precision)
    return bool(lib().nerf_render_infer_supported(ctypes.byref(cfg)))


def render_rays_infer(packed_c, packed_f, rays, n_coarse, n_fine, lindisp, white_bkgd, raw_noise_std, precision, rnd):
    """nerf_render_rays_infer: the whole no-grad render_rays of `rays` in one launch.  rnd: the optional draws {t_rand, noise_c,
    u, noise_f}.  Returns the dict of render._field_pass's outputs (rgb_c, disp_c, acc_c, raw_c[, rgb_f, disp_f, acc_f, raw_f,
    z_std])."""
    L = lib()
    n, dev = rays.shape[0], rays.device
    fine = n_fine > 0
    S2 = n_coarse + n_fine
    cfg = render_cfg(n_coarse, n_fine, lindisp, white_bkgd, raw_noise_std, precision)
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    rgb, disp, acc, raw = e(n, 3), e(n), e(n), e(n, S2, 4)
    rgb0, disp0, acc0, z_std = (e(n, 3), e(n), e(n), e(n)) if fine else (None, None, None, None)
    ws = WORKSPACE.take(L.nerf_render_workspace_floats(ctypes.byref(cfg), n, 0), dev)
    opt = lambda k: _ptr(rnd[k], k) if rnd.get(k) is not None else None
    try:
        with _timed("render_infer_kernel", FLOP_FWD3_PER_POINT * n * (n_coarse + (S2 if fine else 0)), 0.0):
            _check(L.nerf_render_rays_infer(ctypes.byref(cfg), _ptr(packed_c, "packed3"), _ptr(packed_f, "packed3") if packed_f is not None else None,
                                            _ptr(rays, "rays"), rays.shape[1], n, opt("t_rand"), opt("noise_c"), opt("u"), opt("noise_f"),
                                            _ptr(rgb), _ptr(disp), _ptr(acc), _ptr(raw), _ptr(rgb0) if fine else None,
                                            _ptr(disp0) if fine else None, _ptr(acc0) if fine else None, _ptr(z_std) if fine else None,
                                            _ptr(ws), _stream()), "nerf_render_rays_infer")
    finally:        # stream-ordered: the next lease is written by kernels enqueued after this one
        WORKSPACE.give(ws)
    if not fine:
        return {"rgb_c": rgb, "disp_c": disp, "acc_c": acc, "raw_c": raw}
    return {"rgb_f": rgb, "disp_f": disp, "acc_f": acc, "raw_f": raw, "rgb_c": rgb0, "disp_c": disp0, "acc_c": acc0, "z_std": z_std}


class RangeMonitor:
    """The guard rail of the fp16 split's range (|activation| and |scaled delta| < 65520; beyond it `raw` / the gradient turn NaN): every
    `every`-th saving forward on fp16x3 / fp16x3w is followed by nerf_range_scan over what it saved, the delta chains of the same step
    by a scan of their deltas, the result words travel to pinned host memory without a synchronisation, and the NEXT calls poll the
    copies' events -- when a value has reached 32768 (half the range) a RuntimeWarning names the way out BEFORE the NaN:
    set_precision("bf16x3") (fp32's exponent range).  Replaces the reference's DEBUG-gated NaN / Inf check (run_nerf.py:414-416).
    every = 0 switches it off; report() is the on-demand form."""

    def __init__(self):
        self.every = int(os.environ.get("NERF_RANGE_CHECK_EVERY", "64"))
        self.calls = 0
        self.words = {}             # device -> int32[4]: (flag, max pattern) of the rows, (flag, max pattern) of the deltas
        self.inflight = []          # (pinned int32[4], event)
        self.max_seen = 0.0         # largest activation any finished scan has seen
        self.max_delta = 0.0        # largest |scaled delta| (the chain runs on s * d_raw with max|s d_raw| in [16, 32))
        self.warned_at = {"activation": 0.0, "scaled delta": 0.0}
        self.warnings = 0
        self.delta_scans_due = 0    # delta chains of the current step still to be scanned

    @staticmethod
    def _f16(bits):
        import numpy as np
        v = float(np.array([bits & 0xffff], dtype=np.uint16).view(np.float16)[0])
        return float("inf") if v != v else v       # a NaN pattern in the buffer: the overflow has already happened

    def _scan(self, bufs, n_rays):
        dev = bufs[0][0].device
        w = self.words.get(dev)
        if w is None:
            w = self.words[dev] = torch.zeros(4, dtype=torch.int32, device=dev)
        ns = list(n_rays) if isinstance(n_rays, (list, tuple)) else [n_rays] * len(bufs)       # (one ray count per buffer, or one for all)
        for (buf, S), n in zip(bufs, ns):
            _check(lib().nerf_range_scan(buf.data_ptr(), int(n), int(S), w.data_ptr(), _stream()), "nerf_range_scan")
        host = torch.empty(4, dtype=torch.int32, pin_memory=True)
        host.copy_(w, non_blocking=True)
        w.zero_()                   # (stream-ordered behind the copy: the next scan starts from zero)
        ev = torch.cuda.Event()
        ev.record()
        self.inflight.append((host, ev))

    def after_forward(self, acts, n_rays):
        """acts: [(act buffer, n_samples)] of one saving fp16 forward over n_rays rays (a list: one count per buffer -- the compacted
        passes of the grid path evaluate different numbers of one-sample records)"""
        self.poll()
        if self.every <= 0:
            return
        self.calls += 1
        if (self.calls - 1) % self.every:
            return
        self._scan(acts, n_rays)
        self.delta_scans_due = len(acts)        # ... and the delta chains of this step's backward

    def after_dgrad(self, delta, n_rays, n_samples):
        """called by field_bwd between the delta chain and the weight-gradient GEMM"""
        if self.delta_scans_due > 0:
            self.delta_scans_due -= 1
            self._scan([(delta, n_samples)], n_rays)

    def poll(self, wait=False):
        import warnings
        while self.inflight and (wait or self.inflight[0][1].query()):
            host, ev = self.inflight.pop(0)
            ev.synchronize()
            for what, flag, top in (("activation", int(host[0]), int(host[1])), ("scaled delta", int(host[2]), int(host[3]))):
                val = self._f16(top)
                if what == "activation":
                    self.max_seen = max(self.max_seen, val)
                else:
                    self.max_delta = max(self.max_delta, val)
                if flag and val > self.warned_at[what]:       # again only when it got worse
                    self.warned_at[what] = val
                    self.warnings += 1
                    where = ("`raw` (and the loss) turn" if what == "activation" else "the parameter gradients turn")
                    warnings.warn(f"nerf-pytorch_amd: {'an' if what == 'activation' else 'a'} {what} of the fp16x3 datapath reached {val:.4g}; the fp16 split's "
                                  f"operands end at 65504 -- beyond that {where} NaN.  Switch to nerf_pytorch_amd.set_precision(\"bf16x3\") (the same "
                                  "kernels with bf16 parts: fp32's exponent range) or to \"fp32\" before it does; weights and optimizer state carry over "
                                  "unchanged.", RuntimeWarning, stacklevel=3)

    def report(self):
        """wait for the scans in flight; {"max_activation", "max_scaled_delta", "limit", "warnings"}"""
        self.poll(wait=True)
        return {"max_activation": self.max_seen, "max_scaled_delta": self.max_delta, "warn_at": 32768.0, "limit": 65504.0,
                "warnings": self.warnings, "every": self.every}


RANGE_MONITOR = RangeMonitor()


def field_fwd(packed, rays, z_vals, save_act=False, precision="fp32", guard_packed=None, raw=None, next_guard=None, act=None):
    """act (with save_act): a save buffer the caller leased (at least act_floats(n, S, precision) floats) instead of a lease of that size.
    guard_packed (precision "fp16_fp8c"): the fp16x3 repack of the same parameters for the last-sample guard, or the string
    "done" when an earlier call's next_guard has already written this pass's last samples into `raw`.
    next_guard = (fp16x3 repack of the refining pass's network, that pass's preallocated raw [n, S_next, 4]): the guard launch also
    evaluates the refining pass's last sample (its depth is this pass's last depth)."""
    n, stride = rays.shape
    S = z_vals.shape[1]
    if raw is None:
        raw = torch.empty((n, S, 4), dtype=torch.float32, device=rays.device)
    elif tuple(raw.shape) != (n, S, 4) or raw.dtype != torch.float32 or not raw.is_contiguous():
        raise NerfHipError(f"field_fwd: raw= must be a contiguous float32 [{n}, {S}, 4] tensor")
    if not save_act:
        act = None
    elif act is None:
        act = WORKSPACE.take(act_floats(n, S, precision), rays.device)
    elif act.numel() < act_floats(n, S, precision) or act.dtype != torch.float32 or not act.is_contiguous():
        raise NerfHipError(f"field_fwd: act= must be a contiguous float32 buffer of at least {act_floats(n, S, precision)} floats")
    dp = DATAPATHS.get(precision, DATAPATHS["fp32"])
    if save_act and dp.save_label is None:
        raise NerfHipError(f"field_fwd: \"{precision}\" is an inference class (no saved activations); train on \"fp16x3\"")
    if precision == "fp16_fp8c" and guard_packed is None:
        raise NerfHipError("field_fwd: \"fp16_fp8c\" needs guard_packed= (the fp16x3 repack) for the last-sample guard")
    with _timed(dp.save_label if save_act else dp.fwd_label, (FLOP_FWD3_PER_POINT if dp.family else FLOP_FWD_PER_POINT) * n * S,
                (dp.bytes_save if save_act else 16.0) * n * S):
        if dp.family:
            _check(lib().nerf_field_fwd_split(_ptr(packed, "packed3"), _ptr(rays, "rays"), stride, _ptr(z_vals, "z_vals"), n, S,
                                              _ptr(raw), _ptr(act, "act", True), dp.save_split if save_act else dp.fwd_split, _stream()),
                   "nerf_field_fwd_split")
        else:
            _check(lib().nerf_field_fwd(_ptr(packed, "packed"), _ptr(rays, "rays"), stride, _ptr(z_vals, "z_vals"), n, S,
                                        _ptr(raw), _ptr(act, "act", True), _stream()), "nerf_field_fwd")
    if precision == "fp16_fp8c":        # the guard of the reduced class: every ray's last sample on the three-term fp16 products
        if not (isinstance(guard_packed, str) and guard_packed == "done"):
            nxt, raw_n, S_n = (None, None, 0) if next_guard is None else (next_guard[0], next_guard[1], next_guard[1].shape[1])
            with _timed("field_fwd16r_kernel<fp16> (last samples)", FLOP_FWD3_PER_POINT * n * (1 if nxt is None else 2), 16.0 * n):
                _check(lib().nerf_field_fwd_last_sample(_ptr(guard_packed, "packed3"), _ptr(rays, "rays"), stride, _ptr(z_vals, "z_vals"),
                                                        n, S, _ptr(raw), _ptr(nxt, "packed3", True), _ptr(raw_n, "raw", True), S_n,
                                                        _stream()), "nerf_field_fwd_last_sample")
    return raw, act


def raw2outputs(raw, z_vals, rays_d, dir_stride, noise, raw_noise_std, white_bkgd, want_weights=True, want_depth=True,
                rays_d_offset=0):
    """rays_d: tensor whose element [rays_d_offset] is ray 0's first direction component."""
    n, S = z_vals.shape
    dev = raw.device
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    disp = torch.empty((n,), dtype=torch.float32, device=dev)
    acc = torch.empty((n,), dtype=torch.float32, device=dev)
    weights = torch.empty((n, S), dtype=torch.float32, device=dev) if want_weights else None
    depth = torch.empty((n,), dtype=torch.float32, device=dev) if want_depth else None
    dptr = _ptr(rays_d, "rays_d") + 4 * rays_d_offset
    _check(lib().nerf_raw2outputs(_ptr(raw, "raw"), _ptr(z_vals, "z_vals"), dptr, dir_stride, n, S,
                                  _ptr(noise, "noise", True), float(raw_noise_std), int(bool(white_bkgd)),
                                  _ptr(rgb), _ptr(disp), _ptr(acc), _ptr(weights, "w", True), _ptr(depth, "d", True),
                                  _stream()), "nerf_raw2outputs")
    return rgb, disp, acc, weights, depth


def raw2outputs_bwd(raw, z_vals, rays_d, dir_stride, noise, raw_noise_std, white_bkgd, d_rgb, d_acc, d_disp,
                    rays_d_offset=0, d_weights=None, d_depth=None, d_rays_d=None, d_z_vals=None):
    """d_raw; with d_rays_d ([n, 3]) and / or d_z_vals ([n, S]) preallocated fp32 tensors, also the geometry adjoint written into them
    (nerf_raw2outputs_bwd_geom: d_raw bit-identical)"""
    n, S = z_vals.shape
    d_raw = torch.empty((n, S, 4), dtype=torch.float32, device=raw.device)
    dptr = _ptr(rays_d, "rays_d") + 4 * rays_d_offset
    if d_rays_d is not None or d_z_vals is not None:
        _check(lib().nerf_raw2outputs_bwd_geom(_ptr(raw, "raw"), _ptr(z_vals, "z_vals"), dptr, dir_stride, n, S,
                                               _ptr(noise, "noise", True), float(raw_noise_std), int(bool(white_bkgd)),
                                               _ptr(d_rgb, "d_rgb"), _ptr(d_acc, "d_acc", True), _ptr(d_disp, "d_disp", True),
                                               _ptr(d_weights, "d_weights", True), _ptr(d_depth, "d_depth", True), _ptr(d_raw),
                                               _ptr(d_rays_d, "d_rays_d", True), _ptr(d_z_vals, "d_z_vals", True), _stream()),
               "nerf_raw2outputs_bwd_geom")
        return d_raw
    _check(lib().nerf_raw2outputs_bwd(_ptr(raw, "raw"), _ptr(z_vals, "z_vals"), dptr, dir_stride, n, S,
                                      _ptr(noise, "noise", True), float(raw_noise_std), int(bool(white_bkgd)),
                                      _ptr(d_rgb, "d_rgb"), _ptr(d_acc, "d_acc", True), _ptr(d_disp, "d_disp", True),
                                      _ptr(d_weights, "d_weights", True), _ptr(d_depth, "d_depth", True),
                                      _ptr(d_raw), _stream()), "nerf_raw2outputs_bwd")
    return d_raw


def _near_far_ptr(near_far, nf_stride, nf_offset, n):
    """pointer to ray 0's near and the float stride between rays: near_far is a tensor whose element [nf_offset] is ray 0's near, with
    ray r's near / far nf_stride floats further on (default: the row length of a 2-D tensor; 0 = one pair for all rays)"""
    if nf_stride is None:
        nf_stride = near_far.shape[-1] if (isinstance(near_far, torch.Tensor) and near_far.dim() == 2) else 0
    nf_stride, nf_offset = int(nf_stride), int(nf_offset)
    base = _ptr(near_far, "near_far")
    if nf_stride < 0 or nf_offset < 0 or (n > 0 and nf_offset + (n - 1) * nf_stride + 2 > near_far.numel()):
        raise NerfHipError(f"near_far holds {near_far.numel()} floats: too few for {n} rays at stride {nf_stride}, offset {nf_offset}")
    return base + 4 * nf_offset, nf_stride


def distortion(weights, z_vals, near_far, nf_stride=None, nf_offset=0):
    """loss [n] of nerf_distortion_fwd: the distortion loss of the compositing weights [n, S] on the depths z_vals [n, S] (non-decreasing
    per ray: the caller's contract).  near_far: see _near_far_ptr (ray records: nf_stride=11, nf_offset=6)."""
    n, S = z_vals.shape
    if tuple(weights.shape) != (n, S):
        raise NerfHipError(f"weights {tuple(weights.shape)} and z_vals {tuple(z_vals.shape)} differ in shape")
    nfp, stride = _near_far_ptr(near_far, nf_stride, nf_offset, n)
    loss = torch.empty((n,), dtype=torch.float32, device=z_vals.device)
    _check(lib().nerf_distortion_fwd(_ptr(weights, "weights"), _ptr(z_vals, "z_vals"), nfp, stride, n, S, _ptr(loss), _stream()),
           "nerf_distortion_fwd")
    return loss


def distortion_bwd(weights, z_vals, near_far, d_loss, out=None, accumulate=False, nf_stride=None, nf_offset=0):
    """d_weights [n, S] = d_loss [n] * d loss / d weights (nerf_distortion_bwd), recomputed from the inputs; written into `out` (a new
    tensor without one), or added to what `out` holds with accumulate=True"""
    n, S = z_vals.shape
    if tuple(weights.shape) != (n, S) or tuple(d_loss.shape) != (n,):
        raise NerfHipError(f"weights {tuple(weights.shape)}, z_vals {tuple(z_vals.shape)} and d_loss {tuple(d_loss.shape)} do not belong together")
    if out is None:
        if accumulate:
            raise NerfHipError("accumulate=True needs the tensor to add to (out=)")
        out = torch.empty((n, S), dtype=torch.float32, device=z_vals.device)
    elif tuple(out.shape) != (n, S):
        raise NerfHipError(f"out {tuple(out.shape)} is not [{n}, {S}]")
    nfp, stride = _near_far_ptr(near_far, nf_stride, nf_offset, n)
    _check(lib().nerf_distortion_bwd(_ptr(weights, "weights"), _ptr(z_vals, "z_vals"), nfp, stride, n, S, _ptr(d_loss, "d_loss"),
                                     _ptr(out, "out"), int(bool(accumulate)), _stream()), "nerf_distortion_bwd")
    return out


def _interlevel_shapes(proposal_weights, proposal_z, weights, z_vals):
    n, P = proposal_z.shape
    S = z_vals.shape[1]
    if tuple(proposal_weights.shape) != (n, P) or tuple(weights.shape) != (n, S) or z_vals.shape[0] != n:
        raise NerfHipError(f"proposal_weights {tuple(proposal_weights.shape)}, proposal_z {tuple(proposal_z.shape)}, weights "
                           f"{tuple(weights.shape)} and z_vals {tuple(z_vals.shape)} do not belong together")
    return n, P, S


def interlevel(proposal_weights, proposal_z, weights, z_vals):
    """loss [n] of nerf_interlevel_fwd: the interlevel loss of the proposal weights [n, P] on the depths proposal_z [n, P] against the
    target weights [n, S] on z_vals [n, S] (both sets of depths non-decreasing per ray: the caller's contract)"""
    n, P, S = _interlevel_shapes(proposal_weights, proposal_z, weights, z_vals)
    loss = torch.empty((n,), dtype=torch.float32, device=z_vals.device)
    _check(lib().nerf_interlevel_fwd(_ptr(proposal_weights, "proposal_weights"), _ptr(proposal_z, "proposal_z"), P, _ptr(weights, "weights"),
                                     _ptr(z_vals, "z_vals"), S, n, _ptr(loss), _stream()), "nerf_interlevel_fwd")
    return loss


def interlevel_bwd(proposal_weights, proposal_z, weights, z_vals, d_loss, out=None, accumulate=False):
    """d_proposal_weights [n, P] = d_loss [n] * d loss / d proposal_weights (nerf_interlevel_bwd), recomputed from the inputs; written into
    `out` (a new tensor without one), or added to what `out` holds with accumulate=True"""
    n, P, S = _interlevel_shapes(proposal_weights, proposal_z, weights, z_vals)
    if tuple(d_loss.shape) != (n,):
        raise NerfHipError(f"d_loss {tuple(d_loss.shape)} is not [{n}]")
    if out is None:
        if accumulate:
            raise NerfHipError("accumulate=True needs the tensor to add to (out=)")
        out = torch.empty((n, P), dtype=torch.float32, device=z_vals.device)
    elif tuple(out.shape) != (n, P):
        raise NerfHipError(f"out {tuple(out.shape)} is not [{n}, {P}]")
    _check(lib().nerf_interlevel_bwd(_ptr(proposal_weights, "proposal_weights"), _ptr(proposal_z, "proposal_z"), P, _ptr(weights, "weights"),
                                     _ptr(z_vals, "z_vals"), S, n, _ptr(d_loss, "d_loss"), _ptr(out, "out"), int(bool(accumulate)),
                                     _stream()), "nerf_interlevel_bwd")
    return out


def sample_fine(z_vals, weights, n_fine, u, u_lin, want_samples=False):
    n, Sc = z_vals.shape
    dev = z_vals.device
    z_all = torch.empty((n, Sc + n_fine), dtype=torch.float32, device=dev)
    z_std = torch.empty((n,), dtype=torch.float32, device=dev)
    z_samples = torch.empty((n, n_fine), dtype=torch.float32, device=dev) if want_samples else None
    _check(lib().nerf_sample_fine(_ptr(z_vals, "z_vals"), _ptr(weights, "weights"), n, Sc, n_fine,
                                  _ptr(u, "u", True), _ptr(u_lin, "u_lin", True), _ptr(z_all),
                                  _ptr(z_samples, "z_samples", True), _ptr(z_std), _stream()), "nerf_sample_fine")
    return z_all, z_std, z_samples


def sample_pdf(bins, weights, n_samples, u, u_lin):
    n, nb = bins.shape
    out = torch.empty((n, n_samples), dtype=torch.float32, device=bins.device)
    _check(lib().nerf_sample_pdf(_ptr(bins, "bins"), _ptr(weights, "weights"), n, nb, n_samples,
                                 _ptr(u, "u", True), _ptr(u_lin, "u_lin", True), _ptr(out), _stream()),
           "nerf_sample_pdf")
    return out


# Dead-tile skipping in the backward of the split datapaths (include/nerf_hip.h): the delta chain and the weight-gradient GEMM leave out
# the 32-point tiles whose d_raw is all +-0.  NERF_BWD_SKIP_DEAD=0 (read once per process, here and in the library): dense everywhere.
BWD_SKIP_DEAD = os.environ.get("NERF_BWD_SKIP_DEAD", "1") != "0"
_LIVE_LISTS = {}        # device -> int32 words of the live-tile list of the pass in flight (grown on demand, never per step)
LAST_LIVE = None        # the list the last sparse field_bwd used (tools / tests read the counts back AFTER the timed region), or None


def live_list(n_rays, n_samples, device):
    """the cached live-tile list buffer of `device`, at least nerf_live_tiles_words(n_rays, n_samples) words (stream-ordered reuse:
    the next pass's launches are enqueued behind this pass's readers)"""
    words = lib().nerf_live_tiles_words(n_rays, n_samples)
    buf = _LIVE_LISTS.get(device)
    if buf is None or buf.numel() < words:
        buf = _LIVE_LISTS[device] = torch.zeros(max(words, 1 << 16), dtype=torch.int32, device=device)
    return buf


BYTES_INPUT_GRAD_PER_POINT = 2 * (256 + 256 + 128)      # deltas the input-gradient kernel reads per point (16-bit words; x2 fp32 / hi + lo)


def field_bwd(packed, act, d_raw, grad, accumulate, precision="fp32", params=None, input_grad=None):
    """Parameter gradients of one field evaluation into the flat vector `grad`.  `params`: the canonical (flat) parameter
    vector `packed` was made from -- required by the split datapaths, whose folded feature layer needs Wf, bf
    and Wv[:, :256] to turn G = delta_hv^T h7 into their gradients (csrc/nerf_common.h).
    grad=None: no weight gradient (frozen network: dgrad only).  input_grad = (rays, z_vals, d_rays [n, 11], accumulate): the
    gradient w.r.t. the ray records from the same deltas (nerf_field_input_grad; needs params=, the live fp32 weights)."""
    if (precision != "fp32" or input_grad is not None) and params is None:
        raise NerfHipError("field_bwd: the split datapaths and the input gradient need params= (the flat parameter vector)")
    n, S, _ = d_raw.shape
    L = lib()
    dev = d_raw.device
    delta = WORKSPACE.take(delta_floats(n, S, precision), dev)
    partial = WORKSPACE.take(L.nerf_wgrad_partial_floats(n, S), dev) if grad is not None else None
    try:
        return _field_bwd(L, packed, act, d_raw, grad, accumulate, precision, delta, partial, n, S, params, input_grad)
    finally:        # stream-ordered: the next lease is written by kernels enqueued after these
        WORKSPACE.give(delta)
        WORKSPACE.give(partial)


def field_input_grad(params, delta, rays, z_vals, d_rays, accumulate, precision="fp32"):
    """nerf_field_input_grad: d_rays [n, 11] (+)= dL/d(ray records) of the evaluation whose dgrad left `delta`"""
    n, S = z_vals.shape
    P = n * S
    with _timed("field_input_grad_kernel", 2.0 * P * (2 * 63 * 256 + 27 * 128),
                BYTES_INPUT_GRAD_PER_POINT * P * (1 if DATAPATHS[precision].family == 1 else 2)):
        _check(lib().nerf_field_input_grad(_ptr(params, "params"), _ptr(delta, "delta"), _ptr(rays, "rays"), rays.shape[1],
                                           _ptr(z_vals, "z_vals"), n, S, _ptr(d_rays, "d_rays"), int(bool(accumulate)), _stream()),
               "nerf_field_input_grad")
    return d_rays


def embed_bwd(x, n_freqs, d_out):
    """nerf_embed_bwd: d/dx of embed(x) . d_out"""
    x = x.contiguous()
    d_x = torch.empty_like(x)
    _check(lib().nerf_embed_bwd(_ptr(x, "x"), x.numel() // 3, int(n_freqs), _ptr(d_out.contiguous(), "d_out"), _ptr(d_x), 0, _stream()),
           "nerf_embed_bwd")
    return d_x


def _field_bwd(L, packed, act, d_raw, grad, accumulate, precision, delta, partial, n, S, params, input_grad=None):
    dp = DATAPATHS.get(precision, DATAPATHS["fp32"])
    if dp.save_split is None:       # nothing trains on it: the fp32 entry points
        dp = DATAPATHS["fp32"]
    split = dp.save_split
    # what the forward wrote into `act` (the library's own record, nerf_buffer_layout); the weight-gradient call below passes
    # datapath = -1 ("as recorded"), and a mismatched pairing is refused by the library (NERF_E_BADARG)
    kind = buffer_layout(act)[0]
    if split is not None and kind == -1:
        raise NerfHipError("field_bwd: `act` is not a save buffer this library's forward wrote (no layout record): the split "
                           "datapaths cannot guess its tiling and element type")
    P = n * S
    # the sparse forms, unless somebody else reads this pass's deltas: the input gradient and the range monitor's delta scan would
    # meet the tiles nobody wrote
    global LAST_LIVE
    live = None
    if split is not None and BWD_SKIP_DEAD and input_grad is None and not (dp.fp16_saves and RANGE_MONITOR.delta_scans_due > 0):
        live = live_list(n, S, d_raw.device)
    LAST_LIVE = live
    with _timed(dp.dgrad_label, (FLOP_DGRAD3_PER_POINT if dp.family else FLOP_DGRAD_PER_POINT) * P, dp.bytes_dgrad * P):
        if live is not None:
            _check(L.nerf_field_dgrad_split_live(_ptr(packed, "packed3"), _ptr(act, "act"), _ptr(d_raw, "d_raw"), n, S, _ptr(delta), split,
                                                 live.data_ptr(), _stream()), "nerf_field_dgrad_split_live")
        elif split is not None:
            _check(L.nerf_field_dgrad_split(_ptr(packed, "packed3"), _ptr(act, "act"), _ptr(d_raw, "d_raw"), n, S, _ptr(delta), split, _stream()),
                   "nerf_field_dgrad_split")
        else:
            _check(L.nerf_field_dgrad(_ptr(packed, "packed"), _ptr(act, "act"), _ptr(d_raw, "d_raw"), n, S, _ptr(delta),
                                      _stream()), "nerf_field_dgrad")
    if dp.fp16_saves:
        RANGE_MONITOR.after_dgrad(delta, n, S)      # (scans the deltas on the steps whose forward was scanned; nothing otherwise)
    if input_grad is not None:
        rays, z_vals, d_rays, acc_rays = input_grad
        field_input_grad(params, delta, rays, z_vals, d_rays, acc_rays, precision)
    if grad is None:
        return None
    gemm16 = split is not None          # 16-bit operands streamed straight into the MFMA (wgrad1_kernel)
    datapath = -1
    args = (_ptr(act, "act"), _ptr(delta), _ptr(d_raw, "d_raw"), n, S, _ptr(partial), _ptr(grad, "grad"),
            int(bool(accumulate)), datapath)
    tail = (_ptr(params, "params", True), _stream())
    wgrad_phase = L.nerf_field_wgrad_phase
    if live is not None:
        wgrad_phase = L.nerf_field_wgrad_phase_live
        tail = (tail[0], live.data_ptr(), tail[1])
    if TIMER is None:
        _check(wgrad_phase(*args, 7, *tail), "nerf_field_wgrad_phase")
        return grad
    if gemm16:      # all 12 jobs stream 16-bit operands straight into the MFMA
        with _timed(dp.gemm_label, FLOP_WGRAD3_PER_POINT * P, dp.bytes_gemm * P):
            _check(wgrad_phase(*args, 3, *tail), "nerf_field_wgrad_phase")
    else:
        with _timed("wgrad256_kernel", FLOP_WGRAD_BIG_PER_POINT * P, BYTES_WGRAD_BIG_PER_POINT * P):
            _check(wgrad_phase(*args, 1, *tail), "nerf_field_wgrad_phase")
        with _timed("wgrad_kernel(narrow jobs)", (FLOP_WGRAD_PER_POINT - FLOP_WGRAD_BIG_PER_POINT) * P, BYTES_WGRAD_SMALL_PER_POINT * P):
            _check(wgrad_phase(*args, 2, *tail), "nerf_field_wgrad_phase")
    # chunks of partial sums the reduction reads (csrc/field_bwd.hip, wgrad_chunks)
    n_chunks = min((19 if P < 400000 else 39) if gemm16 else 128, max(1, (P + 255) // 256))
    with _timed("wgrad_reduce_kernel", 0.0, 4.0 * N_PARAMS * (n_chunks + 1)):
        _check(wgrad_phase(*args, 4, *tail), "nerf_field_wgrad_phase")
    return grad


# ---- occupancy grid (csrc/occupancy.hip; the user-facing object is occupancy.OccupancyGrid)
class NerfOccGrid(ctypes.Structure):
    """include/nerf_hip.h NerfOccGrid"""
    _fields_ = [("lo", ctypes.c_float * 3), ("scale", ctypes.c_float * 3), ("res", ctypes.c_int * 3), ("outside_skip", ctypes.c_int),
                ("bits", ctypes.c_void_p)]


def _words(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise NerfHipError(f"{name} must be a contiguous int32 tensor on the GPU")
    return t.data_ptr()


def occ_desc(lo, scale, res, outside_skip, bits):
    """the NerfOccGrid descriptor of a grid whose bit words are the int32 device tensor `bits`"""
    n_words = (int(res[0]) * int(res[1]) * int(res[2]) + 31) // 32
    if bits.numel() != n_words:
        raise NerfHipError(f"occupancy grid {tuple(res)} needs {n_words} words, got {bits.numel()}")
    return NerfOccGrid((ctypes.c_float * 3)(*[float(v) for v in lo]), (ctypes.c_float * 3)(*[float(v) for v in scale]),
                       (ctypes.c_int * 3)(*[int(v) for v in res]), int(bool(outside_skip)), _words(bits, "bits"))


def occ_compact(desc, rays, z_vals, slot=None, records=None, z_stop=None):
    """nerf_occ_compact: (slot int32 [n * S], records fp32 [n * S, 11] of which the first M rows are written, count int32 [1] = M on
    the device).  slot / records: flat fp32 scratch of at least n * S / 11 n * S words (hb.WORKSPACE leases) or None (allocated).
    z_stop (fp32 [n], occ_stop_depth's): nerf_occ_compact_stop -- the samples with z >= z_stop[ray] are dropped as well; None: the
    entry point without a stop."""
    n, stride = rays.shape
    S = z_vals.shape[1]
    P = n * S
    dev = rays.device
    L = lib()
    slot = torch.empty(max(P, 1), dtype=torch.int32, device=dev) if slot is None else slot[:max(P, 1)].view(torch.int32)
    records = (torch.empty(max(P, 1) * 11, dtype=torch.float32, device=dev) if records is None else records[:max(P, 1) * 11]).view(-1, 11)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    scratch = WORKSPACE.take(max(L.nerf_occ_scratch_words(P), 1), dev)
    if z_stop is not None and tuple(z_stop.shape) != (n,):
        raise NerfHipError("occ_compact: z_stop must hold one depth per ray")
    try:
        if z_stop is None:
            with _timed("occ_compact (count + scan + write)", 0.0, 12.0 * P):
                _check(L.nerf_occ_compact(ctypes.byref(desc), _ptr(rays, "rays"), stride, _ptr(z_vals, "z_vals"), n, S, slot.data_ptr(),
                                          _ptr(records, "records"), count.data_ptr(), scratch.data_ptr(), _stream()), "nerf_occ_compact")
        else:
            with _timed("occ_compact_stop (count + scan + write)", 0.0, 12.0 * P + 4.0 * n):
                _check(L.nerf_occ_compact_stop(ctypes.byref(desc), _ptr(rays, "rays"), stride, _ptr(z_vals, "z_vals"), _ptr(z_stop, "z_stop"),
                                               n, S, slot.data_ptr(), _ptr(records, "records"), count.data_ptr(), scratch.data_ptr(),
                                               _stream()), "nerf_occ_compact_stop")
    finally:        # stream-ordered, like every lease
        WORKSPACE.give(scratch)
    return slot[:P], records, count


def occ_expand(slot, raw_c, raw):
    """nerf_occ_expand: raw [..., 4] (preallocated, contiguous) <- raw_c rows by slot, zeros where slot < 0"""
    P = slot.numel()
    if raw.numel() != 4 * P:
        raise NerfHipError("occ_expand: raw must hold 4 floats per slot")
    with _timed("occ_expand_kernel", 0.0, 20.0 * P):
        _check(lib().nerf_occ_expand(_words(slot, "slot"), _ptr(raw_c, "raw_c"), P, _ptr(raw, "raw"), _stream()), "nerf_occ_expand")
    return raw


def occ_mark(sigma, samples_per_cell, threshold, words):
    """nerf_occ_mark: words (int32 view of the grid's bits, or of a slice of it that starts at a multiple of 32 cells) from sigma
    [n_cells * samples_per_cell]"""
    n_cells = sigma.numel() // int(samples_per_cell)
    if words.numel() != (n_cells + 31) // 32:
        raise NerfHipError("occ_mark: one word per 32 cells")
    _check(lib().nerf_occ_mark(_ptr(sigma, "sigma"), n_cells, int(samples_per_cell), float(threshold), _words(words, "words"), _stream()),
           "nerf_occ_mark")
    return words


def occ_dilate(bits, res):
    """nerf_occ_dilate: the 3x3x3 OR of a grid's bit words, as a new tensor"""
    out = torch.empty_like(bits)
    _check(lib().nerf_occ_dilate(_words(bits, "bits"), int(res[0]), int(res[1]), int(res[2]), _words(out, "out"), _stream()), "nerf_occ_dilate")
    return out


def occ_gather(slot, d_raw, d_raw_c):
    """nerf_occ_gather: d_raw_c [M, ..., 4] (preallocated; M = the number of slots >= 0) <- the rows of d_raw [..., 4] by slot"""
    P = slot.numel()
    if d_raw.numel() != 4 * P:
        raise NerfHipError("occ_gather: d_raw must hold 4 floats per slot")
    if d_raw_c.numel() == 0:        # M = 0: no slot is >= 0, nothing to write
        return d_raw_c
    with _timed("occ_gather_kernel", 0.0, 20.0 * P):
        _check(lib().nerf_occ_gather(_words(slot, "slot"), _ptr(d_raw, "d_raw"), P, _ptr(d_raw_c, "d_raw_c"), _stream()), "nerf_occ_gather")
    return d_raw_c


def occ_fold_rays(slot, z_vals, d_rec, d_rays, accumulate=False):
    """nerf_occ_fold_rays: d_rays [n, 11] (+)= the per-ray sums of the compacted records' gradient d_rec [M, 11] (slot / z_vals: [n, S])"""
    n, S = z_vals.shape
    if slot.numel() != n * S or tuple(d_rays.shape) != (n, 11) or d_rec.dim() != 2 or d_rec.shape[1] != 11:
        raise NerfHipError("occ_fold_rays: slot [n * S], z_vals [n, S], d_rec [M, 11], d_rays [n, 11]")
    if d_rec.numel() == 0:          # M = 0: never read, but the entry point refuses a null pointer
        d_rec = torch.empty((1, 11), dtype=torch.float32, device=d_rays.device)
    with _timed("occ_fold_rays_kernel", 0.0, 8.0 * n * S):
        _check(lib().nerf_occ_fold_rays(_words(slot, "slot"), _ptr(z_vals, "z_vals"), _ptr(d_rec, "d_rec"), n, S, _ptr(d_rays, "d_rays"),
                                        int(bool(accumulate)), _stream()), "nerf_occ_fold_rays")
    return d_rays


def occ_density_update(sigma, samples_per_cell, decay, density):
    """nerf_occ_density_update: density (a contiguous run of a DensityGrid's cells) <- max(density * decay, max_k sigma), in place"""
    n_cells = density.numel()
    if sigma.numel() != n_cells * int(samples_per_cell):
        raise NerfHipError("occ_density_update: sigma must hold samples_per_cell values per cell")
    _check(lib().nerf_occ_density_update(_ptr(sigma, "sigma"), n_cells, int(samples_per_cell), float(decay), _ptr(density, "density"),
                                         _stream()), "nerf_occ_density_update")
    return density


def occ_ray_span(desc, rays):
    """nerf_occ_ray_span: (span fp32 [n, 2], hit int32 [n]) of rays [n, >= 8] -- the ray's interval clipped to the first / last
    occupied stretch it crosses, (near, far) unchanged and hit = 0 where it crosses none"""
    if rays.dim() != 2 or rays.shape[1] < 8:
        raise NerfHipError("occ_ray_span: rays [n, >= 8] (o, d, near, far, ...)")
    n, stride = rays.shape
    span = torch.empty((n, 2), dtype=torch.float32, device=rays.device)
    hit = torch.empty(n, dtype=torch.int32, device=rays.device)
    if n == 0:
        return span, hit
    with _timed("occ_ray_span_kernel", 0.0, 44.0 * n):
        _check(lib().nerf_occ_ray_span(ctypes.byref(desc), _ptr(rays, "rays"), stride, n, _ptr(span, "span"), hit.data_ptr(), _stream()),
               "nerf_occ_ray_span")
    return span, hit


def occ_proposal_weights(desc, density, outside_sigma, rays, z_vals, want_sigma=False):
    """nerf_occ_proposal_weights: (weights fp32 [n, S], sigma fp32 [n, S] or None) of rays [n, >= 6] / z_vals [n, S] -- the compositing
    weights with the grid's density per cell (fp32 [cells]) as sigma; outside the box outside_sigma (0 for a grid that skips there)"""
    if rays.dim() != 2 or rays.shape[1] < 6 or z_vals.dim() != 2 or z_vals.shape[0] != rays.shape[0]:
        raise NerfHipError("occ_proposal_weights: rays [n, >= 6] (o, d, ...), z_vals [n, S]")
    n, stride = rays.shape
    S = z_vals.shape[1]
    if density.numel() != desc.res[0] * desc.res[1] * desc.res[2]:
        raise NerfHipError("occ_proposal_weights: one density per cell of the grid")
    weights = torch.empty((n, S), dtype=torch.float32, device=rays.device)
    sigma = torch.empty((n, S), dtype=torch.float32, device=rays.device) if want_sigma else None
    if n == 0:
        return weights, sigma
    with _timed("occ_proposal_weights_kernel", 0.0, (16.0 if want_sigma else 12.0) * n * S):
        _check(lib().nerf_occ_proposal_weights(ctypes.byref(desc), _ptr(density, "density"), float(outside_sigma), _ptr(rays, "rays"), stride,
                                               _ptr(z_vals, "z_vals"), n, S, _ptr(weights), _ptr(sigma, "sigma", True), _stream()),
               "nerf_occ_proposal_weights")
    return weights, sigma


def stop_threshold(eps):
    """fp32(1 - eps), computed in double: what the running sum of the coarse weights is compared with (include/nerf_hip.h)"""
    import numpy as np
    return float(np.float32(1.0 - float(eps)))


def occ_stop_depth(z_vals, weights, eps):
    """nerf_occ_stop_depth: z_stop fp32 [n] of z_vals / weights [n, S] -- per ray the depth of the sample behind the first one at which
    the left-to-right fp32 sum of the weights reaches fp32(1 - eps), +inf where it never does or nothing lies behind"""
    if z_vals.dim() != 2 or tuple(weights.shape) != tuple(z_vals.shape):
        raise NerfHipError("occ_stop_depth: z_vals and weights [n, S]")
    n, S = z_vals.shape
    z_stop = torch.empty(n, dtype=torch.float32, device=z_vals.device)
    if n == 0:
        return z_stop
    with _timed("occ_stop_depth_kernel", 0.0, 4.0 * n * S + 8.0 * n):
        _check(lib().nerf_occ_stop_depth(_ptr(z_vals, "z_vals"), _ptr(weights, "weights"), n, S, stop_threshold(eps), _ptr(z_stop), _stream()),
               "nerf_occ_stop_depth")
    return z_stop


def _march_io(who, desc, rays, u, n_slots, flags, density=None, unpaired=False):
    """the checks, the timing block (<who>_kernel, entered around the launch) and the outputs the three marches share:
    (n, stride, timed, z_vals fp32 [n, n_slots], z_stop fp32 [n], `flags` int32 [n] each)"""
    if rays.dim() != 2 or rays.shape[1] < 8:
        raise NerfHipError(f"{who}: rays [n, >= 8] (o, d, near, far, ...)")
    n, stride = rays.shape
    if u is not None and tuple(u.shape) != (n,):
        raise NerfHipError(f"{who}: u must hold one offset per ray")
    if unpaired:
        raise NerfHipError(f"{who}: density and eps come together (the stop form) or not at all")
    if density is not None and density.numel() != desc.res[0] * desc.res[1] * desc.res[2]:
        raise NerfHipError(f"{who}: one density per cell of the grid")
    out = [n, stride, _timed(who + "_kernel", 0.0, (4.0 * int(n_slots) + 40.0 + 4.0 * flags) * n),
           torch.empty((n, int(n_slots)), dtype=torch.float32, device=rays.device), torch.empty(n, dtype=torch.float32, device=rays.device)]
    for _ in range(flags):
        out.append(torch.empty(n, dtype=torch.int32, device=rays.device))
    return out


def occ_march(desc, rays, u, n_steps, n_slots):
    """nerf_occ_march: (z_vals fp32 [n, n_slots], z_stop fp32 [n], truncated int32 [n]) of rays [n, >= 8] -- per ray the n_steps equal
    steps over [near, far] that fall in occupied cells (plus one closing step behind every occupied run), padded with the stop depth
    that nerf_occ_compact_stop drops; u: fp32 [n] in [0, 1), the offset of the ray's steps, or None (0.5)"""
    n, stride, timed, z_vals, z_stop, truncated = _march_io("occ_march", desc, rays, u, n_slots, 1)
    M, S = int(n_steps), int(n_slots)
    with timed:
        _check(lib().nerf_occ_march(ctypes.byref(desc), _ptr(rays, "rays"), stride, _ptr(u, "u", True), n, M, S, _ptr(z_vals), _ptr(z_stop),
                                    truncated.data_ptr(), _stream()), "nerf_occ_march")
    return z_vals, z_stop, truncated


def march_stop_threshold(eps):
    """tau = fp32(-ln(eps)), computed in double: what the grid's accumulated optical depth is compared with (include/nerf_hip.h)"""
    import math
    import numpy as np
    return float(np.float32(-math.log(float(eps))))


def occ_march_stop(desc, density, outside_sigma, rays, u, n_steps, n_slots, eps):
    """nerf_occ_march_stop: (z_vals fp32 [n, n_slots], z_stop fp32 [n], truncated int32 [n], stopped int32 [n]) of rays [n, >= 8] --
    occ_march over a DensityGrid's densities (fp32 [cells]; outside the box outside_sigma, as occ_proposal_weights takes them) that stops
    emitting where the grid's own transmittance has fallen to eps (0 < eps < 1); a stopped ray's stop depth is the first candidate not
    emitted"""
    n, stride, timed, z_vals, z_stop, truncated, stopped = _march_io("occ_march_stop", desc, rays, u, n_slots, 2, density)
    M, S = int(n_steps), int(n_slots)
    with timed:
        _check(lib().nerf_occ_march_stop(ctypes.byref(desc), _ptr(density, "density"), float(outside_sigma), _ptr(rays, "rays"), stride,
                                         _ptr(u, "u", True), n, M, S, march_stop_threshold(eps), _ptr(z_vals), _ptr(z_stop),
                                         truncated.data_ptr(), stopped.data_ptr(), _stream()), "nerf_occ_march_stop")
    return z_vals, z_stop, truncated, stopped


def occ_march_step(desc, density, outside_sigma, rays, u, step_size, n_steps, n_slots, fit=0, eps=None):
    """nerf_occ_march_step: (z_vals fp32 [n, n_slots], z_stop fp32 [n], truncated int32 [n], level int32 [n], stopped int32 [n] or None) of
    rays [n, >= 8] -- the march in steps of step_size along the ray (a length in the scene: the depth step is step_size / |d|), at most
    n_steps candidates in front of far, and per ray the step doubled up to `fit` times until the emitted steps fit the slots (level: how
    often).  density None (eps None): occ_march's rule per level, stopped is None; density fp32 [cells] with eps: occ_march_stop's"""
    n, stride, timed, z_vals, z_stop, truncated, level, *stopped = _march_io(
        "occ_march_step", desc, rays, u, n_slots, 2 if density is None else 3, density, unpaired=(density is None) != (eps is None))
    stopped = stopped[0] if stopped else None
    M, S = int(n_steps), int(n_slots)
    with timed:
        _check(lib().nerf_occ_march_step(ctypes.byref(desc), _ptr(density, "density", True), float(outside_sigma), _ptr(rays, "rays"), stride,
                                         _ptr(u, "u", True), n, float(step_size), M, S, int(fit),
                                         0.0 if eps is None else march_stop_threshold(eps), _ptr(z_vals), _ptr(z_stop),
                                         truncated.data_ptr(), level.data_ptr(), None if stopped is None else stopped.data_ptr(), _stream()),
               "nerf_occ_march_step")
    return z_vals, z_stop, truncated, level, stopped


def view_planes(near, far):
    """(near_m, far_m) = (fp32(near (1 - 2^-10)), fp32(far (1 + 2^-10))), computed in double: the depth range nerf_occ_view_carve tests
    the corners of a cell against (include/nerf_hip.h)"""
    import numpy as np
    return float(np.float32(float(near) * (1.0 - 2.0 ** -10))), float(np.float32(float(far) * (1.0 + 2.0 ** -10)))


def occ_view_carve(desc, width, cams, H, W, near_m, far_m, margin_px, sat, seen, carved_words, accumulate=False):
    """nerf_occ_view_carve: seen (int32 [cells], preallocated) (+)= per cell the number of the cameras cams (fp32 [V, 16]: c2w row-major,
    fx, fy, cx, cy) that see it; with sat (int32 [V, H + 1, W + 1], the summed-area tables of the masks) carved_words (int32 [words],
    preallocated) (|)= the cells some camera carves.  sat and carved_words are both tensors or both None.  Returns (seen, carved_words)."""
    n_cells = desc.res[0] * desc.res[1] * desc.res[2]
    V = cams.shape[0] if cams.dim() == 2 else -1
    if cams.dim() != 2 or cams.shape[1] != 16 or V < 1:
        raise NerfHipError("occ_view_carve: cams [V >= 1, 16] (c2w row-major, fx, fy, cx, cy)")
    if seen.numel() != n_cells or (carved_words is not None and carved_words.numel() != (n_cells + 31) // 32):
        raise NerfHipError("occ_view_carve: seen holds one count per cell, carved_words one word per 32 cells")
    if (sat is None) != (carved_words is None):
        raise NerfHipError("occ_view_carve: sat and carved_words come together (with masks) or not at all")
    if sat is not None and tuple(sat.shape) != (V, int(H) + 1, int(W) + 1):
        raise NerfHipError("occ_view_carve: sat [V, H + 1, W + 1]")
    w3 = (ctypes.c_float * 3)(*[float(v) for v in width])
    with _timed("occ_view_carve_kernel", 0.0, 4.0 * n_cells + 64.0 * V):
        _check(lib().nerf_occ_view_carve(ctypes.byref(desc), w3, _ptr(cams, "cams"), V, int(H), int(W), float(near_m), float(far_m),
                                         float(margin_px), None if sat is None else _words(sat, "sat"), int(bool(accumulate)),
                                         _words(seen, "seen"), None if carved_words is None else _words(carved_words, "carved_words"),
                                         _stream()), "nerf_occ_view_carve")
    return seen, carved_words


# ---- isosurface (csrc/isosurface.hip; the user-facing functions are in mesh.py)
def _iso_volume(who, volume, keep_words):
    """(nx, ny, nz, nodes, cubes) of a lattice volume fp32 [nx, ny, nz] and its optional keep words (int32, one bit per cube)"""
    _ptr(volume, "volume")
    if volume.dim() != 3:
        raise NerfHipError(f"{who}: volume [nx, ny, nz]")
    nx, ny, nz = (int(v) for v in volume.shape)
    cubes = (nx - 1) * (ny - 1) * (nz - 1)
    if keep_words is not None and keep_words.numel() != (cubes + 31) // 32:
        raise NerfHipError(f"{who}: keep_words holds one bit per cube, {(cubes + 31) // 32} words")
    return nx, ny, nz, nx * ny * nz, cubes


def iso_count(volume, level, keep_words=None):
    """nerf_iso_count: (counts int32 [2] on the device = (V, F), scratch int32) of the mesh of volume (fp32 [nx, ny, nz], values at the
    lattice nodes) at `level`; keep_words (int32, one bit per cube, or None) restricts it to the kept cubes.  scratch carries the block
    offsets to iso_emit."""
    nx, ny, nz, nodes, cubes = _iso_volume("iso_count", volume, keep_words)
    words = lib().nerf_iso_scratch_words(nx, ny, nz)
    scratch = torch.empty(max(words, 1), dtype=torch.int32, device=volume.device)
    counts = torch.empty(2, dtype=torch.int32, device=volume.device)
    # both count passes read the volume once (the neighbours come from the caches) and the keep bits; the scans walk the block counts
    with _timed("iso_count (edges + scan + cubes + scan)", 0.0, 8.0 * nodes + cubes / 4.0 + 8.0 * (words - 7 * nodes)):
        _check(lib().nerf_iso_count(_ptr(volume, "volume"), nx, ny, nz, float(level), None if keep_words is None else _words(keep_words, "keep_words"),
                                    scratch.data_ptr(), counts.data_ptr(), _stream()), "nerf_iso_count")
    return counts, scratch


def iso_emit(volume, level, lo, step, keep_words, scratch, n_vertices, n_faces):
    """nerf_iso_emit: (vertices fp32 [V, 3], faces int32 [F, 3]) after iso_count on the same volume, level and keep_words, whose scratch
    and read-back counts (V > 0) this takes; lo / step: the position of node 0 and the lattice step per axis"""
    nx, ny, nz, nodes, cubes = _iso_volume("iso_emit", volume, keep_words)
    V, F = int(n_vertices), int(n_faces)
    if V < 1 or F < 1 or scratch.numel() < lib().nerf_iso_scratch_words(nx, ny, nz):
        raise NerfHipError("iso_emit: the counts (V, F >= 1) and the scratch of iso_count on this volume")
    vertices = torch.empty((V, 3), dtype=torch.float32, device=volume.device)
    faces = torch.empty((F, 3), dtype=torch.int32, device=volume.device)
    lo3 = (ctypes.c_float * 3)(*[float(v) for v in lo])
    step3 = (ctypes.c_float * 3)(*[float(v) for v in step])
    # vertices: the volume, 28 B per node of edge ranks, the positions; faces: the volume, three ranks read and three indices written per triangle
    with _timed("iso_emit (vertices + faces)", 0.0, 8.0 * nodes + 28.0 * nodes + 12.0 * V + cubes / 8.0 + 24.0 * F):
        _check(lib().nerf_iso_emit(_ptr(volume, "volume"), nx, ny, nz, float(level), lo3, step3,
                                   None if keep_words is None else _words(keep_words, "keep_words"), _words(scratch, "scratch"),
                                   _ptr(vertices), faces.data_ptr(), _stream()), "nerf_iso_emit")
    return vertices, faces


# ---- baked field (csrc/baked.hip; the user-facing object is baked.BakedField)
BAKED_ROW_HALVES = (4, 16, 32)      # fp16 values per table row for sh_degree 0, 1, 2
BAKED_STOPPED = 1 << 30             # the flag nerf_baked_render sets in n_samples


def baked_render(desc, node_index, table, sh_degree, rays, u, step_size, max_steps, stop_eps=0.0, white_bkgd=False):
    """nerf_baked_render: (rgb_map fp32 [n, 3], disp_map, acc_map, depth_map fp32 [n], n_samples int32 [n], stopped bool [n]) of rays
    [n, >= 11] rendered from a baked field: node_index int32 [one per lattice node of the grid], table fp16 [rows, W] with row 0 zero;
    u: fp32 [n] in [0, 1) or None (0.5); stopped: the rays whose transmittance fell below stop_eps at the end of a round"""
    deg = int(sh_degree)
    if deg not in (0, 1, 2):
        raise NerfHipError(f"baked_render: sh_degree must be 0, 1 or 2, got {sh_degree!r}")
    if rays.dim() != 2 or rays.shape[1] < 11:
        raise NerfHipError("baked_render: rays [n, >= 11] (o, d, near, far, viewdir)")
    n, stride = rays.shape
    if u is not None and tuple(u.shape) != (n,):
        raise NerfHipError("baked_render: u must hold one offset per ray")
    nodes = (desc.res[0] + 1) * (desc.res[1] + 1) * (desc.res[2] + 1)
    if node_index.numel() != nodes:
        raise NerfHipError(f"baked_render: node_index holds one entry per lattice node, {nodes}")
    if not (isinstance(table, torch.Tensor) and table.is_cuda and table.dtype == torch.float16 and table.is_contiguous() and table.dim() == 2
            and table.shape[0] >= 1 and table.shape[1] == BAKED_ROW_HALVES[deg]):
        raise NerfHipError(f"baked_render: table must be a contiguous fp16 tensor [rows >= 1, {BAKED_ROW_HALVES[deg]}] on the GPU")
    dev = rays.device
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    disp, acc, depth = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
    n_samples = torch.empty(n, dtype=torch.int32, device=dev)
    if n > 0:
        # per ray 44 B in and 28 B out; what the kept candidates gather depends on the scene and is not counted
        with _timed("baked_render_kernel", 0.0, 72.0 * n):
            _check(lib().nerf_baked_render(ctypes.byref(desc), _words(node_index, "node_index"), table.data_ptr(), int(table.shape[0]), deg,
                                           _ptr(rays, "rays"), stride, _ptr(u, "u", True), n, float(step_size), int(max_steps), float(stop_eps),
                                           int(bool(white_bkgd)), _ptr(rgb), _ptr(disp), _ptr(acc), _ptr(depth), n_samples.data_ptr(),
                                           _stream()), "nerf_baked_render")
    stopped = (n_samples & BAKED_STOPPED) != 0
    return rgb, disp, acc, depth, n_samples & (BAKED_STOPPED - 1), stopped


# ---- baked field, training (csrc/baked_train.hip; the user-facing object is baked.BakedTrainer)
BAKED_RECORD_WORDS = 12             # fp32 words per sample record of nerf_baked_train_fwd
BAKED_MAX_SAMPLES = 1 << 30         # records of one call


def _baked_rays(who, rays, u):
    if not (isinstance(rays, torch.Tensor) and rays.is_cuda) or rays.dim() != 2 or rays.shape[1] < 11:
        raise NerfHipError(f"{who}: rays [n, >= 11] (o, d, near, far, viewdir) on the GPU")
    if u is not None and tuple(u.shape) != (rays.shape[0],):
        raise NerfHipError(f"{who}: u must hold one offset per ray")
    return int(rays.shape[0]), int(rays.shape[1])


def baked_count(desc, rays, u, step_size, max_steps):
    """nerf_baked_count: int32 [n], the kept candidates of every ray [n, >= 11] -- baked_render's n_samples with stop_eps = 0, without
    reading a table"""
    n, stride = _baked_rays("baked_count", rays, u)
    counts = torch.zeros(n, dtype=torch.int32, device=rays.device)
    if n > 0:
        with _timed("baked_count_kernel", 0.0, 48.0 * n):
            _check(lib().nerf_baked_count(ctypes.byref(desc), _ptr(rays, "rays"), stride, _ptr(u, "u", True), n, float(step_size),
                                          int(max_steps), counts.data_ptr(), _stream()), "nerf_baked_count")
    return counts


def baked_train_fwd(desc, node_index, table, sh_degree, rays, u, step_size, max_steps, white_bkgd, offsets, total):
    """nerf_baked_train_fwd: (rgb_map fp32 [n, 3], acc_map, depth_map fp32 [n], records fp32 [max(total, 1), 12]) -- baked_render's bits
    with stop_eps = 0 and one record per kept sample, ray-major; offsets int32 [n + 1] = the exclusive running sum of baked_count's
    counts, total = offsets[n] as a Python int"""
    deg = int(sh_degree)
    if deg not in (0, 1, 2):
        raise NerfHipError(f"baked_train_fwd: sh_degree must be 0, 1 or 2, got {sh_degree!r}")
    n, stride = _baked_rays("baked_train_fwd", rays, u)
    nodes = (desc.res[0] + 1) * (desc.res[1] + 1) * (desc.res[2] + 1)
    if node_index.numel() != nodes:
        raise NerfHipError(f"baked_train_fwd: node_index holds one entry per lattice node, {nodes}")
    if not (isinstance(table, torch.Tensor) and table.is_cuda and table.dtype == torch.float16 and table.is_contiguous() and table.dim() == 2
            and table.shape[0] >= 1 and table.shape[1] == BAKED_ROW_HALVES[deg]):
        raise NerfHipError(f"baked_train_fwd: table must be a contiguous fp16 tensor [rows >= 1, {BAKED_ROW_HALVES[deg]}] on the GPU")
    total = int(total)
    if offsets.numel() != n + 1 or not (0 <= total <= BAKED_MAX_SAMPLES):
        raise NerfHipError(f"baked_train_fwd: offsets holds n + 1 entries and 0 <= total <= 2^30 samples, got {offsets.numel()} and {total}")
    dev = rays.device
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    acc, depth = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
    records = torch.empty((max(total, 1), BAKED_RECORD_WORDS), dtype=torch.float32, device=dev)
    if n > 0:
        # per ray 48 B in and 20 B out, per sample a 48-byte record out; what the samples gather depends on the scene and is not counted
        with _timed("baked_train_fwd_kernel", 0.0, 68.0 * n + 48.0 * total):
            _check(lib().nerf_baked_train_fwd(ctypes.byref(desc), _words(node_index, "node_index"), table.data_ptr(), int(table.shape[0]), deg,
                                              _ptr(rays, "rays"), stride, _ptr(u, "u", True), n, float(step_size), int(max_steps),
                                              int(bool(white_bkgd)), _words(offsets, "offsets"), total, _ptr(records), _ptr(rgb), _ptr(acc),
                                              _ptr(depth), _stream()), "nerf_baked_train_fwd")
    return rgb, acc, depth, records


def baked_train_bwd_samples(records, offsets, total, step_size, white_bkgd, g_rgb, g_acc, g_depth):
    """nerf_baked_train_bwd_samples: fp32 [max(total, 1), 4] = (dL/dv0, dL/dl_R, dL/dl_G, dL/dl_B) per sample record from the upstream
    gradients g_rgb [n, 3], g_acc [n], g_depth [n] of baked_train_fwd's outputs"""
    n = offsets.numel() - 1
    total = int(total)
    if tuple(g_rgb.shape) != (n, 3) or tuple(g_acc.shape) != (n,) or tuple(g_depth.shape) != (n,) or records.shape[0] < total:
        raise NerfHipError("baked_train_bwd_samples: g_rgb [n, 3], g_acc [n], g_depth [n] and `total` records")
    grads = torch.empty((max(total, 1), 4), dtype=torch.float32, device=records.device)
    if n > 0 and total > 0:
        with _timed("baked_train_bwd_samples_kernel", 0.0, 20.0 * n + 48.0 * total):       # 32 B of a record in, 16 B out
            _check(lib().nerf_baked_train_bwd_samples(_ptr(records, "records"), _words(offsets, "offsets"), n, total, float(step_size),
                                                      int(bool(white_bkgd)), _ptr(g_rgb, "g_rgb"), _ptr(g_acc, "g_acc"),
                                                      _ptr(g_depth, "g_depth"), _ptr(grads), _stream()), "nerf_baked_train_bwd_samples")
    return grads


def baked_train_bwd_rows(desc, row_node, sh_degree, rays, records, sample_grads, order, cell_start, total):
    """nerf_baked_train_bwd_rows: fp32 [n_rows, W], the gradient of the table: per row the sum over its adjacent cells (corner order) and
    each cell's samples (the order of `order`: int32 [total], the samples sorted by cell, stable; cell_start int32 [cells + 1]) of
    corner weight x contribution.  Two calls give the same bits."""
    deg = int(sh_degree)
    if deg not in (0, 1, 2):
        raise NerfHipError(f"baked_train_bwd_rows: sh_degree must be 0, 1 or 2, got {sh_degree!r}")
    n, stride = _baked_rays("baked_train_bwd_rows", rays, None)
    total = int(total)
    cells = desc.res[0] * desc.res[1] * desc.res[2]
    if order.numel() < total or cell_start.numel() != cells + 1 or records.shape[0] < total or sample_grads.shape[0] < total:
        raise NerfHipError(f"baked_train_bwd_rows: `total` records, sample gradients and entries of order, and cell_start [{cells + 1}]")
    n_rows = int(row_node.numel())
    grad = torch.empty((n_rows, BAKED_ROW_HALVES[deg]), dtype=torch.float32, device=rays.device)
    # per term a 32-byte piece of a record, 16 B of sample gradients and 12 B of the ray; per row 4 W bytes out
    with _timed("baked_train_bwd_rows_kernel", 0.0, 4.0 * grad.numel() + 8.0 * 64.0 * total):
        _check(lib().nerf_baked_train_bwd_rows(ctypes.byref(desc), _words(row_node, "row_node"), n_rows, deg, _ptr(rays, "rays"), stride, n,
                                               _ptr(records, "records"), _ptr(sample_grads, "sample_grads"), _words(order, "order"),
                                               _words(cell_start, "cell_start"), total, _ptr(grad), _stream()), "nerf_baked_train_bwd_rows")
    return grad


def baked_train_bwd_rays(desc, node_index, table, sh_degree, rays, records, sample_grads, offsets, total):
    """nerf_baked_train_bwd_rays (csrc/baked_rays.hip): fp32 [n, 11], the gradient of baked_train_fwd's outputs with respect to the ray
    records -- columns 0:3 (o), 3:6 (d) and 8:11 (viewdir); columns 6 and 7 are zeros -- from the forward's records and
    baked_train_bwd_samples' sample gradients.  Per ray a fixed order of summation: two calls give the same bits."""
    deg = int(sh_degree)
    if deg not in (0, 1, 2):
        raise NerfHipError(f"baked_train_bwd_rays: sh_degree must be 0, 1 or 2, got {sh_degree!r}")
    n, stride = _baked_rays("baked_train_bwd_rays", rays, None)
    nodes = (desc.res[0] + 1) * (desc.res[1] + 1) * (desc.res[2] + 1)
    if node_index.numel() != nodes:
        raise NerfHipError(f"baked_train_bwd_rays: node_index holds one entry per lattice node, {nodes}")
    if not (isinstance(table, torch.Tensor) and table.is_cuda and table.dtype == torch.float16 and table.is_contiguous() and table.dim() == 2
            and table.shape[0] >= 1 and table.shape[1] == BAKED_ROW_HALVES[deg]):
        raise NerfHipError(f"baked_train_bwd_rays: table must be a contiguous fp16 tensor [rows >= 1, {BAKED_ROW_HALVES[deg]}] on the GPU")
    total = int(total)
    if offsets.numel() != n + 1 or not (0 <= total <= BAKED_MAX_SAMPLES) or records.shape[0] < total or sample_grads.shape[0] < total:
        raise NerfHipError("baked_train_bwd_rays: offsets holds n + 1 entries, and `total` (0 .. 2^30) records and sample gradients")
    d_rays = torch.empty((n, 11), dtype=torch.float32, device=rays.device)
    if n > 0:
        # per sample 32 B of the record, 16 B of sample gradients and 32 B of node indices (the rows it gathers depend on the scene and
        # are not counted, as in baked_train_fwd); per ray 20 B in and 44 B out
        with _timed("baked_train_bwd_rays_kernel", 0.0, 64.0 * n + 80.0 * total):
            _check(lib().nerf_baked_train_bwd_rays(ctypes.byref(desc), _words(node_index, "node_index"), table.data_ptr(), int(table.shape[0]),
                                                   deg, _ptr(rays, "rays"), stride, n, _ptr(records, "records"),
                                                   _ptr(sample_grads, "sample_grads"), _words(offsets, "offsets"), total, _ptr(d_rays),
                                                   _stream()), "nerf_baked_train_bwd_rays")
    return d_rays


# ---- baked field, regularisers (csrc/baked_reg.hip; the user-facing method is baked.BakedTrainer.regularizers)
def _baked_reg_args(who, desc, node_index, row_node, values, sh_degree, scales, eps):
    deg = int(sh_degree)
    if deg not in (0, 1, 2):
        raise NerfHipError(f"{who}: sh_degree must be 0, 1 or 2, got {sh_degree!r}")
    W = BAKED_ROW_HALVES[deg]
    if not (isinstance(values, torch.Tensor) and values.is_cuda and values.dtype == torch.float32 and values.is_contiguous()
            and values.dim() == 2 and values.shape[0] >= 1 and values.shape[1] == W):
        raise NerfHipError(f"{who}: values must be a contiguous fp32 tensor [rows >= 1, {W}] on the GPU")
    nodes = (desc.res[0] + 1) * (desc.res[1] + 1) * (desc.res[2] + 1)
    n_rows = int(values.shape[0])
    if node_index.numel() != nodes or row_node.numel() != n_rows:
        raise NerfHipError(f"{who}: node_index holds one entry per lattice node, {nodes}, and row_node one per row, {n_rows}")
    sx, sy, sz = (float(s) for s in scales)
    return deg, W, n_rows, nodes, sx, sy, sz, float(eps)


def baked_reg_fwd(desc, node_index, row_node, values, sh_degree, scales, eps):
    """nerf_baked_reg_fwd: terms fp32 [n_rows, 3] of the fp32 table `values` [n_rows, W]: per stored row the total-variation term of the
    density column, the sum of the colour columns' terms and the Cauchy term log1p(2 max(sigma, 0)^2); zeros for row 0.  scales = (sx, sy,
    sz), min(cell edge) / (cell edge along the axis)."""
    deg, W, n_rows, nodes, sx, sy, sz, eps = _baked_reg_args("baked_reg_fwd", desc, node_index, row_node, values, sh_degree, scales, eps)
    terms = torch.empty((n_rows, 3), dtype=torch.float32, device=values.device)
    # the table in once (the three forward neighbours come from cache), 12 B per row out, both index arrays in
    with _timed("baked_reg_fwd_kernel", 0.0, 4.0 * W * n_rows + 12.0 * n_rows + 4.0 * n_rows + 4.0 * nodes):
        _check(lib().nerf_baked_reg_fwd(ctypes.byref(desc), _words(node_index, "node_index"), _words(row_node, "row_node"), _ptr(values, "values"),
                                        n_rows, deg, sx, sy, sz, eps, _ptr(terms), _stream()), "nerf_baked_reg_fwd")
    return terms


def baked_reg_bwd(desc, node_index, row_node, values, sh_degree, scales, eps, g):
    """nerf_baked_reg_bwd: fp32 [n_rows, W], the gradient with respect to `values` of g[0] sum(terms[:, 0]) + g[1] sum(terms[:, 1]) +
    g[2] sum(terms[:, 2]) (g: fp32 [3] on the GPU), gathered per row without atomics.  Two calls give the same bits."""
    deg, W, n_rows, nodes, sx, sy, sz, eps = _baked_reg_args("baked_reg_bwd", desc, node_index, row_node, values, sh_degree, scales, eps)
    if tuple(g.shape) != (3,):
        raise NerfHipError("baked_reg_bwd: g holds the three upstream gradients")
    grad = torch.empty((n_rows, W), dtype=torch.float32, device=values.device)
    # the table in once if the 13-row gather is served by cache, the gradient out, both index arrays in
    with _timed("baked_reg_bwd_kernel", 0.0, 4.0 * W * n_rows + 4.0 * W * n_rows + 4.0 * n_rows + 4.0 * nodes):
        _check(lib().nerf_baked_reg_bwd(ctypes.byref(desc), _words(node_index, "node_index"), _words(row_node, "row_node"), _ptr(values, "values"),
                                        n_rows, deg, sx, sy, sz, eps, _ptr(g, "g"), _ptr(grad), _stream()), "nerf_baked_reg_bwd")
    return grad


# ---- hash-grid encoding (csrc/hash_encode.hip; hashgrid.HashEncoding builds the record)
HASH_MAX_LEVELS = 32


class NerfHashGrid(ctypes.Structure):
    """include/nerf_hip.h NerfHashGrid"""
    _fields_ = [("n_levels", ctypes.c_int), ("n_features", ctypes.c_int), ("log2_hashmap_size", ctypes.c_int), ("reserved", ctypes.c_int),
                ("lo", ctypes.c_float * 3), ("inv_extent", ctypes.c_float * 3), ("level_resolution", ctypes.c_int * HASH_MAX_LEVELS),
                ("level_dense", ctypes.c_int * HASH_MAX_LEVELS), ("level_offset", ctypes.c_longlong * (HASH_MAX_LEVELS + 1))]


def _hash_points(who, points, rays, z_vals):
    """(points pointer, rays pointer, ray stride, z pointer, samples per ray, number of points): points [P, 3], or rays [N, >= 6] with
    z_vals [N, S] (the points o + d z)"""
    if points is not None:
        if rays is not None or z_vals is not None:
            raise NerfHipError(f"{who}: give points or rays + z_vals, not both")
        if points.dim() != 2 or points.shape[1] != 3:
            raise NerfHipError(f"{who}: points must be [P, 3]")
        P = int(points.shape[0])
        return (_ptr(points, "points") if P else None), None, 0, None, 1, P
    if rays is None or z_vals is None or rays.dim() != 2 or z_vals.dim() != 2 or rays.shape[0] != z_vals.shape[0] or rays.shape[1] < 6:
        raise NerfHipError(f"{who}: rays [N, >= 6] and z_vals [N, S] are required without points")
    P = int(z_vals.numel())
    S = max(int(z_vals.shape[1]), 1)
    return None, (_ptr(rays, "rays") if P else None), int(rays.shape[1]), (_ptr(z_vals, "z_vals") if P else None), S, P


def _hash_cols(who, t, lo, width, P):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()
            and t.shape[0] == P and 0 <= lo and lo + width <= t.shape[1]):
        raise NerfHipError(f"{who}: needs a contiguous fp32 matrix [{P}, >= {lo + width}] on the GPU")
    return (t.data_ptr() + 4 * lo if P else None), int(t.shape[1])


def hash_encode_fwd(desc, embeddings, out, col=0, points=None, rays=None, z_vals=None):
    """nerf_hash_encode_fwd: writes the encoding of the points into columns col .. col + L F of the row-major fp32 matrix `out` [P, >= col
    + L F]; the other columns are untouched.  P == 0 launches nothing."""
    pp, rp, stride, zp, S, P = _hash_points("hash_encode_fwd", points, rays, z_vals)
    L, F = desc.n_levels, desc.n_features
    if tuple(embeddings.shape) != (desc.level_offset[L], F):
        raise NerfHipError(f"hash_encode_fwd: embeddings must be [{desc.level_offset[L]}, {F}]")
    op, ld = _hash_cols("hash_encode_fwd", out, col, L * F, P)
    # per point and level 8 rows in (random: whole 4 F byte rows), L F floats out
    with _timed("hash_fwd_kernel", 0.0, P * L * (8.0 * 4 * F + 4.0 * F)):
        _check(lib().nerf_hash_encode_fwd(ctypes.byref(desc), _ptr(embeddings, "embeddings"), pp, rp, stride, zp, S, P, op, ld, _stream()),
               "nerf_hash_encode_fwd")
    return out


def hash_scratch(desc, device):
    """a zeroed accumulator for hash_encode_bwd: int64 [nerf_hash_scratch_words]; a complete backward leaves it zero"""
    return torch.zeros(lib().nerf_hash_scratch_words(ctypes.byref(desc)), dtype=torch.int64, device=device)


def hash_encode_bwd(desc, d_out, col=0, points=None, rays=None, z_vals=None, scratch=None, phases=3, d_embeddings=None):
    """nerf_hash_encode_bwd: fp32 [rows_total, F], the gradient of the table from columns col .. col + L F of d_out [P, >= col + L F],
    accumulated in 64-bit fixed point (two calls give the same bits; M = max |d_out| == 0: zeros, not finite: NaN).  scratch: a
    hash_scratch() the caller keeps (left zero), else a fresh one.  phases: 1 the maximum + the scatter (returns None), 2 the finishing
    pass, 3 both."""
    pp, rp, stride, zp, S, P = _hash_points("hash_encode_bwd", points, rays, z_vals)
    L, F = desc.n_levels, desc.n_features
    dp, ld = _hash_cols("hash_encode_bwd", d_out, col, L * F, P)
    if scratch is None:
        scratch = hash_scratch(desc, d_out.device)
    rows = desc.level_offset[L]
    if not (scratch.is_cuda and scratch.dtype == torch.int64 and scratch.is_contiguous() and scratch.numel() == rows * F + 1):
        raise NerfHipError(f"hash_encode_bwd: scratch must be hash_scratch(desc, device): int64 [{rows * F + 1}] on the GPU")
    if phases & 2 and d_embeddings is None:
        d_embeddings = torch.empty((rows, F), dtype=torch.float32, device=d_out.device)
    args = lambda ph: (ctypes.byref(desc), pp, rp, stride, zp, S, P, dp, ld, scratch.data_ptr(),
                       None if d_embeddings is None else _ptr(d_embeddings, "d_embeddings"), ph, _stream())
    if phases & 1:      # P L F words read twice (maximum, scatter), 8 F adds of 8 bytes per point and level
        with _timed("hash_scatter_kernel", 0.0, P * L * (8.0 * F + 64.0 * F)):
            _check(lib().nerf_hash_encode_bwd(*args(1)), "nerf_hash_encode_bwd")
    if phases & 2:      # the accumulator in and out (zeroed), the gradient out
        with _timed("hash_finish_kernel", 0.0, rows * F * 20.0):
            _check(lib().nerf_hash_encode_bwd(*args(2)), "nerf_hash_encode_bwd")
    return d_embeddings


def hash_input_grad(desc, embeddings, d_x, col, points, rays, z_vals, views_col, multires_views, accumulate=False):
    """nerf_hash_input_grad: the gradient with respect to the points from columns col .. col + L F of d_x [P, >= col + L F] (DESIGN.md
    3.28).  Point mode (points [P, 3]): returns d_points [P, 3].  Ray mode (rays [N, >= 6] + z_vals [N, S]): returns d_rays [N, 11] by
    nerf_field_input_grad's column contract, columns 8:11 from the 3 + 6 multires_views view columns of d_x at views_col (an index into
    d_x's columns, not relative to col; < 0: none, zeros); `accumulate`: a d_rays [N, 11] tensor to add to (its columns 6:8 stay),
    returned.  No atomics: two calls give the same bits."""
    pp, rp, stride, zp, S, P = _hash_points("hash_input_grad", points, rays, z_vals)
    L, F = desc.n_levels, desc.n_features
    if tuple(embeddings.shape) != (desc.level_offset[L], F):
        raise NerfHipError(f"hash_input_grad: embeddings must be [{desc.level_offset[L]}, {F}]")
    dp, ld = _hash_cols("hash_input_grad", d_x, col, L * F, P)
    ray_mode = points is None
    if not ray_mode and (views_col >= 0 or (accumulate is not None and accumulate is not False)):
        raise NerfHipError("hash_input_grad: view columns and accumulate belong to ray mode")
    if ray_mode and rays.shape[1] < 11 and views_col >= 0:
        raise NerfHipError("hash_input_grad: view columns need ray records of 11 columns")
    vc = -1 if views_col < 0 else int(views_col) - int(col)         # (the library counts from the pointer it is handed)
    dev = d_x.device
    d_points = d_rays = work = None
    acc = 0
    if ray_mode:
        N = int(rays.shape[0])
        if isinstance(accumulate, torch.Tensor):
            if tuple(accumulate.shape) != (N, 11):
                raise NerfHipError(f"hash_input_grad: accumulate must be a d_rays tensor [{N}, 11]")
            d_rays, acc = accumulate, 1
        elif accumulate:
            raise NerfHipError("hash_input_grad: accumulate is False or the d_rays tensor to add to")
        else:
            d_rays = (torch.empty if P else torch.zeros)((N, 11), dtype=torch.float32, device=dev)      # (no samples: nothing is launched)
        work = torch.empty(lib().nerf_hash_input_grad_workspace_floats(P), dtype=torch.float32, device=dev)
    else:
        d_points = torch.empty((P, 3), dtype=torch.float32, device=dev)
    opt = lambda t: None if t is None or t.numel() == 0 else _ptr(t)
    # per point and level 8 rows in (the forward's), L F floats of d_x; 12 bytes out (ray mode: written and read once more)
    with _timed("hash_point_grad_kernel", 0.0, P * L * (8.0 * 4 * F + 4.0 * F) + 12.0 * P):
        _check(lib().nerf_hash_input_grad(ctypes.byref(desc), _ptr(embeddings, "embeddings"), pp, rp, stride, zp, S, P, dp, ld, vc,
                                          int(multires_views), opt(d_points), opt(d_rays), opt(work), acc, _stream()), "nerf_hash_input_grad")
    return d_rays if ray_mode else d_points


# Bumped by every raw-pointer update of parameters (the fused Adam kernel writes through data_ptr(), which does not
# advance the tensors' autograd version counters): NeRF.packed_params() keys its fragment-repack cache on it.
PARAM_EPOCH = 0             # total number of raw-pointer updates (any vector)
_PARAM_EPOCHS = {}          # ... per updated vector (keyed by the device address of its storage)


def _epoch_key(t):
    # the STORAGE a vector lives in, not the address of its first element: FlatAdam hands the kernel the run of parameters that
    # have gradients, which starts anywhere inside a network's flat vector (frozen first layer, heads-only fine-tuning)
    return t.untyped_storage().data_ptr()


def param_epoch(flat):
    """number of raw-pointer (fused Adam) updates of the storage THIS flat parameter vector lives in: an optimizer step on an
    unrelated network neither invalidates another network's fragment repack nor trips the stale-parameter guard of its pending
    backward; a step on any part of this network's vector does both"""
    return _PARAM_EPOCHS.get(_epoch_key(flat), 0)


def adam_step(params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step):
    """In-place fused Adam over flat fp32 vectors (one launch)."""
    global PARAM_EPOCH
    PARAM_EPOCH += 1
    _PARAM_EPOCHS[_epoch_key(params)] = _PARAM_EPOCHS.get(_epoch_key(params), 0) + 1
    n = params.numel()
    _check(lib().nerf_adam_step(_ptr(params, "params"), _ptr(grads, "grads"), _ptr(exp_avg, "exp_avg"),
                                _ptr(exp_avg_sq, "exp_avg_sq"), n, float(lr), float(beta1), float(beta2), float(eps),
                                int(step), _stream()), "nerf_adam_step")
