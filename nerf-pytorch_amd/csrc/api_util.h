// Shared by the extern "C" translation units (api.hip, render_abi.hip): error reporting, the decoders of the public datapath
// codes and the buffer-tag registry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stddef.h>
#include "../../include/nerf_hip.h"
#include "launchers.h"

namespace nerf_api {

using nerf::Datapath;
using nerf::DatapathDesc;
using nerf::FwdMode;

inline thread_local char g_err[384] = "";

inline int fail_arg(const char* fn, const char* what) {
    snprintf(g_err, sizeof(g_err), "%s: %s", fn, what);
    return NERF_E_BADARG;
}
inline int done(const char* fn, hipError_t e) {
    if (e == hipSuccess) return 0;
    snprintf(g_err, sizeof(g_err), "%s: HIP error %d (%s)", fn, (int)e, hipGetErrorString(e));
    return (int)e;
}

// ---- the public datapath codes (the table at the top of include/nerf_hip.h), per datapath in Datapath order; -1: none.  Each
// vocabulary is decoded once, at the extern "C" boundary (false = no such code); below it everything speaks nerf::Datapath.
struct PublicCodes { int split, wgrad, precision; };
constexpr PublicCodes CODES[nerf::N_DATAPATHS] = {{-1, 0, 0}, {0, 4, 1}, {1, 5, 3}, {5, 6, 5}};
inline bool decode_code(int PublicCodes::*vocabulary, int code, Datapath* dp) {
    for (int i = 0; i < nerf::N_DATAPATHS; ++i)
        if (code >= 0 && CODES[i].*vocabulary == code) { *dp = (Datapath)i; return true; }
    return false;
}
// `datapath` of nerf_field_wgrad_phase[_live] (-1, "as recorded", is the caller's business) and NerfRenderCfg.precision
inline bool decode_wgrad_datapath(int code, Datapath* dp) { return decode_code(&PublicCodes::wgrad, code, dp); }
inline bool decode_precision(int code, Datapath* dp) { return decode_code(&PublicCodes::precision, code, dp); }
// `split` of nerf_field_fwd_split / nerf_field_dgrad_split[_live] / nerf_pack_params_split[_pair] (each accepts a subset); 2 / 3: the
// reduced inference forward of F16X3, 3 with the last sample left out
struct SplitCode { bool ok; Datapath dp; FwdMode mode; };
inline SplitCode decode_split(int code) {
    SplitCode c{true, Datapath::F16X3, code == 2 ? FwdMode::Reduced : code == 3 ? FwdMode::ReducedSkipLast : FwdMode::Full};
    if (c.mode == FwdMode::Full) c.ok = decode_code(&PublicCodes::split, code, &c.dp);
    return c;
}
// the layout family of nerf_*_floats_dp / nerf_debug_layout: a datapath of that family (sizes and offsets do not depend on the 16-bit type)
inline bool decode_family(int family, Datapath* dp) {
    for (int i = 0; i < nerf::N_DATAPATHS; ++i)
        if (nerf::DATAPATHS[i].family == family) { *dp = (Datapath)i; return true; }
    return false;
}

// ---- buffer tags.  The save buffer of a forward (`act`) and the delta buffer of a dgrad exist in one layout per datapath
// (nerf_common.h; the kinds: launchers.h); which one a buffer holds is decided by the entry point that WROTE it, and the entry
// point that reads it must agree.  The library remembers, per buffer address, what its own entry points last wrote there (host
// memory only: a small table, nothing on the device, no pointer is ever dereferenced) so that a mismatched pairing is refused with
// NERF_E_BADARG instead of computing garbage, and so that nerf_field_wgrad_phase(datapath = -1) can pick the datapath
// itself.  Buffers the library has not seen (copied, produced elsewhere) are not checked.
struct BufTag { int is_delta; Datapath dp; int n_rays, n_samples; unsigned long seq; };      // dp: whose forward / dgrad wrote the buffer
inline int tag_kind(const BufTag& t) { return t.is_delta ? (int)nerf::desc(t.dp).delta : (int)nerf::desc(t.dp).act; }
void tag_record(const void* buf, int is_delta, Datapath dp, int n_rays, int n_samples);
bool tag_lookup(const void* buf, BufTag* out);

// floats of a save / delta buffer in dp's layout
size_t act_floats(int n_rays, int n_samples, Datapath dp);
size_t delta_floats(int n_rays, int n_samples, Datapath dp);

inline bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d) |
             reinterpret_cast<uintptr_t>(e)) & 15) == 0;
}

}  // namespace nerf_api

#define REQUIRE(cond, what) do { if (!(cond)) return nerf_api::fail_arg(__func__, what); } while (0)
