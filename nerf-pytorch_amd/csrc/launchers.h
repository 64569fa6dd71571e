// Host-side launch interface between api.hip and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

namespace nerf {

// ---- the datapaths.  The public integer codes (the table at the top of include/nerf_hip.h) are decoded once, at the extern "C"
// boundary (api_util.h); everything below it speaks these.  ActLayoutKind / DeltaKind: what nerf_buffer_layout reports (public values).
enum ActLayoutKind { ACT_ROWS_F32 = 0, ACT_TILE16_BF16 = 4, ACT_TILE16_F16 = 5, ACT_TILE16_F16X2 = 6 /* hi + lo words (two-word saves) */ };
enum DeltaKind { DELTA_ROWS_F32 = 0, DELTA_TILE32_BF16 = 2, DELTA_TILE32_F16 = 3, DELTA_TILE32_F16X2 = 4 };
enum class Datapath { F32, BF16X3, F16X3, F16X3W };
constexpr int N_DATAPATHS = 4;
// the reduced inference forward ("fp16_fp8c": fp16 main term + fp8 corrections, field_ring8.h) is F16X3 in a forward-only mode: it
// saves nothing, and its repack is the third pack form.  ReducedSkipLast leaves every ray's last sample to launch_field_fwd16r_last.
enum class FwdMode { Full, Reduced, ReducedSkipLast };
struct DatapathDesc {
    bool split;             // on the weight-ring kernels: three-term split products, folded feature layer, tiled 16-bit saves
    bool f16;               // fp16 parts (else bf16; csrc/split_types.h)
    bool two_word;          // hi + lo words saved, three-term weight-gradient GEMM
    ActLayoutKind act;      // what its forward writes
    DeltaKind delta;        // what its dgrad writes
    int family;             // layout family of the *_dp size entry points: 0 fp32 rows, 1 16-bit tiles, 2 hi + lo tiles
};
constexpr DatapathDesc DATAPATHS[N_DATAPATHS] = {
    {false, false, false, ACT_ROWS_F32, DELTA_ROWS_F32, 0},
    {true, false, false, ACT_TILE16_BF16, DELTA_TILE32_BF16, 1},
    {true, true, false, ACT_TILE16_F16, DELTA_TILE32_F16, 1},
    {true, true, true, ACT_TILE16_F16X2, DELTA_TILE32_F16X2, 2},
};
constexpr const DatapathDesc& desc(Datapath dp) { return DATAPATHS[(int)dp]; }

struct CompositeArgs {
    const float* raw;       // [N][S][4]
    const float* z;         // [N][S]
    const float* dirs;      // ray directions: dirs[r*dir_stride + 0..2]
    const float* noise;     // [N][S] standard normal, nullable
    float noise_std;
    int dir_stride, n_rays, S, white_bkgd;
    // forward outputs (weights / depth nullable)
    float* rgb; float* disp; float* acc; float* weights; float* depth;
    // backward inputs / output
    const float* d_rgb;     // [N][3]
    const float* d_acc;     // [N] nullable
    const float* d_disp;    // [N] nullable
    float* d_raw;           // [N][S][4]
    const float* d_weights; // [N][S] nullable: upstream gradient of the `weights` output
    const float* d_depth;   // [N] nullable: upstream gradient of `depth_map`
    // geometry adjoint (nerf_raw2outputs_bwd_geom; both NULL = the plain adjoint w.r.t. raw, unchanged)
    float* d_dirs;          // [N][3] nullable: dL/d rays_d through dists = dz * |rays_d| (written)
    float* d_z;             // [N][S] nullable: dL/d z_vals through dists and the depth integral (written)
};

// distortion loss of the compositing weights (ray_device.h: distortion_ray)
struct DistortionArgs {
    const float* w;         // [N][S] compositing weights
    const float* z;         // [N][S] depths, non-decreasing per ray
    const float* near_far;  // near_far[r*nf_stride + 0..1] = the ray's near, far
    int nf_stride, n_rays, S;
    float* loss;            // [N]                                       (forward)
    const float* d_loss;    // [N] upstream gradient                     (adjoint)
    float* d_w;             // [N][S] written, or added to with accumulate (adjoint)
    int accumulate;
};

// interlevel loss of proposal weights against a target histogram (ray_device.h: interlevel_ray)
struct InterlevelArgs {
    const float* wp;        // [N][P] proposal weights
    const float* zp;        // [N][P] proposal depths, non-decreasing per ray
    const float* w;         // [N][S] target weights (a constant of the graph)
    const float* z;         // [N][S] target depths, non-decreasing per ray
    int n_rays, P, S;
    float* loss;            // [N]                                       (forward)
    const float* d_loss;    // [N] upstream gradient                     (adjoint)
    float* d_wp;            // [N][P] written, or added to with accumulate (adjoint)
    int accumulate;
};

struct FineArgs {
    // direct == 0: in0 = coarse depths z[N][Sc], in1 = coarse weights[N][Sc]
    //              bins = mid-points, pdf from weights[1:-1]               (run_nerf.py:392-393)
    // direct == 1: in0 = bins[N][nb], in1 = weights[N][nb-1]               (sample_pdf as called standalone)
    const float* in0; const float* in1;
    const float* u;         // [N][Nf] uniform draws, nullable -> u_lin
    const float* u_lin;     // [Nf] torch.linspace(0,1,Nf)
    float* z_all;           // [N][Sc+Nf] sorted union (direct == 0 only), nullable
    float* z_samples;       // [N][Nf] nullable
    float* z_std;           // [N] nullable
    int n_rays, n_in, Nf, direct;   // n_in = Sc (direct == 0) or nb (direct == 1)
};

// render_rays without gradients in one launch (render_fused.hip)
struct RenderInferArgs {
    const float* packed_c;  // packed3 of the coarse network
    const float* packed_f;  // packed3 of the fine network (== packed_c when there is none)
    const float* rays;
    int ray_stride, n_rays, n_c, n_f, lindisp, white_bkgd;
    float noise_std;
    const float* t_rand;    // [N][n_c] or null
    const float* noise_c;   // [N][n_c] or null
    const float* u;         // [N][n_f] or null (deterministic: linspace)
    const float* noise_f;   // [N][n_c + n_f] or null
    // coarse pass (the only pass when n_f == 0: then these ARE the outputs)
    float *z_c, *raw_c, *w_c, *rgb_c, *disp_c, *acc_c;
    // fine pass
    float *z_f, *z_std, *raw_f, *rgb_f, *disp_f, *acc_f;
    int split;              // 16-bit type of the three-term split the packed buffers were made for: DatapathDesc::f16
};
bool render_infer_fused_ok(int n_c, int n_f);
hipError_t launch_render_infer(const RenderInferArgs& a, hipStream_t stream);

hipError_t launch_pack(const float* canon_params, float* packed, hipStream_t stream);
hipError_t launch_sample_coarse(const float* rays, int ray_stride, int n_rays, const float* t_vals, int S,
                                int lindisp, const float* t_rand, float* z_out, hipStream_t stream);
constexpr int MSE_SCRATCH_FLOATS = 256 + 1;      // per-block partial sums + the ticket word of mse_fwd_kernel
// max |fp16| pattern over packed words (range check of the fp16 split's saved rows / deltas): words[1] = max pattern, words[0] |= (>= 0x7800)
hipError_t launch_range_scan(const unsigned* rows, size_t n_words, unsigned* words, hipStream_t stream);
hipError_t launch_mse_fwd(const float* x, const float* y, long n, float* scratch, float* out, hipStream_t stream);
hipError_t launch_mse_bwd(const float* x, const float* y, long n, const float* g, float* dx, hipStream_t stream);
hipError_t launch_embed(const float* x, long n_pts, int n_freqs, float* out, hipStream_t stream);
hipError_t launch_embed_bwd(const float* x, long n_pts, int n_freqs, const float* d_out, float* d_x, int accumulate, hipStream_t stream);
// input gradients of one field evaluation from its deltas (field_input_grad.hip); kind = what the dgrad wrote there
hipError_t launch_field_input_grad(const float* params, const float* delta, DeltaKind kind, const float* rays, int ray_stride,
                                   const float* z_vals, int n_rays, int S, float* d_rays, int accumulate, hipStream_t stream);
hipError_t launch_make_rays(int H, int W, const float* K9, const float* pose12, const float* pose_static12, int ndc,
                            float near, float far, float* rays, int ray_stride, hipStream_t stream);
hipError_t launch_assemble_rays(const float* rays_o, const float* rays_d, long n, int ndc, int H, int W, float focal,
                                float near, float far, float* rays, int ray_stride, hipStream_t stream);
hipError_t launch_sample_ray_batch(int H, int W, const float* K9, const float* pose_dev, int pose_stride, const float* image, int h0, int w0,
                                   int nh, int nw, int n_rand, unsigned key0, unsigned key1, float* rays, float* target, int* pixels,
                                   hipStream_t stream);
hipError_t launch_sample_ray_views(int H, int W, const float* K9, const int* view_ids, int n_views, int n_table, const float* poses,
                                   long pose_view_stride, int pose_row_stride, const float* images, long image_view_stride,
                                   unsigned first, unsigned n_out, unsigned key0, unsigned key1, float* rays, float* target, int* pixels,
                                   int* views, hipStream_t stream);
hipError_t launch_ray_pose_grad(int W, const float* K9, const float* d_rays, int n_rays, const int* pixels, const int* views, int n_views,
                                float* d_pose, int accumulate, hipStream_t stream);
hipError_t launch_composite(const CompositeArgs& a, bool bwd, hipStream_t stream);
hipError_t launch_distortion(const DistortionArgs& a, bool bwd, hipStream_t stream);
hipError_t launch_interlevel(const InterlevelArgs& a, bool bwd, hipStream_t stream);
hipError_t launch_sample_fine(const FineArgs& a, hipStream_t stream);
hipError_t launch_field_fwd(const float* packed, const float* rays, int ray_stride, const float* z_vals,
                            int n_rays, int S, float* raw, float* act, hipStream_t stream);
hipError_t launch_field_bwd(const float* packed, const float* act, const float* d_raw, int n_rays, int S,
                            float* delta, float* partial, float* grad, int accumulate, hipStream_t stream);
hipError_t launch_field_dgrad(const float* packed, const float* act, const float* d_raw, int n_rays, int S,
                              float* delta, hipStream_t stream);
// live (split datapaths, nullable): the live-tile list the delta chain of the same pass wrote; the GEMM streams the live tiles only
hipError_t launch_field_wgrad(const float* act, const float* delta, const float* d_raw, int n_rays, int S,
                              float* partial, float* grad, int accumulate, Datapath dp,
                              int phases, hipStream_t stream, const float* params,      // canonical parameters: required by the split datapaths
                              const unsigned* live = nullptr);
size_t wgrad_partial_floats(long P);
hipError_t launch_adam(float* p, const float* g, float* m, float* v, int n, float lr, float b1, float b2, float eps, int step,
                       hipStream_t stream);
void pack_table_host(int* out);
void pack3_table_host(int* out);
void pack16_table_host(int* out);
// the (hi, lo) fragment repack of a split datapath; mode Reduced: the reduced inference stream on top of F16X3's
hipError_t launch_pack3_sel(const float* canon_params, float* packed, int streams, hipStream_t stream, Datapath dp, FwdMode mode);
hipError_t launch_pack3_pair(const float* params_a, float* packed_a, const float* params_b, float* packed_b, int streams, hipStream_t stream, Datapath dp);
// largest launches of the 16-point forward: n_rays * S points in all, and with saving (4.8 KB per point: 2^26 points = 320 GB)
constexpr long FWD16R_MAX_POINTS = (1L << 31) - 1, FWD16R_MAX_SAVED_POINTS = 1L << 26;
// dp: a split datapath (its repack in packed3); a mode other than Full needs F16X3 and act == nullptr
hipError_t launch_field_fwd16r(const float* packed3, const float* rays, int ray_stride, const float* z_vals,
                               int n_rays, int S, float* raw, float* act, Datapath dp, FwdMode mode, hipStream_t stream);
hipError_t launch_field_fwd16r_last(const float* packed3, const float* rays, int ray_stride, const float* z_vals,
                                    int n_rays, int S, float* raw, const float* packed3_next, float* raw_next, int S_next,
                                    hipStream_t stream);
hipError_t launch_field_dgrad3r(const float* packed3, const float* act, const float* d_raw, int n_rays, int S,
                                float* delta, Datapath dp, hipStream_t stream, unsigned* live = nullptr);

// The live-tile list of one backward pass (caller-owned words; written by launch_field_dgrad3r, read by the delta chain and the
// weight-gradient GEMM).  Tile t = points 32 t .. 32 t + 31 of the launch; dead = all 128 words of its d_raw are +-0.
//   [0] count of live tiles   [1] n_tiles   [2], [3] zero
//   [LIVE_HEADER + i]   the live tile numbers, ascending, i < count (n_tiles words reserved)
//   [bitmap + w]        bit b = tile 32 w + b is live (n_words words)
//   [prefix + w]        live tiles before tile 32 w (n_words + 1 words: the last one = count)
constexpr unsigned LIVE_HEADER = 4;
// the kernels read the list (words an EARLIER launch wrote) through the constant address space: a uniform address becomes a scalar load
typedef const unsigned __attribute__((address_space(4)))* const_words;
__device__ inline const_words as_const_words(const unsigned* p) { return (const_words)(uintptr_t)p; }
struct LiveTiles { unsigned n_tiles, n_words; size_t bitmap, prefix, total; };
__host__ __device__ inline LiveTiles live_tiles(unsigned n_tiles) {
    LiveTiles l;
    l.n_tiles = n_tiles;
    l.n_words = (n_tiles + 31) / 32;
    l.bitmap = LIVE_HEADER + (size_t)n_tiles;
    l.prefix = l.bitmap + l.n_words;
    l.total = (l.prefix + l.n_words + 1 + 3) & ~(size_t)3;
    return l;
}
// NERF_BWD_FOLD_LAUNCHES=0 in the environment (read per call, as NERF_WG_MERGE_ALPHA is): the small launches around the heavy
// kernels in their separate forms -- delta_amax_kernel<true> and replicate_dir_bf16_kernel instead of bwd_prologue_kernel,
// wgrad_reduce_kernel + wgrad_fold_kernel instead of wgrad_reduce_fold_kernel, derive_folded_kernel + pack3_all_kernel instead of
// pack3_fused_kernel.  Same bits either way: the comparison side of tests/test_gpu_bwd_prologue.py, test_gpu_reduce_fold.py and
// test_gpu_repack_one_launch.py.
inline bool fold_launches() {
    const char* e = getenv("NERF_BWD_FOLD_LAUNCHES");
    return !(e && e[0] == '0');
}
// The per-ray direction encoding replicated for the weight-gradient GEMM ([ray][feature][8 copies], field_bwd.hip) when a ray's
// samples fill whole tiles (S % 32 == 0): with a live-tile list it is launch_field_dgrad3r that writes it into the save buffer
// (it depends on the forward's save alone) and launch_field_wgrad that relies on it -- a contract of the two *_live entry points
// (include/nerf_hip.h), no state in between.  Without a list, or with ragged rays, the weight-gradient call expands as ever.
hipError_t launch_replicate_dir(const float* act, int n_rays, int S, Datapath dp, hipStream_t stream);
// one 16-byte record of that replication: eight copies of the 16-bit hi word of x (LO: of the remainder x - hi); SP: split_types.h
template <typename SP, bool LO>
__device__ inline void dir_record(float x, unsigned (&w)[4]) {
    if (LO) {
        const unsigned short h = SP::cvt1(x);
        if constexpr (SP::F16) x = x - (float)__builtin_bit_cast(_Float16, h);
        else x = x - __uint_as_float((unsigned)h << 16);
    }
    const unsigned pk = SP::cvt_pk(x, x);
    w[0] = w[1] = w[2] = w[3] = pk;
}

// ---- EXPERIMENT, not in the default build (NERF_LIVE_GROUPS = 0): dead point groups inside live tiles.  Measured slower than whole
// tiles (profiles/r16_dead_groups_measurements.md); the source stays so that those rows can be reproduced:
//   tools/build_variant.sh groups -DNERF_LIVE_GROUPS=1    (2: the dead pieces are zero-filled in LDS instead of fetched from the zero line)
// and NERF_BWD_LIVE_GROUP = 16 or 8 in the environment of a process that loads that library (NERF_HIP_LIB); 32 or unset = whole tiles.
// In such a build the list buffer (nerf_live_tiles_words) has live_groups(n_tiles).total words and the *_live entry points use them.
// Group liveness, appended BEHIND the words above.  A group is G consecutive points of a tile, dead when all 4 G words of its d_raw
// are +-0.  The masks are kept at 8-point granularity whatever G is; a 16-point group is live when either of its halves is.
//   [ext + 0]       dead 8-point groups inside LIVE tiles     [ext + 1]  dead 16-point groups inside live tiles
//   [ext + 2]       the G this list was written for           [ext + 3]  zero
//   [gmask + w]     nibble j (bits 4 j .. 4 j + 3) = tile 8 w + j: bit k = points 8 k .. 8 k + 7 of the tile carry something
//                   (4 * n_words words: every tile the bitmap has a bit for; tiles past the launch read 0)
//   [zero + i]      LIVE_ZERO_WORDS zero words (16-byte aligned): the source of a dead group's DMA pieces
#ifndef NERF_LIVE_GROUPS
#define NERF_LIVE_GROUPS 0
#endif
constexpr unsigned LIVE_ZERO_WORDS = 64;
struct LiveGroups { size_t ext, gmask, zero, total; };
__host__ __device__ inline LiveGroups live_groups(unsigned n_tiles) {
    const LiveTiles t = live_tiles(n_tiles);
    LiveGroups g;
    g.ext = t.total;
    g.gmask = g.ext + 4;
    g.zero = g.gmask + 4 * (size_t)t.n_words;
    g.total = g.zero + LIVE_ZERO_WORDS;
    return g;
}
// the group size of this process: 32 (whole tiles) in the default build whatever the environment says
inline int live_group() {
#if NERF_LIVE_GROUPS
    static const int g = [] { const char* e = getenv("NERF_BWD_LIVE_GROUP"); const int v = e ? atoi(e) : 32; return (v == 8 || v == 16) ? v : 32; }();
    return g;
#else
    return 32;
#endif
}

}  // namespace nerf
