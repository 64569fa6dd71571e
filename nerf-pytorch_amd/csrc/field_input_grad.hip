// Gradients of one field evaluation w.r.t. its INPUTS: the ray records (o, d, view direction) of a render_rays pass, or the points
// and view directions of query_points (S = 1, z = 0, d = 0).  Runs after the dgrad of the same evaluation and reads what exists at
// that point -- the deltas of layers 0 and 5 and of the view branch (dL/d pre-activation, DeltaLayout / DeltaLayout3), the launch's
// delta scale word (fp16 split), the live fp32 weights, z_vals and the rays -- and writes d_rays[n_rays][11]:
//   per point   g_exyz = W0^T d0 + W5[:, 0:63]^T d5 (63),  g_edir = Wv[:, 256:283]^T dv (27),
//               g_x = g_exyz[0:3] + sum_k 2^k (g_sin_k * cos(2^k x) - g_cos_k * sin(2^k x))      (x = o + z d)
//   per ray     d_o = sum_s g_x,  d_d = sum_s z_s g_x,  d_vd = the same chain applied once to sum_s g_edir,  near / far: 0
// (the compositing's |d| term of d_d comes from nerf_raw2outputs_bwd_geom).
//
// One wavefront per ray, lane = sample (s = lane, lane + 64, ...), per-lane sums in sample order, then a fixed xor butterfly: no
// float atomics, the result does not depend on scheduling.  S = 1 (point mode): one lane per point, no reduction.
// Products: the 16-bit delta words are exact fp16 / bf16 values, converted to fp32 and contracted with the fp32 weights by fmaf
// (fp32 products and accumulation: at least the class of the datapaths' parameter gradients); the fp16 split's power-of-two delta
// scale is removed exactly at the end.  The weights are wave-uniform (scalar loads, shared by the 64 lanes).
#include <hip/hip_runtime.h>
#include "nerf_common.h"
#include "launchers.h"
#include "api_util.h"

namespace nerf {

// d/dx of posenc (run_nerf_helpers.py:15-45) for one 3-vector: g(i) = dL/d[x, sin(2^0 x), cos(2^0 x), ..., sin(2^(L-1) x), cos(...)][i]
// sin / cos of the exact argument 2^k x (sincosf), no recurrence.  L_C > 0: the band count as a constant and g a register array -- the
// band loop stays rolled (one sincosf body, not L_C inlined copies: 256 VGPRs otherwise) and picks band k's six entries by selects, so
// g is never indexed at run time (which would put it in scratch); L_C = 0: `L` at run time, g reads memory.
template <int L_C, typename G>
__device__ __forceinline__ void posenc_bwd3(const float x[3], G g, int L, float out[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = g(c);
#pragma unroll 1
    for (int k = 0; k < (L_C > 0 ? L_C : L); ++k) {
        const float f = __int_as_float((127 + k) << 23);
        float gs[3], gc[3];
        if (L_C > 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                gs[c] = 0.0f; gc[c] = 0.0f;
#pragma unroll
                for (int kk = 0; kk < (L_C > 0 ? L_C : 1); ++kk)
                    if (kk == k) { gs[c] = g(3 + 6 * kk + c); gc[c] = g(3 + 6 * kk + 3 + c); }
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) { gs[c] = g(3 + 6 * k + c); gc[c] = g(3 + 6 * k + 3 + c); }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float sn, cs;
            sincosf(x[c] * f, &sn, &cs);
            out[c] += f * (gs[c] * cs - gc[c] * sn);
        }
    }
}

// KIND: DeltaKind (launchers.h) -- 0 fp32 point-major rows, 2 bf16 32-point tiles, 3 fp16 tiles (scaled), 4 fp16 hi + lo tiles (scaled)
template <int KIND>
struct DeltaRead {
    const float* base;
    size_t lo;          // words from a region to its lo mirror (KIND 4)
    __device__ __forceinline__ float operator()(size_t region, int F, size_t p, int f) const {
        if (KIND == 0) return base[region + p * F + f];
        const unsigned short* t = reinterpret_cast<const unsigned short*>(base + region);
        const size_t ix = tile_index(p, F, f);
        if (KIND == 2) return __uint_as_float((unsigned)t[ix] << 16);
        float v = (float)__builtin_bit_cast(_Float16, t[ix]);
        if (KIND == 4) v += (float)__builtin_bit_cast(_Float16, reinterpret_cast<const unsigned short*>(base + lo + region)[ix]);
        return v;
    }
};

template <int KIND, bool POINT>
__global__ __launch_bounds__(256) void field_input_grad_kernel(const float* __restrict__ params, const float* __restrict__ delta,
                                                               const float* __restrict__ rays, int ray_stride,
                                                               const float* __restrict__ z_vals, int n_rays, int S,
                                                               float* __restrict__ d_rays, int accumulate) {
    constexpr Canon cn = canon();
    const int lane = threadIdx.x & 63;
    const int ray = POINT ? (int)(blockIdx.x * blockDim.x + threadIdx.x) : (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (ray >= n_rays) return;
    const size_t P = (size_t)n_rays * S;
    size_t r0, r5, rv, lo = 0;
    float inv_s = 1.0f;
    if (KIND == 0) {
        const DeltaLayout dl = delta_layout(P);
        r0 = dl.h[0]; r5 = dl.h[SKIP + 1]; rv = dl.hv;
    } else {
        const DeltaLayout3 dl = delta_layout3(P, KIND == 4);
        r0 = dl.h[0]; r5 = dl.h[SKIP + 1]; rv = dl.hv; lo = dl.lo;
        if (KIND != 2) inv_s = __uint_as_float(delta_scale_bits(reinterpret_cast<const unsigned*>(delta + dl.scale)[0], true));
    }
    const DeltaRead<KIND> rd{delta, lo};
    const float* W0 = params + cn.w[0];
    const float* W5 = params + cn.w[SKIP + 1];
    const float* Wv = params + cn.wv + W;
    const float* rr = rays + (size_t)ray * ray_stride;
    const float o[3] = {rr[0], rr[1], rr[2]}, d[3] = {rr[3], rr[4], rr[5]};
    float so[3] = {0.f, 0.f, 0.f}, sd[3] = {0.f, 0.f, 0.f}, sv[IN_DIR];
#pragma unroll
    for (int j = 0; j < IN_DIR; ++j) sv[j] = 0.0f;
    for (int s = POINT ? 0 : lane; s < S; s += POINT ? 1 : 64) {
        const size_t p = (size_t)ray * S + s;
        float ge[IN_XYZ], gd[IN_DIR];
#pragma unroll
        for (int j = 0; j < IN_XYZ; ++j) ge[j] = 0.0f;
#pragma unroll
        for (int j = 0; j < IN_DIR; ++j) gd[j] = 0.0f;
        for (int i = 0; i < W; ++i) {
            const float d0 = rd(r0, W, p, i), d5 = rd(r5, W, p, i);
            const float* w0 = W0 + i * IN_XYZ;
            const float* w5 = W5 + i * (W + IN_XYZ);
#pragma unroll
            for (int j = 0; j < IN_XYZ; ++j) ge[j] = fmaf(w5[j], d5, fmaf(w0[j], d0, ge[j]));
        }
        for (int k = 0; k < WV; ++k) {
            const float dv = rd(rv, WV, p, k);
            const float* wv = Wv + k * (W + IN_DIR);
#pragma unroll
            for (int j = 0; j < IN_DIR; ++j) gd[j] = fmaf(wv[j], dv, gd[j]);
        }
#pragma unroll
        for (int j = 0; j < IN_XYZ; ++j) ge[j] *= inv_s;
        const float z = z_vals[p];
        float x[3], gx[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = o[c] + d[c] * z;           // the forward's sample point (run_nerf.py:381)
        posenc_bwd3<L_XYZ>(x, [&](int i) { return ge[i]; }, L_XYZ, gx);
#pragma unroll
        for (int c = 0; c < 3; ++c) { so[c] += gx[c]; sd[c] += z * gx[c]; }
#pragma unroll
        for (int j = 0; j < IN_DIR; ++j) sv[j] += gd[j];
    }
    if (!POINT) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) { so[c] += __shfl_xor(so[c], m); sd[c] += __shfl_xor(sd[c], m); }
        }
#pragma unroll
        for (int j = 0; j < IN_DIR; ++j) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) sv[j] += __shfl_xor(sv[j], m);
        }
        if (lane != 0) return;
    }
#pragma unroll
    for (int j = 0; j < IN_DIR; ++j) sv[j] *= inv_s;
    const float vd[3] = {rr[8], rr[9], rr[10]};
    float gv[3];
    posenc_bwd3<L_DIR>(vd, [&](int i) { return sv[i]; }, L_DIR, gv);
    float out[11] = {so[0], so[1], so[2], sd[0], sd[1], sd[2], 0.0f, 0.0f, gv[0], gv[1], gv[2]};
    float* dst = d_rays + (size_t)ray * 11;
#pragma unroll
    for (int c = 0; c < 11; ++c) dst[c] = accumulate ? dst[c] + out[c] : out[c];
}

hipError_t launch_field_input_grad(const float* params, const float* delta, DeltaKind kind, const float* rays, int ray_stride,
                                   const float* z_vals, int n_rays, int S, float* d_rays, int accumulate, hipStream_t stream) {
    if (n_rays <= 0) return hipSuccess;
    const bool pt = S == 1;
    const dim3 grid((unsigned)(pt ? (n_rays + 255) / 256 : (n_rays + 3) / 4)), block(256);
#define NERF_IG(K)                                                                                                             \
    if (pt) hipLaunchKernelGGL((field_input_grad_kernel<K, true>), grid, block, 0, stream, params, delta, rays, ray_stride, z_vals, \
                               n_rays, S, d_rays, accumulate);                                                                  \
    else hipLaunchKernelGGL((field_input_grad_kernel<K, false>), grid, block, 0, stream, params, delta, rays, ray_stride, z_vals,  \
                            n_rays, S, d_rays, accumulate);
    switch (kind) {
        case DELTA_ROWS_F32: NERF_IG(DELTA_ROWS_F32) break;
        case DELTA_TILE32_BF16: NERF_IG(DELTA_TILE32_BF16) break;
        case DELTA_TILE32_F16: NERF_IG(DELTA_TILE32_F16) break;
        case DELTA_TILE32_F16X2: NERF_IG(DELTA_TILE32_F16X2) break;
        default: return hipErrorInvalidValue;
    }
#undef NERF_IG
    return hipGetLastError();
}

// Embedder.embed's adjoint (the standalone encoding, ray_ops.hip embed_kernel): d_x[n][3] (+)= d/dx of out[n][3 + 6 L] . d_out
__global__ void embed_bwd_kernel(const float* __restrict__ x, long n_pts, int n_freqs, const float* __restrict__ d_out,
                                 float* __restrict__ d_x, int accumulate) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pts) return;
    const float xp[3] = {x[p * 3], x[p * 3 + 1], x[p * 3 + 2]};
    float g[3];
    const float* go = d_out + p * (3 + 6 * n_freqs);
    posenc_bwd3<0>(xp, [=](int i) { return go[i]; }, n_freqs, g);
#pragma unroll
    for (int c = 0; c < 3; ++c) d_x[p * 3 + c] = accumulate ? d_x[p * 3 + c] + g[c] : g[c];
}

hipError_t launch_embed_bwd(const float* x, long n_pts, int n_freqs, const float* d_out, float* d_x, int accumulate, hipStream_t stream) {
    if (n_pts <= 0) return hipSuccess;
    hipLaunchKernelGGL(embed_bwd_kernel, dim3((unsigned)((n_pts + 255) / 256)), dim3(256), 0, stream, x, n_pts, n_freqs, d_out, d_x,
                       accumulate);
    return hipGetLastError();
}

}  // namespace nerf

using namespace nerf_api;

extern "C" {

int nerf_field_input_grad(const float* params, const float* delta, const float* rays, int ray_stride, const float* z_vals,
                          int n_rays, int n_samples, float* d_rays, int accumulate, void* stream) {
    REQUIRE(params && delta && rays && z_vals && d_rays, "null pointer");
    REQUIRE(n_rays >= 0 && n_samples >= 1, "bad size");
    REQUIRE(ray_stride >= 11, "rays must carry view directions (ray_stride >= 11)");
    BufTag t;
    REQUIRE(tag_lookup(delta, &t) && t.is_delta, "delta is not a buffer this library's dgrad wrote (no layout record)");
    REQUIRE(t.n_rays == n_rays && t.n_samples == n_samples, "delta buffer was written for another ray / sample count");
    return done(__func__, nerf::launch_field_input_grad(params, delta, nerf::desc(t.dp).delta, rays, ray_stride, z_vals, n_rays, n_samples, d_rays,
                                                        accumulate, (hipStream_t)stream));
}

int nerf_raw2outputs_bwd_geom(const float* raw, const float* z_vals, const float* rays_d, int dir_stride, int n_rays,
                              int n_samples, const float* noise, float raw_noise_std, int white_bkgd,
                              const float* d_rgb, const float* d_acc, const float* d_disp, const float* d_weights,
                              const float* d_depth, float* d_raw, float* d_rays_d, float* d_z_vals, void* stream) {
    REQUIRE(raw && z_vals && rays_d && d_rgb && d_raw, "null pointer");
    REQUIRE(d_rays_d || d_z_vals, "null pointer (d_rays_d and d_z_vals both NULL: use nerf_raw2outputs_bwd)");
    REQUIRE(dir_stride >= 3 && n_rays >= 0 && n_samples >= 1 && n_samples <= 4096, "bad size");
    REQUIRE(!(raw_noise_std > 0.0f) || noise, "raw_noise_std > 0 needs noise draws");
    nerf::CompositeArgs a{raw, z_vals, rays_d, raw_noise_std > 0.0f ? noise : nullptr, raw_noise_std,
                          dir_stride, n_rays, n_samples, white_bkgd,
                          nullptr, nullptr, nullptr, nullptr, nullptr, d_rgb, d_acc, d_disp, d_raw, d_weights, d_depth,
                          d_rays_d, d_z_vals};
    return done(__func__, nerf::launch_composite(a, true, (hipStream_t)stream));
}

int nerf_embed_bwd(const float* x, long n_pts, int n_freqs, const float* d_out, float* d_x, int accumulate, void* stream) {
    REQUIRE(x && d_out && d_x, "null pointer");
    REQUIRE(n_pts >= 0 && n_freqs >= 0 && n_freqs <= 30, "bad size");
    return done(__func__, nerf::launch_embed_bwd(x, n_pts, n_freqs, d_out, d_x, accumulate, (hipStream_t)stream));
}

}  // extern "C"
