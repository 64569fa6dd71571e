// Gradient of the hash-grid encoding with respect to its POINTS, and through them to ray records (include/nerf_hip.h, section
// "hash-grid encoding"; hashgrid.HashEncoding.point_grad_reference and hashgrid.views_grad_reference are the definition).
//   per point and level   v_c  = sum_k d_x[p][l F + k] E[row_c][k]                        (k ascending)
//                         df_x = sum_c +-((w_y w_z) v_c), + where bit 0 of c is set       (c ascending; df_y: (w_x w_z), bit 1; df_z:
//                                                                                          (w_x w_y), bit 2)
//                         g_a += (df_a R) inv_extent[a], exactly 0 on an axis outside the box   (l ascending)
// A GATHER of the forward's rows: cell, weights and slots come from hash_device.h, so they cannot differ from the forward's.
//   hash_point_grad_kernel : lane = point, the levels walked inside the kernel in ascending order (l is wave-uniform: a wavefront
//                            gathers one level's rows at a time, the level's numbers are scalar loads from the kernel argument), so the
//                            sum over levels needs neither a second pass nor an atomic.  Writes [P][3]: d_points, or the workspace.
//   hash_fold_rays_kernel  : ray mode's second launch.  One wavefront per ray: lane takes samples lane, lane + 64, ... ascending, then a
//                            fixed xor butterfly -> d_rays[N][11] by nerf_field_input_grad's column contract (0:3 = sum g, 3:6 = sum z g,
//                            6:8 = 0, 8:11 = the view columns' adjoint applied ONCE to the column sums over the ray's samples).
// No atomics: two calls give the same bits.  Every index is clamped before an address is formed (locate), so a non-finite coordinate
// reads inside the table; only its own row of the output is affected.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hash_host.h"

using namespace nerf_api;
using namespace nerf_hash;

namespace {

constexpr int BLOCK = 256;
constexpr int FOLD_THREADS = 256;               // 4 waves = 4 rays per block
constexpr int FOLD_RAYS = FOLD_THREADS / 64;
constexpr int MAX_VIEW_FREQS = 16;

template <int F>
__global__ void __launch_bounds__(BLOCK) hash_point_grad_kernel(Levels lv, PointSrc src, long P, int L, const float* __restrict__ E,
                                                               const float* __restrict__ d_x, int ld, float* __restrict__ out) {
    const long p = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    float x[3];
    load_point(src, p, x);
    const unsigned outside = outside_axes(lv, x);
    const float* g = d_x + p * ld;
    float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int l = 0; l < L; ++l) {
        const Cell c = locate(lv, l, x);
        const long long off = lv.offset[l];
        float d[F];
#pragma unroll
        for (int k = 0; k < F; ++k) d[k] = g[l * F + k];
        float df[3];
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {
            float e[F];
            load_row<F>(E, off + corner_slot(lv, l, c, corner), e);
            float v = d[0] * e[0];
#pragma unroll
            for (int k = 1; k < F; ++k) v = v + d[k] * e[k];
            const float wx = (corner & 1) ? c.f[0] : 1.0f - c.f[0];
            const float wy = (corner & 2) ? c.f[1] : 1.0f - c.f[1];
            const float wz = (corner & 4) ? c.f[2] : 1.0f - c.f[2];
            const float t[3] = {(wy * wz) * v, (wx * wz) * v, (wx * wy) * v};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (corner == 0) df[a] = -t[a];
                else df[a] = ((corner >> a) & 1) ? df[a] + t[a] : df[a] - t[a];
            }
        }
        const float Rf = (float)lv.res[l];
#pragma unroll
        for (int a = 0; a < 3; ++a) acc[a] = acc[a] + (((outside >> a) & 1u) ? 0.0f : (df[a] * Rf) * lv.inv_extent[a]);
    }
    float* o = out + 3 * p;
    o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
}

__device__ __forceinline__ float wave_sum(float v) {
    // butterfly: every lane ends with the same sum, the order of the additions is fixed by the lane numbers alone
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ void __launch_bounds__(FOLD_THREADS) hash_fold_rays_kernel(const float* __restrict__ rays, int ray_stride, const float* __restrict__ z_vals,
                                                                     const float* __restrict__ g, const float* __restrict__ d_x, int ld,
                                                                     int views_col, int Lv, int n_rays, int S, float* __restrict__ d_rays,
                                                                     int accumulate) {
    const int ray = blockIdx.x * FOLD_RAYS + (threadIdx.x >> 6);
    if (ray >= n_rays) return;          // (whole waves leave: the shuffles below see full waves)
    const int lane = threadIdx.x & 63;
    const size_t base = (size_t)ray * S;
    float a[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = lane; j < S; j += 64) {
        const float z = z_vals[base + j];
        const float* gp = g + (base + j) * 3;
        const float gx = gp[0], gy = gp[1], gz = gp[2];
        a[0] += gx; a[1] += gy; a[2] += gz;
        a[3] += z * gx; a[4] += z * gy; a[5] += z * gz;      // (one product rounding each: -ffp-contract=off)
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) a[c] = wave_sum(a[c]);
    float v[3] = {0.0f, 0.0f, 0.0f};
    if (views_col >= 0) {       // the adjoint of [vd, sin 2^0 vd, cos 2^0 vd, ...] (nerf_build_inputs) on the column sums
        const float* vd = rays + (size_t)ray * ray_stride + (ray_stride - 3);
        const float* dv = d_x + views_col;
        float t[3] = {0.0f, 0.0f, 0.0f};
        for (int j = lane; j < S; j += 64) {
            const float* row = dv + (base + j) * ld;
            t[0] += row[0]; t[1] += row[1]; t[2] += row[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = wave_sum(t[c]);
#pragma unroll 1
        for (int k = 0; k < Lv; ++k) {
            float s[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            for (int j = lane; j < S; j += 64) {
                const float* row = dv + (base + j) * ld + 3 + 6 * k;
#pragma unroll
                for (int c = 0; c < 6; ++c) s[c] += row[c];
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) s[c] = wave_sum(s[c]);
            const float f = __int_as_float((127 + k) << 23);        // 2^k
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float sn, cs;
                sincosf(vd[c] * f, &sn, &cs);
                v[c] = v[c] + f * (s[c] * cs - s[3 + c] * sn);
            }
        }
    }
    if (lane == 0) {
        float* o = d_rays + (size_t)ray * 11;
        if (accumulate) {
#pragma unroll
            for (int c = 0; c < 6; ++c) o[c] += a[c];
            o[8] += v[0]; o[9] += v[1]; o[10] += v[2];
        } else {
#pragma unroll
            for (int c = 0; c < 6; ++c) o[c] = a[c];
            o[6] = 0.0f; o[7] = 0.0f;
            o[8] = v[0]; o[9] = v[1]; o[10] = v[2];
        }
    }
}

}  // namespace

extern "C" {

size_t nerf_hash_input_grad_workspace_floats(long n_points) { return n_points > 0 ? 3 * (size_t)n_points : 0; }

int nerf_hash_input_grad(const NerfHashGrid* grid, const float* embeddings, const float* points, const float* rays, int ray_stride,
                         const float* z_vals, int n_samples, long n_points, const float* d_x, int ld_d_x, int views_col, int multires_views,
                         float* d_points, float* d_rays, float* workspace, int accumulate, void* stream) {
    Levels lv;
    PointSrc src;
    if (check_grid(__func__, grid, &lv) || check_points(__func__, points, rays, ray_stride, z_vals, n_samples, n_points, &src)) return NERF_E_BADARG;
    const int L = grid->n_levels, F = grid->n_features;
    const bool ray_mode = points == nullptr;
    if (ld_d_x < L * F) return fail_arg(__func__, "ld_d_x < n_levels * n_features");
    if (views_col >= 0) {
        if (!ray_mode) return fail_arg(__func__, "views_col: the view columns belong to ray mode (points must be null)");
        if (multires_views < -1 || multires_views > MAX_VIEW_FREQS) return fail_arg(__func__, "multires_views must be -1 .. 16");
        const int width = multires_views < 0 ? 3 : 3 + 6 * multires_views;
        if (views_col < L * F || ld_d_x < views_col + width) return fail_arg(__func__, "the view columns must lie behind the encoding's, inside ld_d_x");
    }
    if (!ray_mode && accumulate) return fail_arg(__func__, "accumulate belongs to ray mode");
    if (n_points == 0) return 0;        // nothing is read or written
    if (!embeddings || !d_x) return fail_arg(__func__, "null pointer");
    if ((reinterpret_cast<uintptr_t>(embeddings) & (4 * F - 1)) != 0) return fail_arg(__func__, "embeddings must be aligned to a row (4 F bytes)");
    float* out;
    if (ray_mode) {
        if (!d_rays || !workspace) return fail_arg(__func__, "null pointer (ray mode needs d_rays and the workspace)");
        if (d_points) return fail_arg(__func__, "d_points belongs to point mode");
        if (views_col >= 0 && ray_stride < 11) return fail_arg(__func__, "view columns need ray records of 11 columns");
        out = workspace;
    } else {
        if (!d_points) return fail_arg(__func__, "null pointer");
        if (d_rays) return fail_arg(__func__, "d_rays belongs to ray mode");
        out = d_points;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 g((unsigned)((n_points + BLOCK - 1) / BLOCK)), b(BLOCK);
    if (F == 1) hipLaunchKernelGGL(hash_point_grad_kernel<1>, g, b, 0, st, lv, src, n_points, L, embeddings, d_x, ld_d_x, out);
    else if (F == 2) hipLaunchKernelGGL(hash_point_grad_kernel<2>, g, b, 0, st, lv, src, n_points, L, embeddings, d_x, ld_d_x, out);
    else hipLaunchKernelGGL(hash_point_grad_kernel<4>, g, b, 0, st, lv, src, n_points, L, embeddings, d_x, ld_d_x, out);
    if (ray_mode) {
        const long n_rays = n_points / n_samples;
        hipLaunchKernelGGL(hash_fold_rays_kernel, dim3((unsigned)((n_rays + FOLD_RAYS - 1) / FOLD_RAYS)), dim3(FOLD_THREADS), 0, st, rays, ray_stride,
                           z_vals, workspace, d_x, ld_d_x, views_col, multires_views < 0 ? 0 : multires_views, (int)n_rays, n_samples, d_rays,
                           accumulate);
    }
    return done(__func__, hipGetLastError());
}

}  // extern "C"
