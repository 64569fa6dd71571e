// Multiresolution hash-grid encoding (include/nerf_hip.h, section "hash-grid encoding"; hashgrid.HashEncoding; DESIGN.md 3.27;
// hashgrid.HashEncoding.encode_reference / table_grad_reference are the definition).
//   nerf_hash_encode_fwd : out[p][l F + k] = sum_c w_c E[off_l + slot_c][k], a GATHER.  Lane = point, level = blockIdx.y: a wavefront
//                          reads one level's rows.  Writes a column range of a wider row-major matrix (leading dimension ld_out).
//   nerf_hash_encode_bwd : d_E from d_out, a SCATTER-ADD -- the one the project has.  Made order-independent by adding 64-bit INTEGERS:
//                          pass 1  M = max |d_out| (an integer atomic max of the fp32 bit patterns: |x| orders like its bits, and
//                                  every NaN sorts above +inf),
//                          pass 2  k = llrint((double)(w_c g) 2^q) added to scratch[row][k] with a 64-bit integer atomic add,
//                                  q = 61 - e - ceil(log2 P), M = m 2^e,
//                          pass 3  d_E = (float)((double)acc 2^-q); the scratch is left zero.
//                          Integer addition is associative, so the bits do not depend on the order the adds arrive in.
// The level tables (resolution, first row, dense or hashed) come from the host (NerfHashGrid): no powf on the device.  Every index is
// clamped before an address is formed, so a non-finite coordinate reads and adds inside the table.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hash_host.h"

using namespace nerf_api;
using namespace nerf_hash;

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_BLOCKS_MAX = 1024;

template <int F>
__global__ void __launch_bounds__(BLOCK) hash_fwd_kernel(Levels lv, PointSrc src, long P, const float* __restrict__ E,
                                                        float* __restrict__ out, int ld_out) {
    const long p = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    const int l = blockIdx.y;
    float x[3];
    load_point(src, p, x);
    Cell c = locate(lv, l, x);
    const long long off = lv.offset[l];
    float acc[F];
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
        const float w = corner_weight(c, corner);
        float v[F];
        load_row<F>(E, off + corner_slot(lv, l, c, corner), v);
#pragma unroll
        for (int k = 0; k < F; ++k) acc[k] = corner == 0 ? w * v[k] : acc[k] + w * v[k];
    }
    float* o = out + p * ld_out + l * F;
#pragma unroll
    for (int k = 0; k < F; ++k) o[k] = acc[k];
}

// pass 1: state[0] = max over the bit patterns of |d_out| (state[0] is zero on entry)
__global__ void __launch_bounds__(BLOCK) hash_absmax_kernel(const float* __restrict__ d_out, int ld, int cols, long n, unsigned* __restrict__ state) {
    unsigned m = 0;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) {
        const long r = i / cols;
        m = max(m, __float_as_uint(d_out[r * ld + (i - r * cols)]) & 0x7fffffffu);
    }
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, d));
    if ((threadIdx.x & 63) == 0 && m != 0) atomicMax(state, m);
}

// pass 2: lane = point, level = blockIdx.y
template <int F>
__global__ void __launch_bounds__(BLOCK) hash_scatter_kernel(Levels lv, PointSrc src, long P, int log2_P, const float* __restrict__ d_out, int ld,
                                                            const unsigned* __restrict__ state, unsigned long long* __restrict__ acc) {
    const long p = (long)blockIdx.x * BLOCK + threadIdx.x;
    const unsigned mbits = state[0];
    if (p >= P || mbits == 0 || mbits >= 0x7f800000u) return;        // nothing to add / the finishing pass writes NaN
    const double scale = exp2_double(grad_exponent(mbits, log2_P));
    const int l = blockIdx.y;
    float x[3];
    load_point(src, p, x);
    Cell c = locate(lv, l, x);
    const long long off = lv.offset[l];
    float g[F];
#pragma unroll
    for (int k = 0; k < F; ++k) g[k] = d_out[p * ld + l * F + k];
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
        const float w = corner_weight(c, corner);
        unsigned long long* row = acc + (off + corner_slot(lv, l, c, corner)) * F;
#pragma unroll
        for (int k = 0; k < F; ++k) {
            const float t = w * g[k];
            const long long q = __double2ll_rn((double)t * scale);
            if (q != 0) atomicAdd(row + k, (unsigned long long)q);      // (two's complement: an unsigned add of the same bits)
        }
    }
}

// pass 3: one lane per element of the table; leaves the accumulator zero
__global__ void __launch_bounds__(BLOCK) hash_finish_kernel(long long n, int log2_P, const unsigned* __restrict__ state, long long* __restrict__ acc,
                                                           float* __restrict__ d_emb) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const unsigned mbits = state[0];
    float r;
    if (mbits >= 0x7f800000u) r = __uint_as_float(0x7fc00000u);
    else if (mbits == 0) r = 0.0f;
    else r = (float)((double)acc[i] * exp2_double(-grad_exponent(mbits, log2_P)));
    acc[i] = 0;
    d_emb[i] = r;
}

int ceil_log2(long P) {
    int b = 0;
    while ((1l << b) < P) ++b;
    return b;
}

}  // namespace

extern "C" {

size_t nerf_hash_scratch_words(const NerfHashGrid* grid) {
    Levels lv;
    if (check_grid(__func__, grid, &lv)) return 0;
    return (size_t)grid->level_offset[grid->n_levels] * (size_t)grid->n_features + 1;
}

int nerf_hash_encode_fwd(const NerfHashGrid* grid, const float* embeddings, const float* points, const float* rays, int ray_stride,
                         const float* z_vals, int n_samples, long n_points, float* out, int ld_out, void* stream) {
    Levels lv;
    PointSrc src;
    if (check_grid(__func__, grid, &lv) || check_points(__func__, points, rays, ray_stride, z_vals, n_samples, n_points, &src)) return NERF_E_BADARG;
    const int L = grid->n_levels, F = grid->n_features;
    if (ld_out < L * F) return fail_arg(__func__, "ld_out < n_levels * n_features");
    if (n_points == 0) return 0;        // nothing is read or written
    if (!embeddings || !out) return fail_arg(__func__, "null pointer");
    if ((reinterpret_cast<uintptr_t>(embeddings) & (4 * F - 1)) != 0) return fail_arg(__func__, "embeddings must be aligned to a row (4 F bytes)");
    const dim3 g((unsigned)((n_points + BLOCK - 1) / BLOCK), (unsigned)L), b(BLOCK);
    hipStream_t st = (hipStream_t)stream;
    if (F == 1) hipLaunchKernelGGL(hash_fwd_kernel<1>, g, b, 0, st, lv, src, n_points, embeddings, out, ld_out);
    else if (F == 2) hipLaunchKernelGGL(hash_fwd_kernel<2>, g, b, 0, st, lv, src, n_points, embeddings, out, ld_out);
    else hipLaunchKernelGGL(hash_fwd_kernel<4>, g, b, 0, st, lv, src, n_points, embeddings, out, ld_out);
    return done(__func__, hipGetLastError());
}

int nerf_hash_encode_bwd(const NerfHashGrid* grid, const float* points, const float* rays, int ray_stride, const float* z_vals, int n_samples,
                         long n_points, const float* d_out, int ld_d_out, long long* scratch, float* d_embeddings, int phases, void* stream) {
    Levels lv;
    PointSrc src;
    if (check_grid(__func__, grid, &lv) || check_points(__func__, points, rays, ray_stride, z_vals, n_samples, n_points, &src)) return NERF_E_BADARG;
    const int L = grid->n_levels, F = grid->n_features;
    if (ld_d_out < L * F) return fail_arg(__func__, "ld_d_out < n_levels * n_features");
    if (phases < 1 || phases > 3) return fail_arg(__func__, "phases: 1 scatter, 2 finish, 3 both");
    if (!scratch || ((phases & 2) && !d_embeddings)) return fail_arg(__func__, "null pointer");
    if ((reinterpret_cast<uintptr_t>(scratch) & 7) != 0) return fail_arg(__func__, "scratch must be 8-byte aligned");
    if (n_points > 0 && (phases & 1) && !d_out) return fail_arg(__func__, "null pointer");
    const long long n_acc = grid->level_offset[L] * (long long)F;
    unsigned* state = reinterpret_cast<unsigned*>(scratch + n_acc);      // the word behind the accumulator: bits of max |d_out|
    const int log2_P = ceil_log2(n_points < 1 ? 1 : n_points);
    hipStream_t st = (hipStream_t)stream;
    if (phases & 1) {
        hipError_t e = hipMemsetAsync(state, 0, 8, st);
        if (e != hipSuccess) return done(__func__, e);
        if (n_points > 0) {
            const long n = n_points * (long)(L * F);
            long nb = (n + BLOCK - 1) / BLOCK;
            if (nb > MAX_BLOCKS_MAX) nb = MAX_BLOCKS_MAX;
            hipLaunchKernelGGL(hash_absmax_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, st, d_out, ld_d_out, L * F, n, state);
            const dim3 g((unsigned)((n_points + BLOCK - 1) / BLOCK), (unsigned)L), b(BLOCK);
            unsigned long long* acc = reinterpret_cast<unsigned long long*>(scratch);
            if (F == 1) hipLaunchKernelGGL(hash_scatter_kernel<1>, g, b, 0, st, lv, src, n_points, log2_P, d_out, ld_d_out, state, acc);
            else if (F == 2) hipLaunchKernelGGL(hash_scatter_kernel<2>, g, b, 0, st, lv, src, n_points, log2_P, d_out, ld_d_out, state, acc);
            else hipLaunchKernelGGL(hash_scatter_kernel<4>, g, b, 0, st, lv, src, n_points, log2_P, d_out, ld_d_out, state, acc);
        }
    }
    if (phases & 2)
        hipLaunchKernelGGL(hash_finish_kernel, dim3((unsigned)((n_acc + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, n_acc, log2_P, state, scratch,
                           d_embeddings);
    return done(__func__, hipGetLastError());
}

}  // extern "C"
