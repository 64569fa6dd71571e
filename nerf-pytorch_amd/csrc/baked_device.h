// What the kernels that walk a baked field share (baked.hip: nerf_baked_render; baked_train.hip: nerf_baked_count and
// nerf_baked_train_fwd): the row layout, the ray's set-up, the classification of candidate k and the arithmetic of one kept sample --
// one copy, so the training forward renders the bits of the inference render and the count walks the render's kept set.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "grid_device.h"
#include "ray_device.h"

namespace nerf_baked {

using nerf_grid::GridArgs;
using nerf_grid::Pt;

constexpr int BAKED_THREADS = 256;
constexpr int BAKED_RAYS = BAKED_THREADS / 64;

typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));

// B = (DEG + 1)^2 basis functions; a row is sigma, then B coefficients per colour channel, zero-padded to W halves
template <int DEG> struct RowOf {
    static constexpr int B = (DEG + 1) * (DEG + 1);
    static constexpr int V = 1 + 3 * B;                 // values used
    static constexpr int W = DEG == 0 ? 4 : (DEG == 1 ? 16 : 32);
};

// acc[0 .. V) += w * row[0 .. V): one product, one addition per value (no contraction)
template <int DEG>
__device__ __forceinline__ void add_row(const _Float16* __restrict__ row, float w, float* acc) {
    constexpr int V = RowOf<DEG>::V;
    if (DEG == 0) {
        const half4_t h = *reinterpret_cast<const half4_t*>(row);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = acc[j] + w * (float)h[j];
    } else {
#pragma unroll
        for (int q = 0; q < RowOf<DEG>::W / 8; ++q) {
            const half8_t h = *reinterpret_cast<const half8_t*>(row + 8 * q);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (8 * q + j < V) acc[8 * q + j] = acc[8 * q + j] + w * (float)h[j];
        }
    }
}

// The real spherical harmonics of degree <= DEG at (x, y, z), in the order and with the signs of baked.sh_basis
template <int DEG>
__device__ __forceinline__ void sh_basis(float x, float y, float z, float* Y) {
    Y[0] = 0.28209479177387814f;
    if (DEG >= 1) {
        Y[1] = -0.4886025119029199f * y;
        Y[2] = 0.4886025119029199f * z;
        Y[3] = -0.4886025119029199f * x;
    }
    if (DEG >= 2) {
        const float xx = x * x, yy = y * y, zz = z * z;
        Y[4] = 1.0925484305920792f * (x * y);
        Y[5] = -1.0925484305920792f * (y * z);
        Y[6] = 0.31539156525252005f * (2.0f * zz - xx - yy);
        Y[7] = -1.0925484305920792f * (x * z);
        Y[8] = 0.5462742152960396f * (xx - yy);
    }
}

// The ray of a wave: o and d in scalar registers (the wave has one ray), near, far and the depth of a step; false: an invalid ray
struct RaySetup { float r[6], near, far, dz; };
__device__ __forceinline__ bool ray_setup(const float* __restrict__ ray_in, float ds, RaySetup* s) {
    s->near = ray_in[6]; s->far = ray_in[7];
    bool ok = s->near < s->far;
#pragma unroll
    for (int c = 0; c < 8; ++c) ok = ok && fabsf(ray_in[c]) < INFINITY;     // (a NaN fails the comparison)
#pragma unroll
    for (int c = 0; c < 6; ++c) s->r[c] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ray_in[c])));
    s->dz = ds / nerf_grid::dir_norm(s->r);                 // (IEEE division: hipcc's default for fp32)
    return ok && s->dz > 0.0f && s->dz < INFINITY;          // (d = 0, an overflowing |d|, a NaN: no step)
}

// Candidate k of a ray: its depth, whether it is valid (k < M and z < far), and -- keep -- whether it is valid, inside the box and in
// an occupied cell; then (ix, iy, iz) is its cell and (tx, ty, tz) its grid coordinates
struct Candidate { float z, tx, ty, tz; int ix, iy, iz; bool valid, keep; };
__device__ __forceinline__ Candidate candidate(const GridArgs& g, const RaySetup& s, float uu, int k, int M) {
    Candidate c;
    c.z = s.near + ((float)k + uu) * s.dz;                  // (no contraction)
    c.valid = k < M && c.z < s.far;                         // (a NaN fails the comparison)
    const Pt p = nerf_grid::sample_point(s.r, c.z);
    const bool inside = nerf_grid::grid_coords(g, p, &c.tx, &c.ty, &c.tz);
    c.keep = false;
    c.ix = c.iy = c.iz = 0;
    if (c.valid && inside) {
        c.ix = (int)floorf(c.tx); c.iy = (int)floorf(c.ty); c.iz = (int)floorf(c.tz);
        c.keep = nerf_grid::cell_bit(g, nerf_grid::cell_index(g, c.ix, c.iy, c.iz));
    }
    return c;
}

// A kept sample: the blend of the eight corner rows of its cell in corner order 000 001 .. 111 with the weights (wx wy) wz, sigma
// clamped at 0 behind the blend, the colours of the blended coefficients in the ray's basis Y, alpha and the step's transmittance
struct Sample { float fx, fy, fz, v0, e, alpha, t1, c0, c1, c2; };
template <int DEG>
__device__ __forceinline__ Sample sample_value(const int* __restrict__ node_index, const _Float16* __restrict__ table, unsigned n_rows, int ny,
                                               int nz, const Candidate& c, const float* Y, float ds) {
    constexpr int B = RowOf<DEG>::B, V = RowOf<DEG>::V, W = RowOf<DEG>::W;
    Sample s;
    s.fx = c.tx - floorf(c.tx); s.fy = c.ty - floorf(c.ty); s.fz = c.tz - floorf(c.tz);     // (exact)
    const float wx[2] = {1.0f - s.fx, s.fx}, wy[2] = {1.0f - s.fy, s.fy}, wz[2] = {1.0f - s.fz, s.fz};
    const unsigned n0 = ((unsigned)c.ix * (unsigned)ny + (unsigned)c.iy) * (unsigned)nz + (unsigned)c.iz;
    unsigned row[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const unsigned n = n0 + ((unsigned)((q >> 2) & 1) * (unsigned)ny + (unsigned)((q >> 1) & 1)) * (unsigned)nz + (unsigned)(q & 1);
        const unsigned i = (unsigned)node_index[n];
        row[q] = i < n_rows ? i : 0u;
    }
    float v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = 0.0f;
#pragma unroll
    for (int q = 0; q < 8; ++q)
        add_row<DEG>(table + (size_t)row[q] * W, wx[(q >> 2) & 1] * wy[(q >> 1) & 1] * wz[q & 1], v);
    const float sg = fmaxf(v[0], 0.0f);
    float l0 = 0.0f, l1 = 0.0f, l2 = 0.0f;
#pragma unroll
    for (int b = 0; b < B; ++b) {
        l0 = l0 + v[1 + b] * Y[b];
        l1 = l1 + v[1 + B + b] * Y[b];
        l2 = l2 + v[1 + 2 * B + b] * Y[b];
    }
    s.v0 = v[0];
    s.c0 = nerf::sigmoidf_(l0); s.c1 = nerf::sigmoidf_(l1); s.c2 = nerf::sigmoidf_(l2);
    s.e = expf(-sg * ds);
    s.alpha = 1.0f - s.e;
    s.t1 = 1.0f - s.alpha + 1e-10f;
    return s;
}

// One round of 64 candidates added to the ray's integrals: the wave scans 1 - alpha + 1e-10 (1 in lanes that keep nothing), the exclusive
// value times the carried T is the lane's transmittance -- returned --, five butterfly sums add the round and lane 63's inclusive value
// carries T on
struct RayIntegrals { float T = 1.0f, r = 0.0f, g = 0.0f, b = 0.0f, acc = 0.0f, depth = 0.0f; };
__device__ __forceinline__ float composite_round(RayIntegrals& A, float alpha, float t1, float c0, float c1, float c2, bool keep, float z, int lane) {
    const float incl = nerf::wave_incl_scan_mul(t1, lane);
    float excl = __shfl_up(incl, 1);
    if (lane == 0) excl = 1.0f;
    const float T = A.T * excl;
    const float w = alpha * T;
    A.r = A.r + nerf::wave_sum(w * c0);
    A.g = A.g + nerf::wave_sum(w * c1);
    A.b = A.b + nerf::wave_sum(w * c2);
    A.acc = A.acc + nerf::wave_sum(w);
    A.depth = A.depth + nerf::wave_sum(keep ? w * z : 0.0f);     // (a candidate that is not kept may lie at inf)
    A.T = A.T * __shfl(incl, 63);
    return T;
}

}  // namespace nerf_baked
