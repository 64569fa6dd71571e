// Device side of the multiresolution hash-grid encoding (hash_encode.hip): the level tables as a kernel argument, a
// point's cell and weights on one level, a corner's row, and the exponent of the fixed-point table gradient.  The forward and the
// backward share every function here, so the two cannot disagree on a slot or a weight.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/nerf_hip.h"

namespace nerf_hash {

// what the kernels read of a NerfHashGrid (by value: level-uniform scalar loads)
struct Levels {
    int res[NERF_HASH_MAX_LEVELS];
    long long offset[NERF_HASH_MAX_LEVELS];
    unsigned dense_mask;        // bit l: level l is a dense lattice
    unsigned hash_mask;         // T - 1
    float lo[3], inv_extent[3];
};

// the points: [P][3], or o + d z of ray records and their depths (separate multiply and add, as nerf_build_inputs)
struct PointSrc {
    const float* points;
    const float* rays;
    const float* z;
    int ray_stride, n_samples;
};

__device__ inline void load_point(const PointSrc& s, long p, float (&x)[3]) {
    if (s.points) {
        x[0] = s.points[3 * p]; x[1] = s.points[3 * p + 1]; x[2] = s.points[3 * p + 2];
    } else {
        const float* rp = s.rays + (p / s.n_samples) * s.ray_stride;
        const float zz = s.z[p];
        x[0] = rp[0] + rp[3] * zz; x[1] = rp[1] + rp[4] * zz; x[2] = rp[2] + rp[5] * zz;
    }
}

struct Cell { int i[3]; float f[3]; };

// u = clamp((x - lo) inv_extent, 0, 1), p = u R, i = min(floor(p), R - 1), f = p - i.  fmaxf / fminf drop a NaN, and the index is
// clamped from below as well: no coordinate forms an address outside the level.
__device__ inline Cell locate(const Levels& lv, int l, const float (&x)[3]) {
    Cell c;
    const int R = lv.res[l];
    const float Rf = (float)R;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float u = fminf(fmaxf((x[a] - lv.lo[a]) * lv.inv_extent[a], 0.0f), 1.0f);
        const float p = u * Rf;
        const int i = max(min((int)floorf(p), R - 1), 0);
        c.i[a] = i;
        c.f[a] = p - (float)i;
    }
    return c;
}

// bit a: axis a of x lies outside the box, t = (x - lo) inv_extent < 0 or > 1 with locate's own t (before its clamp): there the
// encoding does not depend on that coordinate.  A NaN compares false: not outside.
__device__ inline unsigned outside_axes(const Levels& lv, const float (&x)[3]) {
    unsigned m = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float t = (x[a] - lv.lo[a]) * lv.inv_extent[a];
        m |= (t < 0.0f || t > 1.0f) ? 1u << a : 0u;
    }
    return m;
}

// corner: bit 0 x, bit 1 y, bit 2 z;  w = (wx wy) wz
__device__ inline float corner_weight(const Cell& c, int corner) {
    const float wx = (corner & 1) ? c.f[0] : 1.0f - c.f[0];
    const float wy = (corner & 2) ? c.f[1] : 1.0f - c.f[1];
    const float wz = (corner & 4) ? c.f[2] : 1.0f - c.f[2];
    return (wx * wy) * wz;
}

// the corner's row within its level: the lattice index of a dense level, the hash of a hashed one (wrapping uint32 arithmetic)
__device__ inline unsigned corner_slot(const Levels& lv, int l, const Cell& c, int corner) {
    const unsigned ix = (unsigned)c.i[0] + (corner & 1), iy = (unsigned)c.i[1] + ((corner >> 1) & 1), iz = (unsigned)c.i[2] + ((corner >> 2) & 1);
    if ((lv.dense_mask >> l) & 1u) {
        const unsigned n = (unsigned)lv.res[l] + 1u;
        return ix + iy * n + iz * n * n;
    }
    return (ix ^ (iy * 2654435761u) ^ (iz * 805459861u)) & lv.hash_mask;
}

// one row of the table: F floats in one 4 F byte load
template <int F> struct RowT;
template <> struct RowT<1> { using type = float; };
template <> struct RowT<2> { using type = float2; };
template <> struct RowT<4> { using type = float4; };
template <int F> __device__ inline void load_row(const float* __restrict__ E, long long row, float (&v)[F]) {
    const typename RowT<F>::type r = reinterpret_cast<const typename RowT<F>::type*>(E)[row];       // one 4 F byte load (rows are aligned)
    const float* rf = reinterpret_cast<const float*>(&r);
#pragma unroll
    for (int k = 0; k < F; ++k) v[k] = rf[k];
}

// q = 61 - e - ceil(log2 P) with M = m 2^e, 0.5 <= m < 1 (frexp), from the bit pattern of a finite M > 0
__device__ inline int grad_exponent(unsigned mbits, int log2_P) {
    int e;
    frexpf(__uint_as_float(mbits), &e);
    return 61 - e - log2_P;
}

// 2^q as a double, -1022 <= q <= 1023 (|q| stays below 300 here)
__device__ inline double exp2_double(int q) { return __longlong_as_double((long long)(1023 + q) << 52); }

}  // namespace nerf_hash
