// Rendering a baked field: no network, the grid itself holds density and colour (include/nerf_hip.h, section "baked field").
//   nerf_baked_render : per ray the world-space march of nerf_occ_march_step's level 0 over an occupancy grid, and at every kept candidate
//                       the trilinear blend of the eight lattice nodes of its cell -- one fp16 row per stored node: sigma and the
//                       spherical-harmonic coefficients of the colour logits --, composited on the spot: BakedField.render_rays
//                       (nerf-pytorch_amd/baked.py; BakedField.render_rays_reference is the definition).
// One wavefront per ray, BAKED_RAYS rays per block, the walk of occ_march_walk_kernel<WorldSteps, false> (occupancy.hip): a round takes 64
// candidates, lane l builds z_k of k = k0 + l with the march's expression and classifies it with the march's functions (grid_device.h),
// so the kept candidates are the reference's bit for bit.  A round whose keep ballot is empty ends there.  In a round that keeps
// something, a kept lane loads the eight node indices of its cell and gathers the eight rows (16-byte loads; 8 bytes at degree 0),
// blends them in fp32 in corner order 000 001 .. 111 (x the slowest bit) with weights (wx wy) wz, clamps sigma at 0 behind the blend,
// and turns the blended coefficients into colours with the ray's SH basis (evaluated once, in front of the loop) and the colour head's
// sigmoid.  alpha = 1 - expf(-sigma ds); the wave scans 1 - alpha + 1e-10 (1 in lanes that keep nothing: composite_ray's expression),
// the exclusive value times the carried T is the lane's transmittance, five butterfly sums add the round to the ray's integrals and
// lane 63's inclusive value carries T on.  The walk ends at the first round whose first candidate is not valid (the valid candidates
// are a prefix), at max_steps, or -- stop_eps > 0 -- behind the first round at whose end T < stop_eps.
// Everything the wave branches on is wave-uniform (ballots, the round, T after the scan); no atomics, no LDS: the same inputs give the
// same bits.  A node index outside the table reads row 0 (zeros) instead of memory it does not own.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "api_util.h"
#include "grid_device.h"
#include "ray_device.h"

using namespace nerf_api;
using namespace nerf_grid;

namespace {

constexpr int BAKED_THREADS = 256;
constexpr int BAKED_RAYS = BAKED_THREADS / 64;
constexpr int BAKED_STOPPED = 1 << 30;          // the flag in n_samples (include/nerf_hip.h)

typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));

struct BakedArgs {
    const int* node_index;
    const _Float16* table;
    unsigned n_rows;
    const float* rays;
    int ray_stride;
    const float* u;             // one offset per ray, or null: 0.5
    int n_rays;
    float ds;
    int M;
    float stop_eps;
    int white_bkgd;
    float* rgb;
    float* disp;
    float* acc;
    float* depth;
    int* n_samples;
};

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

template <int DEG>
__global__ __launch_bounds__(BAKED_THREADS) void baked_render_kernel(GridArgs g, BakedArgs a) {
    constexpr int B = RowOf<DEG>::B, V = RowOf<DEG>::V, W = RowOf<DEG>::W;
    const int ray = blockIdx.x * BAKED_RAYS + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;        // (whole waves leave: the ballots and shuffles below see full waves)
    const int lane = threadIdx.x & 63;
    const float* ray_in = a.rays + (size_t)ray * a.ray_stride;
    const float near = ray_in[6], far = ray_in[7];
    bool ok = near < far;
#pragma unroll
    for (int c = 0; c < 8; ++c) ok = ok && fabsf(ray_in[c]) < INFINITY;     // (a NaN fails the comparison)
    // o and d in scalar registers: the wave has one ray
    float r[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) r[c] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ray_in[c])));
    const float dz = a.ds / dir_norm(r);                    // (IEEE division: hipcc's default for fp32)
    ok = ok && dz > 0.0f && dz < INFINITY;                  // (d = 0, an overflowing |d|, a NaN: no step)
    float Y[B];
    sh_basis<DEG>(ray_in[8], ray_in[9], ray_in[10], Y);
    float T = 1.0f, s_r = 0.0f, s_g = 0.0f, s_b = 0.0f, s_acc = 0.0f, s_depth = 0.0f;
    int count = 0, stopped = 0;
    if (ok) {
        const float uu = a.u ? a.u[ray] : 0.5f;
        const int ny = g.res[1] + 1, nz = g.res[2] + 1;     // nodes per axis
        for (int k0 = 0; k0 < a.M; k0 += 64) {
            const int k = k0 + lane;
            const float z = near + ((float)k + uu) * dz;    // (no contraction)
            const bool valid = k < a.M && z < far;          // (a NaN fails the comparison)
            const unsigned long long vm = __ballot(valid);
            if (!(vm & 1ull)) break;
            const Pt p = sample_point(r, z);
            float tx, ty, tz;
            const bool inside = grid_coords(g, p, &tx, &ty, &tz);
            bool keep = false;
            int ix = 0, iy = 0, iz = 0;
            if (valid && inside) {
                ix = (int)floorf(tx); iy = (int)floorf(ty); iz = (int)floorf(tz);
                keep = cell_bit(g, cell_index(g, ix, iy, iz));
            }
            const unsigned long long km = __ballot(keep);
            if (km) {
                float alpha = 0.0f, t1 = 1.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
                if (keep) {
                    const float fx = tx - floorf(tx), fy = ty - floorf(ty), fz = tz - floorf(tz);     // (exact)
                    const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy}, wz[2] = {1.0f - fz, fz};
                    const unsigned n0 = ((unsigned)ix * (unsigned)ny + (unsigned)iy) * (unsigned)nz + (unsigned)iz;
                    unsigned row[8];
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const unsigned n = n0 + ((unsigned)((c >> 2) & 1) * (unsigned)ny + (unsigned)((c >> 1) & 1)) * (unsigned)nz + (unsigned)(c & 1);
                        const unsigned i = (unsigned)a.node_index[n];
                        row[c] = i < a.n_rows ? i : 0u;
                    }
                    float v[V];
#pragma unroll
                    for (int j = 0; j < V; ++j) v[j] = 0.0f;
#pragma unroll
                    for (int c = 0; c < 8; ++c)
                        add_row<DEG>(a.table + (size_t)row[c] * W, wx[(c >> 2) & 1] * wy[(c >> 1) & 1] * wz[c & 1], v);
                    const float sg = fmaxf(v[0], 0.0f);
                    float l0 = 0.0f, l1 = 0.0f, l2 = 0.0f;
#pragma unroll
                    for (int b = 0; b < B; ++b) {
                        l0 = l0 + v[1 + b] * Y[b];
                        l1 = l1 + v[1 + B + b] * Y[b];
                        l2 = l2 + v[1 + 2 * B + b] * Y[b];
                    }
                    c0 = nerf::sigmoidf_(l0); c1 = nerf::sigmoidf_(l1); c2 = nerf::sigmoidf_(l2);
                    alpha = 1.0f - expf(-sg * a.ds);
                    t1 = 1.0f - alpha + 1e-10f;
                }
                const float incl = nerf::wave_incl_scan_mul(t1, lane);
                float excl = __shfl_up(incl, 1);
                if (lane == 0) excl = 1.0f;
                const float w = alpha * (T * excl);
                s_r = s_r + nerf::wave_sum(w * c0);
                s_g = s_g + nerf::wave_sum(w * c1);
                s_b = s_b + nerf::wave_sum(w * c2);
                s_acc = s_acc + nerf::wave_sum(w);
                s_depth = s_depth + nerf::wave_sum(keep ? w * z : 0.0f);     // (a candidate that is not kept may lie at inf)
                T = T * __shfl(incl, 63);
                count += __popcll(km);
                if (T < a.stop_eps) {           // (stop_eps = 0: never)
                    stopped = 1;
                    break;
                }
            }
            if (!((vm >> 63) & 1ull)) break;    // the valid candidates are a prefix: this round was the last
        }
    }
    if (lane == 0) {
        const float bg = a.white_bkgd ? 1.0f - s_acc : 0.0f;
        a.rgb[(size_t)ray * 3] = s_r + bg; a.rgb[(size_t)ray * 3 + 1] = s_g + bg; a.rgb[(size_t)ray * 3 + 2] = s_b + bg;
        const float ratio = s_depth / s_acc;
        // torch.max(1e-10, ratio) propagates NaN (0/0 on empty rays): composite_ray's expression
        const float m = (ratio != ratio) ? ratio : fmaxf(1e-10f, ratio);
        a.disp[ray] = 1.0f / m;
        a.acc[ray] = s_acc;
        a.depth[ray] = s_depth;
        a.n_samples[ray] = count | (stopped ? BAKED_STOPPED : 0);
    }
}

}  // namespace

extern "C" {

int nerf_baked_render(const NerfOccGrid* grid, const int* node_index, const void* table, int n_rows, int sh_degree, const float* rays,
                      int ray_stride, const float* u, int n_rays, float step_size, int max_steps, float stop_eps, int white_bkgd,
                      float* rgb_map, float* disp_map, float* acc_map, float* depth_map, int* n_samples, void* stream) {
    GridArgs g;
    if (int rc = check_grid(__func__, grid, &g)) return rc;
    REQUIRE(node_index && table && rays && rgb_map && disp_map && acc_map && depth_map && n_samples, "null pointer");
    REQUIRE(sh_degree >= 0 && sh_degree <= 2, "bad sh_degree (0, 1 or 2)");
    REQUIRE(ray_stride >= 11 && n_rays >= 0, "bad size (ray records need 11 columns)");
    REQUIRE(n_rows >= 1, "bad n_rows (row 0, the zero row, is always there)");
    REQUIRE(step_size > 0.0f && step_size < INFINITY, "bad step_size (finite and > 0)");                // (a NaN fails the comparison)
    REQUIRE(max_steps >= 1 && max_steps <= (1 << 24), "bad max_steps (1..2^24: a candidate's number is exact in fp32)");
    REQUIRE(stop_eps >= 0.0f && stop_eps < 1.0f, "bad stop_eps (0 <= stop_eps < 1)");                     // (a NaN fails the comparison)
    REQUIRE((reinterpret_cast<uintptr_t>(table) & 15) == 0, "table must be 16-byte aligned");
    if (n_rays == 0) return 0;
    BakedArgs a;
    a.node_index = node_index; a.table = static_cast<const _Float16*>(table); a.n_rows = (unsigned)n_rows;
    a.rays = rays; a.ray_stride = ray_stride; a.u = u; a.n_rays = n_rays; a.ds = step_size; a.M = max_steps; a.stop_eps = stop_eps;
    a.white_bkgd = white_bkgd != 0;
    a.rgb = rgb_map; a.disp = disp_map; a.acc = acc_map; a.depth = depth_map; a.n_samples = n_samples;
    const unsigned blocks = (unsigned)((n_rays + BAKED_RAYS - 1) / BAKED_RAYS);
    hipStream_t st = (hipStream_t)stream;
    if (sh_degree == 0) baked_render_kernel<0><<<blocks, BAKED_THREADS, 0, st>>>(g, a);
    else if (sh_degree == 1) baked_render_kernel<1><<<blocks, BAKED_THREADS, 0, st>>>(g, a);
    else baked_render_kernel<2><<<blocks, BAKED_THREADS, 0, st>>>(g, a);
    return done(__func__, hipGetLastError());
}

}  // extern "C"
