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
#include "baked_device.h"

using namespace nerf_api;
using namespace nerf_grid;
using namespace nerf_baked;

namespace {

constexpr int BAKED_STOPPED = 1 << 30;          // the flag in n_samples (include/nerf_hip.h)

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

// (the row layout, the ray's set-up, the candidates and the arithmetic of a kept sample: baked_device.h, shared with baked_train.hip)
template <int DEG>
__global__ __launch_bounds__(BAKED_THREADS) void baked_render_kernel(GridArgs g, BakedArgs a) {
    constexpr int B = RowOf<DEG>::B;
    const int ray = blockIdx.x * BAKED_RAYS + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;        // (whole waves leave: the ballots and shuffles below see full waves)
    const int lane = threadIdx.x & 63;
    const float* ray_in = a.rays + (size_t)ray * a.ray_stride;
    RaySetup rs;
    const bool ok = ray_setup(ray_in, a.ds, &rs);
    float Y[B];
    sh_basis<DEG>(ray_in[8], ray_in[9], ray_in[10], Y);
    RayIntegrals A;
    int count = 0, stopped = 0;
    if (ok) {
        const float uu = a.u ? a.u[ray] : 0.5f;
        const int ny = g.res[1] + 1, nz = g.res[2] + 1;     // nodes per axis
        for (int k0 = 0; k0 < a.M; k0 += 64) {
            const Candidate cd = candidate(g, rs, uu, k0 + lane, a.M);
            const float z = cd.z;
            const bool keep = cd.keep;
            const unsigned long long vm = __ballot(cd.valid);
            if (!(vm & 1ull)) break;
            const unsigned long long km = __ballot(keep);
            if (km) {
                float alpha = 0.0f, t1 = 1.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
                if (keep) {
                    const Sample sm = sample_value<DEG>(a.node_index, a.table, a.n_rows, ny, nz, cd, Y, a.ds);
                    c0 = sm.c0; c1 = sm.c1; c2 = sm.c2;
                    alpha = sm.alpha;
                    t1 = sm.t1;
                }
                composite_round(A, alpha, t1, c0, c1, c2, keep, z, lane);
                count += __popcll(km);
                if (A.T < a.stop_eps) {           // (stop_eps = 0: never)
                    stopped = 1;
                    break;
                }
            }
            if (!((vm >> 63) & 1ull)) break;    // the valid candidates are a prefix: this round was the last
        }
    }
    if (lane == 0) {
        const float bg = a.white_bkgd ? 1.0f - A.acc : 0.0f;
        a.rgb[(size_t)ray * 3] = A.r + bg; a.rgb[(size_t)ray * 3 + 1] = A.g + bg; a.rgb[(size_t)ray * 3 + 2] = A.b + bg;
        const float ratio = A.depth / A.acc;
        // torch.max(1e-10, ratio) propagates NaN (0/0 on empty rays): composite_ray's expression
        const float m = (ratio != ratio) ? ratio : fmaxf(1e-10f, ratio);
        a.disp[ray] = 1.0f / m;
        a.acc[ray] = A.acc;
        a.depth[ray] = A.depth;
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
