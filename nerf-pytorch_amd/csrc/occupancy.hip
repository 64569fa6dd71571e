// Occupancy-grid empty-space skipping, for rendering and for training (include/nerf_hip.h, section "occupancy grid").
//   nerf_occ_compact : classify the sample points o + d z of one pass against a bit grid and compact the occupied ones into
//                      n_samples = 1 ray records (pt, 0, 0, 0, 0, 0, viewdir) that nerf_field_fwd / nerf_field_fwd_split evaluate;
//   nerf_occ_expand  : scatter the network's answers back to raw[N][S][4], exact zeros for the skipped samples;
//   nerf_occ_mark    : densities of K samples per cell -> grid bits;   nerf_occ_dilate: 3x3x3 OR of a grid;
//   nerf_occ_gather  : the adjoint of nerf_occ_expand, d_raw[N][S][4] -> the M rows the delta chain runs on;
//   nerf_occ_fold_rays : per-point input gradients [M][11] -> per-ray gradients [N][11] (the column contract of
//                      nerf_field_input_grad), one wavefront per ray, a fixed-order reduction;
//   nerf_occ_density_update : density[c] = max(density[c] * decay, max_k sigma[c][k]) (occupancy.DensityGrid).
//   nerf_occ_ray_span : per ray the first and the last occupied cell it crosses inside [near, far] (two walks over the bits), the
//                      interval render_rays(clip_to_occupancy=True) samples instead of [near, far].
//   nerf_occ_proposal_weights : the compositing weights of a ray's samples with the DensityGrid's own density per cell as sigma --
//                      what render_rays(proposal="grid") draws its importance samples from instead of a coarse network's weights.
//   nerf_occ_stop_depth : per ray the depth behind which the transmittance the coarse weights imply has fallen below eps -- a strictly
//                      left-to-right fp32 running sum of the weights against 1 - eps -- and nerf_occ_compact_stop, the compaction that
//                      also drops the samples at or behind it: render_rays(early_stop_eps=eps).
//   nerf_occ_march   : per ray M equal steps over [near, far], the ones in occupied cells (and one closing step behind every occupied
//                      run) emitted into S slots, with the stop depth that makes nerf_occ_compact_stop drop the padding:
//                      render_rays(proposal="march").
//   nerf_occ_march_stop : the same walk over a DensityGrid, which also adds up the grid's own optical depth and stops emitting where the
//                      grid's transmittance has fallen to eps: render_rays(proposal="march", march_stop_eps=eps).
//   nerf_occ_march_step : either walk in steps of one world-space length along the ray, capped at M candidates, with a per-ray fit: a
//                      ray whose emitted steps overflow its slots walks again with the step doubled, up to `fit` times:
//                      render_rays(proposal="march", march_step_size=ds, march_fit=J).
//                      The three are one kernel, occ_march_walk_kernel<Steps, STOP>: Steps (EqualSteps, WorldSteps) says how a candidate
//                      becomes a depth, when it counts and whether there are levels; STOP adds the stop on the optical depth.
//   nerf_occ_view_carve : the cells of a grid projected into a set of training cameras -- per cell the number of cameras whose frustum
//                      it touches and, with silhouette masks, whether some camera sees only background behind it (the visual hull):
//                      OccupancyGrid.from_views, DensityGrid.restrict_to_views.  Needs no network.
// The compaction is deterministic: a count per block of OCC_TILE points, an exclusive scan of the block counts, then the
// write -- inside a block the position of a point is a wave ballot + popcount and a prefix over the block's wave counts, so the
// list is in stable ray-major, sample-minor order and no atomic decides anything.
// Classification is the arithmetic of OccupancyGrid.occupied (nerf-pytorch_amd/occupancy.py): per axis one fp32 subtraction and one
// fp32 multiplication (the library is built with -ffp-contract=off), inside iff 0 <= t < R, cell = floor(t).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "api_util.h"
#include "grid_device.h"     // GridArgs, sample_point, the classification, dir_norm, check_grid: shared with baked.hip
#include "ray_device.h"
#include "scan_device.h"       // occ_scan_kernel: the scan between the count and the write

using namespace nerf_api;
using namespace nerf_grid;

namespace {

constexpr int OCC_THREADS = 256;                // 4 waves
constexpr int OCC_ITERS = 4;
constexpr int OCC_TILE = OCC_THREADS * OCC_ITERS;   // points per block
constexpr int OCC_WAVES = OCC_THREADS / 64;

// lanes below this one whose bit is set in a wave ballot
__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// point of iteration `it` of thread `tid` in block `b`: consecutive lanes take consecutive points (coalesced z reads), a wave's
// 64 points of one iteration are contiguous in the ray-major order
// (32-bit: a call holds fewer than 2^31 - OCC_TILE points, and p / S stays a 32-bit division)
__device__ __forceinline__ unsigned point_of(unsigned b, int it, int tid) { return b * OCC_TILE + it * OCC_THREADS + tid; }

// STOP (nerf_occ_compact_stop): a sample at or behind its ray's stop depth is dropped before the grid is looked at -- it reads no bit
// word.  !(z >= z_stop): a NaN on either side stops nothing.
template <bool STOP>
__device__ __forceinline__ bool in_front(const float* __restrict__ z_stop, unsigned ray, float z) {
    if (!STOP) return true;
    return !(z >= z_stop[ray]);
}

template <bool STOP>
__global__ __launch_bounds__(OCC_THREADS) void occ_count_kernel(GridArgs g, const float* __restrict__ rays, int ray_stride,
                                                                const float* __restrict__ z_vals, const float* __restrict__ z_stop,
                                                                unsigned P, unsigned S, int* __restrict__ block_count) {
    __shared__ int wave_n[OCC_WAVES];
    const int tid = threadIdx.x;
    int n = 0;
#pragma unroll
    for (int it = 0; it < OCC_ITERS; ++it) {
        const unsigned p = point_of(blockIdx.x, it, tid);
        bool occ = false;
        if (p < P) {
            const unsigned ray = p / S;
            const float z = z_vals[p];
            occ = in_front<STOP>(z_stop, ray, z) && occupied(g, sample_point(rays + (size_t)ray * ray_stride, z));
        }
        n += __popcll(__ballot(occ));
    }
    if ((tid & 63) == 0) wave_n[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < OCC_WAVES; ++w) s += wave_n[w];
        block_count[blockIdx.x] = s;
    }
}

template <bool STOP>
__global__ __launch_bounds__(OCC_THREADS) void occ_write_kernel(GridArgs g, const float* __restrict__ rays, int ray_stride,
                                                                const float* __restrict__ z_vals, const float* __restrict__ z_stop,
                                                                unsigned P, unsigned S, const int* __restrict__ block_offset,
                                                                int* __restrict__ slot, float* __restrict__ records) {
    __shared__ int wave_n[OCC_ITERS][OCC_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6;
    bool occ[OCC_ITERS];
    int below[OCC_ITERS];
    Pt pt[OCC_ITERS];
#pragma unroll
    for (int it = 0; it < OCC_ITERS; ++it) {
        const unsigned p = point_of(blockIdx.x, it, tid);
        occ[it] = false;
        pt[it] = Pt{0.0f, 0.0f, 0.0f};
        if (p < P) {
            const unsigned ray = p / S;
            const float z = z_vals[p];
            pt[it] = sample_point(rays + (size_t)ray * ray_stride, z);
            occ[it] = in_front<STOP>(z_stop, ray, z) && occupied(g, pt[it]);
        }
        const unsigned long long m = __ballot(occ[it]);
        below[it] = lanes_below(m);
        if ((tid & 63) == 0) wave_n[it][wave] = __popcll(m);
    }
    __syncthreads();
    int base = block_offset[blockIdx.x];
#pragma unroll
    for (int it = 0; it < OCC_ITERS; ++it) {
        int before = base;
#pragma unroll
        for (int w = 0; w < OCC_WAVES; ++w) {
            const int c = wave_n[it][w];
            if (w < wave) before += c;
            base += c;
        }
        const unsigned p = point_of(blockIdx.x, it, tid);
        if (p < P) {
            const int s = occ[it] ? before + below[it] : -1;
            slot[p] = s;
            if (occ[it]) {
                const float* ray = rays + (size_t)(p / S) * ray_stride;
                float* r = records + (size_t)s * 11;
                r[0] = pt[it].x; r[1] = pt[it].y; r[2] = pt[it].z;
                r[3] = 0.0f; r[4] = 0.0f; r[5] = 0.0f; r[6] = 0.0f; r[7] = 0.0f;
                r[8] = ray[8]; r[9] = ray[9]; r[10] = ray[10];
            }
        }
    }
}

__global__ __launch_bounds__(256) void occ_expand_kernel(const int* __restrict__ slot, const float4* __restrict__ raw_c, long P,
                                                         float4* __restrict__ raw) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int s = slot[p];
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (s >= 0) v = raw_c[s];
    raw[p] = v;
}

// one thread per cell; lanes 0 and 32 of a wave each store one whole word of the ballot (a word is written once, by one lane)
__device__ __forceinline__ void store_ballot_words(bool set, long cell, long n_cells_up32, unsigned* __restrict__ bits) {
    const unsigned long long m = __ballot(set);
    const int lane = threadIdx.x & 63;
    if ((lane & 31) == 0 && cell < n_cells_up32) bits[cell >> 5] = lane ? (unsigned)(m >> 32) : (unsigned)m;
}

__global__ __launch_bounds__(256) void occ_mark_kernel(const float* __restrict__ sigma, long n_cells, int K, float threshold,
                                                       unsigned* __restrict__ words) {
    const long cell = (long)blockIdx.x * 256 + threadIdx.x;
    bool set = false;
    if (cell < n_cells) {
        const float* s = sigma + cell * K;
        for (int k = 0; k < K; ++k) set = set || (s[k] > threshold);
    }
    store_ballot_words(set, cell, (n_cells + 31) & ~31L, words);
}

__global__ __launch_bounds__(256) void occ_dilate_kernel(const unsigned* __restrict__ in, int Rx, int Ry, int Rz, unsigned* __restrict__ out) {
    const long n_cells = (long)Rx * Ry * Rz;
    const long cell = (long)blockIdx.x * 256 + threadIdx.x;
    bool set = false;
    if (cell < n_cells) {
        const int iz = (int)(cell % Rz), iy = (int)((cell / Rz) % Ry), ix = (int)(cell / ((long)Rz * Ry));
        for (int dx = -1; dx <= 1; ++dx)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dz = -1; dz <= 1; ++dz) {
                    const int x = ix + dx, y = iy + dy, z = iz + dz;
                    if (x < 0 || x >= Rx || y < 0 || y >= Ry || z < 0 || z >= Rz) continue;     // clamped at the faces
                    const unsigned c = ((unsigned)x * (unsigned)Ry + (unsigned)y) * (unsigned)Rz + (unsigned)z;
                    set = set || ((in[c >> 5] >> (c & 31u)) & 1u);
                }
    }
    store_ballot_words(set, cell, (n_cells + 31) & ~31L, out);
}

// the adjoint of occ_expand_kernel: one float4 per lane; the slots >= 0 are a bijection onto 0..M-1, so every row is written once
__global__ __launch_bounds__(256) void occ_gather_kernel(const int* __restrict__ slot, const float4* __restrict__ d_raw, long P,
                                                         float4* __restrict__ d_raw_c) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int s = slot[p];
    if (s >= 0) d_raw_c[s] = d_raw[p];
}

constexpr int FOLD_THREADS = 256;               // 4 waves = 4 rays per block
constexpr int FOLD_RAYS = FOLD_THREADS / 64;

__device__ __forceinline__ float wave_sum(float v) {
    // butterfly: every lane ends with the same sum, the order of the additions is fixed by the lane numbers alone
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// One wavefront per ray: lane l takes samples l, l + 64, ... in ascending order, then the butterfly.  A record's point is o + d z
// (d pt / d o = 1, d pt / d d = z) and its view direction is the ray's: columns 0:3, 3:6 and 8:11 of nerf_field_input_grad's contract.
__global__ __launch_bounds__(FOLD_THREADS) void occ_fold_rays_kernel(const int* __restrict__ slot, const float* __restrict__ z_vals,
                                                                      const float* __restrict__ d_rec, int n_rays, int S,
                                                                      float* __restrict__ d_rays, int accumulate) {
    const int ray = blockIdx.x * FOLD_RAYS + (threadIdx.x >> 6);
    if (ray >= n_rays) return;          // (whole waves leave: the shuffles below see full waves)
    const int lane = threadIdx.x & 63;
    const size_t base = (size_t)ray * S;
    float a[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = lane; j < S; j += 64) {
        const int s = slot[base + j];
        if (s < 0) continue;
        const float z = z_vals[base + j];
        const float* g = d_rec + (size_t)s * 11;
        const float gx = g[0], gy = g[1], gz = g[2];
        a[0] += gx; a[1] += gy; a[2] += gz;
        a[3] += z * gx; a[4] += z * gy; a[5] += z * gz;      // (one product rounding each: -ffp-contract=off)
        a[6] += g[8]; a[7] += g[9]; a[8] += g[10];
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) a[c] = wave_sum(a[c]);
    if (lane == 0) {
        float* o = d_rays + (size_t)ray * 11;
        if (accumulate) {
#pragma unroll
            for (int c = 0; c < 6; ++c) o[c] += a[c];
            o[8] += a[6]; o[9] += a[7]; o[10] += a[8];
        } else {
#pragma unroll
            for (int c = 0; c < 6; ++c) o[c] = a[c];
            o[6] = 0.0f; o[7] = 0.0f;
            o[8] = a[6]; o[9] = a[7]; o[10] = a[8];
        }
    }
}

// one thread per cell, in place: m = max_k sigma (a NaN counts as -inf), density = m > density * decay ? m : density * decay
__global__ __launch_bounds__(256) void occ_density_update_kernel(const float* __restrict__ sigma, long n_cells, int K, float decay,
                                                                 float* __restrict__ density) {
    const long cell = (long)blockIdx.x * 256 + threadIdx.x;
    if (cell >= n_cells) return;
    const float* s = sigma + cell * K;
    float m = -INFINITY;
    for (int k = 0; k < K; ++k) {
        const float v = s[k];
        if (v > m) m = v;
    }
    const float d = density[cell] * decay;
    density[cell] = m > d ? m : d;
}

// ---- nerf_occ_ray_span: the occupied span of a ray (OccupancyGrid.ray_span_reference is the definition)
// Two lanes per ray.  The even lane walks the ray forwards over [near, far]; the odd lane walks the REVERSED ray g(s) = go + (-gd) s
// over [-far, -near], so "the last occupied cell" is the first one of the same code and every quantity of the odd lane is the exact
// negation of the even lane's (IEEE negation, division and multiplication are sign-symmetric).  The halves meet in one shuffle.
// A wave's time is its longest walk; with the two walks side by side that is max(front, back) instead of front + back, and the launch
// (n_rays / 32 one-wave blocks) is bound by the serial stepping of its longest walk, not short of lanes: 4096 rays are 128 waves on
// 1024 SIMDs (measured: the same time for 4096 and 32768 rays, proportional to the resolution).
//
// Arithmetic.  Grid coordinates of the ray, once: go = (o - lo) * scale, gd = d * scale (fp32, not contracted); a plane k of axis a is
// crossed at s = (k - go_a) * (1 / gd_a).  Every s comes from the integer plane index, never from an accumulated step.  Its error,
// in cells along the fastest axis (times m = max_a |gd_a|), is a few ulp of |go_a| + |k| <= a few ulp of 2 R: with R <= 512 that is
// <= 2^-11 cell (ulp(1024) = 2^-13, four of them), with R <= 128 <= 2^-13.  Hence the two constants, both 2^-10 cell:
//   SPAN_PAD   the result is widened by pad = 2^-10 / m on either side -- above the error of an end point, so a sample the fp32
//              classifier calls occupied next to the first / last cell stays inside; it also makes far' > near' on every hit;
//   SPAN_THICK a stretch (one cell, or one stretch outside the box) counts only when its fp32 length exceeds 2^-10 cell.  A stretch
//              the float64 definition calls thick (> 2^-9) measures > 2^-9 - 2 * 2^-11 = 2^-10 here and is kept; a cell the float64
//              ray never enters (two crossings swapped by rounding) measures < 2 * 2^-11 and is dropped.
// Both walks are for loops of at most Rx + Ry + Rz + 3 steps (a step raises or lowers one cell index by one and leaves the box after
// at most Rx + Ry + Rz of them); running into the bound ends the walk with the unclipped end.
constexpr int SPAN_THREADS = 64;                // one wave = 32 rays per block
constexpr float SPAN_PAD = 0.0009765625f;       // 2^-10 cell
constexpr float SPAN_THICK = 0.0009765625f;     // 2^-10 cell
constexpr int SPAN_BATCH = 8;                   // steps whose bit words are loaded together (measured: 1 / 4 / 8 -> 51 / 46 / 44 us at 128^3)

// cell index of coordinate p at the start of a walk, clamped into the grid (a start on a face of the box rounds to either side of
// it; a NaN becomes 0)
__device__ __forceinline__ int start_cell(float p, int R) { return (int)fminf(fmaxf(floorf(p), 0.0f), (float)(R - 1)); }

// One axis of a walk: step (+1, -1, or 0 for a direction component that is zero or whose reciprocal overflows), the reciprocal, and
// the parameter of the next plane.  An axis that does not move has next = +inf and is never chosen.
struct SpanAxis {
    float go, inv, next;
    int i, step, R;
    __device__ __forceinline__ float plane() const { return ((float)(i + (step > 0 ? 1 : 0)) - go) * inv; }
    __device__ __forceinline__ void set_next() { next = step == 0 ? INFINITY : plane(); }
};

// First occupied stretch of g(s) = go + gd s over [a, b] (a < b, all finite), as its start parameter: true and *first, or false
__device__ __forceinline__ bool first_occupied(const GridArgs& g, const float go[3], const float gd[3], float a, float b, float m,
                                               float* first) {
    SpanAxis ax[3];
    float s_in = a, s_out = b;
    bool crosses = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float R = (float)g.res[k];
        const float inv = 1.0f / gd[k];
        const bool moves = gd[k] != 0.0f && fabsf(inv) < INFINITY;
        ax[k].go = go[k]; ax[k].R = g.res[k];
        ax[k].inv = moves ? inv : 0.0f;
        ax[k].step = moves ? (gd[k] > 0.0f ? 1 : -1) : 0;
        if (moves) {
            const float s0 = (0.0f - go[k]) * inv, s1 = (R - go[k]) * inv;      // (finite * finite: never a NaN)
            s_in = fmaxf(s_in, fminf(s0, s1));
            s_out = fminf(s_out, fmaxf(s0, s1));
        } else if (!(go[k] >= 0.0f && go[k] < R)) {
            crosses = false;
        }
    }
    crosses = crosses && s_in < s_out;
    const bool outside_counts = g.outside_skip == 0;
    if (!crosses) {             // [a, b] is one stretch outside the box
        *first = a;
        return outside_counts && (b - a) * m > SPAN_THICK;
    }
    if (outside_counts && (s_in - a) * m > SPAN_THICK) {        // a stretch in front of the box
        *first = a;
        return true;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ax[k].i = start_cell(go[k] + gd[k] * s_in, g.res[k]);
        ax[k].set_next();
    }
    const int bound = g.res[0] + g.res[1] + g.res[2] + 3;
    float s = s_in;
    bool left_box = false;
    // SPAN_BATCH steps at a time: the cells of the next steps do not depend on the bits, so their words are loaded together (one
    // L2 latency per batch instead of one per cell) and looked at in walk order afterwards
    for (int n = 0; n < bound && !left_box; n += SPAN_BATCH) {
        unsigned word[SPAN_BATCH], bit[SPAN_BATCH];
        float s0[SPAN_BATCH], s1[SPAN_BATCH];
#pragma unroll
        for (int j = 0; j < SPAN_BATCH; ++j) {
            word[j] = 0u; bit[j] = 0u; s0[j] = s; s1[j] = s;
            if (left_box) continue;
            // the axis whose plane comes first (ties: x before y before z); selects, no branches: the lanes of a wave step
            // different axes, and a branch per axis would run all three bodies one after the other
            const bool c0 = ax[0].next <= ax[1].next && ax[0].next <= ax[2].next;
            const bool c1 = !c0 && ax[1].next <= ax[2].next;
            const float nx = c0 ? ax[0].next : (c1 ? ax[1].next : ax[2].next);
            const unsigned c = ((unsigned)ax[0].i * (unsigned)g.res[1] + (unsigned)ax[1].i) * (unsigned)g.res[2] + (unsigned)ax[2].i;
            word[j] = g.bits[c >> 5];       // (the indices are inside the grid as long as the walk has not left the box)
            bit[j] = c & 31u;
            s1[j] = fminf(nx, s_out);
            if (!(nx < s_out)) { left_box = true; continue; }
            s = fmaxf(s, nx);
#pragma unroll
            for (int a3 = 0; a3 < 3; ++a3) {
                const bool me = a3 == 0 ? c0 : (a3 == 1 ? c1 : !(c0 || c1));        // (an axis that does not move has next = +inf: never me)
                ax[a3].i += me ? ax[a3].step : 0;
                ax[a3].next = me ? ax[a3].plane() : ax[a3].next;
                left_box = left_box || (unsigned)ax[a3].i >= (unsigned)ax[a3].R;
            }
        }
#pragma unroll
        for (int j = 0; j < SPAN_BATCH; ++j)
            if (((word[j] >> bit[j]) & 1u) && (s1[j] - s0[j]) * m > SPAN_THICK) {
                *first = s0[j];
                return true;
            }
    }
    *first = a;
    if (!left_box) return true;         // the bound: the unclipped end
    if (outside_counts && (b - s_out) * m > SPAN_THICK) {       // nothing in the box, a stretch behind it
        *first = s_out;
        return true;
    }
    return false;
}

__global__ __launch_bounds__(SPAN_THREADS) void occ_ray_span_kernel(GridArgs g, const float* __restrict__ rays, int ray_stride, int n_rays,
                                                                    float* __restrict__ span, int* __restrict__ hit) {
    const int t = blockIdx.x * SPAN_THREADS + threadIdx.x;
    const int ray = t >> 1;
    const bool back = t & 1;
    const bool live = ray < n_rays;         // (no early return: the shuffle below wants both lanes of a pair, and a pair is all live or all not)
    float r[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (live) {
        const float* p = rays + (size_t)ray * ray_stride;
#pragma unroll
        for (int c = 0; c < 8; ++c) r[c] = p[c];
    }
    bool ok = live && r[6] < r[7];
#pragma unroll
    for (int c = 0; c < 8; ++c) ok = ok && fabsf(r[c]) < INFINITY;      // (a NaN fails the comparison)
    float go[3], gd[3], m = 0.0f;
    const float sign = back ? -1.0f : 1.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        go[k] = (r[k] - g.lo[k]) * g.scale[k];
        gd[k] = sign * (r[3 + k] * g.scale[k]);
        m = fmaxf(m, fabsf(gd[k]));
        ok = ok && fabsf(go[k]) < INFINITY;
    }
    ok = ok && m > 0.0f && m < INFINITY;
    float first = 0.0f;
    bool found = false;
    if (ok) found = first_occupied(g, go, gd, back ? -r[7] : r[6], back ? -r[6] : r[7], m, &first);
    // the own end in t: near' = max(near, t_first - pad) or far' = min(far, t_last + pad)
    const float pad = SPAN_PAD / m;
    const float end = back ? fminf(r[7], pad - first) : fmaxf(r[6], first - pad);
    const float other = __shfl_xor(end, 1);
    const int other_found = __shfl_xor((int)found, 1);
    if (live && !back) {
        const bool h = found && other_found && end < other;
        float2 out;
        out.x = h ? end : r[6];
        out.y = h ? other : r[7];
        *reinterpret_cast<float2*>(span + (size_t)ray * 2) = out;
        hit[ray] = h ? 1 : 0;
    }
}

// ---- nerf_occ_proposal_weights (DensityGrid.proposal_sigma is the definition of the lookup)
// One wavefront per ray, the launch shape and the arithmetic of composite_ray<false> (ray_device.h) with sigma_i looked up in the grid:
// lane l owns the C = ceil(S / 64) consecutive samples from l C on, multiplies their 1 - alpha + 1e-10 into a segment product, the
// wave scans the products, and the lane walks its segment again for w_i = alpha_i T_i.  Same operations in the same order, so the
// weights are those nerf_raw2outputs gives for raw = (0, 0, 0, sigma) without noise, bit for bit.  No colours, no ray integrals.
// LDS: 2 S floats (alpha_i, 1 - alpha_i + 1e-10); each lane touches only its own segment: no synchronisation.
__device__ __forceinline__ float proposal_sigma(const GridArgs& g, const float* __restrict__ density, float outside_sigma, const Pt& p) {
    unsigned c;
    if (!cell_of(g, p, &c)) return g.outside_skip ? 0.0f : outside_sigma;
    return cell_bit(g, c) ? density[c] : 0.0f;
}

__global__ __launch_bounds__(64) void occ_proposal_weights_kernel(GridArgs g, const float* __restrict__ density, float outside_sigma,
                                                                   const float* __restrict__ rays, int ray_stride,
                                                                   const float* __restrict__ z_vals, int S, float* __restrict__ weights,
                                                                   float* __restrict__ sigma_out) {
    extern __shared__ float sm[];
    const int ray = blockIdx.x, lane = threadIdx.x;
    const int C = (S + 63) >> 6;
    const int lo = lane * C, hi = min(lo + C, S);
    const float* r = rays + (size_t)ray * ray_stride;
    const float* z = z_vals + (size_t)ray * S;
    const float dn = dir_norm(r);
    float* s_alpha = sm;            // alpha_i
    float* s_t = sm + S;            // 1 - alpha_i + 1e-10
    float seg = 1.0f;
    for (int i = lo; i < hi; ++i) {
        const float zi = z[i];
        float dist = (i + 1 < S) ? (z[i + 1] - zi) : 1e10f;
        dist = dist * dn;
        const float sg = proposal_sigma(g, density, outside_sigma, sample_point(r, zi));
        if (sigma_out) sigma_out[(size_t)ray * S + i] = sg;
        const float ex = expf(-fmaxf(sg, 0.0f) * dist);
        const float al = 1.0f - ex;
        const float t = 1.0f - al + 1e-10f;
        s_alpha[i] = al;
        s_t[i] = t;
        seg *= t;
    }
    const float incl = nerf::wave_incl_scan_mul(seg, lane);
    float T = __shfl_up(incl, 1);
    if (lane == 0) T = 1.0f;
    for (int i = lo; i < hi; ++i) {
        weights[(size_t)ray * S + i] = s_alpha[i] * T;
        T *= s_t[i];
    }
}

// ---- nerf_occ_stop_depth (occupancy.stop_depth_reference is the definition)
// A block takes STOP_RAYS rays and walks their weights in tiles of STOP_RAYS x STOP_COLS through LDS.  Loading: consecutive lanes take
// consecutive samples of one ray (a wave reads one 256-byte run per ray: coalesced).  Summing: lane r of wave 0 owns ray r and adds its
// row left to right, one fp32 addition per sample -- the contract, which is what makes np.cumsum(dtype=float32) a bit-exact reference;
// a row is STOP_COLS + 1 words long, so the 32 lanes of a half-wave read 32 different banks.  The other three waves only load.  z_vals
// is touched once per ray, at the sample behind the crossing (4 B per ray; staging the whole array would move S times as much).  The
// block leaves as soon as every one of its rays has crossed.
constexpr int STOP_RAYS = 64;
constexpr int STOP_COLS = 64;
constexpr int STOP_THREADS = 256;

__global__ __launch_bounds__(STOP_THREADS) void occ_stop_depth_kernel(const float* __restrict__ z_vals, const float* __restrict__ weights,
                                                                      int n_rays, int S, float threshold, float* __restrict__ z_stop) {
    __shared__ float tile[STOP_RAYS][STOP_COLS + 1];
    const int tid = threadIdx.x;
    const int ray0 = blockIdx.x * STOP_RAYS;
    const int col = tid & (STOP_COLS - 1);
    const int my_ray = ray0 + tid;              // (meaningful for wave 0 only)
    const bool walker = tid < STOP_RAYS && my_ray < n_rays;
    float a = 0.0f;
    int crossed = -1;
    for (int c0 = 0; c0 < S; c0 += STOP_COLS) {
#pragma unroll 4
        for (int row = tid / STOP_COLS; row < STOP_RAYS; row += STOP_THREADS / STOP_COLS) {
            const int r = ray0 + row, c = c0 + col;
            tile[row][col] = (r < n_rays && c < S) ? weights[(size_t)r * S + c] : 0.0f;
        }
        __syncthreads();
        if (walker && crossed < 0) {
            const int n = min(STOP_COLS, S - c0);
            for (int j = 0; j < n; ++j) {
                a = a + tile[tid][j];
                if (a >= threshold) {           // (a NaN never is, and poisons a: such a ray never stops)
                    crossed = c0 + j;
                    break;
                }
            }
        }
        if (__syncthreads_and(!walker || crossed >= 0)) break;      // (also the barrier in front of the next tile's stores)
    }
    if (walker) z_stop[my_ray] = (crossed >= 0 && crossed + 1 < S) ? z_vals[(size_t)my_ray * S + crossed + 1] : INFINITY;
}

// ---- nerf_occ_march, nerf_occ_march_stop, nerf_occ_march_step: one walk
// (OccupancyGrid.march_reference / march_step_reference and DensityGrid.march_stop_reference / march_step_stop_reference are the definitions)
// One wavefront per ray, MARCH_RAYS rays per block.  A round takes 64 candidates: lane l builds z_k of k = k0 + l, asks whether it is
// `valid`, and classifies it with sample_point / occupied -- the compaction's own functions, so the compaction sees the bits this kernel
// saw.  The keep mask is a ballot; the closing candidates are (keep << 1 | carry) & ~keep & valid, carry being lane 63's keep bit of the
// round before; a lane's rank is the emitted lanes below it plus the running base.  Ranks below S - 1 store their depth, rank S - 1 is
// the stop depth (one shuffle hands it to every lane), and the wave leaves the walk once the base has passed S - 1: a ray that fills its
// slots in the first rounds never looks at the rest of its M candidates.  The valid candidates are a prefix of 0 .. M - 1, so a round
// whose lane 63 is not valid is the ray's last.  Then the lanes pad the row with the stop depth.
//
// STOP: the ray also stops emitting at the first valid candidate in front of which the grid's own optical depth A_k = sum_{j < k} c_j
// has reached tau = -ln(eps).  Per round the lane builds c of its candidate -- proposal_sigma at the point it classified (0 where the
// candidate is not kept, where sigma <= 0 and where sigma is a NaN) times the interval up to the NEXT candidate (built from k + 1 by
// the same expression; far where that one is not valid) times |d|, occ_proposal_weights_kernel's order of operations --, the wave scans
// c (nerf::wave_incl_scan_add: the order of the additions is the definition's), A = depth + the inclusive sum of the lane below, and
// one ballot of A >= tau finds the cut lane.  The emit mask keeps the lanes below the cut; a truncation hit inside what is left wins
// (the slot limit bites first), otherwise the stop depth is the cut lane's z.  A NaN in A fails the comparison and poisons every later
// A: such a ray never stops.
//
// Steps: how candidate k becomes a depth, when it counts, and whether the walk has levels.
//   EqualSteps  M equal steps over [near, far]: t = (k + u) / M, z = near * (1 - t) + far * t; valid while k < M; one level.
//   WorldSteps  steps of one length ds along the ray: dz = (ds / |d|) * 2^level, z = near + (k + u) * dz -- one addition, one
//               multiplication, one addition --; valid while k < M and z < far.  The fit: a ray whose emitted candidates overflow its
//               slots at a level below `fit` starts again with the doubled step; the plain stores of the later level overwrite its row
//               (ranks 0 .. S - 2 that the later level does not reach are covered by the padding loop, which starts at
//               min(base, S - 1) of the LAST level).  A ray leaves the kernel at the first level that fits.
// Everything the wave branches on is wave-uniform (ballots, the level, the round); no atomics, no LDS.
constexpr int MARCH_THREADS = 256;
constexpr int MARCH_RAYS = MARCH_THREADS / 64;

struct MarchArgs {
    const float* density;       // STOP: one sigma per cell, and what counts outside the box
    float outside_sigma;
    const float* rays;
    int ray_stride;
    const float* u;             // one offset per ray, or null: 0.5
    int n_rays;
    float ds;                   // WorldSteps: the step's length along the ray
    int M, S;
    int fit;                    // WorldSteps: the highest level
    float tau;                  // STOP
    float* z_vals;
    float* z_stop;
    int* truncated;
    int* level;                 // WorldSteps
    int* stopped;               // STOP
};

struct EqualSteps {
    static constexpr bool LEVELS = false;
    float near, far, Mf;
    int M;
    __device__ __forceinline__ bool start(const MarchArgs& a, float near_, float far_, float) {
        near = near_; far = far_; M = a.M; Mf = (float)a.M;
        return true;
    }
    __device__ __forceinline__ void set_level(int) {}
    __device__ __forceinline__ float depth(int k, float uu) const {
        const float t = ((float)k + uu) / Mf;               // (IEEE division: hipcc's default for fp32)
        return near * (1.0f - t) + far * t;                 // run_nerf.py:360 (no contraction)
    }
    __device__ __forceinline__ bool valid(int k, float) const { return k < M; }
};

struct WorldSteps {
    static constexpr bool LEVELS = true;
    float near, far, dz0, dz;
    int M;
    __device__ __forceinline__ bool start(const MarchArgs& a, float near_, float far_, float dn) {
        near = near_; far = far_; M = a.M;
        dz0 = a.ds / dn;                                    // (IEEE division: hipcc's default for fp32)
        return dz0 > 0.0f && dz0 < INFINITY;                // (d = 0, an overflowing |d|, a NaN: no step)
    }
    __device__ __forceinline__ void set_level(int lvl) { dz = dz0 * (float)(1 << lvl); }     // (exact, or +inf: then no candidate is valid)
    __device__ __forceinline__ float depth(int k, float uu) const { return near + ((float)k + uu) * dz; }   // (no contraction)
    __device__ __forceinline__ bool valid(int k, float z) const { return k < M && z < far; }                // (a NaN fails the comparison)
};

template <class Steps, bool STOP>
__global__ __launch_bounds__(MARCH_THREADS) void occ_march_walk_kernel(GridArgs g, MarchArgs a) {
    const int ray = blockIdx.x * MARCH_RAYS + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;        // (whole waves leave: the ballots and shuffles below see full waves)
    const int lane = threadIdx.x & 63;
    const int S = a.S;
    const float* ray_in = a.rays + (size_t)ray * a.ray_stride;
    float* zrow = a.z_vals + (size_t)ray * S;
    const float near = ray_in[6], far = ray_in[7];
    bool ok = near < far;
#pragma unroll
    for (int c = 0; c < 8; ++c) ok = ok && fabsf(ray_in[c]) < INFINITY;     // (a NaN fails the comparison)
    // o and d, read once (the pointers inside a struct promise no __restrict__: behind a store to zrow the compiler would load them again
    // in every round) and held in scalar registers: the wave has one ray
    float r[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) r[c] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ray_in[c])));
    const float dn = (STOP || Steps::LEVELS) ? dir_norm(r) : 0.0f;
    Steps steps;
    ok = steps.start(a, near, far, dn) && ok;
    if (!ok) {
        for (int j = lane; j < S; j += 64) zrow[j] = far;
        if (lane == 0) {
            a.z_stop[ray] = -INFINITY;
            a.truncated[ray] = 0;
            if (Steps::LEVELS) a.level[ray] = 0;
            if (STOP) a.stopped[ray] = 0;
        }
        return;
    }
    const float uu = a.u ? a.u[ray] : 0.5f;
    const int last = S - 1;
    int lvl = 0, base, trunc, stp;
    float stop;
    for (;; ++lvl) {
        steps.set_level(lvl);
        base = 0; trunc = 0; stp = 0;
        stop = far;
        unsigned long long carry = 0ull;
        float depth = 0.0f;             // STOP: A in front of the round's first candidate
        bool more = true;
        for (int k0 = 0; k0 < a.M && base <= last && !stp && more; k0 += 64) {
            const int k = k0 + lane;
            const float z = steps.depth(k, uu);
            const bool valid = steps.valid(k, z);
            const unsigned long long vm = __ballot(valid);
            more = (vm >> 63) & 1ull;
            const Pt p = sample_point(r, z);
            const bool keep = valid && occupied(g, p);
            const unsigned long long km = __ballot(keep);
            unsigned long long em = km | (((km << 1) | carry) & ~km & vm);
            carry = km >> 63;
            unsigned long long cut = 0ull;
            int cut_lane = 64;
            if (STOP) {
                float c = 0.0f;
                if (keep) {
                    const float z1 = steps.depth(k + 1, uu);
                    const float zn = steps.valid(k + 1, z1) ? z1 : far;
                    const float sg = proposal_sigma(g, a.density, a.outside_sigma, p);
                    const float dist = (zn - z) * dn;
                    c = (sg > 0.0f ? sg : 0.0f) * dist;     // (a NaN sigma fails the comparison: 0)
                }
                const float incl = nerf::wave_incl_scan_add(c, lane);
                float below = __shfl_up(incl, 1);
                if (lane == 0) below = 0.0f;
                cut = __ballot(valid && depth + below >= a.tau);
                if (cut) {
                    cut_lane = __ffsll((long long)cut) - 1;
                    em &= (1ull << cut_lane) - 1ull;
                }
                depth = depth + __shfl(incl, 63);
            }
            const int rank = base + lanes_below(em);
            const bool emit = (em >> lane) & 1ull;
            if (emit && rank < last) zrow[rank] = z;
            const unsigned long long hit = __ballot(emit && rank == last);
            if (hit) {
                stop = __shfl(z, __ffsll((long long)hit) - 1);
                trunc = 1;
            } else if (cut) {
                stop = __shfl(z, cut_lane);
                stp = 1;
            }
            base += __popcll(em);
        }
        if (!Steps::LEVELS || !trunc || lvl >= a.fit) break;
        // the next level's stores land on this level's, from other lanes of the same wave: a wave's vector stores are performed in
        // issue order, which is what wavefront scope asks for (no instruction, the compiler keeps the order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
    for (int j = min(base, last) + lane; j < S; j += 64) zrow[j] = stop;
    if (lane == 0) {
        a.z_stop[ray] = stop;
        a.truncated[ray] = trunc;
        if (Steps::LEVELS) a.level[ray] = lvl;
        if (STOP) a.stopped[ray] = stp;
    }
}

// ---- nerf_occ_view_carve (OccupancyGrid.view_counts_reference / carved_reference are the definitions)
// One thread per cell.  The cell's corner coordinates -- two per axis, lo + float(i + o) * width -- are built once and stay in
// registers; the loop over the views is wave-uniform, so the 16 floats of a camera record (c2w row-major, fx, fy, cx, cy) are the same
// address for every lane.  Per view the eight corners go through the camera once: d = p - t, x / y / s as three products added left to
// right, the six inside-tests as running ANDs of "this corner fails test k" (a NaN fails every test: a NaN camera sees nothing), and,
// with masks, the projected pixel (i, j) by one IEEE division each with running minima and maxima.  A camera carves only where all
// eight corners have s >= near_m, every i and j is finite and the rectangle [floor(min - m), ceil(max + m)] lies inside the image: only
// then are the four words of its summed-area table loaded.  No atomics: a cell's count is its own thread's, and a word of the carved
// bits is stored whole by one lane from the wave's ballot (accumulate: that lane ORs into the word it owns).
constexpr int CARVE_THREADS = 256;

struct CarveArgs {
    float lo[3], width[3];
    int res[3];
    const float* cams;          // [n_views][16]
    int n_views, H, W;
    float near_m, far_m, m;
    const int* sat;             // [n_views][H + 1][W + 1], or null: no carving
    int accumulate;
    int* seen;
    unsigned* carved;
};

__global__ __launch_bounds__(CARVE_THREADS) void occ_view_carve_kernel(CarveArgs a) {
    const long n_cells = (long)a.res[0] * a.res[1] * a.res[2];
    const long cell = (long)blockIdx.x * CARVE_THREADS + threadIdx.x;
    const bool live = cell < n_cells;       // (no early return: the ballot below wants whole waves)
    int count = 0;
    bool carved = false;
    if (live) {
        const int iz = (int)(cell % a.res[2]), iy = (int)((cell / a.res[2]) % a.res[1]), ix = (int)(cell / ((long)a.res[2] * a.res[1]));
        float px[2], py[2], pz[2];
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            px[o] = a.lo[0] + (float)(ix + o) * a.width[0];
            py[o] = a.lo[1] + (float)(iy + o) * a.width[1];
            pz[o] = a.lo[2] + (float)(iz + o) * a.width[2];
        }
        const float m = a.m;
        const float w_hi = (float)(a.W - 1) + m, h_hi = (float)(a.H - 1) + m;
        const size_t sat_row = (size_t)a.W + 1, sat_view = ((size_t)a.H + 1) * sat_row;
        for (int v = 0; v < a.n_views; ++v) {
            const float* __restrict__ c = a.cams + (size_t)v * 16;
            const float fx = c[12], fy = c[13], cx = c[14], cy = c[15];
            const float i_lo = -m - cx, i_hi = w_hi - cx, j_lo = -m - cy, j_hi = h_hi - cy;
            bool f_near = true, f_far = true, f_l = true, f_r = true, f_t = true, f_b = true;       // "every corner so far fails this test"
            bool all_near = true, finite = true;
            float i_min = INFINITY, i_max = -INFINITY, j_min = INFINITY, j_max = -INFINITY;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float dx = px[(k >> 2) & 1] - c[3], dy = py[(k >> 1) & 1] - c[7], dz = pz[k & 1] - c[11];
                const float x = dx * c[0] + dy * c[4] + dz * c[8];
                const float y = dx * c[1] + dy * c[5] + dz * c[9];
                const float s = -(dx * c[2] + dy * c[6] + dz * c[10]);
                const float fxx = fx * x, fyy = fy * y;
                const bool near_ok = s >= a.near_m;
                f_near = f_near && !near_ok;
                f_far = f_far && !(s <= a.far_m);
                f_l = f_l && !(fxx >= i_lo * s);
                f_r = f_r && !(fxx <= i_hi * s);
                f_t = f_t && !(-fyy >= j_lo * s);
                f_b = f_b && !(-fyy <= j_hi * s);
                if (a.sat) {
                    const float pi = fxx / s + cx, pj = cy - fyy / s;       // (IEEE division: hipcc's default for fp32)
                    all_near = all_near && near_ok;
                    finite = finite && fabsf(pi) < INFINITY && fabsf(pj) < INFINITY;       // (a NaN fails the comparison)
                    i_min = fminf(i_min, pi); i_max = fmaxf(i_max, pi);
                    j_min = fminf(j_min, pj); j_max = fmaxf(j_max, pj);
                }
            }
            if (!(f_near || f_far || f_l || f_r || f_t || f_b)) ++count;
            if (a.sat && all_near && finite) {
                const float i0 = floorf(i_min - m), i1 = ceilf(i_max + m), j0 = floorf(j_min - m), j1 = ceilf(j_max + m);
                if (i0 >= 0.0f && i1 <= (float)(a.W - 1) && j0 >= 0.0f && j1 <= (float)(a.H - 1)) {     // else the camera abstains
                    const int* __restrict__ t = a.sat + (size_t)v * sat_view;
                    const size_t r0 = (size_t)(int)j0 * sat_row, r1 = ((size_t)(int)j1 + 1) * sat_row;
                    const size_t c0 = (size_t)(int)i0, c1 = (size_t)(int)i1 + 1;
                    const int n = t[r1 + c1] - t[r0 + c1] - t[r1 + c0] + t[r0 + c0];
                    carved = carved || n == 0;
                }
            }
        }
        a.seen[cell] = a.accumulate ? a.seen[cell] + count : count;
    }
    if (a.carved) {
        const unsigned long long mask = __ballot(carved);
        const int lane = threadIdx.x & 63;
        if ((lane & 31) == 0 && cell < ((n_cells + 31) & ~31L)) {
            const unsigned w = lane ? (unsigned)(mask >> 32) : (unsigned)mask;
            unsigned* out = a.carved + (cell >> 5);
            *out = a.accumulate ? (*out | w) : w;
        }
    }
}

inline long occ_blocks(long n_points) { return (n_points + OCC_TILE - 1) / OCC_TILE; }

// nerf_occ_compact (STOP false, z_stop unused) and nerf_occ_compact_stop
template <bool STOP>
int compact(const char* fn, const NerfOccGrid* grid, const float* rays, int ray_stride, const float* z_vals, const float* z_stop, int n_rays,
            int n_samples, int* slot, float* records, int* count, int* scratch, void* stream) {
    GridArgs g;
    if (int rc = check_grid(fn, grid, &g)) return rc;
    if (!(rays && z_vals && (z_stop || !STOP) && slot && records && count && scratch)) return fail_arg(fn, "null pointer");
    if (!(ray_stride >= 11 && n_rays >= 0 && n_samples >= 1)) return fail_arg(fn, "bad size (ray records need 11 columns)");
    const long P = (long)n_rays * n_samples;
    if (!(P < (1L << 31) - OCC_TILE)) return fail_arg(fn, "too many points for one call");
    hipStream_t st = (hipStream_t)stream;
    if (P == 0) return done(fn, hipMemsetAsync(count, 0, sizeof(int), st));
    const int nb = (int)occ_blocks(P);
    occ_count_kernel<STOP><<<nb, OCC_THREADS, 0, st>>>(g, rays, ray_stride, z_vals, z_stop, (unsigned)P, (unsigned)n_samples, scratch);
    occ_scan_kernel<<<1, SCAN_THREADS, 0, st>>>(scratch, nb, count);
    occ_write_kernel<STOP><<<nb, OCC_THREADS, 0, st>>>(g, rays, ray_stride, z_vals, z_stop, (unsigned)P, (unsigned)n_samples, scratch, slot,
                                                       records);
    return done(fn, hipGetLastError());
}

// the sizes the three march entry points take alike
int check_march_sizes(const char* fn, int ray_stride, int n_rays, int n_steps, int n_slots) {
    if (!(ray_stride >= 8 && n_rays >= 0 && n_steps >= 1 && n_steps <= 16384 && n_slots >= 1 && n_slots <= 4096))
        return fail_arg(fn, "bad size (ray records need 8 columns, 1..16384 steps, 1..4096 slots)");
    return 0;
}

// the march of checked arguments: a.density chooses the stop form, `world` the steps
int launch_march(const char* fn, const GridArgs& g, const MarchArgs& a, bool world, void* stream) {
    if (a.n_rays == 0) return 0;
    const unsigned blocks = (unsigned)((a.n_rays + MARCH_RAYS - 1) / MARCH_RAYS);
    hipStream_t st = (hipStream_t)stream;
    if (world) {
        if (a.density) occ_march_walk_kernel<WorldSteps, true><<<blocks, MARCH_THREADS, 0, st>>>(g, a);
        else occ_march_walk_kernel<WorldSteps, false><<<blocks, MARCH_THREADS, 0, st>>>(g, a);
    } else {
        if (a.density) occ_march_walk_kernel<EqualSteps, true><<<blocks, MARCH_THREADS, 0, st>>>(g, a);
        else occ_march_walk_kernel<EqualSteps, false><<<blocks, MARCH_THREADS, 0, st>>>(g, a);
    }
    return done(fn, hipGetLastError());
}

// the one body of the three march entry points (fn: the public function's name).  MARCH_PLAIN and MARCH_STOP take equal steps, without
// and with the densities; MARCH_STEP takes world-space steps, and whether density and stopped are there chooses its stop form.
enum MarchForm { MARCH_PLAIN, MARCH_STOP, MARCH_STEP };
int march_entry(const char* fn, MarchForm form, const NerfOccGrid* grid, const float* density, float outside_sigma, const float* rays,
                int ray_stride, const float* u, int n_rays, float step_size, int n_steps, int n_slots, int fit, float tau, float* z_vals,
                float* z_stop, int* truncated, int* level, int* stopped, void* stream) {
    const bool world = form == MARCH_STEP;
    GridArgs g;
    if (int rc = check_grid(fn, grid, &g)) return rc;
    bool have = rays && z_vals && z_stop && truncated;                  // what every form needs
    if (form == MARCH_STOP) have = have && density && stopped;
    if (form == MARCH_STEP) have = have && level;
    if (!have) return fail_arg(fn, "null pointer");
    if (world && (density != nullptr) != (stopped != nullptr))
        return fail_arg(fn, "null pointer (density and stopped come together: the stop form, or neither)");
    if (int rc = check_march_sizes(fn, ray_stride, n_rays, n_steps, n_slots)) return rc;
    if (world && !(fit >= 0 && fit <= 8)) return fail_arg(fn, "bad fit (0..8 doublings of the step)");
    if (world && !(step_size > 0.0f && step_size < INFINITY)) return fail_arg(fn, "bad step_size (finite and > 0)");     // (a NaN fails the comparison)
    if (density && !(tau > 0.0f)) return fail_arg(fn, "bad threshold (tau = -ln(eps) must be > 0)");                    // (a NaN fails the comparison)
    MarchArgs a;
    a.rays = rays; a.ray_stride = ray_stride; a.u = u; a.n_rays = n_rays; a.M = n_steps; a.S = n_slots;
    a.z_vals = z_vals; a.z_stop = z_stop; a.truncated = truncated;
    a.ds = step_size; a.fit = fit; a.level = level;                                         // WorldSteps
    a.density = density; a.outside_sigma = outside_sigma; a.tau = tau; a.stopped = stopped;    // STOP
    return launch_march(fn, g, a, world, stream);
}

}  // namespace

extern "C" {

size_t nerf_occ_scratch_words(long n_points) { return n_points > 0 ? (size_t)occ_blocks(n_points) : 0; }

int nerf_occ_compact(const NerfOccGrid* grid, const float* rays, int ray_stride, const float* z_vals, int n_rays, int n_samples,
                     int* slot, float* records, int* count, int* scratch, void* stream) {
    return compact<false>(__func__, grid, rays, ray_stride, z_vals, nullptr, n_rays, n_samples, slot, records, count, scratch, stream);
}

int nerf_occ_compact_stop(const NerfOccGrid* grid, const float* rays, int ray_stride, const float* z_vals, const float* z_stop, int n_rays,
                          int n_samples, int* slot, float* records, int* count, int* scratch, void* stream) {
    return compact<true>(__func__, grid, rays, ray_stride, z_vals, z_stop, n_rays, n_samples, slot, records, count, scratch, stream);
}

int nerf_occ_stop_depth(const float* z_vals, const float* weights, int n_rays, int n_samples, float threshold, float* z_stop, void* stream) {
    REQUIRE(z_vals && weights && z_stop, "null pointer");
    REQUIRE(n_rays >= 0 && n_samples >= 1 && n_samples <= 4096, "bad size (1..4096 samples)");
    if (n_rays == 0) return 0;
    occ_stop_depth_kernel<<<(unsigned)((n_rays + STOP_RAYS - 1) / STOP_RAYS), STOP_THREADS, 0, (hipStream_t)stream>>>(
        z_vals, weights, n_rays, n_samples, threshold, z_stop);
    return done(__func__, hipGetLastError());
}

int nerf_occ_march(const NerfOccGrid* grid, const float* rays, int ray_stride, const float* u, int n_rays, int n_steps, int n_slots,
                   float* z_vals, float* z_stop, int* truncated, void* stream) {
    return march_entry(__func__, MARCH_PLAIN, grid, nullptr, 0.0f, rays, ray_stride, u, n_rays, 0.0f, n_steps, n_slots, 0, 0.0f, z_vals, z_stop,
                       truncated, nullptr, nullptr, stream);
}

int nerf_occ_march_stop(const NerfOccGrid* grid, const float* density, float outside_sigma, const float* rays, int ray_stride, const float* u,
                        int n_rays, int n_steps, int n_slots, float tau, float* z_vals, float* z_stop, int* truncated, int* stopped,
                        void* stream) {
    return march_entry(__func__, MARCH_STOP, grid, density, outside_sigma, rays, ray_stride, u, n_rays, 0.0f, n_steps, n_slots, 0, tau, z_vals,
                       z_stop, truncated, nullptr, stopped, stream);
}

int nerf_occ_march_step(const NerfOccGrid* grid, const float* density, float outside_sigma, const float* rays, int ray_stride, const float* u,
                        int n_rays, float step_size, int n_steps, int n_slots, int fit, float tau, float* z_vals, float* z_stop,
                        int* truncated, int* level, int* stopped, void* stream) {
    return march_entry(__func__, MARCH_STEP, grid, density, outside_sigma, rays, ray_stride, u, n_rays, step_size, n_steps, n_slots, fit, tau,
                       z_vals, z_stop, truncated, level, stopped, stream);
}

int nerf_occ_expand(const int* slot, const float* raw_c, long n_points, float* raw, void* stream) {
    REQUIRE(slot && raw_c && raw, "null pointer");
    REQUIRE(n_points >= 0 && n_points < (1L << 31), "bad size");
    REQUIRE(((reinterpret_cast<uintptr_t>(raw_c) | reinterpret_cast<uintptr_t>(raw)) & 15) == 0, "raw_c and raw must be 16-byte aligned");
    if (n_points == 0) return 0;
    occ_expand_kernel<<<(unsigned)((n_points + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        slot, reinterpret_cast<const float4*>(raw_c), n_points, reinterpret_cast<float4*>(raw));
    return done(__func__, hipGetLastError());
}

int nerf_occ_mark(const float* sigma, long n_cells, int samples_per_cell, float threshold, unsigned* words, void* stream) {
    REQUIRE(sigma && words, "null pointer");
    REQUIRE(n_cells >= 0 && n_cells <= 512L * 512 * 512 && samples_per_cell >= 1, "bad size");
    if (n_cells == 0) return 0;
    occ_mark_kernel<<<(unsigned)((n_cells + 255) / 256), 256, 0, (hipStream_t)stream>>>(sigma, n_cells, samples_per_cell, threshold, words);
    return done(__func__, hipGetLastError());
}

int nerf_occ_dilate(const unsigned* bits_in, int rx, int ry, int rz, unsigned* bits_out, void* stream) {
    REQUIRE(bits_in && bits_out, "null pointer");
    REQUIRE(bits_in != bits_out, "the dilation is not in place: bits_out must be a second buffer");
    REQUIRE(rx >= 1 && rx <= 512 && ry >= 1 && ry <= 512 && rz >= 1 && rz <= 512, "grid resolution must be 1..512 per axis");
    const long n_cells = (long)rx * ry * rz;
    occ_dilate_kernel<<<(unsigned)((n_cells + 255) / 256), 256, 0, (hipStream_t)stream>>>(bits_in, rx, ry, rz, bits_out);
    return done(__func__, hipGetLastError());
}

int nerf_occ_gather(const int* slot, const float* d_raw, long n_points, float* d_raw_c, void* stream) {
    REQUIRE(slot && d_raw && d_raw_c, "null pointer");
    REQUIRE(n_points >= 0 && n_points < (1L << 31), "bad size");
    REQUIRE(((reinterpret_cast<uintptr_t>(d_raw) | reinterpret_cast<uintptr_t>(d_raw_c)) & 15) == 0, "d_raw and d_raw_c must be 16-byte aligned");
    if (n_points == 0) return 0;
    occ_gather_kernel<<<(unsigned)((n_points + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        slot, reinterpret_cast<const float4*>(d_raw), n_points, reinterpret_cast<float4*>(d_raw_c));
    return done(__func__, hipGetLastError());
}

int nerf_occ_fold_rays(const int* slot, const float* z_vals, const float* d_rec, int n_rays, int n_samples, float* d_rays, int accumulate,
                       void* stream) {
    REQUIRE(slot && z_vals && d_rec && d_rays, "null pointer");
    REQUIRE(n_rays >= 0 && n_samples >= 1 && (long)n_rays * n_samples < (1L << 31), "bad size");
    if (n_rays == 0) return 0;
    occ_fold_rays_kernel<<<(unsigned)((n_rays + FOLD_RAYS - 1) / FOLD_RAYS), FOLD_THREADS, 0, (hipStream_t)stream>>>(
        slot, z_vals, d_rec, n_rays, n_samples, d_rays, accumulate != 0);
    return done(__func__, hipGetLastError());
}

int nerf_occ_density_update(const float* sigma, long n_cells, int samples_per_cell, float decay, float* density, void* stream) {
    REQUIRE(sigma && density, "null pointer");
    REQUIRE(n_cells >= 0 && n_cells <= 512L * 512 * 512 && samples_per_cell >= 1, "bad size");
    if (n_cells == 0) return 0;
    occ_density_update_kernel<<<(unsigned)((n_cells + 255) / 256), 256, 0, (hipStream_t)stream>>>(sigma, n_cells, samples_per_cell, decay, density);
    return done(__func__, hipGetLastError());
}

int nerf_occ_ray_span(const NerfOccGrid* grid, const float* rays, int ray_stride, int n_rays, float* span, int* hit, void* stream) {
    GridArgs g;
    if (int rc = check_grid(__func__, grid, &g)) return rc;
    REQUIRE(rays && span && hit, "null pointer");
    REQUIRE(ray_stride >= 8 && n_rays >= 0 && n_rays < (1 << 30), "bad size (ray records need 8 columns)");
    REQUIRE((reinterpret_cast<uintptr_t>(span) & 7) == 0, "span must be 8-byte aligned");
    if (n_rays == 0) return 0;
    const unsigned lanes = 2u * (unsigned)n_rays;
    occ_ray_span_kernel<<<(lanes + SPAN_THREADS - 1) / SPAN_THREADS, SPAN_THREADS, 0, (hipStream_t)stream>>>(g, rays, ray_stride, n_rays, span, hit);
    return done(__func__, hipGetLastError());
}

int nerf_occ_view_carve(const NerfOccGrid* grid, const float width[3], const float* cams, int n_views, int H, int W, float near_m,
                        float far_m, float margin_px, const int* sat, int accumulate, int* seen, unsigned* carved_words, void* stream) {
    REQUIRE(grid && width && cams && seen, "null pointer");        // (grid->bits is not read: the cells are projected, not looked up)
    REQUIRE((sat != nullptr) == (carved_words != nullptr), "null pointer (sat and carved_words come together: with masks, or neither)");
    REQUIRE(n_views >= 1 && H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "bad size (at least one view, images of 1..16384 pixels a side)");
    REQUIRE(margin_px >= 0.0f && margin_px < INFINITY, "bad margin_px (finite and >= 0)");      // (a NaN fails the comparison)
    CarveArgs a;
    for (int k = 0; k < 3; ++k) {
        REQUIRE(grid->res[k] >= 1 && grid->res[k] <= 512, "grid resolution must be 1..512 per axis");
        a.lo[k] = grid->lo[k];
        a.width[k] = width[k];
        a.res[k] = grid->res[k];
    }
    a.cams = cams; a.n_views = n_views; a.H = H; a.W = W;
    a.near_m = near_m; a.far_m = far_m; a.m = margin_px;
    a.sat = sat; a.accumulate = accumulate != 0; a.seen = seen; a.carved = carved_words;
    const long n_cells = (long)a.res[0] * a.res[1] * a.res[2];
    occ_view_carve_kernel<<<(unsigned)((n_cells + CARVE_THREADS - 1) / CARVE_THREADS), CARVE_THREADS, 0, (hipStream_t)stream>>>(a);
    return done(__func__, hipGetLastError());
}

int nerf_occ_proposal_weights(const NerfOccGrid* grid, const float* density, float outside_sigma, const float* rays, int ray_stride,
                              const float* z_vals, int n_rays, int n_samples, float* weights, float* sigma, void* stream) {
    GridArgs g;
    if (int rc = check_grid(__func__, grid, &g)) return rc;
    REQUIRE(density && rays && z_vals && weights, "null pointer");
    REQUIRE(ray_stride >= 6 && n_rays >= 0 && n_samples >= 1 && n_samples <= 4096, "bad size (ray records need 6 columns, 1..4096 samples)");
    if (n_rays == 0) return 0;
    occ_proposal_weights_kernel<<<(unsigned)n_rays, 64, 2 * (size_t)n_samples * sizeof(float), (hipStream_t)stream>>>(
        g, density, outside_sigma, rays, ray_stride, z_vals, n_samples, weights, sigma);
    return done(__func__, hipGetLastError());
}

}  // extern "C"
