// Fine-tuning a baked field: the render of baked.hip with a deterministic backward to the table's rows (include/nerf_hip.h, section
// "baked field, training"; baked.BakedTrainer; BakedTrainer.render_rays_reference is the definition).  Four entry points:
//   nerf_baked_count             : per ray the number of kept candidates -- the walk of nerf_baked_render without the table (the same
//                                  functions of baked_device.h, so the kept set is the render's bit for bit; never a stop).
//   nerf_baked_train_fwd         : the render with stop_eps = 0 (baked_device.h: the bits of nerf_baked_render), which also writes one
//                                  record per kept sample at offsets[ray] + its rank among the ray's kept samples.  The rank is the count
//                                  of the rounds before plus the popcount of the keep ballot below the lane: no atomic decides a position,
//                                  the records are ray-major and sample-minor.
//   nerf_baked_train_bwd_samples : one wavefront per ray over its records BACK TO FRONT in rounds of 64: S_k = sum_{j > k} q_j w_j is a
//                                  wave suffix scan (summed directly: ray_device.h, wave_incl_scan_add_rev) plus the suffix carried from
//                                  the rounds behind, never a total minus a prefix.  Writes (dL/dv0, dL/dl_R, dL/dl_G, dL/dl_B) per sample.
//   nerf_baked_train_bwd_rows    : the per-destination sum.  A group of W lanes owns one stored row, lane = column: a lane adds its
//                                  column's terms one after the other -- the row's adjacent cells in corner order 000 001 .. 111, each
//                                  cell's samples in the order of the inverted index (ascending (ray, k)) --, weight x contribution, one
//                                  product and one addition per term, and stores the column.  The sum has three levels in that same
//                                  order (a ray's run inside a cell, the cell, the row), so a row that hundreds of samples reach
//                                  rounds like a short sum.  No lane ever adds into another's sum, so the order of summation is the
//                                  order written here and two launches give the same bits.
// A record is 12 words (48 bytes, three 16-byte stores): cell, ray (int32), fx, fy, fz, z, e = expf(-sigma ds), T, c_R, c_G, c_B, gate
// (1.0 where the blended v0 >= 0: torch.clamp(min=0)'s gate, else 0.0).  alpha = 1 - e and t = 1 - alpha + 1e-10 are recomputed from e
// with the forward's expressions, so they are the forward's bits, and d alpha / d sigma = ds e keeps its relative precision where alpha
// is near 1.  No atomics, no LDS, plain loads and stores; every index read from memory is checked against the buffer it addresses.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "api_util.h"
#include "baked_device.h"

using namespace nerf_api;
using namespace nerf_grid;
using namespace nerf_baked;

namespace {

constexpr int REC_WORDS = 12;                   // words per sample record
constexpr int MAX_SAMPLES = 1 << 30;            // records and inverted-index entries are addressed with 32-bit ints
constexpr int MAX_ROWS = 1 << 26;               // n_rows * W threads fit the launch

typedef float float4_t __attribute__((ext_vector_type(4)));

struct WalkArgs {
    const float* rays;
    int ray_stride;
    const float* u;             // one offset per ray, or null: 0.5
    int n_rays;
    float ds;
    int M;
};

__global__ __launch_bounds__(BAKED_THREADS) void baked_count_kernel(GridArgs g, WalkArgs a, int* counts) {
    const int ray = blockIdx.x * BAKED_RAYS + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;        // (whole waves leave: the ballots below see full waves)
    const int lane = threadIdx.x & 63;
    RaySetup rs;
    const bool ok = ray_setup(a.rays + (size_t)ray * a.ray_stride, a.ds, &rs);
    int count = 0;
    if (ok) {
        const float uu = a.u ? a.u[ray] : 0.5f;
        for (int k0 = 0; k0 < a.M; k0 += 64) {
            const Candidate cd = candidate(g, rs, uu, k0 + lane, a.M);
            const unsigned long long vm = __ballot(cd.valid);
            if (!(vm & 1ull)) break;
            count += __popcll(__ballot(cd.keep));
            if (!((vm >> 63) & 1ull)) break;    // the valid candidates are a prefix: this round was the last
        }
    }
    if (lane == 0) counts[ray] = count;
}

struct FwdArgs {
    const int* node_index;
    const _Float16* table;
    unsigned n_rows;
    int white_bkgd;
    const int* offsets;         // [n_rays + 1]: the first record of every ray
    int total;                  // records in the buffer
    float* records;
    float* rgb;
    float* acc;
    float* depth;
};

template <int DEG>
__global__ __launch_bounds__(BAKED_THREADS) void baked_train_fwd_kernel(GridArgs g, WalkArgs a, FwdArgs f) {
    constexpr int B = RowOf<DEG>::B;
    const int ray = blockIdx.x * BAKED_RAYS + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;
    const int lane = threadIdx.x & 63;
    const float* ray_in = a.rays + (size_t)ray * a.ray_stride;
    RaySetup rs;
    const bool ok = ray_setup(ray_in, a.ds, &rs);
    float Y[B];
    sh_basis<DEG>(ray_in[8], ray_in[9], ray_in[10], Y);
    RayIntegrals A;
    int count = 0;
    if (ok) {
        const float uu = a.u ? a.u[ray] : 0.5f;
        const int ny = g.res[1] + 1, nz = g.res[2] + 1;     // nodes per axis
        const int first = f.offsets[ray];
        for (int k0 = 0; k0 < a.M; k0 += 64) {
            const Candidate cd = candidate(g, rs, uu, k0 + lane, a.M);
            const unsigned long long vm = __ballot(cd.valid);
            if (!(vm & 1ull)) break;
            const unsigned long long km = __ballot(cd.keep);
            if (km) {
                Sample sm;
                sm.fx = sm.fy = sm.fz = sm.v0 = sm.e = 0.0f;
                sm.alpha = 0.0f; sm.t1 = 1.0f; sm.c0 = sm.c1 = sm.c2 = 0.0f;
                if (cd.keep) sm = sample_value<DEG>(f.node_index, f.table, f.n_rows, ny, nz, cd, Y, a.ds);
                const float T = composite_round(A, sm.alpha, sm.t1, sm.c0, sm.c1, sm.c2, cd.keep, cd.z, lane);
                const int pos = first + count + __popcll(km & ((1ull << lane) - 1ull));
                if (cd.keep && pos >= 0 && pos < f.total) {         // (the offsets are the count kernel's: the check never fails then)
                    float4_t* rec = reinterpret_cast<float4_t*>(f.records + (size_t)pos * REC_WORDS);
                    float4_t r0, r1, r2;
                    r0.x = __int_as_float((int)cell_index(g, cd.ix, cd.iy, cd.iz)); r0.y = __int_as_float(ray); r0.z = sm.fx; r0.w = sm.fy;
                    r1.x = sm.fz; r1.y = cd.z; r1.z = sm.e; r1.w = T;
                    r2.x = sm.c0; r2.y = sm.c1; r2.z = sm.c2; r2.w = sm.v0 >= 0.0f ? 1.0f : 0.0f;
                    rec[0] = r0; rec[1] = r1; rec[2] = r2;
                }
                count += __popcll(km);
            }
            if (!((vm >> 63) & 1ull)) break;
        }
    }
    if (lane == 0) {
        const float bg = f.white_bkgd ? 1.0f - A.acc : 0.0f;
        f.rgb[(size_t)ray * 3] = A.r + bg; f.rgb[(size_t)ray * 3 + 1] = A.g + bg; f.rgb[(size_t)ray * 3 + 2] = A.b + bg;
        f.acc[ray] = A.acc;
        f.depth[ray] = A.depth;
    }
}

struct SamplesArgs {
    const float* records;
    const int* offsets;
    int n_rays;
    int total;
    float ds;
    int white_bkgd;
    const float* g_rgb;
    const float* g_acc;
    const float* g_depth;
    float* sample_grads;        // [total][4]
};

__global__ __launch_bounds__(BAKED_THREADS) void baked_train_bwd_samples_kernel(SamplesArgs a) {
    const int ray = blockIdx.x * BAKED_RAYS + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;
    const int lane = threadIdx.x & 63;
    const int first = max(a.offsets[ray], 0);
    const int n = min(a.offsets[ray + 1], a.total) - first;
    if (n <= 0) return;                 // (wave-uniform)
    const float G0 = a.g_rgb[(size_t)ray * 3], G1 = a.g_rgb[(size_t)ray * 3 + 1], G2 = a.g_rgb[(size_t)ray * 3 + 2];
    const float ga = a.white_bkgd ? a.g_acc[ray] - ((G0 + G1) + G2) : a.g_acc[ray];       // rgb_map = sum w c + 1 - acc
    const float gd = a.g_depth[ray];
    float carry = 0.0f;                 // sum of q w over the rounds behind this one
    for (int i0 = ((n - 1) >> 6) << 6; i0 >= 0; i0 -= 64) {
        const int i = i0 + lane;
        const bool act = i < n;
        float4_t r1 = {0.0f, 0.0f, 1.0f, 0.0f}, r2 = {0.0f, 0.0f, 0.0f, 0.0f};
        if (act) {
            const float4_t* rec = reinterpret_cast<const float4_t*>(a.records + (size_t)(first + i) * REC_WORDS);
            r1 = rec[1]; r2 = rec[2];
        }
        const float z = r1.y, e = r1.z, T = r1.w, c0 = r2.x, c1 = r2.y, c2 = r2.z;
        const float alpha = 1.0f - e;                   // the forward's bits
        const float t = 1.0f - alpha + 1e-10f;
        const float w = alpha * T;
        const float q = ((G0 * c0 + G1 * c1) + G2 * c2) + ga + gd * z;
        const float x = act ? q * w : 0.0f;
        const float incl = nerf::wave_incl_scan_add_rev(x, lane);
        float behind = __shfl_down(incl, 1);
        if (lane == 63) behind = 0.0f;
        const float S = behind + carry;
        carry = carry + __shfl(incl, 0);
        if (act) {
            const float dalpha = q * T - S / t;
            float4_t out;
            out.x = r2.w != 0.0f ? dalpha * (a.ds * e) : 0.0f;          // d alpha / d sigma = ds exp(-sigma ds), behind the clamp's gate
            out.y = w * G0 * (c0 * (1.0f - c0));
            out.z = w * G1 * (c1 * (1.0f - c1));
            out.w = w * G2 * (c2 * (1.0f - c2));
            reinterpret_cast<float4_t*>(a.sample_grads)[(size_t)(first + i)] = out;
        }
    }
}

struct RowsArgs {
    const int* row_node;        // [n_rows]: the lattice node of a row, -1 for row 0
    int n_rows;
    const float* rays;
    int ray_stride;
    int n_rays;
    const float* records;
    const float* sample_grads;
    const int* order;           // [total]: the samples sorted by cell, stable
    const int* cell_start;      // [cells + 1]: the first entry of every cell in order
    int total;
    float* grad;                // [n_rows][W]
};

template <int DEG>
__global__ __launch_bounds__(BAKED_THREADS) void baked_train_bwd_rows_kernel(GridArgs g, RowsArgs a) {
    constexpr int B = RowOf<DEG>::B, V = RowOf<DEG>::V, W = RowOf<DEG>::W;
    const long long gid = (long long)blockIdx.x * BAKED_THREADS + threadIdx.x;
    const int row = (int)(gid / W), col = (int)(gid % W);
    if (row >= a.n_rows) return;
    const int nx = g.res[0] + 1, ny = g.res[1] + 1, nz = g.res[2] + 1;
    const int node = a.row_node[row];
    float sum = 0.0f;
    if (col < V && node >= 0 && node < nx * ny * nz) {
        const int k = node % nz, j = (node / nz) % ny, i = node / (nz * ny);
        const int ch = col == 0 ? -1 : (col - 1) / B, b = col == 0 ? 0 : (col - 1) % B;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int ox = (c >> 2) & 1, oy = (c >> 1) & 1, oz = c & 1;         // the node is corner (ox, oy, oz) of cell (i - ox, j - oy, k - oz)
            const int ci = i - ox, cj = j - oy, ck = k - oz;
            if (ci < 0 || ci >= g.res[0] || cj < 0 || cj >= g.res[1] || ck < 0 || ck >= g.res[2]) continue;
            const unsigned cell = cell_index(g, ci, cj, ck);
            const int s0 = max(a.cell_start[cell], 0), s1 = min(a.cell_start[cell + 1], a.total);
            // three levels, each in the order written: a ray's run of samples in the cell, the cell's runs, the row's cells -- a
            // running sum never grows past its own level, which keeps the rounding of a heavily sampled row near a short sum's
            float cell_sum = 0.0f, run_sum = 0.0f;
            unsigned run_ray = 0xffffffffu;
            for (int s = s0; s < s1; ++s) {
                const unsigned id = (unsigned)a.order[s];
                if (id >= (unsigned)a.total) continue;
                const float4_t* rec = reinterpret_cast<const float4_t*>(a.records + (size_t)id * REC_WORDS);
                const float4_t r0 = rec[0];
                const float fx = r0.z, fy = r0.w, fz = a.records[(size_t)id * REC_WORDS + 4];
                const float4_t gs = reinterpret_cast<const float4_t*>(a.sample_grads)[id];
                const float w = (ox ? fx : 1.0f - fx) * (oy ? fy : 1.0f - fy) * (oz ? fz : 1.0f - fz);
                const unsigned r = (unsigned)__float_as_int(r0.y);
                if (r != run_ray) {             // the ray's run is over: it joins the cell's sum
                    cell_sum = cell_sum + run_sum;
                    run_sum = 0.0f;
                    run_ray = r;
                }
                float term = gs.x;
                if (ch >= 0) {
                    float Y[B];
                    if (DEG > 0 && r < (unsigned)a.n_rays) {
                        const float* vd = a.rays + (size_t)r * a.ray_stride + 8;
                        sh_basis<DEG>(vd[0], vd[1], vd[2], Y);
                    } else {
                        sh_basis<0>(0.0f, 0.0f, 0.0f, Y);
#pragma unroll
                        for (int q = 1; q < B; ++q) Y[q] = 0.0f;
                    }
                    float y = Y[0];
#pragma unroll
                    for (int q = 1; q < B; ++q) y = b == q ? Y[q] : y;         // (static indices: Y stays in registers)
                    term = (ch == 0 ? gs.y : (ch == 1 ? gs.z : gs.w)) * y;
                }
                run_sum = run_sum + w * term;
            }
            sum = sum + (cell_sum + run_sum);
        }
    }
    a.grad[(size_t)row * W + col] = sum;        // (row 0, rows without a node and the padding columns: zeros)
}

}  // namespace

#define REQUIRE_WALK() do { \
    REQUIRE(ray_stride >= 11 && n_rays >= 0, "bad size (ray records need 11 columns)"); \
    REQUIRE(step_size > 0.0f && step_size < INFINITY, "bad step_size (finite and > 0)"); \
    REQUIRE(max_steps >= 1 && max_steps <= (1 << 24), "bad max_steps (1..2^24: a candidate's number is exact in fp32)"); } while (0)

extern "C" {

int nerf_baked_count(const NerfOccGrid* grid, const float* rays, int ray_stride, const float* u, int n_rays, float step_size, int max_steps,
                     int* counts, void* stream) {
    GridArgs g;
    if (int rc = check_grid(__func__, grid, &g)) return rc;
    REQUIRE(rays && counts, "null pointer");
    REQUIRE_WALK();
    if (n_rays == 0) return 0;
    const WalkArgs a{rays, ray_stride, u, n_rays, step_size, max_steps};
    const unsigned blocks = (unsigned)((n_rays + BAKED_RAYS - 1) / BAKED_RAYS);
    baked_count_kernel<<<blocks, BAKED_THREADS, 0, (hipStream_t)stream>>>(g, a, counts);
    return done(__func__, hipGetLastError());
}

int nerf_baked_train_fwd(const NerfOccGrid* grid, const int* node_index, const void* table, int n_rows, int sh_degree, const float* rays,
                         int ray_stride, const float* u, int n_rays, float step_size, int max_steps, int white_bkgd, const int* offsets,
                         int total, float* records, float* rgb_map, float* acc_map, float* depth_map, void* stream) {
    GridArgs g;
    if (int rc = check_grid(__func__, grid, &g)) return rc;
    REQUIRE(node_index && table && rays && offsets && records && rgb_map && acc_map && depth_map, "null pointer");
    REQUIRE(sh_degree >= 0 && sh_degree <= 2, "bad sh_degree (0, 1 or 2)");
    REQUIRE_WALK();
    REQUIRE(n_rows >= 1, "bad n_rows (row 0, the zero row, is always there)");
    REQUIRE(total >= 0 && total <= MAX_SAMPLES, "bad total (0..2^30 samples)");
    REQUIRE(aligned16(table), "table must be 16-byte aligned");
    REQUIRE(aligned16(records), "records must be 16-byte aligned");
    if (n_rays == 0) return 0;
    const WalkArgs a{rays, ray_stride, u, n_rays, step_size, max_steps};
    FwdArgs f;
    f.node_index = node_index; f.table = static_cast<const _Float16*>(table); f.n_rows = (unsigned)n_rows; f.white_bkgd = white_bkgd != 0;
    f.offsets = offsets; f.total = total; f.records = records; f.rgb = rgb_map; f.acc = acc_map; f.depth = depth_map;
    const unsigned blocks = (unsigned)((n_rays + BAKED_RAYS - 1) / BAKED_RAYS);
    hipStream_t st = (hipStream_t)stream;
    if (sh_degree == 0) baked_train_fwd_kernel<0><<<blocks, BAKED_THREADS, 0, st>>>(g, a, f);
    else if (sh_degree == 1) baked_train_fwd_kernel<1><<<blocks, BAKED_THREADS, 0, st>>>(g, a, f);
    else baked_train_fwd_kernel<2><<<blocks, BAKED_THREADS, 0, st>>>(g, a, f);
    return done(__func__, hipGetLastError());
}

int nerf_baked_train_bwd_samples(const float* records, const int* offsets, int n_rays, int total, float step_size, int white_bkgd,
                                 const float* g_rgb, const float* g_acc, const float* g_depth, float* sample_grads, void* stream) {
    REQUIRE(records && offsets && g_rgb && g_acc && g_depth && sample_grads, "null pointer");
    REQUIRE(n_rays >= 0, "bad size (n_rays >= 0)");
    REQUIRE(total >= 0 && total <= MAX_SAMPLES, "bad total (0..2^30 samples)");
    REQUIRE(step_size > 0.0f && step_size < INFINITY, "bad step_size (finite and > 0)");
    REQUIRE(aligned16(records, sample_grads), "records and sample_grads must be 16-byte aligned");
    if (n_rays == 0 || total == 0) return 0;
    SamplesArgs a;
    a.records = records; a.offsets = offsets; a.n_rays = n_rays; a.total = total; a.ds = step_size; a.white_bkgd = white_bkgd != 0;
    a.g_rgb = g_rgb; a.g_acc = g_acc; a.g_depth = g_depth; a.sample_grads = sample_grads;
    const unsigned blocks = (unsigned)((n_rays + BAKED_RAYS - 1) / BAKED_RAYS);
    baked_train_bwd_samples_kernel<<<blocks, BAKED_THREADS, 0, (hipStream_t)stream>>>(a);
    return done(__func__, hipGetLastError());
}

int nerf_baked_train_bwd_rows(const NerfOccGrid* grid, const int* row_node, int n_rows, int sh_degree, const float* rays, int ray_stride,
                              int n_rays, const float* records, const float* sample_grads, const int* order, const int* cell_start, int total,
                              float* grad, void* stream) {
    GridArgs g;
    if (int rc = check_grid(__func__, grid, &g)) return rc;
    REQUIRE(row_node && (rays || n_rays == 0) && records && sample_grads && order && cell_start && grad, "null pointer");     // (no rays: no ray buffer)
    REQUIRE(sh_degree >= 0 && sh_degree <= 2, "bad sh_degree (0, 1 or 2)");
    REQUIRE(ray_stride >= 11 && n_rays >= 0, "bad size (ray records need 11 columns)");
    REQUIRE(n_rows >= 1 && n_rows <= MAX_ROWS, "bad n_rows (1..2^26: row 0, the zero row, is always there)");
    REQUIRE(total >= 0 && total <= MAX_SAMPLES, "bad total (0..2^30 samples)");
    REQUIRE(aligned16(records, sample_grads), "records and sample_grads must be 16-byte aligned");
    const int W = sh_degree == 0 ? RowOf<0>::W : (sh_degree == 1 ? RowOf<1>::W : RowOf<2>::W);
    hipStream_t st = (hipStream_t)stream;
    if (n_rays == 0 || total == 0)      // nothing was sampled: the gradient is zero
        return done(__func__, hipMemsetAsync(grad, 0, (size_t)n_rows * W * sizeof(float), st));
    RowsArgs a;
    a.row_node = row_node; a.n_rows = n_rows; a.rays = rays; a.ray_stride = ray_stride; a.n_rays = n_rays; a.records = records;
    a.sample_grads = sample_grads; a.order = order; a.cell_start = cell_start; a.total = total; a.grad = grad;
    const unsigned blocks = (unsigned)(((long long)n_rows * W + BAKED_THREADS - 1) / BAKED_THREADS);
    if (sh_degree == 0) baked_train_bwd_rows_kernel<0><<<blocks, BAKED_THREADS, 0, st>>>(g, a);
    else if (sh_degree == 1) baked_train_bwd_rows_kernel<1><<<blocks, BAKED_THREADS, 0, st>>>(g, a);
    else baked_train_bwd_rows_kernel<2><<<blocks, BAKED_THREADS, 0, st>>>(g, a);
    return done(__func__, hipGetLastError());
}

}  // extern "C"
