// The gradient of the baked training render with respect to its rays (include/nerf_hip.h, section "baked field, training";
// baked.BakedTrainer.render_rays(ray_grad=True); BakedTrainer.render_rays_reference(ray_grad=True) is the definition, DESIGN.md 3.26 the
// closed form).  One entry point:
//   nerf_baked_train_bwd_rays : d_rays [n_rays][11] from the records of nerf_baked_train_fwd and the sample gradients of
//                               nerf_baked_train_bwd_samples.  The depths z are constants: a sample's position x = o + d z moves with o
//                               and d only, the colour with the view direction through the SH basis.
// One wavefront per ray, lane = record, rounds of 64 over offsets[ray] .. offsets[ray + 1].  Per record, with a_0 = dL/dv0 (gated) and
// g_c = dL/dl_c, for the eight corner rows of the sample's cell in corner order 000 001 .. 111 (x the slowest bit):
//   m_q[b]  = (g_R row_q[1 + b] + g_G row_q[1 + B + b]) + g_B row_q[1 + 2B + b]                   b = 0 .. B - 1
//   r_q     = a_0 row_q[0] + m_q[0] Y_0 + m_q[1] Y_1 + ..                                          added left to right
//   dL/df_x = sum_q (q_x ? + : -) (w_y w_z)_q r_q, likewise y and z                                q ascending
//   dL/dY_b = sum_q ((w_x w_y) w_z)_q m_q[b]                                                       q ascending
//   dL/dx   = scale * dL/df;  the record adds dL/dx to d_o, z dL/dx to d_d and (dY/dviewdir)^T dL/dY to d_viewdir.
// THE ORDER OF SUMMATION.  A lane keeps nine accumulators (d_o, d_d, d_viewdir) and adds its records' terms in ascending round order:
// lane l sums the records l, l + 64, l + 128, .. of the ray, one addition per record.  Then one xor butterfly over the 64 lanes,
// partners at distance 32, 16, 8, 4, 2, 1 in turn, finishes each of the nine sums (lanes without a record hold 0); lane 0 stores them.
// No lane's sum depends on timing, so the same inputs give the same bits.  Templated on the degree: all indexing is static -- no scratch,
// no LDS, no atomics.  Every index read from memory (offsets, a record's cell, a node's row) is checked against the buffer it addresses:
// a record whose cell does not exist adds nothing, a row outside the table reads row 0.  Rays without records (misses, invalid rays)
// and the columns 6 and 7 (near, far) are written as zeros.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "api_util.h"
#include "baked_device.h"

using namespace nerf_api;
using namespace nerf_grid;
using namespace nerf_baked;

namespace {

constexpr int REC_WORDS = 12;                   // words per sample record (baked_train.hip)
constexpr int MAX_SAMPLES = 1 << 30;            // records are addressed with 32-bit ints
constexpr int RAY_COLS = 11;                    // columns of d_rays

typedef float float4_t __attribute__((ext_vector_type(4)));

struct RaysArgs {
    const int* node_index;
    const _Float16* table;
    unsigned n_rows;
    const float* rays;
    int ray_stride;
    int n_rays;
    const float* records;
    const float* sample_grads;  // [total][4]
    const int* offsets;         // [n_rays + 1]
    int total;
    float* d_rays;              // [n_rays][11]
};

// v[0 .. V) = row[0 .. V) as fp32: the 16-byte loads of add_row
template <int DEG>
__device__ __forceinline__ void load_row(const _Float16* __restrict__ row, float* v) {
    constexpr int V = RowOf<DEG>::V;
    if (DEG == 0) {
        const half4_t h = *reinterpret_cast<const half4_t*>(row);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (float)h[j];
    } else {
#pragma unroll
        for (int q = 0; q < RowOf<DEG>::W / 8; ++q) {
            const half8_t h = *reinterpret_cast<const half8_t*>(row + 8 * q);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (8 * q + j < V) v[8 * q + j] = (float)h[j];
        }
    }
}

// (dL/dviewdir) = (dY/dviewdir)^T dL/dY: the derivative of sh_basis' polynomials at (x, y, z), added in ascending b
template <int DEG>
__device__ __forceinline__ void sh_basis_bwd(float x, float y, float z, const float* dY, float* dv) {
    dv[0] = dv[1] = dv[2] = 0.0f;
    if (DEG >= 1) {
        dv[1] = -0.4886025119029199f * dY[1];
        dv[2] = 0.4886025119029199f * dY[2];
        dv[0] = -0.4886025119029199f * dY[3];
    }
    if (DEG >= 2) {
        const float c2 = 1.0925484305920792f, c3 = 0.31539156525252005f, c4 = 0.5462742152960396f;
        dv[0] = dv[0] + (c2 * y) * dY[4];           dv[1] = dv[1] + (c2 * x) * dY[4];
        dv[1] = dv[1] - (c2 * z) * dY[5];           dv[2] = dv[2] - (c2 * y) * dY[5];
        dv[0] = dv[0] - (2.0f * c3 * x) * dY[6];    dv[1] = dv[1] - (2.0f * c3 * y) * dY[6];    dv[2] = dv[2] + (4.0f * c3 * z) * dY[6];
        dv[0] = dv[0] - (c2 * z) * dY[7];           dv[2] = dv[2] - (c2 * x) * dY[7];
        dv[0] = dv[0] + (2.0f * c4 * x) * dY[8];    dv[1] = dv[1] - (2.0f * c4 * y) * dY[8];
    }
}

__device__ __forceinline__ float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

template <int DEG>
__global__ __launch_bounds__(BAKED_THREADS) void baked_train_bwd_rays_kernel(GridArgs g, RaysArgs a) {
    constexpr int B = RowOf<DEG>::B, V = RowOf<DEG>::V, W = RowOf<DEG>::W;
    const int ray = blockIdx.x * BAKED_RAYS + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;        // (whole waves leave: the butterfly below sees full waves)
    const int lane = threadIdx.x & 63;
    const int first = __builtin_amdgcn_readfirstlane(max(a.offsets[ray], 0));
    const int n = __builtin_amdgcn_readfirstlane(min(a.offsets[ray + 1], a.total)) - first;
    float acc[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) acc[c] = 0.0f;
    if (n > 0) {                        // (wave-uniform)
        const float* ray_in = a.rays + (size_t)ray * a.ray_stride;
        const float vx = uniform(ray_in[8]), vy = uniform(ray_in[9]), vz = uniform(ray_in[10]);
        float Y[B];
        sh_basis<DEG>(vx, vy, vz, Y);
        const unsigned ry = (unsigned)g.res[1], rz = (unsigned)g.res[2];
        const unsigned n_cells = (unsigned)g.res[0] * ry * rz;          // (at most 512^3)
        const unsigned ny = ry + 1u, nz = rz + 1u;                      // nodes per axis
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            if (i >= n) continue;
            const size_t id = (size_t)(first + i);
            const float4_t* rec = reinterpret_cast<const float4_t*>(a.records + id * REC_WORDS);
            const float4_t r0 = rec[0], r1 = rec[1];
            const float4_t gs = reinterpret_cast<const float4_t*>(a.sample_grads)[id];
            const unsigned cell = (unsigned)__float_as_int(r0.x);
            if (cell >= n_cells) continue;
            const unsigned iz = cell % rz, iy = (cell / rz) % ry, ix = cell / (rz * ry);
            const float fx = r0.z, fy = r0.w, fz = r1.x, z = r1.y;
            const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy}, wz[2] = {1.0f - fz, fz};
            const unsigned n0 = (ix * ny + iy) * nz + iz;
            float df[3] = {0.0f, 0.0f, 0.0f};
            float dY[B];
#pragma unroll
            for (int b = 0; b < B; ++b) dY[b] = 0.0f;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int qx = (q >> 2) & 1, qy = (q >> 1) & 1, qz = q & 1;
                const unsigned node = n0 + ((unsigned)qx * ny + (unsigned)qy) * nz + (unsigned)qz;
                const unsigned idx = (unsigned)a.node_index[node];
                const unsigned row = idx < a.n_rows ? idx : 0u;
                float v[V];
                load_row<DEG>(a.table + (size_t)row * W, v);
                float r = gs.x * v[0];
                const float wq = wx[qx] * wy[qy] * wz[qz];
#pragma unroll
                for (int b = 0; b < B; ++b) {
                    const float m = (gs.y * v[1 + b] + gs.z * v[1 + B + b]) + gs.w * v[1 + 2 * B + b];
                    r = r + m * Y[b];
                    dY[b] = dY[b] + wq * m;
                }
                const float tx = (wy[qy] * wz[qz]) * r, ty = (wx[qx] * wz[qz]) * r, tz = (wx[qx] * wy[qy]) * r;
                df[0] = qx ? df[0] + tx : df[0] - tx;
                df[1] = qy ? df[1] + ty : df[1] - ty;
                df[2] = qz ? df[2] + tz : df[2] - tz;
            }
            float dv[3];
            sh_basis_bwd<DEG>(vx, vy, vz, dY, dv);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float dx = g.scale[c] * df[c];
                acc[c] = acc[c] + dx;
                acc[3 + c] = acc[3 + c] + z * dx;
                acc[6 + c] = acc[6 + c] + dv[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) acc[c] = nerf::wave_sum(acc[c]);    // partners at distance 32, 16, .. 1
    }
    if (lane == 0) {
        float* out = a.d_rays + (size_t)ray * RAY_COLS;
#pragma unroll
        for (int c = 0; c < 6; ++c) out[c] = acc[c];
        out[6] = 0.0f; out[7] = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[8 + c] = acc[6 + c];
    }
}

}  // namespace

extern "C" {

int nerf_baked_train_bwd_rays(const NerfOccGrid* grid, const int* node_index, const void* table, int n_rows, int sh_degree, const float* rays,
                              int ray_stride, int n_rays, const float* records, const float* sample_grads, const int* offsets, int total,
                              float* d_rays, void* stream) {
    GridArgs g;
    if (int rc = check_grid(__func__, grid, &g)) return rc;
    REQUIRE(node_index && table && rays && records && sample_grads && offsets && d_rays, "null pointer");
    REQUIRE(sh_degree >= 0 && sh_degree <= 2, "bad sh_degree (0, 1 or 2)");
    REQUIRE(ray_stride >= 11 && n_rays >= 0, "bad size (ray records need 11 columns)");
    REQUIRE(n_rows >= 1, "bad n_rows (row 0, the zero row, is always there)");
    REQUIRE(total >= 0 && total <= MAX_SAMPLES, "bad total (0..2^30 samples)");
    REQUIRE(aligned16(table), "table must be 16-byte aligned");
    REQUIRE(aligned16(records, sample_grads), "records and sample_grads must be 16-byte aligned");
    if (n_rays == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (total == 0)                     // nothing was sampled: the gradient is zero
        return done(__func__, hipMemsetAsync(d_rays, 0, (size_t)n_rays * RAY_COLS * sizeof(float), st));
    RaysArgs a;
    a.node_index = node_index; a.table = static_cast<const _Float16*>(table); a.n_rows = (unsigned)n_rows; a.rays = rays;
    a.ray_stride = ray_stride; a.n_rays = n_rays; a.records = records; a.sample_grads = sample_grads; a.offsets = offsets; a.total = total;
    a.d_rays = d_rays;
    const unsigned blocks = (unsigned)((n_rays + BAKED_RAYS - 1) / BAKED_RAYS);
    if (sh_degree == 0) baked_train_bwd_rays_kernel<0><<<blocks, BAKED_THREADS, 0, st>>>(g, a);
    else if (sh_degree == 1) baked_train_bwd_rays_kernel<1><<<blocks, BAKED_THREADS, 0, st>>>(g, a);
    else baked_train_bwd_rays_kernel<2><<<blocks, BAKED_THREADS, 0, st>>>(g, a);
    return done(__func__, hipGetLastError());
}

}  // extern "C"
