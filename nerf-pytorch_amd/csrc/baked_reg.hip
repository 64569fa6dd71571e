// Regularisers of a baked field's fp32 master table (include/nerf_hip.h, section "baked field, regularisers"; baked.BakedTrainer.
// regularizers; baked.regularizer_reference is the definition): a total variation of the density column and of the colour columns over
// the stored lattice nodes, and a Cauchy sparsity term on the density.  Two entry points:
//   nerf_baked_reg_fwd : per stored row the three terms (t[n][0], sum over the colour columns of t[n][c], log1p(2 max(v[n][0], 0)^2)).
//   nerf_baked_reg_bwd : the gradient of  g[0] sum t[.][0] + g[1] sum_c t[.][c] + g[2] sum cauchy  with respect to every row, as a GATHER.
// With D_a[n] = s_a (v[n + e_a] - v[n]) where n + e_a lies in the lattice and is stored (else 0) and t[n] = sqrt(((D_x^2 + D_y^2) + D_z^2)
// + eps):
//   forward  reads 4 rows: n, n + e_x, n + e_y, n + e_z.
//   backward reads 13 rows in the order  n;  n + e_x, n + e_y, n + e_z;  then for a = x, y, z:  m = n - e_a, m + e_b, m + e_c  (b < c the two
//            other axes), and adds a lane's six contributions in that order:
//              - s_x D_x[n] / t[n],  - s_y D_y[n] / t[n],  - s_z D_z[n] / t[n],  + s_x D_x[n - e_x] / t[n - e_x],  + s_y .. ,  + s_z ..
//            (a missing n - e_a adds nothing), times the column's weight, plus the Cauchy slope in column 0.  Every t is recomputed
//            with the forward's expression.
// A wavefront owns 64 consecutive rows and works in two phases.  PHASE 1, one lane per row: the row's node, and the rows of the 3 (forward)
// or 12 (backward) neighbours it needs -- 0 where a neighbour lies outside the lattice or is not stored --, every index read from memory
// checked against the buffer it addresses.  The index arithmetic is done once per row, not once per column.  PHASE 2, W rounds: in
// round `it` a group of W lanes owns row 64 / W * it + (its number in the wave), lane = column (nerf_baked_train_bwd_rows' mapping: a row load is
// one coalesced run of 4 W bytes), fetches that row's indices from the lane that made them (a wave shuffle) and does the arithmetic
// without a branch: a missing neighbour loads row 0 -- allocated, never used -- and a select drops what was computed from it.
// The colour sum of the forward is a butterfly over the group's lanes, partners at distance 1, 2, 4, .. W/2 in turn (lane 0 and the
// padding lanes add 0): one fixed order, the same in every lane.  No atomics, no LDS, no lane adds into another's gradient: the same
// inputs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "api_util.h"
#include "baked_device.h"

using namespace nerf_api;
using namespace nerf_grid;
using namespace nerf_baked;

namespace {

constexpr int MAX_ROWS = 1 << 26;               // a row's number times W floats stays far below 2^63 bytes; one wave per 64 rows
constexpr int WAVE = 64;

struct RegArgs {
    const int* node_index;      // [nodes]: the row of a lattice node, 0: not stored
    const int* row_node;        // [n_rows]: the lattice node of a row, -1 for row 0
    const float* values;        // [n_rows][W], the fp32 master
    int n_rows;
    float s[3];                 // min(cell edge) / (cell edge along the axis)
    float eps;
};

// the lattice of a grid and a node of it
struct Lattice { int nx, ny, nz; };
struct Node { int i, j, k; };

__device__ __forceinline__ Lattice lattice_of(const GridArgs& g) { return Lattice{g.res[0] + 1, g.res[1] + 1, g.res[2] + 1}; }

// the node of a row: false for row 0, a row past the table and a row_node entry outside the lattice
__device__ __forceinline__ bool node_of_row(const RegArgs& a, const Lattice& L, int row, Node* n) {
    if (row < 1 || row >= a.n_rows) return false;
    const int node = a.row_node[row];
    if (node < 0 || node >= L.nx * L.ny * L.nz) return false;
    n->k = node % L.nz; n->j = (node / L.nz) % L.ny; n->i = node / (L.nz * L.ny);
    return true;
}

// the row of node (i, j, k), or 0 where it lies outside the lattice or is not stored (an index outside [1, n_rows) is "not stored")
__device__ __forceinline__ int stored_row(const RegArgs& a, const Lattice& L, int i, int j, int k) {
    if (i < 0 || i >= L.nx || j < 0 || j >= L.ny || k < 0 || k >= L.nz) return 0;
    const int r = a.node_index[(i * L.ny + j) * L.nz + k];
    return r > 0 && r < a.n_rows ? r : 0;
}

// column col of row r (r < n_rows by construction: phase 1 made it)
template <int W>
__device__ __forceinline__ float value(const RegArgs& a, int r, int col) { return a.values[(size_t)r * W + col]; }

// D_a of a node with value v whose forward neighbour along a has row r (0: none) and value vn
__device__ __forceinline__ float diff(int r, float vn, float v, float s) { return r ? s * (vn - v) : 0.0f; }

__device__ __forceinline__ float tv_term(float dx, float dy, float dz, float eps) { return sqrtf(((dx * dx + dy * dy) + dz * dz) + eps); }

// the first row of this wave; false: the wave has no row
__device__ __forceinline__ bool wave_rows(const RegArgs& a, int* base, int* lane) {
    *lane = threadIdx.x & (WAVE - 1);
    const long long first = ((long long)blockIdx.x * BAKED_THREADS + threadIdx.x - *lane);
    *base = (int)first;
    return first < a.n_rows;            // (uniform over the wave)
}

template <int DEG>
__global__ __launch_bounds__(BAKED_THREADS) void baked_reg_fwd_kernel(GridArgs g, RegArgs a, float* terms) {
    constexpr int V = RowOf<DEG>::V, W = RowOf<DEG>::W, PER = WAVE / W;        // PER rows per round
    int base, lane;
    if (!wave_rows(a, &base, &lane)) return;
    const Lattice L = lattice_of(g);
    // phase 1: lane = row
    const int row = base + lane;
    Node n;
    const bool live = node_of_row(a, L, row, &n);
    int r0 = 0, r1 = 0, r2 = 0, r3 = 0;
    if (live) {
        r0 = row;
        r1 = stored_row(a, L, n.i + 1, n.j, n.k);
        r2 = stored_row(a, L, n.i, n.j + 1, n.k);
        r3 = stored_row(a, L, n.i, n.j, n.k + 1);
    }
    // phase 2: lane = column of row base + PER it + sub
    const int col = lane % W, sub = lane / W;
    float t_row = 0.0f, colour_row = 0.0f;
#pragma unroll 1
    for (int it = 0; it < W; ++it) {
        const int src = it * PER + sub;
        const int q0 = __shfl(r0, src), q1 = __shfl(r1, src), q2 = __shfl(r2, src), q3 = __shfl(r3, src);
        const float v = value<W>(a, q0, col);
        const float dx = diff(q1, value<W>(a, q1, col), v, a.s[0]);
        const float dy = diff(q2, value<W>(a, q2, col), v, a.s[1]);
        const float dz = diff(q3, value<W>(a, q3, col), v, a.s[2]);
        const float t = q0 && col < V ? tv_term(dx, dy, dz, a.eps) : 0.0f;
        float colour = col == 0 ? 0.0f : t;
#pragma unroll
        for (int d = 1; d < W; d <<= 1) colour = colour + __shfl_xor(colour, d);       // partners at distance 1, 2, 4, ..: the same sum in every lane
        // back to phase 1's layout: the row of lane l was this round's if l / PER == it, and its column 0 sits in lane (l % PER) W
        const float t_back = __shfl(t, (lane % PER) * W), colour_back = __shfl(colour, (lane % PER) * W);
        if (lane / PER == it) { t_row = t_back; colour_row = colour_back; }
    }
    if (row < a.n_rows) {
        float cauchy = 0.0f;
        if (live) {
            const float sg = fmaxf(value<W>(a, row, 0), 0.0f);
            cauchy = log1pf(2.0f * (sg * sg));
        }
        float* out = terms + (size_t)row * 3;
        out[0] = t_row;
        out[1] = colour_row;
        out[2] = cauchy;
    }
}

// s_a D_a[m] / t[m] in this lane's column for the node m behind the lane's own node along AXIS: m's forward difference along AXIS is to
// the lane's own node, whose value is v; qm is m's row (0: none: the term is 0), q1 and q2 the rows of m's forward neighbours along the
// two other axes, ascending
template <int W, int AXIS>
__device__ __forceinline__ float from_behind(const RegArgs& a, int qm, int q1, int q2, int col, float v) {
    constexpr int B1 = AXIS == 0 ? 1 : 0, B2 = AXIS == 2 ? 1 : 2;
    const float vm = value<W>(a, qm, col);
    float d[3];
    d[AXIS] = a.s[AXIS] * (v - vm);
    d[B1] = diff(q1, value<W>(a, q1, col), vm, a.s[B1]);
    d[B2] = diff(q2, value<W>(a, q2, col), vm, a.s[B2]);
    const float term = (a.s[AXIS] * d[AXIS]) / tv_term(d[0], d[1], d[2], a.eps);
    return qm ? term : 0.0f;
}

template <int DEG>
__global__ __launch_bounds__(BAKED_THREADS) void baked_reg_bwd_kernel(GridArgs g, RegArgs a, const float* gw, float* grad) {
    constexpr int V = RowOf<DEG>::V, W = RowOf<DEG>::W, PER = WAVE / W;
    int base, lane;
    if (!wave_rows(a, &base, &lane)) return;
    const Lattice L = lattice_of(g);
    // phase 1: lane = row.  r[0] the row, r[1..3] ahead along x, y, z, then per axis the node behind and its two other forward neighbours
    const int row = base + lane;
    Node n;
    int r[13];
#pragma unroll
    for (int q = 0; q < 13; ++q) r[q] = 0;
    if (node_of_row(a, L, row, &n)) {
        r[0] = row;
        r[1] = stored_row(a, L, n.i + 1, n.j, n.k);
        r[2] = stored_row(a, L, n.i, n.j + 1, n.k);
        r[3] = stored_row(a, L, n.i, n.j, n.k + 1);
        r[4] = stored_row(a, L, n.i - 1, n.j, n.k);
        if (r[4]) { r[5] = stored_row(a, L, n.i - 1, n.j + 1, n.k); r[6] = stored_row(a, L, n.i - 1, n.j, n.k + 1); }
        r[7] = stored_row(a, L, n.i, n.j - 1, n.k);
        if (r[7]) { r[8] = stored_row(a, L, n.i + 1, n.j - 1, n.k); r[9] = stored_row(a, L, n.i, n.j - 1, n.k + 1); }
        r[10] = stored_row(a, L, n.i, n.j, n.k - 1);
        if (r[10]) { r[11] = stored_row(a, L, n.i + 1, n.j, n.k - 1); r[12] = stored_row(a, L, n.i, n.j + 1, n.k - 1); }
    }
    // phase 2: lane = column of row base + PER it + sub
    const int col = lane % W, sub = lane / W;
    const float g0 = gw[0], g1 = gw[1], g2 = gw[2];
#pragma unroll 1
    for (int it = 0; it < W; ++it) {
        const int src = it * PER + sub;
        int q[13];
#pragma unroll
        for (int p = 0; p < 13; ++p) q[p] = __shfl(r[p], src);
        const float v = value<W>(a, q[0], col);
        const float dx = diff(q[1], value<W>(a, q[1], col), v, a.s[0]);
        const float dy = diff(q[2], value<W>(a, q[2], col), v, a.s[1]);
        const float dz = diff(q[3], value<W>(a, q[3], col), v, a.s[2]);
        const float t = tv_term(dx, dy, dz, a.eps);
        float sum = 0.0f;
        sum = sum - (a.s[0] * dx) / t;
        sum = sum - (a.s[1] * dy) / t;
        sum = sum - (a.s[2] * dz) / t;
        sum = sum + from_behind<W, 0>(a, q[4], q[5], q[6], col, v);
        sum = sum + from_behind<W, 1>(a, q[7], q[8], q[9], col, v);
        sum = sum + from_behind<W, 2>(a, q[10], q[11], q[12], col, v);
        float out = (col == 0 ? g0 : g1) * sum;
        const float sg = fmaxf(v, 0.0f);
        const float slope = g2 * ((4.0f * sg) / (1.0f + 2.0f * (sg * sg)));
        out = col == 0 ? out + slope : out;
        out = q[0] && col < V ? out : 0.0f;     // (row 0, rows without a node and the padding columns: zeros)
        if (base + src < a.n_rows) grad[(size_t)(base + src) * W + col] = out;
    }
}

int check_reg(const char* fn, const NerfOccGrid* grid, const int* node_index, const int* row_node, const float* values, int n_rows, int sh_degree,
              float sx, float sy, float sz, float eps, GridArgs* g, RegArgs* a) {
    if (int rc = check_grid(fn, grid, g)) return rc;
    if (!(node_index && row_node && values)) return fail_arg(fn, "null pointer");
    if (!(sh_degree >= 0 && sh_degree <= 2)) return fail_arg(fn, "bad sh_degree (0, 1 or 2)");
    if (!(n_rows >= 1 && n_rows <= MAX_ROWS)) return fail_arg(fn, "bad n_rows (1..2^26: row 0, the zero row, is always there)");
    if (!(eps > 0.0f && eps < INFINITY)) return fail_arg(fn, "bad eps (finite and > 0)");
    if (!(sx > 0.0f && sx < INFINITY && sy > 0.0f && sy < INFINITY && sz > 0.0f && sz < INFINITY)) return fail_arg(fn, "bad axis scale (finite and > 0)");
    a->node_index = node_index; a->row_node = row_node; a->values = values; a->n_rows = n_rows;
    a->s[0] = sx; a->s[1] = sy; a->s[2] = sz; a->eps = eps;
    return 0;
}

inline unsigned blocks_of(int n_rows) { return (unsigned)((n_rows + BAKED_THREADS - 1) / BAKED_THREADS); }      // a thread per row in phase 1

}  // namespace

extern "C" {

int nerf_baked_reg_fwd(const NerfOccGrid* grid, const int* node_index, const int* row_node, const float* values, int n_rows, int sh_degree,
                       float sx, float sy, float sz, float eps, float* terms, void* stream) {
    GridArgs g;
    RegArgs a;
    if (int rc = check_reg(__func__, grid, node_index, row_node, values, n_rows, sh_degree, sx, sy, sz, eps, &g, &a)) return rc;
    REQUIRE(terms, "null pointer");
    REQUIRE(aligned16(values), "values must be 16-byte aligned");
    const unsigned blocks = blocks_of(n_rows);
    hipStream_t st = (hipStream_t)stream;
    if (sh_degree == 0) baked_reg_fwd_kernel<0><<<blocks, BAKED_THREADS, 0, st>>>(g, a, terms);
    else if (sh_degree == 1) baked_reg_fwd_kernel<1><<<blocks, BAKED_THREADS, 0, st>>>(g, a, terms);
    else baked_reg_fwd_kernel<2><<<blocks, BAKED_THREADS, 0, st>>>(g, a, terms);
    return done(__func__, hipGetLastError());
}

int nerf_baked_reg_bwd(const NerfOccGrid* grid, const int* node_index, const int* row_node, const float* values, int n_rows, int sh_degree,
                       float sx, float sy, float sz, float eps, const float* g_terms, float* grad, void* stream) {
    GridArgs g;
    RegArgs a;
    if (int rc = check_reg(__func__, grid, node_index, row_node, values, n_rows, sh_degree, sx, sy, sz, eps, &g, &a)) return rc;
    REQUIRE(g_terms && grad, "null pointer");
    REQUIRE(aligned16(values, grad), "values and grad must be 16-byte aligned");
    const unsigned blocks = blocks_of(n_rows);
    hipStream_t st = (hipStream_t)stream;
    if (sh_degree == 0) baked_reg_bwd_kernel<0><<<blocks, BAKED_THREADS, 0, st>>>(g, a, g_terms, grad);
    else if (sh_degree == 1) baked_reg_bwd_kernel<1><<<blocks, BAKED_THREADS, 0, st>>>(g, a, g_terms, grad);
    else baked_reg_bwd_kernel<2><<<blocks, BAKED_THREADS, 0, st>>>(g, a, g_terms, grad);
    return done(__func__, hipGetLastError());
}

}  // extern "C"
