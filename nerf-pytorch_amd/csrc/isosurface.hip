// Triangle meshes of a scalar volume (include/nerf_hip.h, section "isosurface"): marching tetrahedra on the Kuhn subdivision of a
// lattice of nodes.  mesh.extract_mesh_reference (nerf-pytorch_amd/mesh.py) is the definition; iso_tables.h holds the tables both read.
//   nerf_iso_count : V = the lattice edges that carry a vertex, F = the triangles, and the block offsets of both compactions;
//   nerf_iso_emit  : the vertices in ascending edge id, the triangles in cube / tetrahedron / triangle order.
// Two compactions in occupancy.hip's form -- a count per block, occ_scan_kernel over the block counts, a write -- so the order of both
// lists is the definition's and no atomic decides anything:
//   edges  one work item per (node, class), e = 7 node + class, ISO_TILE items per block.  The flag "crossed and used" is a wave ballot;
//          the write pass stores every item's exclusive rank into prefix[e] (the vertex index of a flagged edge) and the positions of
//          the flagged ones.
//   cubes  one work item per cube.  It loads its 8 node values once, the six tetrahedra reuse them as one 8-bit inside mask; a cube has
//          0..12 triangles, so its rank is an integer prefix inside the wave (__shfl_up) and over the block's wave totals.  The emit
//          pass looks each corner of a triangle up in prefix[].
// Everything a tetrahedron needs from the tables is folded into compile-time constants (the walk over the six is unrolled); only the
// inside mask is a run-time value, and the one lookup it indexes is a chain of selects: no array in scratch, no table in memory.
// Arithmetic of a vertex (-ffp-contract=off, IEEE division): t = (level - a) / (b - a) with a, b made finite, p = p_a + t (p_b - p_a)
// per component with p_a = lo + float(index) * step.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>
#include <utility>
#include "api_util.h"
#include "iso_tables.h"
#include "scan_device.h"

using namespace nerf_api;

namespace {

constexpr int ISO_THREADS = 256;                // 4 waves
constexpr int ISO_WAVES = ISO_THREADS / 64;
constexpr int ISO_ITERS = 4;
constexpr int ISO_TILE = ISO_THREADS * ISO_ITERS;   // edge items per block; a cube block takes ISO_THREADS cubes

struct IsoArgs {
    const float* volume;
    int nx, ny, nz;
    float level;
    const unsigned* keep;       // one bit per cube, or null: every cube
};

// ---- the tables as constants
constexpr unsigned dir_bits(int axis) {         // bit c: class c moves along `axis`
    unsigned m = 0;
    for (int c = 0; c < 7; ++c) m |= (unsigned)ISO_CLASS_DIRS[c][axis] << c;
    return m;
}
constexpr unsigned DIR_X = dir_bits(0), DIR_Y = dir_bits(1), DIR_Z = dir_bits(2);

// a cube corner is the code q = 4 dx + 2 dy + dz
constexpr int axis_code(int axis) { return 4 >> axis; }
constexpr int tet_corner(int t, int i) {
    return i == 0 ? 0 : i == 1 ? axis_code(ISO_PERMS[t][0]) : i == 2 ? (axis_code(ISO_PERMS[t][0]) | axis_code(ISO_PERMS[t][1])) : 7;
}
constexpr bool tet_odd(int t) {
    int inv = 0;
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b) inv += ISO_PERMS[t][a] > ISO_PERMS[t][b];
    return inv & 1;
}
constexpr int class_of_code(int q) {
    for (int c = 0; c < 7; ++c)
        if (4 * ISO_CLASS_DIRS[c][0] + 2 * ISO_CLASS_DIRS[c][1] + ISO_CLASS_DIRS[c][2] == q) return c;
    return -1;
}
// the six edges of tetrahedron t, 6 bits each: the lower corner's code | the edge's class << 3
constexpr unsigned long long tet_edge_codes(int t) {
    unsigned long long r = 0;
    for (int e = 0; e < 6; ++e) {
        const int qa = tet_corner(t, ISO_TET_EDGES[e][0]), qb = tet_corner(t, ISO_TET_EDGES[e][1]);
        r |= (unsigned long long)(qa | (class_of_code(qa ^ qb) << 3)) << (6 * e);
    }
    return r;
}
// the triangles of inside mask m, 3 bits per corner (rows of ISO_TET_EDGES), the odd tetrahedra with their last two corners swapped
constexpr unsigned tris_code(int m, bool odd) {
    unsigned r = 0;
    for (int tri = 0; tri < 2; ++tri)
        for (int v = 0; v < 3; ++v) {
            const int src = odd && v > 0 ? 3 - v : v;
            r |= (unsigned)ISO_TET_TRIS[m][1 + 3 * tri + src] << (3 * (3 * tri + v));
        }
    return r;
}
template <bool ODD, int... M>
__device__ __forceinline__ unsigned tris_of(unsigned m, std::integer_sequence<int, M...>) {
    unsigned r = 0;
    ((r = m == (unsigned)M ? std::integral_constant<unsigned, tris_code(M, ODD)>::value : r), ...);
    return r;
}
// triangles of a tetrahedron with p inside corners: 0 1 2 1 0 (ISO_TET_TRIS' first column)
__device__ __forceinline__ int tris_of_popcount(int p) { return (0x01210 >> (4 * p)) & 15; }

template <int T>
__device__ __forceinline__ unsigned tet_mask(unsigned inside8) {
    return ((inside8 >> tet_corner(T, 0)) & 1u) | (((inside8 >> tet_corner(T, 1)) & 1u) << 1) | (((inside8 >> tet_corner(T, 2)) & 1u) << 2) |
           (((inside8 >> tet_corner(T, 3)) & 1u) << 3);
}

// lanes below this one whose bit is set in a wave ballot
__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__device__ __forceinline__ float finite_of(float v) { return v != v ? -FLT_MAX : fminf(fmaxf(v, -FLT_MAX), FLT_MAX); }

// cube (ci, cj, ck), which may lie outside the lattice: whether it exists and is kept
__device__ __forceinline__ bool cube_kept(const IsoArgs& g, int ci, int cj, int ck) {
    if ((unsigned)ci >= (unsigned)(g.nx - 1) || (unsigned)cj >= (unsigned)(g.ny - 1) || (unsigned)ck >= (unsigned)(g.nz - 1)) return false;
    const unsigned c = ((unsigned)ci * (unsigned)(g.ny - 1) + (unsigned)cj) * (unsigned)(g.nz - 1) + (unsigned)ck;
    return (g.keep[c >> 5] >> (c & 31u)) & 1u;
}

// ---- edges
struct Edge {
    int i, j, k, dx, dy, dz;
    float a, b;                 // the node values at the lower and the upper endpoint, as stored
};

// item e < 7 nodes: whether its edge lies in the lattice, has exactly one endpoint inside and belongs to a kept cube
__device__ __forceinline__ bool edge_flag(const IsoArgs& g, unsigned e, Edge* out) {
    const unsigned node = e / 7u, cls = e - 7u * node;
    Edge ed;
    ed.k = (int)(node % (unsigned)g.nz);
    ed.j = (int)((node / (unsigned)g.nz) % (unsigned)g.ny);
    ed.i = (int)(node / ((unsigned)g.nz * (unsigned)g.ny));
    ed.dx = (DIR_X >> cls) & 1u; ed.dy = (DIR_Y >> cls) & 1u; ed.dz = (DIR_Z >> cls) & 1u;
    ed.a = 0.0f; ed.b = 0.0f;
    *out = ed;
    if (ed.i + ed.dx >= g.nx || ed.j + ed.dy >= g.ny || ed.k + ed.dz >= g.nz) return false;
    ed.a = g.volume[node];
    ed.b = g.volume[node + (unsigned)((ed.dx * g.ny + ed.dy) * g.nz + ed.dz)];
    *out = ed;
    if ((ed.a >= g.level) == (ed.b >= g.level)) return false;       // (a NaN fails the comparison: outside)
    if (!g.keep) return true;       // (every edge of the lattice lies in some cube)
    // the cubes that contain the edge: along an axis the edge moves on, the one it starts in; along the others, both neighbours
    bool used = false;
    for (int sx = 0; sx <= 1 - ed.dx; ++sx)
        for (int sy = 0; sy <= 1 - ed.dy; ++sy)
            for (int sz = 0; sz <= 1 - ed.dz; ++sz) used = used || cube_kept(g, ed.i - sx, ed.j - sy, ed.k - sz);
    return used;
}

// item of iteration `it` of thread `tid` in block `b`: consecutive lanes take consecutive edge ids (32-bit: 7 nodes < 2^31)
__device__ __forceinline__ unsigned item_of(unsigned b, int it, int tid) { return b * ISO_TILE + it * ISO_THREADS + tid; }

__global__ __launch_bounds__(ISO_THREADS) void iso_edge_count_kernel(IsoArgs g, unsigned E, int* __restrict__ block_count) {
    __shared__ int wave_n[ISO_WAVES];
    const int tid = threadIdx.x;
    int n = 0;
#pragma unroll
    for (int it = 0; it < ISO_ITERS; ++it) {
        const unsigned e = item_of(blockIdx.x, it, tid);
        Edge ed;
        const bool flag = e < E && edge_flag(g, e, &ed);
        n += __popcll(__ballot(flag));
    }
    if ((tid & 63) == 0) wave_n[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < ISO_WAVES; ++w) s += wave_n[w];
        block_count[blockIdx.x] = s;
    }
}

struct Lattice { float lo[3], step[3]; };

__global__ __launch_bounds__(ISO_THREADS) void iso_vertex_write_kernel(IsoArgs g, Lattice lat, unsigned E, const int* __restrict__ block_offset,
                                                                       int* __restrict__ prefix, float* __restrict__ vertices) {
    __shared__ int wave_n[ISO_ITERS][ISO_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6;
    int base = block_offset[blockIdx.x];
    // one iteration at a time: the block's running base is the only thing an iteration hands to the next
    for (int it = 0; it < ISO_ITERS; ++it) {
        const unsigned e = item_of(blockIdx.x, it, tid);
        Edge ed;
        const bool flag = e < E && edge_flag(g, e, &ed);
        const unsigned long long m = __ballot(flag);
        if ((tid & 63) == 0) wave_n[it][wave] = __popcll(m);
        __syncthreads();
        int before = base;
#pragma unroll
        for (int w = 0; w < ISO_WAVES; ++w) {
            const int c = wave_n[it][w];
            if (w < wave) before += c;
            base += c;
        }
        if (e < E) {
            const int rank = before + lanes_below(m);
            prefix[e] = rank;
            if (flag) {
                const float a = finite_of(ed.a), b = finite_of(ed.b);
                float t = (g.level - a) / (b - a);          // (IEEE division: hipcc's default for fp32)
                if (t != t) t = 0.5f;                       // both differences overflowed, or a = b = level = -FLT_MAX beside a NaN
                const float ax = lat.lo[0] + (float)ed.i * lat.step[0], bx = lat.lo[0] + (float)(ed.i + ed.dx) * lat.step[0];
                const float ay = lat.lo[1] + (float)ed.j * lat.step[1], by = lat.lo[1] + (float)(ed.j + ed.dy) * lat.step[1];
                const float az = lat.lo[2] + (float)ed.k * lat.step[2], bz = lat.lo[2] + (float)(ed.k + ed.dz) * lat.step[2];
                float* v = vertices + (size_t)rank * 3;
                v[0] = ax + t * (bx - ax);
                v[1] = ay + t * (by - ay);
                v[2] = az + t * (bz - az);
            }
        }
    }
}

// ---- cubes
// cube c < cubes: its first node and the inside bits of its 8 corners by code; false (no triangles) where keep drops it
__device__ __forceinline__ bool cube_corners(const IsoArgs& g, unsigned c, unsigned* node0, unsigned* inside8) {
    if (g.keep && !((g.keep[c >> 5] >> (c & 31u)) & 1u)) return false;
    const unsigned cy = (unsigned)(g.ny - 1), cz = (unsigned)(g.nz - 1);
    const unsigned ck = c % cz, cj = (c / cz) % cy, ci = c / (cz * cy);
    const unsigned n0 = (ci * (unsigned)g.ny + cj) * (unsigned)g.nz + ck;
    unsigned in8 = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float v = g.volume[n0 + (unsigned)((((q >> 2) & 1) * g.ny + ((q >> 1) & 1)) * g.nz + (q & 1))];
        in8 |= (unsigned)(v >= g.level) << q;       // (a NaN fails the comparison: outside)
    }
    *node0 = n0;
    *inside8 = in8;
    return true;
}

template <int... T>
__device__ __forceinline__ int cube_triangles(unsigned inside8, std::integer_sequence<int, T...>) {
    return (tris_of_popcount(__popc(tet_mask<T>(inside8))) + ...);
}

// exclusive prefix of n over the block's threads in thread order, and the block's total: __shfl_up inside the wave, the wave totals in LDS
__device__ __forceinline__ int block_prefix(int n, int* total) {
    __shared__ int wave_n[ISO_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_n[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < ISO_WAVES; ++w) {
        const int c = wave_n[w];
        if (w < wave) before += c;
        all += c;
    }
    *total = all;
    return before + incl - n;
}

__global__ __launch_bounds__(ISO_THREADS) void iso_cube_count_kernel(IsoArgs g, unsigned cubes, int* __restrict__ block_count) {
    const unsigned c = blockIdx.x * ISO_THREADS + threadIdx.x;
    unsigned node0 = 0, inside8 = 0;
    int n = 0;
    if (c < cubes && cube_corners(g, c, &node0, &inside8)) n = cube_triangles(inside8, std::make_integer_sequence<int, 6>());
    int total;
    block_prefix(n, &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// the triangles of tetrahedron T of a cube, written at *out (which moves on): each corner is the rank of its lattice edge
template <int T>
__device__ __forceinline__ void emit_tet(const IsoArgs& g, unsigned inside8, unsigned node0, const int* __restrict__ prefix, int** out) {
    const unsigned m = tet_mask<T>(inside8);
    const int n = tris_of_popcount(__popc(m));
    if (n == 0) return;
    constexpr unsigned long long EDGES = tet_edge_codes(T);
    const unsigned tris = tris_of<tet_odd(T)>(m, std::make_integer_sequence<int, 16>());
    int* f = *out;
    for (int k = 0; k < 3 * n; ++k) {
        const unsigned code = (unsigned)(EDGES >> (6u * ((tris >> (3 * k)) & 7u))) & 63u;
        const unsigned q = code & 7u, cls = code >> 3;
        const unsigned node = node0 + (((q >> 2) & 1u) * (unsigned)g.ny + ((q >> 1) & 1u)) * (unsigned)g.nz + (q & 1u);
        f[k] = prefix[7u * node + cls];
    }
    *out = f + 3 * n;
}

template <int... T>
__device__ __forceinline__ void emit_cube(const IsoArgs& g, unsigned inside8, unsigned node0, const int* __restrict__ prefix, int* out,
                                          std::integer_sequence<int, T...>) {
    (emit_tet<T>(g, inside8, node0, prefix, &out), ...);
}

__global__ __launch_bounds__(ISO_THREADS) void iso_face_emit_kernel(IsoArgs g, unsigned cubes, const int* __restrict__ block_offset,
                                                                    const int* __restrict__ prefix, int* __restrict__ faces) {
    const unsigned c = blockIdx.x * ISO_THREADS + threadIdx.x;
    unsigned node0 = 0, inside8 = 0;
    int n = 0;
    if (c < cubes && cube_corners(g, c, &node0, &inside8)) n = cube_triangles(inside8, std::make_integer_sequence<int, 6>());
    int total;
    const int first = block_offset[blockIdx.x] + block_prefix(n, &total);
    if (n > 0) emit_cube(g, inside8, node0, prefix, faces + (size_t)first * 3, std::make_integer_sequence<int, 6>());
}

// ---- host
struct IsoSizes {
    long nodes, cubes;
    unsigned E;                 // edge items
    int edge_blocks, cube_blocks;
};

bool iso_sizes(int nx, int ny, int nz, IsoSizes* s) {
    if (nx < 2 || ny < 2 || nz < 2) return false;
    const long plane = (long)nx * ny;           // (three ints multiplied at once can overflow 64 bits)
    if (plane >= (1L << 31)) return false;
    s->nodes = plane * nz;
    s->cubes = (long)(nx - 1) * (ny - 1) * (nz - 1);
    // edge ids, vertex and triangle counts are 32-bit: 7 nodes edges, at most 12 triangles per cube
    if (!(7 * s->nodes < (1L << 31) && 12 * s->cubes < (1L << 31))) return false;
    s->E = (unsigned)(7 * s->nodes);
    s->edge_blocks = (int)((7 * s->nodes + ISO_TILE - 1) / ISO_TILE);
    s->cube_blocks = (int)((s->cubes + ISO_THREADS - 1) / ISO_THREADS);
    return true;
}

int check_iso(const char* fn, int nx, int ny, int nz, float level, IsoSizes* s) {
    if (nx < 2 || ny < 2 || nz < 2) return fail_arg(fn, "bad size (at least 2 nodes per axis)");
    if (!iso_sizes(nx, ny, nz, s)) return fail_arg(fn, "bad size (7 * nodes and 12 * cubes must stay below 2^31)");
    if (!(fabsf(level) < INFINITY)) return fail_arg(fn, "bad level (finite)");      // (a NaN fails the comparison)
    return 0;
}

// scratch: prefix[7 nodes] | edge block offsets | cube block offsets
struct IsoScratch { int *prefix, *edge_blocks, *cube_blocks; };
IsoScratch carve(int* scratch, const IsoSizes& s) { return IsoScratch{scratch, scratch + s.E, scratch + s.E + s.edge_blocks}; }

}  // namespace

extern "C" {

size_t nerf_iso_scratch_words(int nx, int ny, int nz) {
    IsoSizes s;
    return iso_sizes(nx, ny, nz, &s) ? (size_t)s.E + (size_t)s.edge_blocks + (size_t)s.cube_blocks : 0;
}

int nerf_iso_count(const float* volume, int nx, int ny, int nz, float level, const unsigned* keep_words, int* scratch, int* counts,
                   void* stream) {
    REQUIRE(volume && scratch && counts, "null pointer");
    IsoSizes s;
    if (int rc = check_iso(__func__, nx, ny, nz, level, &s)) return rc;
    const IsoScratch w = carve(scratch, s);
    const IsoArgs g{volume, nx, ny, nz, level, keep_words};
    hipStream_t st = (hipStream_t)stream;
    iso_edge_count_kernel<<<s.edge_blocks, ISO_THREADS, 0, st>>>(g, s.E, w.edge_blocks);
    occ_scan_kernel<<<1, SCAN_THREADS, 0, st>>>(w.edge_blocks, s.edge_blocks, counts);
    iso_cube_count_kernel<<<s.cube_blocks, ISO_THREADS, 0, st>>>(g, (unsigned)s.cubes, w.cube_blocks);
    occ_scan_kernel<<<1, SCAN_THREADS, 0, st>>>(w.cube_blocks, s.cube_blocks, counts + 1);
    return done(__func__, hipGetLastError());
}

int nerf_iso_emit(const float* volume, int nx, int ny, int nz, float level, const float lo[3], const float step[3],
                  const unsigned* keep_words, int* scratch, float* vertices, int* faces, void* stream) {
    REQUIRE(volume && lo && step && scratch && vertices && faces, "null pointer");
    IsoSizes s;
    if (int rc = check_iso(__func__, nx, ny, nz, level, &s)) return rc;
    const IsoScratch w = carve(scratch, s);
    const IsoArgs g{volume, nx, ny, nz, level, keep_words};
    Lattice lat;
    for (int k = 0; k < 3; ++k) {
        lat.lo[k] = lo[k];
        lat.step[k] = step[k];
    }
    hipStream_t st = (hipStream_t)stream;
    iso_vertex_write_kernel<<<s.edge_blocks, ISO_THREADS, 0, st>>>(g, lat, s.E, w.edge_blocks, w.prefix, vertices);
    iso_face_emit_kernel<<<s.cube_blocks, ISO_THREADS, 0, st>>>(g, (unsigned)s.cubes, w.cube_blocks, w.prefix, faces);
    return done(__func__, hipGetLastError());
}

}  // extern "C"
