// What every kernel that looks a point up in an occupancy grid shares (occupancy.hip, baked.hip): the grid as a kernel argument, the
// sample point of a depth, the classification of a point and the norm of a ray's direction -- one copy, so two files cannot drift apart.
// Classification is the arithmetic of OccupancyGrid.occupied (nerf-pytorch_amd/occupancy.py): per axis one fp32 subtraction and one
// fp32 multiplication (the library is built with -ffp-contract=off), inside iff 0 <= t < R, cell = floor(t).
#pragma once
#include <hip/hip_runtime.h>
#include "api_util.h"

namespace nerf_grid {

struct GridArgs {
    float lo[3], scale[3];
    int res[3];
    int outside_skip;
    const unsigned* bits;
};

struct Pt { float x, y, z; };

__device__ __forceinline__ Pt sample_point(const float* __restrict__ ray, float z) {
    // run_nerf.py:381: pts = rays_o + rays_d * z_vals -- one multiply, one add (no contraction)
    Pt p;
    p.x = ray[0] + ray[3] * z;
    p.y = ray[1] + ray[4] * z;
    p.z = ray[2] + ray[5] * z;
    return p;
}

// |d| of a ray record: three products added left to right, one correctly rounded root (OccupancyGrid._march_rays' dn)
__device__ __forceinline__ float dir_norm(const float* __restrict__ ray) { return sqrtf(ray[3] * ray[3] + ray[4] * ray[4] + ray[5] * ray[5]); }

// The grid coordinates of a point, t = (p - lo) * scale per axis, and whether it lies inside the box
// (a NaN fails every comparison: outside)
__device__ __forceinline__ bool grid_coords(const GridArgs& g, const Pt& p, float* tx, float* ty, float* tz) {
    *tx = (p.x - g.lo[0]) * g.scale[0];
    *ty = (p.y - g.lo[1]) * g.scale[1];
    *tz = (p.z - g.lo[2]) * g.scale[2];
    return *tx >= 0.0f && *tx < (float)g.res[0] && *ty >= 0.0f && *ty < (float)g.res[1] && *tz >= 0.0f && *tz < (float)g.res[2];
}

__device__ __forceinline__ unsigned cell_index(const GridArgs& g, int ix, int iy, int iz) {
    return ((unsigned)ix * (unsigned)g.res[1] + (unsigned)iy) * (unsigned)g.res[2] + (unsigned)iz;
}

// The classification of a point, shared by occupied() and proposal_sigma(): false outside the box, else true and the point's cell in *c
__device__ __forceinline__ bool cell_of(const GridArgs& g, const Pt& p, unsigned* c) {
    float tx, ty, tz;
    if (!grid_coords(g, p, &tx, &ty, &tz)) return false;
    *c = cell_index(g, (int)floorf(tx), (int)floorf(ty), (int)floorf(tz));
    return true;
}

__device__ __forceinline__ bool cell_bit(const GridArgs& g, unsigned c) { return (g.bits[c >> 5] >> (c & 31u)) & 1u; }

__device__ __forceinline__ bool occupied(const GridArgs& g, const Pt& p) {
    unsigned c;
    if (!cell_of(g, p, &c)) return g.outside_skip == 0;
    return cell_bit(g, c);
}

// the kernel argument of a checked NerfOccGrid (fn: the public function's name)
inline int check_grid(const char* fn, const NerfOccGrid* grid, GridArgs* g) {
    if (!grid || !grid->bits) return nerf_api::fail_arg(fn, "null pointer");
    for (int a = 0; a < 3; ++a) {
        if (grid->res[a] < 1 || grid->res[a] > 512) return nerf_api::fail_arg(fn, "grid resolution must be 1..512 per axis");
        g->lo[a] = grid->lo[a];
        g->scale[a] = grid->scale[a];
        g->res[a] = grid->res[a];
    }
    g->outside_skip = grid->outside_skip != 0;
    g->bits = grid->bits;
    return 0;
}

}  // namespace nerf_grid
