// Host side shared by the hash-grid translation units (hash_encode.hip, hash_input_grad.hip): the checks of a NerfHashGrid record and
// of the point source at the extern "C" boundary.  One copy, so the two files cannot accept different records.
#pragma once
#include "api_util.h"
#include "hash_device.h"

namespace nerf_hash {

inline int check_grid(const char* fn, const NerfHashGrid* g, Levels* lv) {
    using nerf_api::fail_arg;
    if (!g) return fail_arg(fn, "null grid");
    if (g->n_levels < 1 || g->n_levels > NERF_HASH_MAX_LEVELS) return fail_arg(fn, "n_levels must be 1 .. 32");
    if (g->n_features != 1 && g->n_features != 2 && g->n_features != 4) return fail_arg(fn, "n_features must be 1, 2 or 4");
    if (g->log2_hashmap_size < 4 || g->log2_hashmap_size > 24) return fail_arg(fn, "log2_hashmap_size must be 4 .. 24");
    const long long T = 1ll << g->log2_hashmap_size;
    long long off = 0;
    for (int l = 0; l < g->n_levels; ++l) {
        const long long R = g->level_resolution[l];
        if (R < 1 || R > (1 << 24)) return fail_arg(fn, "level_resolution must be 1 .. 2^24");
        // (R + 1)^3 <= T without overflow: R + 1 <= 2^8 for T <= 2^24 whenever the cube fits
        const bool fits = R + 1 <= 256 && (R + 1) * (R + 1) * (R + 1) <= T;
        if ((g->level_dense[l] != 0) != fits) return fail_arg(fn, "level_dense disagrees with (R + 1)^3 <= T");
        if (g->level_offset[l] != off) return fail_arg(fn, "level_offset is not the prefix sum of the rows owned");
        off += fits ? (R + 1) * (R + 1) * (R + 1) : T;
        lv->res[l] = (int)R;
        lv->offset[l] = g->level_offset[l];
    }
    if (g->level_offset[g->n_levels] != off) return fail_arg(fn, "level_offset[n_levels] is not the number of rows");
    unsigned dense = 0;
    for (int l = 0; l < g->n_levels; ++l) dense |= (g->level_dense[l] ? 1u : 0u) << l;
    lv->dense_mask = dense;
    lv->hash_mask = (unsigned)(T - 1);
    for (int a = 0; a < 3; ++a) {
        if (!(g->inv_extent[a] > 0.0f) || !(g->lo[a] == g->lo[a])) return fail_arg(fn, "box: lo must be finite and inv_extent > 0");
        lv->lo[a] = g->lo[a];
        lv->inv_extent[a] = g->inv_extent[a];
    }
    return 0;
}

inline int check_points(const char* fn, const float* points, const float* rays, int ray_stride, const float* z_vals, int n_samples, long P,
                        PointSrc* src) {
    using nerf_api::fail_arg;
    if (P < 0 || P > 0x7fffffffL) return fail_arg(fn, "bad number of points");
    if (points) {
        if (rays || z_vals) return fail_arg(fn, "give points OR rays + z_vals");
        *src = PointSrc{points, nullptr, nullptr, 0, 1};
        return 0;
    }
    if (P == 0) { *src = PointSrc{nullptr, nullptr, nullptr, 0, 1}; return 0; }
    if (!rays || !z_vals) return fail_arg(fn, "null pointer (points, or rays + z_vals)");
    if (ray_stride < 6 || n_samples < 1 || P % n_samples) return fail_arg(fn, "rays: stride >= 6, n_samples >= 1, P a multiple of n_samples");
    *src = PointSrc{nullptr, rays, z_vals, ray_stride, n_samples};
    return 0;
}

}  // namespace nerf_hash
