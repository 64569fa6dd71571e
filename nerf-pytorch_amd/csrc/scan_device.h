// The middle launch of every count / scan / write compaction (occupancy.hip, isosurface.hip): an exclusive scan of per-block counts.
#pragma once
#include <hip/hip_runtime.h>

constexpr int SCAN_THREADS = 1024;

// exclusive scan of the block counts in place (one workgroup walks them in SCAN_THREADS-sized pieces with a carry); count[0] = total
static __global__ __launch_bounds__(SCAN_THREADS) void occ_scan_kernel(int* __restrict__ block_count, int n_blocks, int* __restrict__ count) {
    __shared__ int part[SCAN_THREADS / 64];
    __shared__ int carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < n_blocks; base += SCAN_THREADS) {
        const int i = base + tid;
        const int v = i < n_blocks ? block_count[i] : 0;
        int incl = v;       // inclusive scan inside the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) part[wave] = incl;
        __syncthreads();
        int before = carry_s;
        for (int w = 0; w < wave; ++w) before += part[w];
        if (i < n_blocks) block_count[i] = before + incl - v;
        __syncthreads();
        if (tid == SCAN_THREADS - 1) carry_s = before + incl;
        __syncthreads();
    }
    if (tid == 0) count[0] = carry_s;
}
