// blend_order.h -- the blend's heaviest-first order of the tile groups, as a block-wide device
// function for the kernels that write the tile ranges (radix_sort.hip: the row pass's downsweep,
// whose tile-range blocks end with it, and k_tile_runs); blend.hip reads the order (xcd_tile).
#pragma once

#include "gsr_internal.h"

namespace gsr {

// The blend deals groups of kGroupTiles consecutive tiles (four row-adjacent tiles, 16 quadrant
// waves) round-robin over the XCDs (blend.hip xcd_tile).
constexpr uint32_t kGroupTiles = 4;

// Counting sort of the tile groups by a log-scale pair count, descending (one block; order
// within a bucket is arbitrary and does not matter: each wave's output depends only on its own
// quadrant).  Key: 32 steps per octave of (pairs + 1), 1024 buckets.
constexpr int kOrderBuckets = 1024;
__device__ __forceinline__ uint32_t order_key(const uint2 *ranges, uint32_t g, uint32_t n_tiles) {
    uint32_t n = 0;
    const uint32_t t0 = g * kGroupTiles;
#pragma unroll
    for (uint32_t i = 0; i < kGroupTiles; ++i)
        if (t0 + i < n_tiles) {
            const uint2 r = ranges[t0 + i];
            n += r.y - r.x;
        }
    const int k = (int)(__builtin_amdgcn_logf((float)n + 1.0f) * 32.0f);
    return (uint32_t)(kOrderBuckets - 1 - min(k, kOrderBuckets - 1));
}

// All kThreads threads of the block call it.  s_h: kOrderBuckets words, s_w: kThreads / 64.
template <int kThreads>
__device__ __forceinline__ void blend_order_block(const uint2 *ranges, uint32_t n_tiles,
                                                  uint32_t n_groups, uint32_t *order,
                                                  uint32_t *s_h, uint32_t *s_w) {
    constexpr int kPer = kOrderBuckets / kThreads;  // consecutive buckets per thread
    static_assert(kPer * kThreads == kOrderBuckets, "whole buckets per thread");
    const int tid = threadIdx.x;
    for (int i = tid; i < kOrderBuckets; i += kThreads) s_h[i] = 0u;
    __syncthreads();
    for (uint32_t g = tid; g < n_groups; g += kThreads)
        atomicAdd(&s_h[order_key(ranges, g, n_tiles)], 1u);
    __syncthreads();
    // exclusive scan of the bucket counts
    uint32_t c[kPer], sum = 0;
#pragma unroll
    for (int i = 0; i < kPer; ++i) sum += (c[i] = s_h[tid * kPer + i]);
    uint32_t x = sum;
    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_w[w] = x;
    __syncthreads();
    uint32_t base = x - sum;
    for (int i = 0; i < w; ++i) base += s_w[i];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        s_h[tid * kPer + i] = base;
        base += c[i];
    }
    __syncthreads();
    for (uint32_t g = tid; g < n_groups; g += kThreads)
        order[atomicAdd(&s_h[order_key(ranges, g, n_tiles)], 1u)] = g;
}

}  // namespace gsr
