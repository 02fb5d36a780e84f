#pragma once
// The fixed-order workgroup sum of the MD kernels (md.hip, md_bias.hip): no atomics, the same bits run to run.
#include "anihip_common.h"

namespace anihip {

constexpr int MD_BLOCK = 256;   // atoms per chunk, threads per workgroup

// sum of W values per thread over the workgroup, waves and lanes in a fixed order; the result in thread 0
template <int W>
__device__ __forceinline__ void md_block_sum(double (&s)[W])
{
    __shared__ double sh[MD_BLOCK / WAVE][W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[w] += __shfl_xor(s[w], off);
    }
    const int wave = threadIdx.x / WAVE;
    if (lane_id() == 0) {
#pragma unroll
        for (int w = 0; w < W; ++w) sh[wave][w] = s[w];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < W; ++w) s[w] = (sh[0][w] + sh[1][w]) + (sh[2][w] + sh[3][w]);
    }
}
static_assert(MD_BLOCK == 4 * WAVE, "md_block_sum adds four waves");

}  // namespace anihip
