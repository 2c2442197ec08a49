// gs_countrow.hpp — device helpers of the kernels that read rows of the 16-bit count matrix (gs_knn.hip, gs_cluster.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gs {

// entry e (0..7) of one 16-byte load of counts
__device__ __forceinline__ uint32_t count16(const uint4 &x, int e)
{
    const uint32_t w = e < 2 ? x.x : e < 4 ? x.y : e < 6 ? x.z : x.w;
    return (e & 1) ? (w >> 16) : (w & 0xFFFFu);
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}
// exclusive prefix of one value per thread in thread order, and the block total, in a workgroup of NW waves. Two calls that use the same `wsum`
// need a barrier between them
template <int NW>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *wsum, uint32_t &tot)
{
    const uint32_t inc = wave_incl_scan(v);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t before = 0, t = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) { const uint32_t s = wsum[i]; before += i < w ? s : 0; t += s; }
    tot = t;
    return before + inc - v;
}

}  // namespace gs
