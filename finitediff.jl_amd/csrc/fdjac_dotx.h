// dot(x, .) as the JVP sums it (fdjac_jvp.hip), for every kernel that leaves its partial sums where k_jvp_eps reads them -- the contract of
// JvpHooks::have_partials is that they all use THIS traversal and THIS tail: k_dot_partial itself, k_jf_open and k_jf_open_blocks
// (fdjac_jfnk.hip), k_jt_p (fdjac_jftr.hip).  Accumulation is Float64 in either element build.
#pragma once
#include "fdjac_internal.h"

namespace fdjac {

// the wavefront's sum, valid in its lane 0: x_l + x_(l + off), off = 32, 16, .. 1 (the library's one spelling of this tree: the step-size
// reduction of fdjac_eps_dev.h and the Gram-Schmidt dots of fdjac_cscgmres.hip use it too)
__device__ __forceinline__ double wave_sum(double acc)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    return acc;
}

// The tail of ND sums of a workgroup of BLOCK threads: the shuffle tree, then thread 0 adds the wavefronts' sums in ascending order from
// +0.0.  The workgroup's sums come back in acc[] of thread 0 (the other threads hold intermediates).
template <int ND, int BLOCK = kBlock>
__device__ __forceinline__ void dotx_finish(double (&acc)[ND], double (&red)[ND][BLOCK / 64])
{
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        acc[d] = wave_sum(acc[d]);
        if ((threadIdx.x & 63) == 0) red[d][threadIdx.x >> 6] = acc[d];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        double t = 0.0;
        for (int w = 0; w < BLOCK / 64; ++w) t += red[d][w];
        acc[d] = t;
    }
}

// The traversal of n elements on a grid of kBlock threads per workgroup.  PAIRED: pair(i) for the pairs (2 i, 2 i + 1), i < n >> 1,
// grid-stride, and one(n - 1) for an odd n's last element in thread 0 of workgroup 0, after its pairs; otherwise one(i), grid-stride.
template <bool PAIRED, class FP, class FO>
__device__ __forceinline__ void dotx_for_each(int64_t n, FP pair, FO one)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock, first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (PAIRED) {
        const int64_t n2 = n >> 1;
        for (int64_t i = first; i < n2; i += stride) pair(i);
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) one(n - 1);
    } else {
        for (int64_t i = first; i < n; i += stride) one(i);
    }
}

}  // namespace fdjac
