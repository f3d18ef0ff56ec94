// reduce_dev.h -- the wave and workgroup reductions that the row kernels (ops.hip, decode.hip, score.hip, beam.hip) end in: sum and
// maximum over the 64 lanes, the first-maximum merge over (value, index), and the butterfly of a running log-sum-exp.  The wave steps
// are __shfl_xor butterflies: every lane ends with the result, and lane 0 adds in the pairing a __shfl_down tree gives it.  A
// cross-wave FLOAT sum is not here: every site keeps its own order, written out where it is (the results are compared bit for bit).
#pragma once
#include <hip/hip_runtime.h>
#include "sample_dev.h"      // cand_better: THE tie rule; lse_merge

namespace avae {

template <class T>      // float or int
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// (m, s) of a running log-sum-exp (sample_dev.h: lse_add) merged over the 64 lanes, in every lane
__device__ __forceinline__ void lse_wave_merge(float& m, float& s)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64); lse_merge(m, s, om, os); }
}

// the FIRST maximum of a row as (value, index).  The neutral element loses against every number; a NaN never enters.
struct ArgFirst {
    float v = -INFINITY; int i = 0x7fffffff;
    // a thread's own scan in ascending index order: strict >, so the first maximum stays
    __device__ __forceinline__ void take(float x, int idx) { if (x > v) { v = x; i = idx; } }
    // any two records: larger value, then smaller index (order-free for non-NaN values)
    __device__ __forceinline__ void merge(const ArgFirst& o) { if (cand_better(o.v, o.i, v, i)) *this = o; }
    __device__ __forceinline__ void wave_merge()
    {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) merge(ArgFirst{__shfl_xor(v, o, 64), __shfl_xor(i, o, 64)});
    }
    // over the NW waves of the workgroup, after wave_merge(): lane 0 of wave w stores its record at sv[w], si[w] (NW words of LDS
    // each), ONE barrier, then the sweep over the waves in ascending order.  Every thread must call it.  No barrier before the stores
    // (the caller's, where sv / si may still be read: it also covers what else the caller hands over at this point) and none after
    // the sweep.  kAll: every thread sweeps and gets the result; else thread 0 alone does, and the result is valid there only.
    template <int NW, bool kAll>
    __device__ __forceinline__ void block_merge(float* sv, int* si)
    {
        if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = i; }
        __syncthreads();
        if (kAll || threadIdx.x == 0) {
            if (kAll) { v = sv[0]; i = si[0]; }
#pragma unroll
            for (int w = 1; w < NW; ++w) merge(ArgFirst{sv[w], si[w]});
        }
    }
};

// the FIRST minimum in double as (value, index): ArgFirst's sibling for distances (kmeans.hip).  The neutral element loses against
// every number; a NaN never enters.
struct ArgMinFirst {
    double v = INFINITY; int i = 0x7fffffff;
    // a thread's own scan in ascending index order: strict <, so the first minimum stays
    __device__ __forceinline__ void take(double x, int idx) { if (x < v) { v = x; i = idx; } }
    // any two records: smaller value, then smaller index (order-free for non-NaN values)
    __device__ __forceinline__ void merge(const ArgMinFirst& o) { if (o.v < v || (o.v == v && o.i < i)) *this = o; }
    // butterfly over aligned groups of W lanes, in every lane
    template <int W = 64>
    __device__ __forceinline__ void wave_merge()
    {
#pragma unroll
        for (int o = W / 2; o > 0; o >>= 1) merge(ArgMinFirst{__shfl_xor(v, o, 64), __shfl_xor(i, o, 64)});
    }
    // over the NW waves of the workgroup, after wave_merge(): as ArgFirst::block_merge, every thread gets the result, and a barrier
    // follows the sweep (the caller may call it again at once)
    template <int NW>
    __device__ __forceinline__ void block_merge(double* sv, int* si)
    {
        if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = i; }
        __syncthreads();
        v = sv[0]; i = si[0];
        for (int w = 1; w < NW; ++w) merge(ArgMinFirst{sv[w], si[w]});
        __syncthreads();
    }
};

}  // namespace avae
