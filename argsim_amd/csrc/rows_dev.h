// rows_dev.h -- what the double-precision kernels over latent rows share (kmeans.hip, silhouette.hip, dbscan.hip): a row element as the double the
// contract names (for the cosine divided by the row's double norm; a zero row stays zero), the norm of a row by one wave, and the
// workgroup's double sum in its one fixed order.  Internal: not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace avae {

// rn < 0: the rows are taken as they are; rn = 0: a zero row
__device__ __forceinline__ double row_value(float v, double rn) { return rn < 0.0 ? (double)v : (rn > 0.0 ? (double)v / rn : 0.0); }

// the pair passes (silhouette.hip, dbscan.hip) stage rows in LDS as doubles, [element][row] with `rows` rows to an element: the four
// elements e0 .. e0 + 3 of row r, zeros where `on` is false
__device__ __forceinline__ void stage_row4(double* s, int rows, int e0, int r, float4 v, double rn, bool on)
{
    s[e0 * rows + r] = on ? row_value(v.x, rn) : 0.0; s[(e0 + 1) * rows + r] = on ? row_value(v.y, rn) : 0.0;
    s[(e0 + 2) * rows + r] = on ? row_value(v.z, rn) : 0.0; s[(e0 + 3) * rows + r] = on ? row_value(v.w, rn) : 0.0;
}

// one wave per row: the double sum of squares, lane l over elements 4 l .. 4 l + 3, 256 + 4 l .. in index order, then the xor butterfly;
// every lane returns the root
__device__ __forceinline__ double wave_row_norm(const float* __restrict__ x, long long row, int dim)
{
    const int lane = threadIdx.x & 63;
    double s = 0.0;
    for (int c = lane * 4; c < dim; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(x + row * dim + c);
        s += (double)v.x * v.x; s += (double)v.y * v.y; s += (double)v.z * v.z; s += (double)v.w * v.w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return sqrt(s);
}

// the sum of one double per thread over the NW waves of the workgroup, in every thread: the xor butterfly of a wave, then the waves in
// ascending order.  sh: NW doubles; ends in a barrier
template <int NW>
__device__ __forceinline__ double block_sum(double v, double* sh)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sh[0];
    for (int w = 1; w < NW; ++w) s += sh[w];
    __syncthreads();
    return s;
}

}  // namespace avae
