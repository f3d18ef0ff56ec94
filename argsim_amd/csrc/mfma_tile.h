// mfma_tile.h -- the 32x32 MFMA tile primitives shared by the tiled kernels: vector typedefs, the C/D row map, the XCD-aware
// tile map, the predicated fp32 operand staging, the fp32 K-tile step on v_mfma_f32_32x32x2_f32 and the predicated epilogue of a
// grid of 32x32 accumulator tiles.  __device__ __forceinline__ templates only: barriers, s_setprio and the placement of the next
// tile's loads stay in the kernels, which differ there for measured reasons.  Internal; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace avae {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// two floats -> two bf16 (round to nearest even, v_cvt_pk_bf16_f32), `lo` in the low half
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi)
{
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

constexpr int kTileBK = 32;      // depth of an fp32 K tile
// row stride (floats) of a k-contiguous [x][k] tile in LDS.  Why 36: a fragment read is one ds_read_b128 per lane, 32 rows at one k
// offset; with 4 floats of padding consecutive rows start 4 banks apart, so the 16-byte pieces of a lane group fall on disjoint
// banks (conflict free), and every row stays 16-byte aligned
constexpr int kTileLDK = kTileBK + 4;

// C/D map of a 32x32 MFMA tile (v_mfma_f32_32x32x2_f32, v_mfma_f32_32x32x16_bf16): a lane holds column lane & 31; its accumulator
// element r is row (r & 3) + 8 (r >> 2) + 4 h of the tile, h = lane >> 5
__device__ __forceinline__ constexpr int mfma32_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// XCD-aware tile order: workgroups b, b + 8, b + 16, .. share an XCD (round-robin dispatch); each XCD gets a contiguous run of the
// nblk tiles, so that the tiles it works on at one time share operand panels in its L2.  Run of XCD `xcd`: tiles run0 .. run0 + run_n - 1.
__device__ __forceinline__ void xcd_run(int xcd, int nblk, int& run0, int& run_n)
{
    const int q = nblk >> 3, r = nblk & 7;
    run0 = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    run_n = q + (xcd < r ? 1 : 0);
}
// the tile of virtual block `bid`, or -1 where its XCD's run has no such slot
__device__ __forceinline__ int xcd_tile(int bid, int nblk)
{
    int run0, run_n;
    xcd_run(bid & 7, nblk, run0, run_n);
    const int slot = bid >> 3;
    return slot < run_n ? run0 + slot : -1;
}

// stage one fp32 operand tile (ROWS x 32) global -> ROWS/32 float4 registers per thread of a 256-thread workgroup; elements
// beyond X or K1 read as zero
template <bool XC, int ROWS>   // XC: x(m or n)-contiguous storage [k][x];  else k-contiguous [x][k]
__device__ __forceinline__ void load_tile(float4 (&r)[ROWS / 32], const float* __restrict__ P, int ld,
                                          int x0, int X, int k0, int K1, int tid)
{
#pragma unroll
    for (int rep = 0; rep < ROWS / 32; ++rep) {
        int f = tid + 256 * rep;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (XC) {
            int k = k0 + f / (ROWS / 4), x = x0 + ((f % (ROWS / 4)) << 2);
            if (k < K1 && x < X) v = *reinterpret_cast<const float4*>(P + (size_t)k * ld + x);
        } else {
            int x = x0 + (f >> 3), k = k0 + ((f & 7) << 2);
            if (x < X && k < K1) v = *reinterpret_cast<const float4*>(P + (size_t)x * ld + k);
        }
        r[rep] = v;
    }
}

// .. -> LDS: [k][x] rows of ROWS floats, or [x][k] rows of kTileLDK
template <bool XC, int ROWS>
__device__ __forceinline__ void store_tile(float* __restrict__ s, const float4 (&r)[ROWS / 32], int tid)
{
#pragma unroll
    for (int rep = 0; rep < ROWS / 32; ++rep) {
        int f = tid + 256 * rep;
        if (XC) *reinterpret_cast<float4*>(s + (f / (ROWS / 4)) * ROWS + ((f % (ROWS / 4)) << 2)) = r[rep];
        else    *reinterpret_cast<float4*>(s + (f >> 3) * kTileLDK + ((f & 7) << 2)) = r[rep];
    }
}

template <int TM, int TN>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[TM][TN])
{
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// One 32-deep fp32 K tile of a wave's TM x TN MFMA tiles out of the LDS images As (BM rows) and Bs (BN rows): wave (wm, wn)
// owns rows 32 TM wm .. and columns 32 TN wn ...  MFMA operand map (lane l, h = l >> 5, l31 = l & 31): A[i = l31][k = h],
// B[k = h][j = l31].  Step e of quarter q consumes k = 8 q + 4 h + e in lane half h (any pairing of k indices is a valid
// contraction order as long as both operands use the same one), so a k-contiguous operand row feeds four consecutive steps from
// ONE ds_read_b128.  The MFMA issue order -- q, then e, then i, then j -- fixes the bits of every sum.
template <bool A_MC, bool B_NC, int TM, int TN, int BM, int BN>
__device__ __forceinline__ void mfma_ktile(f32x16 (&acc)[TM][TN], const float* As, const float* Bs, int wm, int wn, int h, int l31)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float a[TM][4], b[TN][4];
#pragma unroll
        for (int t = 0; t < TM; ++t) {
            if (A_MC) {
#pragma unroll
                for (int e = 0; e < 4; ++e) a[t][e] = As[(8 * q + 4 * h + e) * BM + 32 * (wm * TM + t) + l31];
            } else {
                float4 v = *reinterpret_cast<const float4*>(As + (32 * (wm * TM + t) + l31) * kTileLDK + 8 * q + 4 * h);
                a[t][0] = v.x; a[t][1] = v.y; a[t][2] = v.z; a[t][3] = v.w;
            }
        }
#pragma unroll
        for (int t = 0; t < TN; ++t) {
            if (B_NC) {
#pragma unroll
                for (int e = 0; e < 4; ++e) b[t][e] = Bs[(8 * q + 4 * h + e) * BN + 32 * (wn * TN + t) + l31];
            } else {
                float4 v = *reinterpret_cast<const float4*>(Bs + (32 * (wn * TN + t) + l31) * kTileLDK + 8 * q + 4 * h);
                b[t][0] = v.x; b[t][1] = v.y; b[t][2] = v.z; b[t][3] = v.w;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
    }
}

// Predicated epilogue of a wave's TM x TN accumulator tiles, the first at (row0, col0), tile (i, j) 32 i rows and 32 j columns
// on: C = alpha acc + bias[col] where row < M and col < N (a null bias adds +0; BIAS = false: no bias term at all, a -0 product
// stays -0).  Per-element predicate and mode branch: ~40 instructions per element, for edge tiles and split-K; the kernels whose
// whole tiles matter keep a straight-line form of their own.  The bookkeeping between two atomics is load-bearing: issued back to back they ran 25 % slower (gemm_f32.hip, epilogue).
enum { kEpiStore = 0, kEpiAccumulate = 1, kEpiAtomic = 2 };
template <int TM, int TN, bool BIAS = true>
__device__ __forceinline__ void epilogue_generic(const f32x16 (&acc)[TM][TN], float* C, int ldc, int M, int N, int row0, int col0,
                                                 int h, int l31, float alpha, const float* bias, int mode)
{
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = col0 + 32 * j + l31;
        if (col >= N) continue;
        const float bv = (BIAS && bias) ? bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row0 + 32 * i + mfma32_row(r, h);
                if (row >= M) continue;
                const float v = BIAS ? alpha * acc[i][j][r] + bv : alpha * acc[i][j][r];
                float* c = C + (size_t)row * ldc + col;
                if (mode == kEpiAtomic) atomicAdd(c, v);
                else if (mode == kEpiAccumulate) *c += v;
                else *c = v;
            }
        }
    }
}

}  // namespace avae
