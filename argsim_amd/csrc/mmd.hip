// mmd.hip -- the unbiased kernel two-sample statistic MMD^2_u of latent rows with a permutation null, for G comparisons of 1 + P
// relabelings each over the same N rows (contract: include/argsim_vae.h, avae_mmd / avae_mmd_relabel).  Every value is a
// double; the rows are fp32 and, for the cosine, divided by their double norm where they are loaded.
//
//   mmd_relabel  one workgroup per (comparison g, relabeling p >= 1): the m valid rows with the smallest (key, row) pairs, key =
//                mix64(c + row), by two radix selects over the keys (their high, then their low 32 bits; the keys are recomputed in every
//                pass, nothing of size N is stored), ties at the pivot by ascending row, whole mask words written by ballot
//   mmd_count    one workgroup per comparison: m and n of relabeling 0
//   mmd_pass     grid = row tiles, one launch per pass of relabelings.  A workgroup owns TI rows i and walks the column tiles of 64 (one
//                mask word) from its own word upwards: 32 elements of the rows and of the columns are staged in LDS as doubles (the next
//                stage's loads in flight), 256 threads hold the TI x 64 squared distances in registers and turn them into kernel values
//                in LDS.  Then every (row i, slot s) has ONE owner thread, which adds the tile's k(i, j), j > i ascending, over the
//                columns on the row's own side of the slot (A columns for an A row, B columns for a B row) into acc[i][s] in LDS.  A
//                slot is a relabeling of the pass or, behind them, the valid rows of a comparison of the pass (U_LL).  After the last
//                tile the rows of a slot are summed by the balanced tree over adjacent rows -> part[tile][side][slot].  A column tile
//                none of whose rows is valid in a comparison that has valid rows in the row tile is skipped.
//   mmd_reduce   thread per (side, slot): the row tiles of a 64-row word by the same tree, then the words ascending -> sums, ull
//   mmd_witness  the same walk as mmd_pass over ALL column tiles (j != i) for relabeling 0 of every comparison -> witness
//   mmd_stat     one workgroup per comparison: |A| = m of every relabeling, stat, pvalue
// The sums have one order, fixed by N alone: columns ascending inside a row, the 64 rows of a word by the balanced binary tree over
// adjacent rows, words ascending.  No float atomics.  Compiled with -ffp-contract=off: every TI computes the same operations.
#include "kernels.h"
#include "reduce_dev.h"
#include "rows_dev.h"

#include <algorithm>

namespace avae {

namespace {

constexpr int TJ = 64, DK = kMmdDK;
typedef unsigned long long u64;

// the bits of word jt that are rows < N
__device__ __forceinline__ u64 word_rows(int jt, int N)
{
    const int left = N - 64 * jt;
    return left >= 64 ? ~0ull : (left <= 0 ? 0ull : ((1ull << left) - 1ull));
}

__global__ __launch_bounds__(256) void mmd_rownorm_kernel(const float* __restrict__ x, int N, int dim, double* __restrict__ rn)
{
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const double v = wave_row_norm(x, row, dim);
    if ((threadIdx.x & 63) == 0) rn[row] = v;
}

// the sum of one int per thread over the four waves, in every thread; sh: 4 ints; ends in a barrier
__device__ __forceinline__ int block_isum(int v, int* sh)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const int s = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return s;
}

// m = |valid & inA|, n = |valid & ~inA| of relabeling p of comparison g over the rows < N (every thread gets both)
__device__ __forceinline__ void side_counts(const u64* __restrict__ valid, const u64* __restrict__ in, int N, int W, int* sh, int* m, int* n)
{
    int cm = 0, cn = 0;
    for (int w = threadIdx.x; w < W; w += 256) {
        const u64 v = valid[w] & word_rows(w, N), a = in[w];
        cm += __popcll(v & a); cn += __popcll(v & ~a);
    }
    *m = block_isum(cm, sh); *n = block_isum(cn, sh);
}

__global__ __launch_bounds__(256) void mmd_count_kernel(const u64* __restrict__ valid, const u64* __restrict__ inA, int N, int W, int P, int* __restrict__ counts)
{
    __shared__ int sh[4];
    const int g = blockIdx.x;
    int m, n;
    side_counts(valid + (size_t)g * W, inA + (size_t)g * (1 + P) * W, N, W, sh, &m, &n);
    if (threadIdx.x == 0) { counts[2 * g] = m; counts[2 * g + 1] = n; }
}

// ---------------------------------------------------------------- generated relabelings
__global__ __launch_bounds__(256) void mmd_relabel_kernel(const u64* __restrict__ valid, u64* __restrict__ inA, int N, int W, int P, uint64_t base)
{
    __shared__ unsigned sh[258];
    __shared__ int shi[4];
    const int g = blockIdx.y, p = 1 + blockIdx.x, tid = threadIdx.x;
    const u64* v = valid + (size_t)g * W;
    u64* out = inA + ((size_t)g * (1 + P) + p) * W;
    int m, nb;
    side_counts(v, inA + (size_t)g * (1 + P) * W, N, W, shi, &m, &nb);
    if (m == 0) { for (int w = tid; w < W; w += 256) out[w] = 0ull; return; }
    const uint64_t c = mix64(base + (((uint64_t)(unsigned)g << 32) | (uint64_t)(unsigned)p));
    auto is_valid = [&](int i) { return ((v[i >> 6] >> (i & 63)) & 1ull) != 0; };
    // the m-th smallest key = the m-th largest inverted key: its high half, then among the keys that share it the low half
    unsigned need1 = 0, ties1 = 0, need2 = 0, ties2 = 0;
    const unsigned hi = kth_largest_key([&](auto f) {
        for (int i = tid; i < N; i += 256) if (is_valid(i)) f((unsigned)(~mix64(c + (uint64_t)i) >> 32));
    }, (unsigned)m, sh, &need1, &ties1);
    const unsigned lo = kth_largest_key([&](auto f) {
        for (int i = tid; i < N; i += 256) if (is_valid(i)) { const uint64_t k = ~mix64(c + (uint64_t)i); if ((unsigned)(k >> 32) == hi) f((unsigned)k); }
    }, need1, sh, &need2, &ties2);
    const uint64_t pivot = ~(((uint64_t)hi << 32) | (uint64_t)lo);
    // rows below the pivot are in; of the ties2 rows at the pivot the first need2 in ascending row order
    const int lane = tid & 63, wave = tid >> 6;
    int seen = 0;                                   // rows at the pivot before this chunk (only counted where not all of them are in)
    for (int base_row = 0; base_row < 64 * W; base_row += 256) {
        const int i = base_row + tid;
        bool in = false, tie = false;
        if (i < N && is_valid(i)) { const uint64_t k = mix64(c + (uint64_t)i); in = k < pivot; tie = k == pivot; }
        if (need2 == ties2) in = in || tie;
        else {                                      // (uniform: every thread takes this branch or none)
            const u64 tb = __ballot(tie);
            if (lane == 0) shi[wave] = __popcll(tb);
            __syncthreads();
            int before = seen;
            for (int w = 0; w < wave; ++w) before += shi[w];
            before += __popcll(tb & ((1ull << lane) - 1ull));
            if (tie && before < (int)need2) in = true;
            seen += shi[0] + shi[1] + shi[2] + shi[3];
            __syncthreads();
        }
        const u64 word = __ballot(in);
        const int w = (base_row >> 6) + wave;
        if (lane == 0 && w < W) out[w] = word;
    }
}

// ---------------------------------------------------------------- the pair pass
__device__ __forceinline__ double kernel_value(const MmdArgs& a, double d2)
{
    if (a.kernel == 1) return -sqrt(d2);
    double k = 0.0;
    for (int b = 0; b < a.nbw; ++b) k += exp(-(a.gamma[b] * d2));
    return k;
}

// the balanced tree over the rows [lo, lo + n) of slot s (n a power of two): adjacent rows first
template <int n>
__device__ __forceinline__ double row_tree(const double* acc, int ns, int s, int lo, u64 bits)
{
    if constexpr (n == 1) return ((bits >> lo) & 1ull) ? acc[(size_t)lo * ns + s] : 0.0;
    else return row_tree<n / 2>(acc, ns, s, lo, bits) + row_tree<n / 2>(acc, ns, s, lo + n / 2, bits);
}

// WIT = false: the relabelings [q0, q0 + nq) and behind them the valid rows of their comparisons; pairs j > i.
// WIT = true: relabeling 0 of every comparison, slot g the A columns and slot G + g the B columns of comparison g; pairs j != i.
// Dynamic LDS, laid out as mmd_lds counts it.
template <int TI, bool WIT>
__global__ __launch_bounds__(256) void mmd_pass_kernel(MmdArgs a, int q0, int nq)
{
    constexpr int NTY = TI < 16 ? TI : 16, RI = TI / NTY, NTX = 256 / NTY, CJ = TJ / NTX;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x, ty = tid / NTX, tx = tid % NTX;
    const int N = a.N, dim = a.dim, W = a.W, P1 = 1 + a.P;
    const int g0 = WIT ? 0 : q0 / P1, nc = WIT ? a.G : (q0 + nq - 1) / P1 - g0 + 1;
    const int ns = WIT ? 2 * a.G : nq + nc;
    double* acc = smem;
    double* Kt = acc + (size_t)ns * TI;
    double* xi = Kt + TI * TJ;
    double* xj = xi + DK * TI;
    double* rni = xj + DK * TJ;
    double* rnj = rni + TI;
    u64* colA = reinterpret_cast<u64*>(rnj + TJ);
    u64* colB = colA + ns;
    u64* rowA = colB + ns;
    u64* rowB = rowA + ns;
    u64* rowV = rowB + ns;                              // kMmdMaxG words: the valid rows of the tile per comparison of the pass
    unsigned char* on = reinterpret_cast<unsigned char*>(rowV + kMmdMaxG);
    const int row0 = blockIdx.x * TI;
    const int nrow = min(TI, N - row0);
    const int jd = row0 >> 6, sh0 = row0 & 63;          // the rows' own word and their first bit in it
    const u64 tile_rows = (TI == 64 ? ~0ull : ((1ull << TI) - 1ull)) & (word_rows(jd, N) >> sh0);

    // slot s -> its comparison and the word row of its relabeling; a slot behind the relabelings is the valid rows of a comparison
    auto slot_g = [&](int s) { return WIT ? (s < a.G ? s : s - a.G) : (s < nq ? (q0 + s) / P1 : g0 + s - nq); };
    auto slot_in = [&](int s, int g) -> const u64* {
        if (WIT) return a.inA + (size_t)g * P1 * W;
        return s < nq ? a.inA + (size_t)(q0 + s) * W : nullptr;
    };
    for (int s = tid; s < ns; s += 256) {
        const int g = slot_g(s);
        const u64 v = (a.valid[(size_t)g * W + jd] >> sh0) & tile_rows;
        const u64* in = slot_in(s, g);
        const u64 ia = in ? in[jd] >> sh0 : ~0ull;
        rowA[s] = v & ia; rowB[s] = v & ~ia;
    }
    for (int c = tid; c < nc; c += 256) rowV[c] = (a.valid[(size_t)(g0 + c) * W + jd] >> sh0) & tile_rows;
    for (int q = tid; q < ns * TI; q += 256) acc[q] = 0.0;
    if (tid < TI) rni[tid] = tid < nrow ? (a.rnorm ? a.rnorm[row0 + tid] : -1.0) : 0.0;
    __syncthreads();
    const int jfirst = WIT ? 0 : jd;
    for (int jt = tid; jt < W; jt += 256) {
        bool need = false;
        if (jt >= jfirst) {
            const u64 wr = word_rows(jt, N);
            for (int c = 0; c < nc; ++c) need = need || (rowV[c] != 0ull && (a.valid[(size_t)(g0 + c) * W + jt] & wr) != 0ull);
        }
        on[jt] = need ? 1 : 0;
    }
    __syncthreads();
    auto next_on = [&](int j) { while (j < W && !on[j]) ++j; return j; };

    int cr[2], ce[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) { const int idx = tid + 256 * u; cr[u] = idx / (DK / 4); ce[u] = 4 * (idx % (DK / 4)); }
    float4 pi[2], pj[2];
    auto fetch = [&](int col0, int j0) {
        const int ncol = min(TJ, N - col0);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int col = j0 + ce[u];
            pi[u] = make_float4(0.f, 0.f, 0.f, 0.f); pj[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (cr[u] < nrow && col < dim) pi[u] = *reinterpret_cast<const float4*>(a.x + (size_t)(row0 + cr[u]) * dim + col);
            if (cr[u] < ncol && col < dim) pj[u] = *reinterpret_cast<const float4*>(a.x + (size_t)(col0 + cr[u]) * dim + col);
        }
    };
    int jt = next_on(jfirst);
    if (jt < W) fetch(64 * jt, 0);
    while (jt < W) {
        const int jn = next_on(jt + 1);
        const int col0 = 64 * jt, ncol = min(TJ, N - col0);
        const u64 wr = word_rows(jt, N);
        for (int s = tid; s < ns; s += 256) {
            const int g = slot_g(s);
            const u64 v = a.valid[(size_t)g * W + jt] & wr;
            const u64* in = slot_in(s, g);
            const u64 ia = in ? in[jt] : ~0ull;
            if (WIT) { const u64 w = s < a.G ? (v & ia) : (v & ~ia); colA[s] = w; colB[s] = w; }
            else { colA[s] = v & ia; colB[s] = v & ~ia; }
        }
        if (tid < TJ) rnj[tid] = tid < ncol ? (a.rnorm ? a.rnorm[col0 + tid] : -1.0) : 0.0;
        double d2[RI][CJ];
#pragma unroll
        for (int i = 0; i < RI; ++i)
#pragma unroll
            for (int j = 0; j < CJ; ++j) d2[i][j] = 0.0;
        for (int j0 = 0; j0 < dim; j0 += DK) {
            __syncthreads();                                    // the stage is free (and, the first time, the column words and rnj are written)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int rl = cr[u], e0 = ce[u];
                const bool in = j0 + e0 < dim;
                if (rl < TI) stage_row4(xi, TI, e0, rl, pi[u], rni[rl], in && rl < nrow);
                stage_row4(xj, TJ, e0, rl, pj[u], rnj[rl], in && rl < ncol);
            }
            __syncthreads();
            if (j0 + DK < dim) fetch(col0, j0 + DK);
            else if (jn < W) fetch(64 * jn, 0);
#pragma unroll 4
            for (int j = 0; j < DK; ++j) {
                double xa[RI], ca[CJ];
#pragma unroll
                for (int i = 0; i < RI; ++i) xa[i] = xi[j * TI + ty * RI + i];
#pragma unroll
                for (int q = 0; q < CJ; ++q) ca[q] = xj[j * TJ + tx * CJ + q];
#pragma unroll
                for (int i = 0; i < RI; ++i)
#pragma unroll
                    for (int q = 0; q < CJ; ++q) { const double d = xa[i] - ca[q]; d2[i][q] = fma(d, d, d2[i][q]); }
            }
        }
#pragma unroll
        for (int i = 0; i < RI; ++i)
#pragma unroll
            for (int q = 0; q < CJ; ++q) Kt[(ty * RI + i) * TJ + tx * CJ + q] = kernel_value(a, d2[i][q]);
        __syncthreads();
        // the owner of (row i, slot s) adds the tile's columns in ascending j: the columns on the row's own side, behind the row itself
        for (int e = tid; e < ns * TI; e += 256) {
            const int i = e / ns, s = e - i * ns;
            u64 w = ((rowA[s] >> i) & 1ull) ? colA[s] : (((rowB[s] >> i) & 1ull) ? colB[s] : 0ull);
            if (jt == jd) {
                const int b = sh0 + i;
                w &= WIT ? ~(1ull << b) : (b >= 63 ? 0ull : (~0ull << (b + 1)));
            }
            if (w == 0ull) continue;
            const double* kr = Kt + i * TJ;
            double r = acc[e];
#pragma unroll
            for (int j = 0; j < TJ; j += 2) {
                const double2 k2 = *reinterpret_cast<const double2*>(kr + j);
                r += ((w >> j) & 1ull) ? k2.x : 0.0;
                r += ((w >> (j + 1)) & 1ull) ? k2.y : 0.0;
            }
            acc[e] = r;
        }
        __syncthreads();                                        // Kt and the column words are free for the next tile
        jt = jn;
    }

    if (WIT) {
        for (int e = tid; e < a.G * TI; e += 256) {
            const int i = e / a.G, g = e - i * a.G;
            if (i >= nrow) continue;
            double w = 0.0;
            const bool ia = (rowA[g] >> i) & 1ull, ib = (rowB[g] >> i) & 1ull;
            if (ia || ib) {
                const double m = (double)(a.counts[2 * g] - (ia ? 1 : 0)), n = (double)(a.counts[2 * g + 1] - (ib ? 1 : 0));
                w = acc[(size_t)i * ns + g] / m - acc[(size_t)i * ns + a.G + g] / n;
            }
            a.witness[(size_t)g * N + row0 + i] = w;
        }
    } else {
        double* out = a.part + (size_t)blockIdx.x * 2 * a.cap;
        for (int s = tid; s < ns; s += 256) {
            out[s] = row_tree<TI>(acc, ns, s, 0, rowA[s]);
            out[a.cap + s] = row_tree<TI>(acc, ns, s, 0, rowB[s]);
        }
    }
}

// the partial of word wd for (side, slot): its 64 / TI row tiles [t0, t0 + n) by the tree over adjacent tiles
template <int n>
__device__ __forceinline__ double tile_tree(const double* __restrict__ part, size_t stride, int t0, int tiles)
{
    if constexpr (n == 1) return t0 < tiles ? part[(size_t)t0 * stride] : 0.0;
    else return tile_tree<n / 2>(part, stride, t0, tiles) + tile_tree<n / 2>(part, stride, t0 + n / 2, tiles);
}

__global__ __launch_bounds__(256) void mmd_reduce_kernel(MmdArgs a, int q0, int nq, int ns, int TI, int tiles)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * ns) return;
    const int side = e / ns, s = e - side * ns;
    if (s >= nq && side == 1) return;
    const double* part = a.part + (size_t)side * a.cap + s;
    const size_t stride = 2 * (size_t)a.cap;
    const int per = 64 / TI;
    double tot = 0.0;
    for (int wd = 0; wd < a.W; ++wd) {
        double t;
        switch (per) {
            case 1: t = tile_tree<1>(part, stride, wd, tiles); break;
            case 2: t = tile_tree<2>(part, stride, 2 * wd, tiles); break;
            case 4: t = tile_tree<4>(part, stride, 4 * wd, tiles); break;
            default: t = tile_tree<8>(part, stride, 8 * wd, tiles); break;
        }
        tot += t;
    }
    if (s < nq) a.sums[2 * (size_t)(q0 + s) + side] = tot;
    else a.ull[q0 / (1 + a.P) + s - nq] = tot;
}

// ---------------------------------------------------------------- the statistic
__global__ __launch_bounds__(256) void mmd_stat_kernel(MmdArgs a, double* __restrict__ stat, double* __restrict__ pvalue, unsigned* __restrict__ bad)
{
    __shared__ int shi[4];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, P1 = 1 + a.P, W = a.W;
    const int m = a.counts[2 * g], n = a.counts[2 * g + 1];
    const u64* v = a.valid + (size_t)g * W;
    // |A| = m of every relabeling: a wave per relabeling, the first violation of the call by an integer minimum
    for (int p = 1 + wave; p < P1; p += 4) {
        const u64* in = a.inA + ((size_t)g * P1 + p) * W;
        int c = 0;
        for (int w = lane; w < W; w += 64) c += __popcll(v[w] & in[w] & word_rows(w, a.N));
        c = wave_sum(c);
        if (lane == 0 && c != m) atomicMin(bad, (unsigned)(g * P1 + p));
    }
    const double dm = (double)m, dn = (double)n, ull = a.ull[g];
    auto value = [&](int p) {
        const double uaa = a.sums[2 * ((size_t)g * P1 + p)], ubb = a.sums[2 * ((size_t)g * P1 + p) + 1];
        const double uab = ull - uaa - ubb;
        return 2.0 * uaa / (dm * (dm - 1.0)) + 2.0 * ubb / (dn * (dn - 1.0)) - 2.0 * uab / (dm * dn);
    };
    const double s0 = value(0);
    int ge = 0;
    for (int p = tid; p < P1; p += 256) {
        const double sv = value(p);
        stat[(size_t)g * P1 + p] = sv;
        if (p >= 1 && sv >= s0) ++ge;
    }
    ge = block_isum(ge, shi);
    if (tid == 0) pvalue[g] = (double)(1 + ge) / (double)P1;
}

__global__ void mmd_flag_kernel(const unsigned* __restrict__ bad, int32_t* __restrict__ stat_out)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *stat_out = *bad == 0xffffffffu ? 0 : (int32_t)(*bad + 1u);
}

template <int TI, bool WIT>
hipError_t launch_pass(hipStream_t st, const MmdArgs& a, int tiles, int q0, int nq, size_t lds)
{
    auto kernel = mmd_pass_kernel<TI, WIT>;
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMmdLds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(tiles), dim3(256), lds, st, a, q0, nq);
    return hipGetLastError();
}

template <bool WIT>
hipError_t launch_ti(hipStream_t st, const MmdArgs& a, int TI, int tiles, int q0, int nq, size_t lds)
{
    switch (TI) {
        case 8: return launch_pass<8, WIT>(st, a, tiles, q0, nq, lds);
        case 16: return launch_pass<16, WIT>(st, a, tiles, q0, nq, lds);
        case 32: return launch_pass<32, WIT>(st, a, tiles, q0, nq, lds);
        case 64: return launch_pass<64, WIT>(st, a, tiles, q0, nq, lds);
    }
    return hipErrorInvalidValue;
}

// the comparisons that the relabelings [q0, q0 + nq) belong to
int pass_comparisons(int q0, int nq, int P) { return (q0 + nq - 1) / (1 + P) - q0 / (1 + P) + 1; }

}  // namespace

size_t mmd_lds(int TI, int ns, int W)
{
    return 8 * ((size_t)ns * TI + (size_t)TI * TJ + (size_t)DK * TI + DK * TJ + TI + TJ + 4 * (size_t)ns + kMmdMaxG) + (size_t)((W + 7) & ~7);
}

// TI: 32 rows, halved down to 8 while there are fewer row tiles than CUs; with the option the largest of 8 .. 64 within it (at least 8).
// nq: as many relabelings per pass as fit the LDS beside the staging (counting the most comparisons a pass of nq can touch), within the
// option.  dim does not enter: the rows are staged 32 elements at a time.
MmdPlan mmd_plan(int N, int dim, int G, int P, int chunk_opt, int cus)
{
    (void)dim;
    MmdPlan p{};
    const int W = (N + 63) / 64, Q = G * (1 + P);
    int ti = 32;
    if (chunk_opt > 0) { ti = 8; while (ti < 64 && 2 * ti <= chunk_opt) ti *= 2; }
    else while (ti > 8 && (N + ti - 1) / ti < cus) ti /= 2;
    int nq = chunk_opt > 0 ? std::min(chunk_opt, Q) : Q;
    auto most = [&](int n) { return std::min(G, (n - 1) / (1 + P) + 2); };
    while (nq > 1 && mmd_lds(ti, nq + most(nq), W) > (size_t)kMmdLds) --nq;
    p.TI = ti; p.nq = nq; p.npass = (Q + nq - 1) / nq; p.tiles = (N + ti - 1) / ti; p.W = W;
    p.cap = nq + most(nq);
    p.lds = 0;
    for (int q0 = 0; q0 < Q; q0 += nq) {
        const int n = std::min(nq, Q - q0);
        p.lds = std::max(p.lds, (int)mmd_pass_lds(p, q0, n, P));
    }
    return p;
}

size_t mmd_pass_lds(const MmdPlan& p, int q0, int nq, int P) { return mmd_lds(p.TI, nq + pass_comparisons(q0, nq, P), p.W); }

hipError_t mmd_relabel(hipStream_t st, const unsigned long long* valid, unsigned long long* inA, int N, int G, int P, uint64_t seed)
{
    if (P < 1) return hipSuccess;
    uint64_t x = seed ^ (8ULL * 0xD6E8FEB86659FD93ULL);      // stream 8 of the generator (sample_dev.h): mix64 on the host
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    x ^= x >> 31;
    mmd_relabel_kernel<<<dim3(P, G), 256, 0, st>>>(valid, inA, N, (N + 63) / 64, P, x);
    return hipGetLastError();
}

hipError_t mmd_prepare(hipStream_t st, const MmdArgs& a, int* counts)
{
    if (a.rnorm) mmd_rownorm_kernel<<<(a.N + 3) / 4, 256, 0, st>>>(a.x, a.N, a.dim, const_cast<double*>(a.rnorm));
    mmd_count_kernel<<<a.G, 256, 0, st>>>(a.valid, a.inA, a.N, a.W, a.P, counts);
    return hipGetLastError();
}

hipError_t mmd_pairs(hipStream_t st, const MmdArgs& a, const MmdPlan& p)
{
    const int Q = a.G * (1 + a.P);
    for (int q0 = 0; q0 < Q; q0 += p.nq) {
        const int nq = std::min(p.nq, Q - q0), ns = nq + pass_comparisons(q0, nq, a.P);
        hipError_t e = launch_ti<false>(st, a, p.TI, p.tiles, q0, nq, mmd_pass_lds(p, q0, nq, a.P));
        if (e != hipSuccess) return e;
        mmd_reduce_kernel<<<(2 * ns + 255) / 256, 256, 0, st>>>(a, q0, nq, ns, p.TI, p.tiles);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t mmd_witness(hipStream_t st, const MmdArgs& a, const MmdPlan& p)
{
    return launch_ti<true>(st, a, p.TI, p.tiles, 0, a.G, mmd_lds(p.TI, 2 * a.G, p.W));
}

hipError_t mmd_stats(hipStream_t st, const MmdArgs& a, double* stat, double* pvalue, unsigned* bad, int32_t* stat_out)
{
    mmd_stat_kernel<<<a.G, 256, 0, st>>>(a, stat, pvalue, bad);
    mmd_flag_kernel<<<1, 64, 0, st>>>(bad, stat_out);
    return hipGetLastError();
}

}  // namespace avae
