// affinity.hip -- affinity propagation of latent rows (contract: include/argsim_vae.h, avae_affinity; host sequence: clustering.cpp;
// DESIGN 4.3k).  Everything works on dense row-major (N, N) fp32 matrices: S the similarities, A the availabilities, R the
// responsibilities.  A call's small state is ApState (kernels.h), zero-filled by the host before the first launch.
//
//   setup      ap_sim_kernel: 16 x 16 pairs per workgroup over the tiles on and above the diagonal, both operands staged in LDS in
//              chunks of 64 dims; per pair ONE chain in double over ascending d (the difference first, then fma), one rounding to
//              fp32, the value written to [i][k] and [k][i]: symmetric by construction, the diagonal an exact +0.
//              ap_hist_kernel / ap_select_kernel: the median of all N^2 entries by a radix select over order_key, 4 passes of 8 bits
//              from the top with integer histograms (LDS, then integer atomics); the two middle ranks ride along in one pass.
//              ap_prep_kernel: the diagonal <- preference, then the perturbation of stream 5.
//   iteration  ap_rows_kernel (a workgroup owns RB rows): one wave per row finds the first maximum, its column and the second
//              maximum of A + S; then every thread walks ITS columns down the RB rows, writes R and sums max(0, R) of the rows i != k
//              in double, ascending i, into the workgroup's row of column partials.
//              ap_cols_kernel (a thread per column): adds the partials in block order, writes A_kk, R_kk + sum as a double, E_k and
//              run_k, and counts the unsettled columns and the exemplars with integer atomics.
//              ap_avail_kernel: A_ik, i != k, elementwise from that vector; thread 0 of workgroup 0 decides the stop.
//   stop       st->stop_at = it + 1 once iteration it ended the loop.  A launch of iteration it returns at once when 0 < stop_at <= it:
//              the workgroups of the deciding launch itself read 0 or it + 1 and carry on either way.  The two counter pairs alternate
//              by iteration parity; the one the next iteration adds into is cleared by the deciding thread (its last reader was the
//              launch before).
//   labels     ap_assign_kernel (rows pass with the exemplar mask), ap_refine_kernel (a thread per column: its cluster's sum in
//              double, ascending i; 64-bit integer atomicMax on (order key, ~j)), ap_promote_kernel, ap_assign_kernel again.
// No kernel waits on another workgroup; every loop is bounded by N, dim or a constant.  No float atomics.
#include "kernels.h"
#include "reduce_dev.h"

#include <float.h>

#include <algorithm>

namespace avae {

namespace {

typedef unsigned long long u64;
constexpr int kSimT = 16, kSimD = 64;      // pairs per side and dims per staged chunk of ap_sim_kernel

__device__ inline float ap_unkey(unsigned k)      // inverse of order_key (key 0, a NaN's, comes back as a NaN)
{
    return (k & 0x80000000u) ? __uint_as_float(k & 0x7fffffffu) : __uint_as_float(~k);
}

__device__ inline bool ap_stopped(const ApState* st, int it)
{
    const int s = st->stop_at;
    return s > 0 && it >= s;
}

// ---------------------------------------------------------------- similarities
// grid = (tiles, tiles), 256 threads; tiles below the diagonal return at once
__global__ __launch_bounds__(256) void ap_sim_kernel(const float* __restrict__ x, int N, int dim, int metric, float* __restrict__ S)
{
    __shared__ float si[kSimT][kSimD + 1], sk[kSimT][kSimD + 1];
    if (blockIdx.x < blockIdx.y) return;
    const int ti = threadIdx.x >> 4, tk = threadIdx.x & 15;
    const int i0 = blockIdx.y * kSimT, k0 = blockIdx.x * kSimT;
    double acc = 0.0, ni = 0.0, nk = 0.0;
    for (int d0 = 0; d0 < dim; d0 += kSimD) {
        for (int e = threadIdx.x; e < kSimT * kSimD; e += 256) {
            const int r = e / kSimD, d = e % kSimD;
            const bool in = d0 + d < dim;
            si[r][d] = (in && i0 + r < N) ? x[(size_t)(i0 + r) * dim + d0 + d] : 0.f;
            sk[r][d] = (in && k0 + r < N) ? x[(size_t)(k0 + r) * dim + d0 + d] : 0.f;
        }
        __syncthreads();
        const int nd = min(kSimD, dim - d0);
        if (metric == 0) {
            for (int d = 0; d < nd; ++d) { const double df = (double)si[ti][d] - (double)sk[tk][d]; acc = fma(df, df, acc); }
        } else {
            for (int d = 0; d < nd; ++d) {
                const double a = si[ti][d], b = sk[tk][d];
                acc = fma(a, b, acc); ni = fma(a, a, ni); nk = fma(b, b, nk);
            }
        }
        __syncthreads();
    }
    const int i = i0 + ti, k = k0 + tk;
    if (i >= N || k >= N || k < i) return;
    float v;
    if (i == k) v = 0.f;
    else if (metric == 0) v = (float)(0.0 - acc);
    else v = (float)(acc / (sqrt(ni) * sqrt(nk)) - 1.0);
    S[(size_t)i * N + k] = v;
    S[(size_t)k * N + i] = v;
}

// ---------------------------------------------------------------- the median of N^2 entries
// pass p (shift 24 - 8 p): the keys that share a rank's prefix so far are counted by their next 8 bits; which = 0 the lower middle
// rank, 1 the upper
__global__ __launch_bounds__(256) void ap_hist_kernel(const float* __restrict__ S, size_t M, int pass, ApState* st)
{
    __shared__ unsigned sh[512];
    sh[threadIdx.x] = 0; sh[256 + threadIdx.x] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const unsigned mask = pass ? ~0u << (shift + 8) : 0u, pa = st->prefix[0], pb = st->prefix[1];
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < M; e += (size_t)gridDim.x * 256) {
        const unsigned key = order_key(S[e]);
        if ((key & mask) == pa) atomicAdd(&sh[(key >> shift) & 255u], 1u);
        if ((key & mask) == pb) atomicAdd(&sh[256 + ((key >> shift) & 255u)], 1u);
    }
    __syncthreads();
    if (sh[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], sh[threadIdx.x]);
    if (sh[256 + threadIdx.x]) atomicAdd(&st->hist[256 + threadIdx.x], sh[256 + threadIdx.x]);
}

// one workgroup of 64: lane 0 / 1 walk their rank's histogram upwards to the bin in which the count crosses the rank, clear the
// histograms for the next pass; after the last pass the median itself
__global__ __launch_bounds__(64) void ap_select_kernel(int pass, unsigned ra, unsigned rb, ApState* st)
{
    __shared__ unsigned sh[512];
    for (int e = threadIdx.x; e < 512; e += 64) { sh[e] = st->hist[e]; st->hist[e] = 0; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int w = threadIdx.x;
        unsigned rank = pass ? st->rank[w] : (w ? rb : ra), below = 0;
        int bin = 255;
        for (int b = 0; b < 256; ++b) {
            const unsigned c = sh[256 * w + b];
            if (rank < below + c) { bin = b; break; }
            below += c;
        }
        st->rank[w] = rank - min(rank, below);
        st->prefix[w] = (pass ? st->prefix[w] : 0u) | ((unsigned)bin << (24 - 8 * pass));
    }
    __syncthreads();
    if (pass == 3 && threadIdx.x == 0) {
        const float lo = ap_unkey(st->prefix[0]), hi = ap_unkey(st->prefix[1]);
        st->pref = ra == rb ? lo : (lo + hi) * 0.5f;
    }
}

// the diagonal <- preference; then S_ik += (2^-23 S_ik + 100 FLT_MIN) normal01(seed, 5, i N + k) in fp32
__global__ __launch_bounds__(256) void ap_prep_kernel(float* __restrict__ S, int N, int use_pref, float pref, int noise, uint64_t seed, const ApState* st)
{
    const float p = use_pref ? pref : st->pref;
    const size_t M = (size_t)N * N, first = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    if (!noise) {
        for (size_t i = first; i < (size_t)N; i += step) S[i * N + i] = p;
        return;
    }
    for (size_t e = first; e < M; e += step) {
        const float s = e % ((size_t)N + 1) == 0 ? p : S[e];
        S[e] = s + (1.1920928955078125e-7f * s + 100.f * FLT_MIN) * normal01(seed, 5, e);
    }
}

// ---------------------------------------------------------------- one iteration
// first maximum (value, column) and the second maximum of a row: the tie rule is cand_better's; a NaN never enters
struct Top2 {
    float m1 = -INFINITY, m2 = -INFINITY; int i1 = 0x7fffffff;
    __device__ __forceinline__ void take(float v, int k)      // ascending k
    {
        if (v > m1) { m2 = m1; m1 = v; i1 = k; }
        else if (v > m2) m2 = v;
    }
    __device__ __forceinline__ void merge(float om1, float om2, int oi1)
    {
        if (cand_better(om1, oi1, m1, i1)) { m2 = fmaxf(m1, om2); m1 = om1; i1 = oi1; }
        else m2 = fmaxf(m2, om1);      // (om2 <= om1)
    }
    __device__ __forceinline__ void wave_merge()
    {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) merge(__shfl_xor(m1, o, 64), __shfl_xor(m2, o, 64), __shfl_xor(i1, o, 64));
    }
};

// grid = row blocks of RB <= kApMaxRB rows
__global__ __launch_bounds__(256) void ap_rows_kernel(const float* __restrict__ S, const float* __restrict__ A, float* __restrict__ R, int N, int RB,
                                                      float lam, int it, double* __restrict__ part, const ApState* st)
{
    __shared__ float sY[kApMaxRB], sY2[kApMaxRB];
    __shared__ int sI[kApMaxRB];
    if (ap_stopped(st, it)) return;
    const int r0 = blockIdx.x * RB, nr = min(RB, N - r0), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < nr; r += 4) {
        const size_t row = (size_t)(r0 + r) * N;
        Top2 t;
#pragma unroll 4
        for (int k = lane; k < N; k += 64) t.take(A[row + k] + S[row + k], k);
        t.wave_merge();
        if (lane == 0) { sY[r] = t.m1; sY2[r] = t.m2; sI[r] = t.i1; }
    }
    __syncthreads();
    const float oml = 1.f - lam;
    for (int k = threadIdx.x; k < N; k += 256) {
        double acc = 0.0;
#pragma unroll 8
        for (int r = 0; r < nr; ++r) {
            const size_t e = (size_t)(r0 + r) * N + k;
            const float y = k == sI[r] ? sY2[r] : sY[r];
            const float rn = lam * R[e] + oml * (S[e] - y);
            R[e] = rn;
            if (r0 + r != k && rn > 0.f) acc += (double)rn;
        }
        part[(size_t)blockIdx.x * N + k] = acc;
    }
}

// grid = ceil(N / 256): a thread per column
__global__ __launch_bounds__(256) void ap_cols_kernel(float* __restrict__ A, const float* __restrict__ R, int N, int nblk, float lam, int it, int conv_iter,
                                                      const double* __restrict__ part, double* __restrict__ cv, int* __restrict__ E, int* __restrict__ run,
                                                      ApState* st)
{
    if (ap_stopped(st, it)) return;
    const int k = blockIdx.x * 256 + threadIdx.x;
    int unsettled = 0, ex = 0;
    if (k < N) {
        double sum = 0.0;
#pragma unroll 8
        for (int b = 0; b < nblk; ++b) sum += part[(size_t)b * N + k];
        const size_t d = (size_t)k * N + k;
        const float rkk = R[d], akk = lam * A[d] + (1.f - lam) * (float)sum;
        A[d] = akk;
        cv[k] = (double)rkk + sum;
        ex = akk + rkk > 0.f ? 1 : 0;
        const int len = (it > 0 && E[k] == ex) ? min(run[k] + 1, 1 << 20) : 1;
        E[k] = ex; run[k] = len;
        unsettled = len < conv_iter ? 1 : 0;
    }
    unsettled = wave_sum(unsettled); ex = wave_sum(ex);
    if ((threadIdx.x & 63) == 0) {
        if (unsettled) atomicAdd(&st->cnt[it & 1][0], unsettled);
        if (ex) atomicAdd(&st->cnt[it & 1][1], ex);
    }
}

// grid = row blocks of RB rows
__global__ __launch_bounds__(256) void ap_avail_kernel(float* __restrict__ A, const float* __restrict__ R, int N, int RB, float lam, int it, int conv_iter,
                                                       const double* __restrict__ cv, ApState* st)
{
    if (ap_stopped(st, it)) return;
    const int r0 = blockIdx.x * RB, nr = min(RB, N - r0);
    const float oml = 1.f - lam;
    for (int k = threadIdx.x; k < N; k += 256) {
        const double c = cv[k];
#pragma unroll 8
        for (int r = 0; r < nr; ++r) {
            if (r0 + r == k) continue;
            const size_t e = (size_t)(r0 + r) * N + k;
            const float rp = R[e], v = (float)(c - (double)(rp > 0.f ? rp : 0.f));
            A[e] = lam * A[e] + oml * (v < 0.f ? v : 0.f);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int unsettled = st->cnt[it & 1][0], K = st->cnt[it & 1][1];
        st->cnt[(it + 1) & 1][0] = 0; st->cnt[(it + 1) & 1][1] = 0;
        st->iters = it + 1; st->K = K;
        if (it >= conv_iter && unsettled == 0 && K > 0) { st->conv = 1; st->stop_at = it + 1; }
    }
}

// ---------------------------------------------------------------- labels
// c_i = argmax over the exemplars k (mask[k] != 0) of S_ik, the lowest k on ties; an exemplar takes itself; -1 where no exemplar's
// similarity is above -inf.  last = 0: into c, and the refinement's words and the next mask are cleared; last = 1: into label (all -1
// without exemplars), and stat.  grid = row blocks of RB rows, one wave per row
__global__ __launch_bounds__(256) void ap_assign_kernel(const float* __restrict__ S, int N, int RB, const int* __restrict__ mask, int last, int32_t* __restrict__ out,
                                                        u64* __restrict__ best, int* __restrict__ next, const ApState* st, int32_t* __restrict__ stat)
{
    const int r0 = blockIdx.x * RB, nr = min(RB, N - r0), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = st->K;
    if (last && blockIdx.x == 0 && threadIdx.x == 0) { stat[0] = st->iters; stat[1] = st->conv; stat[2] = K; stat[3] = 0; }
    if (K <= 0 && !last) return;
    for (int r = wave; r < nr; r += 4) {
        const int i = r0 + r;
        int c = -1;
        if (K > 0) {
            ArgFirst t;
            if (mask[i]) { t.v = 0.f; t.i = i; }
            else {
                const size_t row = (size_t)i * N;
                for (int k = lane; k < N; k += 64) if (mask[k]) t.take(S[row + k], k);
                t.wave_merge();
            }
            c = t.i < N ? t.i : -1;
        }
        if (lane == 0) {
            out[i] = c;
            if (!last) { best[i] = 0; next[i] = 0; }
        }
    }
}

// a thread per column j: the sum of S_ij over the rows of j's cluster in double, ascending i, ONE rounding to fp32
__global__ __launch_bounds__(256) void ap_refine_kernel(const float* __restrict__ S, int N, const int32_t* __restrict__ c, u64* __restrict__ best, const ApState* st)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (st->K <= 0 || j >= N) return;
    const int cj = c[j];
    if (cj < 0 || cj >= N) return;
    double acc = 0.0;
    for (int i = 0; i < N; ++i)
        if (c[i] == cj) acc += (double)S[(size_t)i * N + j];
    atomicMax(&best[cj], ((u64)order_key((float)acc) << 32) | (u64)(unsigned)~j);
}

__global__ __launch_bounds__(256) void ap_promote_kernel(int N, const int* __restrict__ E, const u64* __restrict__ best, int* __restrict__ next, const ApState* st)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (st->K <= 0 || e >= N || !E[e]) return;
    const unsigned j = ~(unsigned)(best[e] & 0xffffffffull);
    next[j < (unsigned)N ? j : (unsigned)e] = 1;
}

__global__ void ap_single_kernel(int32_t* label, int32_t* stat)
{
    label[0] = 0; stat[0] = 0; stat[1] = 1; stat[2] = 1; stat[3] = 0;
}

inline int flat_grid(size_t M) { return (int)std::min<size_t>(2048, (M + 255) / 256); }

#define AP_LAUNCHED() do { const hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

}  // namespace

// rows per workgroup of the row passes, measured: 4 up to 4096 rows, then at most 1024 blocks
int ap_row_block(int N) { return N <= 4096 ? 4 : (N + 1023) / 1024; }

hipError_t ap_single(hipStream_t st, int32_t* label, int32_t* stat)
{
    hipLaunchKernelGGL(ap_single_kernel, dim3(1), dim3(1), 0, st, label, stat);
    return hipGetLastError();
}

hipError_t ap_similarity(hipStream_t st, const float* x, int N, int dim, int metric, float* S)
{
    const int tiles = (N + kSimT - 1) / kSimT;
    hipLaunchKernelGGL(ap_sim_kernel, dim3(tiles, tiles), dim3(256), 0, st, x, N, dim, metric, S);
    return hipGetLastError();
}

hipError_t ap_prepare(hipStream_t st, float* S, int N, int use_pref, float pref, int noise, uint64_t seed, ApState* state)
{
    const size_t M = (size_t)N * N;
    if (!use_pref) {
        for (int pass = 0; pass < 4; ++pass) {
            hipLaunchKernelGGL(ap_hist_kernel, dim3(flat_grid(M)), dim3(256), 0, st, S, M, pass, state);
            AP_LAUNCHED();
            hipLaunchKernelGGL(ap_select_kernel, dim3(1), dim3(64), 0, st, pass, (unsigned)((M - 1) / 2), (unsigned)(M / 2), state);
            AP_LAUNCHED();
        }
    }
    hipLaunchKernelGGL(ap_prep_kernel, dim3(noise ? flat_grid(M) : (N + 255) / 256), dim3(256), 0, st, S, N, use_pref, pref, noise, seed, state);
    return hipGetLastError();
}

hipError_t ap_iteration(hipStream_t st, const ApBuffers& b, int N, float lam, int it, int conv_iter)
{
    const int RB = ap_row_block(N), nblk = (N + RB - 1) / RB;
    hipLaunchKernelGGL(ap_rows_kernel, dim3(nblk), dim3(256), 0, st, b.S, b.A, b.R, N, RB, lam, it, b.part, b.st);
    AP_LAUNCHED();
    hipLaunchKernelGGL(ap_cols_kernel, dim3((N + 255) / 256), dim3(256), 0, st, b.A, b.R, N, nblk, lam, it, conv_iter, b.part, b.cv, b.E, b.run, b.st);
    AP_LAUNCHED();
    hipLaunchKernelGGL(ap_avail_kernel, dim3(nblk), dim3(256), 0, st, b.A, b.R, N, RB, lam, it, conv_iter, b.cv, b.st);
    return hipGetLastError();
}

hipError_t ap_labels(hipStream_t st, const ApBuffers& b, int N, int32_t* label, int32_t* stat)
{
    const int RB = ap_row_block(N), nblk = (N + RB - 1) / RB, cols = (N + 255) / 256;
    hipLaunchKernelGGL(ap_assign_kernel, dim3(nblk), dim3(256), 0, st, b.S, N, RB, b.E, 0, b.c, b.best, b.E2, b.st, stat);
    AP_LAUNCHED();
    hipLaunchKernelGGL(ap_refine_kernel, dim3(cols), dim3(256), 0, st, b.S, N, b.c, b.best, b.st);
    AP_LAUNCHED();
    hipLaunchKernelGGL(ap_promote_kernel, dim3(cols), dim3(256), 0, st, N, b.E, b.best, b.E2, b.st);
    AP_LAUNCHED();
    hipLaunchKernelGGL(ap_assign_kernel, dim3(nblk), dim3(256), 0, st, b.S, N, RB, b.E2, 1, label, b.best, b.E2, b.st, stat);
    return hipGetLastError();
}

}  // namespace avae
