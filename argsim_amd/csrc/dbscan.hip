// dbscan.hip -- density clustering (DBSCAN) of latent rows (contract: include/argsim_vae.h, avae_dbscan).  The pair values
// are doubles; the rows are fp32 and, for the cosine, divided by their double norm where they are loaded.  Everything behind the pair
// pass is integer work on the bit matrix adj[N][W], W = ceil(N / 64): 2 GiB at N = 2^17, which is why N stops there.
//
//   db_pairs     grid = (row tiles, column parts).  A workgroup owns TI rows i and walks its part's columns j in ascending tiles of 64: 32
//                elements of the rows and of the columns are staged in LDS as doubles (the next stage's loads in flight), 256 threads hold
//                the TI x 64 pair sums p(i, j) = sum_e (v_i[e] - v_j[e])^2 in registers, the elements in ascending order whatever TI is.
//                p IS SYMMETRIC BY CONSTRUCTION: (a - b)^2 and (b - a)^2 are the same double, v is the same double whether a row is staged
//                as a row or as a column, and the order of the sum is fixed -- the hooks below rely on adj[i][j] == adj[j][i].  The
//                comparison p <= thr gives a thread its bits of the tile's 64-bit word; the threads of a row OR them into the word in LDS
//                (an integer OR: no order), one thread per row stores the word (a vector store) and counts its bits.  Columns >= N give 0
//                bits.  The (N, N) doubles never reach memory; no float atomics.
//   db_core      core[i] = count[i] >= min_samples as a bit mask (a wave's ballot is the word); the three parent arrays = identity
//   db_hook      round t, one wave per core row: m = the minimum of P[j] over the core bits j of the row (the row's own bit among them).
//                If m < P[i], atomicMin(Q[P[i]], m) and atomicMin(Q[i], m), and round t + 1 has work.  P is only read, Q only written
//                (Q = P on entry): integer minima, whose outcome does not depend on the interleaving.
//   db_jump      P[i] = the root of i in Q (Q only read), and the same into the array the next hook writes.  Hence every round's result,
//                and the number of rounds, is a function of the input alone: tests/dbscan_ref.py restates the rule on the CPU.
//                A round that finds flag[t] == 0 returns at once.  At the fixed point P[i] is the lowest core row of i's component.
//   db_verify    one wave per core row: any core bit j with P[j] != P[i] sets the flag
//   db_number    one workgroup: the exclusive prefix count of the roots (P[i] == i), thread t the rows [t c, t c + c), then the threads'
//                counts in ascending order
//   db_label     one wave per row: a core row takes its root's number; a non-core row the minimum over its core bits, or -1
//   db_stat      one workgroup: integer counts
#include "kernels.h"
#include "reduce_dev.h"
#include "row_parts.h"
#include "rows_dev.h"

#include <algorithm>

namespace avae {

namespace {

constexpr int TJ = kDbTJ, DK = kDbDK;
typedef unsigned long long u64;

__global__ __launch_bounds__(256) void db_rownorm_kernel(const float* __restrict__ x, int N, int dim, double* __restrict__ rn)
{
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const double v = wave_row_norm(x, row, dim);
    if ((threadIdx.x & 63) == 0) rn[row] = v;
}

// ---------------------------------------------------------------- the pair pass
// column tiles [blockIdx.y * chunk, .. + chunk) of the W.  Thread (ty, tx) holds the rows ty RI + i and the columns tx + NTX q of a
// tile: at a fixed q the threads of a wave read consecutive doubles of the column stage.
template <int TI>
__global__ __launch_bounds__(256) void db_pairs_kernel(DbArgs a, int chunk)
{
    constexpr int NTY = TI < 16 ? TI : 16, RI = TI / NTY, NTX = 256 / NTY, CJ = TJ / NTX;
    __shared__ __attribute__((aligned(16))) double xi[DK * TI];
    __shared__ __attribute__((aligned(16))) double xj[DK * TJ];
    __shared__ double rni[TI], rnj[TJ];
    __shared__ u64 word[TI];
    const int tid = threadIdx.x, ty = tid / NTX, tx = tid % NTX;
    const int N = a.N, dim = a.dim;
    const int row0 = blockIdx.x * TI;
    const int nrow = min(TI, N - row0);
    const int tile0 = blockIdx.y * chunk, tile1 = min(tile0 + chunk, a.W);
    const bool cosine = a.rnorm != nullptr;
    const double thr = a.thr;

    if (tid < TI) { rni[tid] = tid < nrow ? (cosine ? a.rnorm[row0 + tid] : -1.0) : 0.0; word[tid] = 0; }
    int cnt = 0;                                                // thread tid < TI: the bits of row tid in this part
    __syncthreads();

    // what this thread stages: per stage of DK elements two float4 of the columns (tile row cr[u], elements ce[u] ..) and, where TI
    // reaches that far, of the rows.  The loads of the next stage -- of the next tile's first, at a tile's last -- are issued before the
    // pair sums of this one and stay in flight behind them
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
    if (tile0 < tile1) fetch(tile0 * TJ, 0);
    for (int t = tile0; t < tile1; ++t) {
        const int col0 = t * TJ;
        const int ncol = min(TJ, N - col0);
        if (tid < TJ) rnj[tid] = tid < ncol ? (cosine ? a.rnorm[col0 + tid] : -1.0) : 0.0;
        double acc[RI][CJ];
#pragma unroll
        for (int i = 0; i < RI; ++i)
#pragma unroll
            for (int q = 0; q < CJ; ++q) acc[i][q] = 0.0;
        for (int j0 = 0; j0 < dim; j0 += DK) {
            __syncthreads();                                    // the stage is free (and, the first time, rnj is written)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int rl = cr[u], e0 = ce[u];
                const bool in = j0 + e0 < dim;
                if (rl < TI) stage_row4(xi, TI, e0, rl, pi[u], rni[rl], in && rl < nrow);
                stage_row4(xj, TJ, e0, rl, pj[u], rnj[rl], in && rl < ncol);
            }
            __syncthreads();
            if (j0 + DK < dim) fetch(col0, j0 + DK);
            else if (t + 1 < tile1) fetch(col0 + TJ, 0);
#pragma unroll 4
            for (int j = 0; j < DK; ++j) {
                double xa[RI], ca[CJ];
#pragma unroll
                for (int i = 0; i < RI; ++i) xa[i] = xi[j * TI + ty * RI + i];
#pragma unroll
                for (int q = 0; q < CJ; ++q) ca[q] = xj[j * TJ + tx + NTX * q];
#pragma unroll
                for (int i = 0; i < RI; ++i)
#pragma unroll
                    for (int q = 0; q < CJ; ++q) { const double d = xa[i] - ca[q]; acc[i][q] = fma(d, d, acc[i][q]); }
            }
        }
        // the thread's bits of the word of each of its rows.  Cosine: a pair with a zero row has p = 2 (distance 1) unless i == j
#pragma unroll
        for (int i = 0; i < RI; ++i) {
            const int rl = ty * RI + i;
            u64 bits = 0;
#pragma unroll
            for (int q = 0; q < CJ; ++q) {
                const int cl = tx + NTX * q;
                double p = acc[i][q];
                if (cosine && (rni[rl] == 0.0 || rnj[cl] == 0.0) && row0 + rl != col0 + cl) p = 2.0;
                if (p <= thr && rl < nrow && cl < ncol) bits |= (u64)1 << cl;
            }
            if (bits) atomicOr(&word[rl], bits);
        }
        __syncthreads();
        if (tid < TI) {                                         // (the next ORs come behind the next stage's barriers)
            const u64 w = word[tid];
            word[tid] = 0;
            if (tid < nrow) { a.adj[(size_t)(row0 + tid) * a.W + t] = w; cnt += __popcll(w); }
        }
    }
    if (tid < nrow && cnt) atomicAdd(&a.count[row0 + tid], cnt);
}

// ---------------------------------------------------------------- core rows
__global__ __launch_bounds__(256) void db_core_kernel(DbArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;               // a wave holds the 64 rows of one mask word
    const bool core = i < a.N && a.count[i] >= a.min_samples;
    const u64 m = __ballot(core);
    if ((threadIdx.x & 63) == 0 && (i >> 6) < a.W) a.cmask[i >> 6] = m;
    if (i < a.N) { a.par[0][i] = i; a.par[1][i] = i; a.par[2][i] = i; }
    if (i == 0) a.flag[0] = 1;
}

__device__ __forceinline__ bool is_core(const DbArgs& a, int i) { return (a.cmask[i >> 6] >> (i & 63)) & 1; }

__device__ __forceinline__ int wave_min_int(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// the minimum of val[j] over the core bits j of row i, by one wave (lane l the words l, l + 64 ..); 0x7fffffff where there is none
__device__ __forceinline__ int core_row_min(const DbArgs& a, int i, const int* __restrict__ val)
{
    const u64* row = a.adj + (size_t)i * a.W;
    int m = 0x7fffffff;
    for (int w = threadIdx.x & 63; w < a.W; w += 64) {
        u64 b = row[w] & a.cmask[w];
        while (b) { const int j = w * 64 + __ffsll((long long)b) - 1; b &= b - 1; m = min(m, val[j]); }
    }
    return wave_min_int(m);
}

__global__ __launch_bounds__(256) void db_hook_kernel(DbArgs a, int t, const int* __restrict__ P, int* __restrict__ Q)
{
    if (a.flag[t] == 0) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.st->rounds = t + 1;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.N || !is_core(a, i)) return;
    const int m = core_row_min(a, i, P);
    if ((threadIdx.x & 63) == 0) {
        const int r = P[i];
        if (m < r) { atomicMin(&Q[r], m); atomicMin(&Q[i], m); a.flag[t + 1] = 1; }
    }
}

__global__ __launch_bounds__(256) void db_jump_kernel(DbArgs a, int t, const int* __restrict__ Q, int* __restrict__ P, int* __restrict__ R)
{
    if (a.flag[t + 1] == 0) return;                             // the hook changed nothing: Q = P
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N || !is_core(a, i)) return;
    int p = Q[i];
    for (int q = Q[p]; q != p; q = Q[p]) p = q;                 // Q[p] < p until the root: at most N steps
    P[i] = p; R[i] = p;
}

__global__ __launch_bounds__(256) void db_verify_kernel(DbArgs a)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.N || !is_core(a, i)) return;
    const int* P = a.par[0];
    const u64* row = a.adj + (size_t)i * a.W;
    const int r = P[i];
    bool bad = false;
    for (int w = threadIdx.x & 63; w < a.W; w += 64) {
        u64 b = row[w] & a.cmask[w];
        while (b) { const int j = w * 64 + __ffsll((long long)b) - 1; b &= b - 1; bad |= P[j] != r; }
    }
    if (bad) a.st->bad = 1;
}

__global__ __launch_bounds__(256) void db_number_kernel(DbArgs a)
{
    __shared__ int s[256];
    const int tid = threadIdx.x, c = (a.N + 255) / 256;
    const int i0 = min(tid * c, a.N), i1 = min(i0 + c, a.N);
    const int* P = a.par[0];
    int n = 0;
    for (int i = i0; i < i1; ++i) n += is_core(a, i) && P[i] == i;
    s[tid] = n;
    __syncthreads();
    int base = 0;
    for (int q = 0; q < tid; ++q) base += s[q];
    for (int i = i0; i < i1; ++i) a.num[i] = (is_core(a, i) && P[i] == i) ? base++ : -1;
    if (tid == 255) a.st->nclusters = base;
}

__global__ __launch_bounds__(256) void db_label_kernel(DbArgs a)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.N) return;
    const int* P = a.par[0];
    int l;
    if (is_core(a, i)) l = a.num[P[i]];
    else {
        // num[P[j]] of a core row j is its cluster's number
        const u64* row = a.adj + (size_t)i * a.W;
        int m = 0x7fffffff;
        for (int w = threadIdx.x & 63; w < a.W; w += 64) {
            u64 b = row[w] & a.cmask[w];
            while (b) { const int j = w * 64 + __ffsll((long long)b) - 1; b &= b - 1; m = min(m, a.num[P[j]]); }
        }
        m = wave_min_int(m);
        l = m == 0x7fffffff ? -1 : m;
    }
    if ((threadIdx.x & 63) == 0) a.label[i] = l;
}

__global__ __launch_bounds__(256) void db_stat_kernel(DbArgs a, int32_t* stat)
{
    __shared__ int sh[3][4];
    int core = 0, border = 0, noise = 0;
    for (int i = threadIdx.x; i < a.N; i += 256) {
        const bool c = is_core(a, i);
        const int l = a.label[i];
        core += c; border += !c && l >= 0; noise += l < 0;
    }
    core = wave_sum(core); border = wave_sum(border); noise = wave_sum(noise);
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = core; sh[1][threadIdx.x >> 6] = border; sh[2][threadIdx.x >> 6] = noise; }
    __syncthreads();
    if (threadIdx.x == 0) {
        stat[0] = a.st->nclusters;
        for (int q = 0; q < 3; ++q) stat[1 + q] = sh[q][0] + sh[q][1] + sh[q][2] + sh[q][3];
        stat[4] = a.st->rounds; stat[5] = a.st->bad; stat[6] = 0; stat[7] = 0;
    }
}

int allowed_ti(int cap)
{
    int ti = 4;
    while (ti < 64 && 2 * ti <= cap) ti *= 2;
    return ti;
}

}  // namespace

size_t db_pairs_lds(int TI) { return 8 * ((size_t)DK * TI + (size_t)DK * TJ + TI + TJ) + 8 * (size_t)TI; }

// TI = 64, halved while half of it still holds all N rows (at least 4); the W column tiles are cut into parts so that there are two
// workgroups per CU where the tiles allow it.  chunk_opt > 0 (option dbscan_chunk, a test aid): its low 8 bits cap TI (0: as above), the
// bits above give the column tiles of a part (0: as above).  dim does not enter: the rows are staged 32 elements at a time.
DbPlan db_plan(int N, int dim, int chunk_opt, int cus)
{
    (void)dim;
    DbPlan p{};
    p.W = (N + TJ - 1) / TJ;
    int ti = 64;
    while (ti > 4 && ti / 2 >= N) ti /= 2;
    if ((chunk_opt & 255) > 0) ti = allowed_ti(chunk_opt & 255);
    p.TI = ti;
    p.rtiles = (N + ti - 1) / ti;
    const RowParts rp = row_parts(p.W, 1, (2 * std::max(cus, 1) + p.rtiles - 1) / p.rtiles, kDbMaxParts, chunk_opt >> 8);
    p.parts = rp.parts; p.chunk = rp.chunk;
    p.lds = (int)db_pairs_lds(ti);
    int lg = 0;
    while ((1 << lg) < N) ++lg;
    p.rounds = std::min(2 * (kDbRoundA * lg + kDbRoundB), kDbMaxRounds);
    return p;
}

hipError_t db_prepare(hipStream_t st, const DbArgs& a)
{
    if (a.rnorm) db_rownorm_kernel<<<(a.N + 3) / 4, 256, 0, st>>>(a.x, a.N, a.dim, const_cast<double*>(a.rnorm));
    return hipGetLastError();
}

hipError_t db_pairs(hipStream_t st, const DbArgs& a, const DbPlan& p)
{
    const dim3 grid(p.rtiles, p.parts);
    switch (p.TI) {
        case 4: db_pairs_kernel<4><<<grid, 256, 0, st>>>(a, p.chunk); break;
        case 8: db_pairs_kernel<8><<<grid, 256, 0, st>>>(a, p.chunk); break;
        case 16: db_pairs_kernel<16><<<grid, 256, 0, st>>>(a, p.chunk); break;
        case 32: db_pairs_kernel<32><<<grid, 256, 0, st>>>(a, p.chunk); break;
        case 64: db_pairs_kernel<64><<<grid, 256, 0, st>>>(a, p.chunk); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t db_core(hipStream_t st, const DbArgs& a)
{
    db_core_kernel<<<(a.N + 255) / 256, 256, 0, st>>>(a);
    return hipGetLastError();
}

// round t: the hook reads par[0] and writes par[1 + t % 2]; the jump reads that, writes par[0] and par[2 - t % 2], the array of round t + 1
hipError_t db_round(hipStream_t st, const DbArgs& a, int t)
{
    int* Q = a.par[1 + (t & 1)];
    db_hook_kernel<<<(a.N + 3) / 4, 256, 0, st>>>(a, t, a.par[0], Q);
    db_jump_kernel<<<(a.N + 255) / 256, 256, 0, st>>>(a, t, Q, a.par[0], a.par[2 - (t & 1)]);
    return hipGetLastError();
}

hipError_t db_finish(hipStream_t st, const DbArgs& a, int32_t* stat)
{
    db_verify_kernel<<<(a.N + 3) / 4, 256, 0, st>>>(a);
    db_number_kernel<<<1, 256, 0, st>>>(a);
    db_label_kernel<<<(a.N + 3) / 4, 256, 0, st>>>(a);
    db_stat_kernel<<<1, 256, 0, st>>>(a, stat);
    return hipGetLastError();
}

}  // namespace avae
