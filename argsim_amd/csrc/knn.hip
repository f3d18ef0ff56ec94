// knn.hip -- exact nearest-neighbour search over latent rows: a fused similarity product + top-k whose (n, N) score panel
// never reaches HBM (contract: include/argsim_vae.h, avae_knn).
//
//   knn_norms  one wave per row of q and of the bank (metrics 1 and 2 only): the fixed-order sum of squares of that row
//              alone, its square root for the cosine.  A second pass over the bank (DESIGN 4.3f states the cost).
//   knn_tile   grid = (query tiles) x (bank parts).  A workgroup walks its part in 128-row bank tiles with the NT K-tile step of
//              mfma_tile.h (k-contiguous operands, 32-deep K tiles, v_mfma_f32_32x32x2_f32, the next K tile's loads in
//              flight); the query tile is 128 rows (2 x 2 waves of 64 x 64) or 32 rows (1 x 4 waves of 32 x 32) where n is
//              small.  The epilogue turns the accumulators into scores, drops what does not beat the query's current k-th best
//              entry (kept per query in LDS) and appends the survivors to the query's LDS candidate list (integer LDS
//              atomics for the slot).  After every bank tile, and whenever a list overflows, a wave ranks the list by counting
//              and keeps its best k: entries are (order_key << 32 | ~column), so one 64-bit compare is (score descending,
//              index ascending) and the outcome does not depend on the order of the appends.  At the end of the part the
//              sorted list goes to the workspace.
//   knn_merge  one workgroup per query ranks the entries of its <= parts + carry sorted lists by counting (beam_select's
//              merge) and writes the (n, k) result.
// A pair's score depends on the two rows and the metric alone: every dot product runs over the same K tiles in the same
// MFMA step order whatever tile, part or launch shape it falls in (rows and K tails are zero filled, and x + 0 = x).  No
// float atomics; the only atomics are integer LDS ones: the same arguments give the same bits.
#include "kernels.h"
#include "mfma_tile.h"
#include "row_parts.h"
#include "sample_dev.h"

#include <algorithm>
#include <type_traits>

namespace avae {

namespace {

typedef unsigned long long u64;

constexpr int kBN = 128;           // bank rows per tile
constexpr int kCap = 64;           // candidate slots per query in LDS: one wave ranks a full list with one entry per lane
constexpr int kKnnMaxK = 32;
constexpr int kMergeLds = 48 * 1024;      // knn_merge: 12 bytes per list entry

// inverse of order_key: the canonical score of a key (-0 comes back as +0, a NaN as the quiet NaN 0x7fc00000)
__device__ __forceinline__ float key_score(unsigned key)
{
    if (key == 0u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

__device__ __forceinline__ u64 pack_entry(unsigned key, int col) { return ((u64)key << 32) | (u64)(0xFFFFFFFFu - (unsigned)col); }

// one wave per row: lane l sums the squares of elements 4 l .. 4 l + 3, then 256 + 4 l .., in index order (fma), the wave by
// an xor butterfly (32, 16, .., 1)
__global__ __launch_bounds__(256) void knn_norms_kernel(const float* __restrict__ q, int n, const float* __restrict__ bank, int N, int dim, int metric,
                                                        float* __restrict__ qn, float* __restrict__ bn)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)n + N) return;
    const float* x = row < n ? q + (size_t)row * dim : bank + (size_t)(row - n) * dim;
    float s = 0.f;
    for (int c = lane * 4; c < dim; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(x + c);
        s = __fmaf_rn(v.x, v.x, s); s = __fmaf_rn(v.y, v.y, s); s = __fmaf_rn(v.z, v.z, s); s = __fmaf_rn(v.w, v.w, s);
    }
    for (int o = 32; o > 0; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o, 64));
    if (lane == 0) {
        const float v = metric == 1 ? __fsqrt_rn(s) : s;
        if (row < n) qn[row] = v; else bn[row - n] = v;
    }
}

struct KnnTileArgs {
    const float* q; const float* bank;
    const float* qn; const float* bn;     // knn_norms' output (metric 1: norms, 2: squared norms), unused at metric 0
    u64* lists;                           // (n, parts, k) sorted entries, 0 = empty
    int n, N, dim, k, metric, parts, chunk;
    int has_self; long long self_off;     // query row i never takes column self_off + i
};

// the score of a pair from its dot product and the two rows' norms (header: "Score of a pair")
__device__ __forceinline__ float pair_score(int metric, float d, float qn, float bn)
{
    if (metric == 1) return (qn == 0.f || bn == 0.f) ? 0.f : __fdiv_rn(d, __fmul_rn(qn, bn));
    if (metric == 2) {
        float t = __fadd_rn(__fsub_rn(qn, __fmul_rn(2.f, d)), bn);
        if (t < 0.f) t = 0.f;             // (a NaN stays a NaN)
        return -t;
    }
    return d;
}

// a wave keeps the best k of row rl's list (c > k entries, one per lane), sorted, and raises the row's admission entry
__device__ __forceinline__ void compact_row(u64* __restrict__ list, int c, int k, int lane, int* cnt, u64* adm)
{
    const u64 v = lane < c ? list[lane] : 0ull;
    int rank = 0;
    for (int i = 0; i < c; ++i) rank += list[i] > v ? 1 : 0;       // (entries are distinct: they hold distinct columns)
    __builtin_amdgcn_wave_barrier();
    if (lane < c && rank < k) list[rank] = v;
    if (lane < c && rank == k - 1) *adm = v;                        // only an entry that beats the k-th can still enter (a tie: the lower column)
    if (lane == 0) *cnt = k;
}

template <int WM, int WN, int TM, int TN, int METRIC>
__global__ __launch_bounds__(256) void knn_tile_kernel(KnnTileArgs a)
{
    constexpr int BM = 32 * WM * TM;
    static_assert(32 * WN * TN == kBN && TN * 16 <= 32, "tile shape");
    __shared__ __attribute__((aligned(16))) float s_tile[(BM + kBN) * kTileLDK];
    __shared__ u64 s_list[BM * kCap];
    __shared__ u64 s_adm[BM];             // a candidate is admitted when its entry > s_adm: 0 until the list has been cut to k, then its k-th entry
    __shared__ int s_cnt[BM];
    __shared__ float s_qn[BM];
    float* As = s_tile;
    float* Bs = s_tile + BM * kTileLDK;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l31 = lane & 31;
    const int wm = wave / WN, wn = wave % WN;
    const int part = blockIdx.x % a.parts, qt = blockIdx.x / a.parts;
    const int m0 = qt * BM;
    long long c_begin; int c_end;
    part_range(part, a.chunk, a.N, c_begin, c_end);
    const int k = a.k, dim = a.dim;
    // query row i never takes column self_off + i; column - row is an int above INT_MIN, which so stands for "no exclusion"
    const int self_d = (a.has_self && a.self_off > -0x7fffffffLL && a.self_off <= 0x7fffffffLL) ? (int)a.self_off : (int)0x80000000;

    for (int i = tid; i < BM; i += 256) {
        s_adm[i] = 0ull; s_cnt[i] = 0;
        s_qn[i] = (METRIC != 0 && m0 + i < a.n) ? a.qn[m0 + i] : 0.f;
    }
    __syncthreads();

    for (int n0 = (int)c_begin; n0 < c_end; n0 += kBN) {
        f32x16 acc[TM][TN];
        zero_acc(acc);

        float4 ra[BM / 32], rb[kBN / 32];
        load_tile<false, BM>(ra, a.q, dim, m0, a.n, 0, dim, tid);
        load_tile<false, kBN>(rb, a.bank, dim, n0, c_end, 0, dim, tid);
        for (int k0 = 0; k0 < dim; k0 += kTileBK) {
            store_tile<false, BM>(As, ra, tid);
            store_tile<false, kBN>(Bs, rb, tid);
            if (k0 + kTileBK < dim) {         // the next K tile's loads go out before the barrier that publishes this one
                load_tile<false, BM>(ra, a.q, dim, m0, a.n, k0 + kTileBK, dim, tid);
                load_tile<false, kBN>(rb, a.bank, dim, n0, c_end, k0 + kTileBK, dim, tid);
            }
            __syncthreads();
            __builtin_amdgcn_s_setprio(1);
            mfma_ktile<false, false, TM, TN, BM, kBN>(acc, As, Bs, wm, wn, h, l31);
            __builtin_amdgcn_s_setprio(0);
            __syncthreads();
        }

        // ---- epilogue: accumulators -> scores in place; `pend` marks the lane's elements that are not yet decided (C/D map: mfma32_row)
        float bn[TN]; int colv[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            colv[j] = n0 + 32 * (wn * TN + j) + l31;
            bn[j] = (METRIC != 0 && colv[j] < c_end) ? a.bn[colv[j]] : 0.f;
        }
        unsigned pend[TM];      // per MFMA tile row i: bit j * 16 + r
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            pend[i] = TN * 16 == 32 ? 0xFFFFFFFFu : (1u << (TN * 16)) - 1u;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float qn = s_qn[32 * (wm * TM + i) + mfma32_row(r, h)];
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j][r] = pair_score(METRIC, acc[i][j][r], qn, bn[j]);
            }
        }
        for (;;) {
            int over = 0;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                if (!pend[i]) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = 32 * (wm * TM + i) + mfma32_row(r, h), row = m0 + rl;
                    const u64 adm = row < a.n ? s_adm[rl] : ~0ull;                 // (no entry beats it: a row beyond n admits nothing)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const unsigned bit = 1u << (j * 16 + r);
                        const u64 ent = pack_entry(order_key(acc[i][j][r]), colv[j]);
                        const bool want = (pend[i] & bit) && ent > adm && colv[j] < c_end && colv[j] - row != self_d;
                        int slot = 0;
                        if (want) {
                            slot = atomicAdd(&s_cnt[rl], 1);
                            if (slot < kCap) s_list[rl * kCap + slot] = ent;
                        }
                        if (slot < kCap) pend[i] &= ~bit;      // decided; else the list is full: again after it has been compacted
                        else over = 1;
                    }
                }
            }
            const int any_over = __syncthreads_or(over);
            for (int rl = wave; rl < BM; rl += 4) {
                const int c = s_cnt[rl];
                if (c > k) compact_row(s_list + rl * kCap, min(c, kCap), k, lane, &s_cnt[rl], &s_adm[rl]);
            }
            __syncthreads();
            if (!any_over) break;
        }
    }

    // the part's list, sorted, into the workspace (every row holds <= k entries here; unused slots are 0 = empty)
    for (int rl = wave; rl < BM; rl += 4) {
        const int row = m0 + rl;
        if (row >= a.n) break;
        const int c = s_cnt[rl];
        const u64 v = lane < c ? s_list[rl * kCap + lane] : 0ull;
        int rank = 0;
        for (int i = 0; i < c; ++i) rank += s_list[rl * kCap + i] > v ? 1 : 0;
        u64* out = a.lists + ((size_t)row * a.parts + part) * k;
        if (lane < c) out[rank] = v;
        else if (lane < k) out[lane] = 0ull;
    }
}

// one workgroup per query: its parts' lists (local columns) and, with carry, the caller's list (global indices) ranked by
// counting under (key descending, global index ascending); every list is sorted, so a scan of another list stops at its
// first entry that is not better.  Dynamic LDS: (parts + carry) k entries of key (4 bytes) and index (8 bytes).
__global__ __launch_bounds__(256) void knn_merge_kernel(const u64* __restrict__ lists, int parts, int k, long long idx_base, int carry,
                                                        long long* __restrict__ out_idx, float* __restrict__ out_score)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ int s_valid;
    const int tid = threadIdx.x, L = parts + (carry ? 1 : 0), total = L * k;
    long long* s_idx = reinterpret_cast<long long*>(s_raw);
    unsigned* s_key = reinterpret_cast<unsigned*>(s_idx + total);
    const size_t row = blockIdx.x;
    if (tid == 0) s_valid = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < parts * k; i += 256) {
        const u64 v = lists[row * parts * k + i];
        s_key[i] = (unsigned)(v >> 32);
        s_idx[i] = v ? idx_base + (long long)(0xFFFFFFFFu - (unsigned)v) : -1;
        mine += v ? 1 : 0;
    }
    if (carry)
        for (int i = tid; i < k; i += 256) {
            const long long gi = out_idx[row * k + i];
            s_idx[parts * k + i] = gi < 0 ? -1 : gi;
            s_key[parts * k + i] = order_key(out_score[row * k + i]);
            mine += gi < 0 ? 0 : 1;
        }
    if (mine) atomicAdd(&s_valid, mine);
    __syncthreads();                                               // (the caller's list has been read: the result may overwrite it)
    for (int e = tid; e < total; e += 256) {
        const long long gi = s_idx[e];
        if (gi < 0) continue;
        const int l = e / k, i = e - l * k;
        const unsigned key = s_key[e];
        int rank = i;                                              // the list is sorted: i of its own are better
        for (int q = 0; q < L && rank < k; ++q) {
            if (q == l) continue;
            for (int j = 0; j < k && rank < k; ++j) {
                const long long gq = s_idx[q * k + j];
                const unsigned kq = s_key[q * k + j];
                if (gq >= 0 && (kq > key || (kq == key && gq < gi))) ++rank; else break;
            }
        }
        if (rank < k) { out_idx[row * k + rank] = gi; out_score[row * k + rank] = key_score(key); }
    }
    if (tid < k && tid >= s_valid) { out_idx[row * k + tid] = -1; out_score[row * k + tid] = -INFINITY; }
}

}  // namespace

// how many parts knn_merge can rank for this k: its lists live in LDS
static int knn_max_parts(int k) { return std::min(512, kMergeLds / (12 * k) - 1); }

// The launch shape, from the problem shape alone.  EVERY threshold here is a first guess: scripts/knn_bench.py has run once
// (profiles/knn_bench.txt) with these values and no other, so none of them has been compared with an alternative:
//   - 32-row query tiles up to 64 queries (the call is bound by the bank stream there, and a narrow tile wastes less of the
//     matrix pipe on padding rows), 128-row tiles above;
//   - enough parts for 4 workgroups per CU of the 32-row form (39 KB of LDS each) or 1 per CU of the 128-row form (104 KB)
//     on 256 CUs, bounded by what knn_merge ranks in LDS and by one 128-row bank tile per part.
// chunk_opt > 0 (option knn_chunk, a test aid) caps the bank rows of a part instead; it is raised where it would give more
// parts than the merge takes.
KnnPlan knn_plan(int n, int N, int k, int chunk_opt)
{
    KnnPlan p{};
    p.qrows = n <= 64 ? 32 : 128;
    p.qtiles = (n + p.qrows - 1) / p.qrows;
    if (N < 1) return p;
    const int max_parts = knn_max_parts(k), target = 256 * (p.qrows == 32 ? 4 : 1);
    const RowParts r = row_parts(N, kBN, std::min(max_parts, (target + p.qtiles - 1) / p.qtiles), max_parts, chunk_opt);
    p.parts = r.parts; p.chunk = r.chunk;
    return p;
}

hipError_t knn_search(hipStream_t st, const KnnArgs& g, const KnnPlan& p, const KnnWs& w)
{
    if (g.n < 1 || g.N < 0 || g.k < 1 || g.k > kKnnMaxK || g.metric < 0 || g.metric > 2 || (g.dim & 3) || g.dim < 4 || g.dim > 1024)
        return hipErrorInvalidValue;
    if (p.parts > knn_max_parts(g.k) || (long long)p.qtiles * std::max(p.parts, 1) > 0x7fffffffLL) return hipErrorInvalidValue;
    if (g.N > 0) {
        if (g.metric != 0) {
            const long long rows = (long long)g.n + g.N;
            hipLaunchKernelGGL(knn_norms_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, g.q, g.n, g.bank, g.N, g.dim, g.metric, w.qn, w.bn);
        }
        KnnTileArgs a{};
        a.q = g.q; a.bank = g.bank; a.qn = w.qn; a.bn = w.bn; a.lists = w.lists;
        a.n = g.n; a.N = g.N; a.dim = g.dim; a.k = g.k; a.metric = g.metric; a.parts = p.parts; a.chunk = p.chunk;
        a.has_self = g.self_base >= 0 ? 1 : 0; a.self_off = g.self_base - g.idx_base;
        const dim3 grid((unsigned)(p.qtiles * p.parts));
        auto launch = [&](auto metric) {
            constexpr int M = decltype(metric)::value;
            if (p.qrows == 32) hipLaunchKernelGGL((knn_tile_kernel<1, 4, 1, 1, M>), grid, dim3(256), 0, st, a);
            else hipLaunchKernelGGL((knn_tile_kernel<2, 2, 2, 2, M>), grid, dim3(256), 0, st, a);
        };
        if (g.metric == 0) launch(std::integral_constant<int, 0>{});
        else if (g.metric == 1) launch(std::integral_constant<int, 1>{});
        else launch(std::integral_constant<int, 2>{});
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int L = p.parts + (g.carry ? 1 : 0);
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)g.n), dim3(256), (size_t)std::max(L, 1) * g.k * 12, st, w.lists, p.parts, g.k, (long long)g.idx_base,
                       g.carry, reinterpret_cast<long long*>(g.out_idx), g.out_score);
    return hipGetLastError();
}

}  // namespace avae
