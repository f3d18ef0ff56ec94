// agg.hip -- aggregate-posterior diagnostics over latent rows (contract: include/argsim_vae.h, avae_agg_logq / avae_latent_moments).
//
//   agg_logq   log q(z_i) = logsumexp_j t(i, j) - log N - (dim / 2) log 2 pi over N bank rows (mu_j, lv_j), the pair term
//              t(i, j) = -1/2 sum_d [(z_id - mu_jd)^2 a_jd + lv_jd], a = exp(-lv), in its DIRECT form on the vector ALUs: the
//              difference is formed before the square (the expansion into two products cancels in the own pair).
//              grid = (query tiles of 128 rows) x (bank parts).  A workgroup walks its part in 64-row bank tiles; z, mu and a
//              are staged through LDS in chunks of 32 dims (a = expf(-lv) and c_j = sum_d lv_jd are formed while the tile is
//              staged).  A thread owns 8 queries x 4 bank rows: thread (ty, tx) of the 16 x 16 layout holds queries ty + 16 i
//              and bank rows tx + 16 j; per 4 dims it reads 16 b128 LDS words for 192 packed fp32 operations (d = z - mu,
//              d * d, fma with a; accumulators are float2: even dims in .x, odd dims in .y).  Across bank tiles a thread keeps
//              an online (max, sum) pair per query; at the end of the part the 16 threads of a query (16 adjacent lanes of one
//              wave) are combined by an xor butterfly 8, 4, 2, 1 and the part's pair goes to the workspace.
//   agg_merge  one thread per query combines the parts' pairs in part order and writes logq.
//   moments    per dimension over the N rows: mean mu, unbiased variance of mu (two passes: the mean, then centred squares), mean
//              exp(lv), mean KL.  Row blocks sum in double, a second small kernel adds the blocks in block order.
// No float atomics; every sum has a fixed order: the same arguments and options give the same bits.
#include "kernels.h"
#include "mfma_tile.h"
#include "row_parts.h"

#include <algorithm>
#include <cmath>

namespace avae {

namespace {

constexpr int kTQ = 128;           // query rows per tile: 16 thread rows x 8
constexpr int kTB = 64;            // bank rows per tile: 16 thread columns x 4
constexpr int kQPT = kTQ / 16, kBPT = kTB / 16;
constexpr int kDC = 32;            // dims per LDS chunk
constexpr int kLD = kDC + 4;       // LDS row stride (floats): conflict-free b128 reads along dim (as kTileLDK, mfma_tile.h)
constexpr int kAggMaxParts = 1024;

struct AggTileArgs {
    const float* z; const float* mu; const float* lv;
    float2* parts_ms;                 // (parts, n): the part's (max, sum exp(t - max)) per query
    float* logqx;                     // (n) or null
    int n, N, dim, parts, chunk;
    int self_base;                    // -1: off; else query i's own bank row is self_base + i
    float cst;                        // (dim / 2) log 2 pi
};

// s exp(m - r) with r the reference of the merged pair: -inf - (-inf) never forms (r is 0 where the merged maximum is -inf)
__device__ __forceinline__ float lse_ref(float m) { return m == -INFINITY ? 0.f : m; }
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2)
{
    const float mn = fmaxf(m, m2), r = lse_ref(mn);
    s = __fadd_rn(__fmul_rn(s, expf(m - r)), __fmul_rn(s2, expf(m2 - r)));
    m = mn;
}

// one chunk of the three operand tiles global -> registers: query rows >= n, bank rows >= c_end and dims >= dim read as zero
// (never beyond the arrays); element tid + 256 rep of a tile is row srow + 32 rep, dims sk .. sk + 3 of the chunk
__device__ __forceinline__ void load_chunk(float4 (&rz)[4], float4 (&rm)[2], float4 (&rl)[2], const AggTileArgs& g, int m0, int n0, int c_end, int k0,
                                           int srow, int sk)
{
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool kin = k0 + sk < g.dim;
#pragma unroll
    for (int rep = 0; rep < 4; ++rep) {
        const int row = m0 + srow + 32 * rep;
        float4 v = zero;
        if (kin && row < g.n) v = *reinterpret_cast<const float4*>(g.z + (size_t)row * g.dim + k0 + sk);
        rz[rep] = v;
    }
#pragma unroll
    for (int rep = 0; rep < 2; ++rep) {
        const int row = n0 + srow + 32 * rep;
        const bool in = kin && row < c_end;
        float4 m = zero, l = zero;
        if (in) {
            m = *reinterpret_cast<const float4*>(g.mu + (size_t)row * g.dim + k0 + sk);
            l = *reinterpret_cast<const float4*>(g.lv + (size_t)row * g.dim + k0 + sk);
        }
        rm[rep] = m; rl[rep] = l;
    }
}

__global__ __launch_bounds__(256, 2) void agg_tile_kernel(AggTileArgs g)
{
    __shared__ __attribute__((aligned(16))) float s_z[kTQ * kLD];
    __shared__ __attribute__((aligned(16))) float s_mu[kTB * kLD];
    __shared__ __attribute__((aligned(16))) float s_a[kTB * kLD];
    __shared__ float s_c[2][kTB];     // c_j of the tile, by tile parity (a tile's epilogue reads while the next tile is staged)

    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int part = blockIdx.x % g.parts, qt = blockIdx.x / g.parts;
    const int m0 = qt * kTQ;
    long long c_begin; int c_end;
    part_range(part, g.chunk, g.N, c_begin, c_end);
    const int dim = g.dim;

    float run_m[kQPT], run_s[kQPT];
#pragma unroll
    for (int i = 0; i < kQPT; ++i) { run_m[i] = -INFINITY; run_s[i] = 0.f; }

    // staging: element f = tid + 256 rep of a tile is row f >> 3, dims 4 (f & 7) .. + 3 of the chunk
    const int srow = tid >> 3, sk = (tid & 7) << 2;
    int par = 0;
    for (long long n0l = c_begin; n0l < c_end; n0l += kTB, par ^= 1) {
        const int n0 = (int)n0l;
        f32x2 acc[kQPT][kBPT];
#pragma unroll
        for (int i = 0; i < kQPT; ++i)
#pragma unroll
            for (int j = 0; j < kBPT; ++j) acc[i][j] = f32x2{0.f, 0.f};
        float csum[2] = {0.f, 0.f};

        float4 rz[4], rm[2], rl[2];
        load_chunk(rz, rm, rl, g, m0, n0, c_end, 0, srow, sk);
        for (int k0 = 0; k0 < dim; k0 += kDC) {
#pragma unroll
            for (int rep = 0; rep < 4; ++rep) *reinterpret_cast<float4*>(s_z + (srow + 32 * rep) * kLD + sk) = rz[rep];
#pragma unroll
            for (int rep = 0; rep < 2; ++rep) {
                const float4 l = rl[rep];
                *reinterpret_cast<float4*>(s_mu + (srow + 32 * rep) * kLD + sk) = rm[rep];
                *reinterpret_cast<float4*>(s_a + (srow + 32 * rep) * kLD + sk) = make_float4(expf(-l.x), expf(-l.y), expf(-l.z), expf(-l.w));
                // c_j: the row's 32 dims of this chunk in index order per lane, the 8 lanes of the row by an xor butterfly 4, 2, 1
                float c = __fadd_rn(__fadd_rn(__fadd_rn(l.x, l.y), l.z), l.w);
                for (int o = 4; o > 0; o >>= 1) c = __fadd_rn(c, __shfl_xor(c, o, 64));
                csum[rep] = __fadd_rn(csum[rep], c);
            }
            if (k0 + kDC >= dim && (tid & 7) == 0) { s_c[par][srow] = csum[0]; s_c[par][srow + 32] = csum[1]; }
            if (k0 + kDC < dim) load_chunk(rz, rm, rl, g, m0, n0, c_end, k0 + kDC, srow, sk);     // the next chunk's loads go out before the barrier that publishes this one
            __syncthreads();
#pragma unroll 1
            for (int q = 0; q < kDC / 4; ++q) {
                float4 zv[kQPT], mv[kBPT], av[kBPT];
#pragma unroll
                for (int i = 0; i < kQPT; ++i) zv[i] = *reinterpret_cast<const float4*>(s_z + (ty + 16 * i) * kLD + 4 * q);
#pragma unroll
                for (int j = 0; j < kBPT; ++j) {
                    mv[j] = *reinterpret_cast<const float4*>(s_mu + (tx + 16 * j) * kLD + 4 * q);
                    av[j] = *reinterpret_cast<const float4*>(s_a + (tx + 16 * j) * kLD + 4 * q);
                }
#pragma unroll
                for (int i = 0; i < kQPT; ++i)
#pragma unroll
                    for (int j = 0; j < kBPT; ++j) {
                        const f32x2 d0 = f32x2{zv[i].x, zv[i].y} - f32x2{mv[j].x, mv[j].y};
                        const f32x2 d1 = f32x2{zv[i].z, zv[i].w} - f32x2{mv[j].z, mv[j].w};
                        acc[i][j] = __builtin_elementwise_fma(d0 * d0, f32x2{av[j].x, av[j].y}, acc[i][j]);
                        acc[i][j] = __builtin_elementwise_fma(d1 * d1, f32x2{av[j].z, av[j].w}, acc[i][j]);
                    }
            }
            __syncthreads();
        }

        // ---- epilogue of the tile: t = -1/2 (acc + c_j); columns beyond the part weigh nothing
        float cj[kBPT]; int col[kBPT];
#pragma unroll
        for (int j = 0; j < kBPT; ++j) { col[j] = n0 + tx + 16 * j; cj[j] = s_c[par][tx + 16 * j]; }
#pragma unroll
        for (int i = 0; i < kQPT; ++i) {
            const int row = m0 + ty + 16 * i;
            float t[kBPT];
#pragma unroll
            for (int j = 0; j < kBPT; ++j) {
                t[j] = col[j] < c_end ? __fmul_rn(-0.5f, __fadd_rn(__fadd_rn(acc[i][j].x, acc[i][j].y), cj[j])) : -INFINITY;
                if (g.logqx && row < g.n && col[j] < c_end && col[j] - row == g.self_base) g.logqx[row] = __fsub_rn(t[j], g.cst);
            }
            const float mn = fmaxf(fmaxf(run_m[i], fmaxf(t[0], t[1])), fmaxf(t[2], t[3])), r = lse_ref(mn);      // (fmaxf drops a NaN; the sum keeps it)
            const float e = __fadd_rn(__fadd_rn(expf(t[0] - r), expf(t[1] - r)), __fadd_rn(expf(t[2] - r), expf(t[3] - r)));
            run_s[i] = __fadd_rn(__fmul_rn(run_s[i], expf(run_m[i] - r)), e);
            run_m[i] = mn;
        }
    }

    // the query's 16 column threads are 16 adjacent lanes: xor butterfly (the two sides add the same two products: same bits)
#pragma unroll
    for (int i = 0; i < kQPT; ++i) {
        float m = run_m[i], s = run_s[i];
        for (int o = 8; o > 0; o >>= 1) {
            const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
            lse_merge(m, s, m2, s2);
        }
        const int row = m0 + ty + 16 * i;
        if (tx == 0 && row < g.n) g.parts_ms[(size_t)part * g.n + row] = make_float2(m, s);
    }
}

__global__ __launch_bounds__(256) void agg_merge_kernel(const float2* __restrict__ parts_ms, int parts, int n, float log_n, float cst, float* __restrict__ logq)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float m = -INFINITY, s = 0.f;
    for (int p = 0; p < parts; ++p) {
        const float2 v = parts_ms[(size_t)p * n + i];
        lse_merge(m, s, v.x, v.y);
    }
    logq[i] = __fsub_rn(__fsub_rn(__fadd_rn(m, logf(s)), log_n), cst);      // (m = -inf, s = 0: -inf)
}

// ---------------------------------------------------------------- moments
// grid (P row blocks, column slabs of 256).  A slab of W <= 256 columns is walked by G = 256 / W row groups: thread (g, c) sums rows
// r0 + g, r0 + g + G, .. of its column in double, the groups are added in group order through LDS.  PASS 0: sums of mu, exp(lv) and
// the KL term; PASS 1: the sum of (mu - mean)^2, mean from pass 0.  part: (P, PASS 0 ? 3 : 1, dim) doubles.
template <int PASS>
__global__ __launch_bounds__(256) void moments_partial_kernel(const float* __restrict__ mu, const float* __restrict__ lv, int N, int dim, int rows_per_block,
                                                              const double* __restrict__ mean, double* __restrict__ part)
{
    constexpr int NS = PASS == 0 ? 3 : 1;
    __shared__ double s_p[NS][256];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.y * 256, W = min(dim - c0, 256), G = 256 / W;
    const int grp = tid / W, c = c0 + tid % W;
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = r0 + rows_per_block < (long long)N ? r0 + rows_per_block : N;
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    if (grp < G) {
        const double mc = PASS == 1 ? mean[c] : 0.0;
        for (long long r = r0 + grp; r < r1; r += G) {
            const double m = (double)mu[(size_t)r * dim + c];
            if (PASS == 0) {
                const double l = (double)lv[(size_t)r * dim + c], e = exp(l);
                acc[0] += m;
                acc[1 % NS] += e;
                acc[2 % NS] += 0.5 * (m * m + e - l - 1.0);
            } else {
                const double d = m - mc;
                acc[0] += d * d;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) s_p[k][tid] = acc[k];
    __syncthreads();
    if (grp == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            double s = 0.0;
            for (int q = 0; q < G; ++q) s += s_p[k][q * W + tid];
            part[((size_t)blockIdx.x * NS + k) * dim + c] = s;
        }
    }
}

// one thread per column adds the row blocks in block order.  PASS 0: out rows 0, 2, 3 and the double mean; PASS 1: out row 1
template <int PASS>
__global__ __launch_bounds__(256) void moments_final_kernel(const double* __restrict__ part, int P, int N, int dim, double* __restrict__ mean, float* __restrict__ out)
{
    constexpr int NS = PASS == 0 ? 3 : 1;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= dim) return;
    double s[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = 0.0;
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] += part[((size_t)p * NS + k) * dim + c];
    if (PASS == 0) {
        const double mn = s[0] / N;
        mean[c] = mn;
        out[c] = (float)mn;
        out[2 * (size_t)dim + c] = (float)(s[1 % NS] / N);
        out[3 * (size_t)dim + c] = (float)(s[2 % NS] / N);
    } else {
        out[(size_t)dim + c] = N > 1 ? (float)(s[0] / (N - 1)) : 0.f;
    }
}

}  // namespace

int moments_blocks(int N) { return std::max(1, std::min(256, (N + 255) / 256)); }

// The launch shape, from the problem shape alone: query tiles of 128 rows, and enough bank parts for 4 workgroups per CU on
// 256 CUs (36 KB of LDS each), at least one 64-row bank tile per part and at most kAggMaxParts parts.  The target is a first
// guess: scripts/agg_bench.py has run with this value and no other.  chunk_opt > 0 (option agg_chunk, a test aid) caps
// the bank rows of a part instead; it is raised where it would give more parts than that.
AggPlan agg_plan(int n, int N, int dim, int chunk_opt)
{
    (void)dim;
    AggPlan p{};
    p.qtiles = (n + kTQ - 1) / kTQ;
    if (N < 1) return p;
    const RowParts r = row_parts(N, kTB, std::min(kAggMaxParts, (1024 + p.qtiles - 1) / std::max(p.qtiles, 1)), kAggMaxParts, chunk_opt);
    p.parts = r.parts; p.chunk = r.chunk;
    return p;
}

// parts_ms: (parts, n) float2, the parts' (max, sum) pairs
hipError_t agg_logq(hipStream_t st, const AggArgs& g, const AggPlan& p, float2* parts_ms)
{
    if (g.n < 1 || g.N < 1 || (g.dim & 3) || g.dim < 4 || g.dim > 1024 || g.self_base < -1 || g.self_base + (long long)g.n > (long long)g.N) return hipErrorInvalidValue;
    if (p.parts < 1 || p.parts > kAggMaxParts || (long long)p.qtiles * p.parts > 0x7fffffffLL || (long long)p.parts * p.chunk < (long long)g.N) return hipErrorInvalidValue;
    if (g.logqx && g.self_base < 0) return hipErrorInvalidValue;
    const float cst = (float)(0.5 * g.dim * std::log(2.0 * M_PI));
    AggTileArgs a{};
    a.z = g.z; a.mu = g.mu; a.lv = g.lv; a.parts_ms = parts_ms; a.logqx = g.logqx;
    a.n = g.n; a.N = g.N; a.dim = g.dim; a.parts = p.parts; a.chunk = p.chunk; a.self_base = (int)g.self_base; a.cst = cst;
    hipLaunchKernelGGL(agg_tile_kernel, dim3((unsigned)(p.qtiles * p.parts)), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(agg_merge_kernel, dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, st, a.parts_ms, p.parts, g.n, (float)std::log((double)g.N), cst, g.logq);
    return hipGetLastError();
}

// mean: dim doubles; part: moments_blocks(N) x 3 x dim doubles
hipError_t latent_moments(hipStream_t st, const float* mu, const float* lv, int N, int dim, float* out, double* mean, double* part)
{
    if (N < 1 || (dim & 3) || dim < 4 || dim > 1024) return hipErrorInvalidValue;
    const int P = moments_blocks(N), rows = (N + P - 1) / P;
    const dim3 grid((unsigned)P, (unsigned)((dim + 255) / 256)), fin((unsigned)((dim + 255) / 256));
    hipLaunchKernelGGL(moments_partial_kernel<0>, grid, dim3(256), 0, st, mu, lv, N, dim, rows, mean, part);
    hipLaunchKernelGGL(moments_final_kernel<0>, fin, dim3(256), 0, st, part, P, N, dim, mean, out);
    hipLaunchKernelGGL(moments_partial_kernel<1>, grid, dim3(256), 0, st, mu, lv, N, dim, rows, mean, part);
    hipLaunchKernelGGL(moments_final_kernel<1>, fin, dim3(256), 0, st, part, P, N, dim, mean, out);
    return hipGetLastError();
}

}  // namespace avae
