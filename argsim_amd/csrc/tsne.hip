// tsne.hip -- exact t-SNE of latent rows (contract: include/argsim_vae.h, avae_tsne; host sequence: clustering.cpp).
// The joint matrix P is dense row-major (N, N) double; the embedding y, its update and its gains are (N, 2) fp32.  A call's small
// state is TsneState (kernels.h), written by tsne_init_kernel before the first iteration.
//
//   setup      the distances are affinity.hip's metric 0 (ap_similarity writes -D; the negation here is exact).
//              tsne_cond_kernel: one workgroup per row, the row of D in LDS, sklearn's bisection on beta with two fixed-order sums per
//              step (a thread's columns ascending, the wave butterfly, the four waves ascending); writes beta and the conditional row.
//              tsne_rowsum_kernel / tsne_sym_kernel: t_i = sum_j (c_ij + c_ji), the total over ascending rows (every workgroup sums
//              it itself, in the one order of total_of), then ONE thread per pair (i, j), (j, i) divides, floors and writes both.
//   iteration  tsne_walk_kernel<false> (grid = row strips x column parts): the part's slice of y staged in LDS; a wave owns a row, its
//              lanes run across the columns, so P is read in whole 512-byte runs; five double accumulators per row (sum q, sum P' q d,
//              sum q^2 d), the wave butterfly, one partial per (row, part).  The loads of P go out eight at a time per lane.
//              tsne_walk_kernel<true>: the same walk for the error terms, on the iterations that compute it; Z from the partials.
//              tsne_update_kernel (ONE workgroup: nothing to wait for): Z over all partials in the order of total_of, the parts of
//              every row added in ascending order, the gradient rounded once, the fp32 state arithmetic with every operation rounded,
//              the gradient norm, then thread 0 does sklearn's bookkeeping, the phase change and the trace.
//   stop       st->stop_at = it + 1 once iteration it ended phase 2.  A launch of iteration it returns at once when 0 < stop_at <= it.
// Floating-point contraction is off in this file: a term of a sum is the same sequence of IEEE operations as in tests/tsne_ref.py, so
// only the ORDER of the sums differs from the reference.  No kernel waits on another workgroup; every loop is bounded by N, the part
// count, 100 or a constant.  No float atomics.
#include "kernels.h"
#include "reduce_dev.h"
#include "row_parts.h"

#include <float.h>

#include <algorithm>

#pragma clang fp contract(off)

namespace avae {

namespace {

constexpr double kEps = 2.220446049250313e-16;      // 2^-52: the floor of P and of Q
constexpr int kCondSteps = 100;
constexpr int kSymT = 32;

// the stop word and the phase in ONE load (they are the state's first two words): false when a launch of iteration `it` finds the
// stop decided
__device__ inline bool ts_live(const TsneState* st, int it, int* phase)
{
    const int2 w = *reinterpret_cast<const int2*>(st);
    *phase = w.y;
    return !(w.x > 0 && it >= w.x);
}

// one double per thread summed over the NW waves of the workgroup: the wave butterfly, then the waves in ascending order.  Every thread
// must call it and gets the result; sh: NW doubles, free again on return
template <int NW>
__device__ __forceinline__ double block_sum(double v, double* sh)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sh[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) r += sh[w];
    __syncthreads();
    return r;
}

// THE order of a total over n values v[k * stride], whatever the workgroup's size (>= 256): thread t < 256 adds k = t, t + 256, ..
// ascending (sixteen loads in flight), then block_sum over the first four waves.  Every thread must call it and gets the result
__device__ __forceinline__ double total_of(const double* __restrict__ v, int n, int stride, double* sh)
{
    double acc = 0.0;
    if (threadIdx.x < 256) {
#pragma unroll 16
        for (int k = threadIdx.x; k < n; k += 256) acc += v[(size_t)k * stride];
    }
    acc = wave_sum(acc);
    if (threadIdx.x < 256 && (threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    const double r = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
    return r;
}

// ---------------------------------------------------------------- conditional probabilities
// grid = N rows, 256 threads, dynamic LDS: 4 doubles, then the row's N distances
__global__ __launch_bounds__(256) void tsne_cond_kernel(const float* __restrict__ S, int N, double want, double tol, double sum0, double* __restrict__ C,
                                                        double* __restrict__ beta_out)
{
    extern __shared__ double dsm[];
    double* sh = dsm;
    float* row = reinterpret_cast<float*>(dsm + 4);
    const int i = blockIdx.x;
    for (int j = threadIdx.x; j < N; j += 256) row[j] = -S[(size_t)i * N + j];
    __syncthreads();
    double beta = 1.0, lo = -INFINITY, hi = INFINITY, used = 1.0, s = 1.0;
    for (int l = 0; l < kCondSteps; ++l) {
        double acc = 0.0;
        for (int j = threadIdx.x; j < N; j += 256)
            if (j != i) acc += exp(-(double)row[j] * beta);
        s = block_sum<4>(acc, sh);
        if (s == 0.0) s = sum0;
        acc = 0.0;
        for (int j = threadIdx.x; j < N; j += 256)
            if (j != i) { const double d = row[j]; acc += d * (exp(-d * beta) / s); }
        const double diff = (log(s) + beta * block_sum<4>(acc, sh)) - want;
        used = beta;
        if (fabs(diff) <= tol) break;
        if (diff > 0.0) { lo = beta; beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0; }
        else { hi = beta; beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0; }
    }
    if (threadIdx.x == 0) beta_out[i] = used;
    for (int j = threadIdx.x; j < N; j += 256) C[(size_t)i * N + j] = j == i ? 0.0 : exp(-(double)row[j] * used) / s;
}

// ---------------------------------------------------------------- the joint matrix
// grid = N rows: t_i = sum_j (c_ij + c_ji)
__global__ __launch_bounds__(256) void tsne_rowsum_kernel(const double* __restrict__ C, int N, double* __restrict__ rs)
{
    __shared__ double sh[4];
    const int i = blockIdx.x;
    double acc = 0.0;
    for (int j = threadIdx.x; j < N; j += 256) acc += C[(size_t)i * N + j] + C[(size_t)j * N + i];
    acc = block_sum<4>(acc, sh);
    if (threadIdx.x == 0) rs[i] = acc;
}

// grid = (tiles, tiles) of 32 x 32 pairs; tiles below the diagonal return at once.  In place: the thread of (i, j), j > i, reads both
// conditionals and writes both entries
__global__ __launch_bounds__(256) void tsne_sym_kernel(double* __restrict__ P, int N, const double* __restrict__ rs)
{
    __shared__ double sh[4];
    if (blockIdx.x < blockIdx.y) return;
    const double tot = fmax(total_of(rs, N, 1, sh), kEps);
    for (int e = threadIdx.x; e < kSymT * kSymT; e += 256) {
        const int i = blockIdx.y * kSymT + e / kSymT, j = blockIdx.x * kSymT + e % kSymT;
        if (i >= N || j >= N || j < i) continue;
        if (i == j) { P[(size_t)i * N + i] = 0.0; continue; }
        const double v = fmax((P[(size_t)i * N + j] + P[(size_t)j * N + i]) / tot, kEps);
        P[(size_t)i * N + j] = v;
        P[(size_t)j * N + i] = v;
    }
}

// ---------------------------------------------------------------- start of the loop
// cold: update 0, gains 1, with init 1 the random start; the trace's entries are NaN (warm: those from it0 on); thread 0 writes the state
__global__ __launch_bounds__(256) void tsne_init_kernel(TsneArgs a, int it0, int warm, int init, uint64_t seed, const double* __restrict__ prog)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (!warm && e < 2 * a.N) {
        a.upd[e] = 0.f; a.gains[e] = 1.f;
        if (init == 1) a.y[e] = __fmul_rn(1e-4f, normal01(seed, 6, (uint64_t)e));
    }
    if (a.trace && e >= (warm ? it0 : 0) && e < a.max_iter) { a.trace[e] = NAN; a.trace[a.max_iter + e] = NAN; }
    if (e == 0) {
        TsneState* st = a.st;
        st->stop_at = 0; st->last_it = it0 - 1; st->how = 0; st->p1_last = -1; st->pad[0] = st->pad[1] = 0;
        st->last_err = NAN; st->p1_err = NAN;
        if (warm) { st->best_error = prog[0]; st->best_iter = (int)prog[1]; st->phase = prog[2] == 1.0 ? 1 : 2; }
        else { st->best_error = DBL_MAX; st->best_iter = it0; st->phase = it0 < a.exag_iter ? 1 : 2; }
    }
}

// ---------------------------------------------------------------- one iteration
// whether iteration `it` of `phase` computes the error
__device__ __forceinline__ bool ts_computes(const TsneArgs& a, int it, int phase)
{
    return (it + 1) % a.nic == 0 || it == (phase == 1 ? a.X - 1 : a.max_iter - 1);
}
// grid = (row strips of a.rs rows, column parts of a.chunk <= kTsneMaxChunk columns).  A lane takes its columns kWalkU at a time: the
// loads of P first, all in flight, then the arithmetic in ascending column order.  A column beyond the part, or the row's own, enters
// as an exact zero term (x + 0 = x: the sums keep their bits)
constexpr int kWalkU = 8;
template <bool kErr>
__global__ __launch_bounds__(256) void tsne_walk_kernel(TsneArgs a, int it)
{
    extern __shared__ float2 sy[];      // a.chunk entries (a static 32 KB would hold a CU to five workgroups)
    __shared__ double sh[4];
    int phase;
    if (!ts_live(a.st, it, &phase)) return;
    const int N = a.N;
    double Z = 1.0;
    if (kErr) {
        if (!ts_computes(a, it, phase)) return;
        Z = total_of(a.part, N * a.parts, 5, sh);
    }
    const double scale = phase == 1 ? a.ee : 1.0;
    const int c0 = blockIdx.y * a.chunk, c1 = min(c0 + a.chunk, N), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float2* __restrict__ y2 = reinterpret_cast<const float2*>(a.y);
    for (int c = threadIdx.x; c < c1 - c0; c += 256) sy[c] = y2[c0 + c];
    __syncthreads();
    const int r0 = blockIdx.x * a.rs;
    for (int r = wave; r < a.rs && r0 + r < N; r += 4) {
        const int i = r0 + r;
        const float2 yi = y2[i];
        const double yi0 = yi.x, yi1 = yi.y;
        const double* __restrict__ Pi = a.P + (size_t)i * N;
        double sz = 0.0, a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
        for (int j0 = c0 + lane; j0 < c1; j0 += 64 * kWalkU) {
            double pv[kWalkU];
#pragma unroll
            for (int u = 0; u < kWalkU; ++u) pv[u] = Pi[min(j0 + 64 * u, c1 - 1)];
#pragma unroll
            for (int u = 0; u < kWalkU; ++u) {
                const int j = j0 + 64 * u;
                const bool on = j < c1 && j != i;
                const float2 yj = sy[min(j, c1 - 1) - c0];
                const double p = on ? scale * pv[u] : 0.0;
                const double d0 = yi0 - (double)yj.x, d1 = yi1 - (double)yj.y;
                const double q = on ? 1.0 / (1.0 + (d0 * d0 + d1 * d1)) : 0.0;
                if (kErr) sz += on ? p * log(fmax(p, kEps) / fmax(q / Z, kEps)) : 0.0;
                else {
                    const double pq = p * q, q2 = q * q;
                    sz += q; a0 += pq * d0; a1 += pq * d1; b0 += q2 * d0; b1 += q2 * d1;
                }
            }
        }
        sz = wave_sum(sz);
        if (kErr) {
            if (lane == 0) a.errp[(size_t)i * a.parts + blockIdx.y] = sz;
        } else {
            a0 = wave_sum(a0); a1 = wave_sum(a1); b0 = wave_sum(b0); b1 = wave_sum(b1);
            if (lane == 0) {
                double* o = a.part + ((size_t)i * a.parts + blockIdx.y) * 5;
                o[0] = sz; o[1] = a0; o[2] = a1; o[3] = b0; o[4] = b1;
            }
        }
    }
}

// ONE workgroup of 1024
__global__ __launch_bounds__(1024) void tsne_update_kernel(TsneArgs a, int it)
{
    __shared__ double sh[16];
    __shared__ int s_reset;
    TsneState* st = a.st;
    int phase;
    if (!ts_live(st, it, &phase)) return;
    const int N = a.N;
    const bool check = (it + 1) % a.nic == 0, comp = ts_computes(a, it, phase);
    const float m = phase == 1 ? 0.5f : 0.8f;
    const double Z = total_of(a.part, N * a.parts, 5, sh);
    double err = NAN;
    if (comp) err = total_of(a.errp, N * a.parts, 1, sh);
    double gacc = 0.0;
    for (int r = threadIdx.x; r < N; r += 1024) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        const double* __restrict__ row = a.part + (size_t)r * a.parts * 5;
#pragma unroll 4
        for (int p = 0; p < a.parts; ++p) {
            const double* o = row + p * 5;
            s[0] += o[1]; s[1] += o[2]; s[2] += o[3]; s[3] += o[4];
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int e = 2 * r + c;
            const float g = (float)(4.0 * (s[c] - s[2 + c] / Z));
            if (a.grad) a.grad[e] = g;
            float u = a.upd[e], ga = a.gains[e];
            ga = __fmul_rn(u, g) < 0.f ? __fadd_rn(ga, 0.2f) : __fmul_rn(ga, 0.8f);
            ga = fmaxf(ga, 0.01f);
            const float gp = __fmul_rn(g, ga);
            u = __fsub_rn(__fmul_rn(m, u), __fmul_rn(a.lr, gp));
            a.y[e] = __fadd_rn(a.y[e], u);
            a.upd[e] = u; a.gains[e] = ga;
            gacc += (double)gp * (double)gp;
        }
    }
    double gn = NAN;
    if (check) gn = sqrt(block_sum<16>(gacc, sh));
    if (threadIdx.x == 0) {
        st->last_it = it;
        if (comp) st->last_err = err;
        if (a.trace) {
            if (comp) a.trace[it] = err;
            if (check) a.trace[a.max_iter + it] = gn;
        }
        int ended = 0;
        if (check) {
            if (err < st->best_error) { st->best_error = err; st->best_iter = it; }
            else if (it - st->best_iter > (phase == 1 ? a.X : a.nwp)) ended = 1;
            if (!ended && gn <= a.min_gn) ended = 2;
        }
        int reset = 0;
        if (phase == 1) {
            st->p1_last = it; st->p1_err = err;
            if (ended || it == a.exag_iter - 1) { st->phase = 2; st->best_error = DBL_MAX; st->best_iter = it + 1; reset = 1; }
        } else if (ended) { st->how = ended; st->stop_at = it + 1; }
        s_reset = reset;
    }
    __syncthreads();
    if (s_reset)      // phase 2 starts fresh: every thread resets the rows it has just written
        for (int r = threadIdx.x; r < N; r += 1024) { a.upd[2 * r] = a.upd[2 * r + 1] = 0.f; a.gains[2 * r] = a.gains[2 * r + 1] = 1.f; }
}

__global__ void tsne_finish_kernel(const TsneState* st, double* kl, int32_t* stat, double* prog)
{
    kl[0] = st->last_err; kl[1] = st->p1_err;
    stat[0] = st->last_it; stat[1] = st->how; stat[2] = st->p1_last; stat[3] = 0;
    if (prog) { prog[0] = st->best_error; prog[1] = (double)st->best_iter; prog[2] = (double)st->phase; prog[3] = 0.0; }
}

#define TS_LAUNCHED() do { const hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

}  // namespace

// rows per workgroup, column parts and columns per part of the walks: at most about 1024 workgroups (every wave resident at once), a
// part of at most kTsneMaxChunk columns
TsnePlan tsne_plan(int N, int chunk_opt)
{
    TsnePlan p;
    p.rs = N <= 4096 ? 4 : 16;
    const int strips = (N + p.rs - 1) / p.rs;
    const int want = std::max(std::max(1024 / strips, 1), (N + kTsneMaxChunk - 1) / kTsneMaxChunk);
    const RowParts rp = row_parts(N, 64, want, 256, chunk_opt > 0 ? std::min(chunk_opt, kTsneMaxChunk) : 0);
    p.parts = rp.parts; p.chunk = rp.chunk;
    return p;
}

hipError_t tsne_conditionals(hipStream_t st, const float* S, int N, double perplexity, double* C, double* beta)
{
    const size_t lds = 4 * sizeof(double) + (size_t)N * sizeof(float);
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(tsne_cond_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(tsne_cond_kernel, dim3(N), dim3(256), lds, st, S, N, std::log(perplexity), (double)1e-5f, (double)1e-8f, C, beta);
    return hipGetLastError();
}

hipError_t tsne_joint(hipStream_t st, double* P, int N, double* rowsum)
{
    hipLaunchKernelGGL(tsne_rowsum_kernel, dim3(N), dim3(256), 0, st, P, N, rowsum);
    TS_LAUNCHED();
    const int tiles = (N + kSymT - 1) / kSymT;
    hipLaunchKernelGGL(tsne_sym_kernel, dim3(tiles, tiles), dim3(256), 0, st, P, N, rowsum);
    return hipGetLastError();
}

hipError_t tsne_init(hipStream_t st, const TsneArgs& a, int it0, int warm, int init, uint64_t seed, const double* prog)
{
    const int n = std::max(2 * a.N, a.max_iter);
    hipLaunchKernelGGL(tsne_init_kernel, dim3((n + 255) / 256), dim3(256), 0, st, a, it0, warm, init, seed, prog);
    return hipGetLastError();
}

hipError_t tsne_iteration(hipStream_t st, const TsneArgs& a, int it)
{
    const dim3 grid((a.N + a.rs - 1) / a.rs, a.parts);
    const size_t lds = (size_t)a.chunk * sizeof(float2);      // <= 32 KB
    hipLaunchKernelGGL(tsne_walk_kernel<false>, grid, dim3(256), lds, st, a, it);
    TS_LAUNCHED();
    // the error's walk where an iteration may compute it: a check, or the last planned iteration of either phase (the kernel knows which)
    if ((it + 1) % a.nic == 0 || it == a.X - 1 || it == a.max_iter - 1) {
        hipLaunchKernelGGL(tsne_walk_kernel<true>, grid, dim3(256), lds, st, a, it);
        TS_LAUNCHED();
    }
    hipLaunchKernelGGL(tsne_update_kernel, dim3(1), dim3(1024), 0, st, a, it);
    return hipGetLastError();
}

hipError_t tsne_finish(hipStream_t st, const TsneArgs& a, double* kl, int32_t* stat, double* prog)
{
    hipLaunchKernelGGL(tsne_finish_kernel, dim3(1), dim3(1), 0, st, a.st, kl, stat, prog);
    return hipGetLastError();
}

}  // namespace avae
