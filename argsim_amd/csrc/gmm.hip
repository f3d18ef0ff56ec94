// gmm.hip -- Gaussian mixture of latent rows with diagonal or spherical covariances: EM with R restarts side by side (contract:
// include/argsim_vae.h, avae_gmm_fit / avae_gmm_score).  The rows are fp32; every other value is a double.
//
//   gm_e         grid = (row tiles) x (component parts) x (restarts).  64 rows x 64 components per stage, 16 x 16 threads with 4 x 4 pairs
//                each: 32 columns of the rows, the means and the precisions are staged in LDS as doubles, a pair's q = sum (x - mu)^2 p
//                runs over the columns in ascending order (gm_tile_t: THE one place a t_ic is formed).  A thread keeps a running (max,
//                sum exp) and the first maximum per row over its components: the (N, k) panel never reaches memory.
//   gm_merge     a row's parts in ascending order -> lse_i; the bound's partial over 256 rows
//   gm_m         grid = (row slices) x (blocks of 16 components) x (restarts).  Per tile of 64 rows: t_ic again (gm_tile_t), r_ic = exp(t_ic -
//                lse_i) into LDS, then wave w adds r x and r x^2 of components 4 w .. 4 w + 3 for the columns lane, lane + 64 .. row by row
//                in ascending order; one partial (sum r, sum r x, sum r x^2) per (slice, component)
//   gm_params    one workgroup per (component, restart): the slices' partials in ascending order, mean, variance, spherical mean, and
//                what the E-step takes from them (gm_derive: precisions, half log determinant, the bad-variance flag)
//   gm_decide    one workgroup per restart: the bound, the weights, the constants of t_ic, the stop
// Reduction orders are fixed by the plan alone (gm_plan): no float atomics.  The same arguments give the same bits.
#include "kernels.h"
#include "row_parts.h"
#include "rows_dev.h"

#include <algorithm>

namespace avae {

namespace {

constexpr int kDK = 32;            // columns per LDS stage
constexpr double kLog2Pi = 1.8378770664093454835606594728112;
constexpr double kTenEps = 10.0 * 2.220446049250313e-16;

// a running log-sum-exp as (max, sum of exp(t - max)): one more term
__device__ __forceinline__ void lse_take(double& m, double& s, double t)
{
    if (t > m) { s = s * exp(m - t) + 1.0; m = t; }
    else if (m > -INFINITY) s += exp(t - m);
}
// ... another running pair behind this one
__device__ __forceinline__ void lse_join(double& m, double& s, double om, double os)
{
    if (om > m) { s = s * exp(m - om) + os; m = om; }
    else if (om > -INFINITY) s += os * exp(om - m);
}

// the FIRST maximum in double as (value, index); the neutral element loses against every number, a NaN never enters
struct ArgMaxFirst {
    double v = -INFINITY; int i = 0x7fffffff;
    __device__ __forceinline__ void take(double x, int idx) { if (x > v) { v = x; i = idx; } }
    __device__ __forceinline__ void merge(const ArgMaxFirst& o) { if (o.v > v || (o.v == v && o.i < i)) *this = o; }
};

template <int CB>
struct GmLds {
    __attribute__((aligned(16))) double xs[kDK][kGmTile];
    __attribute__((aligned(16))) double ms[kDK][16 * CB];
    __attribute__((aligned(16))) double qs[kDK][16 * CB];
};

// t_ic of rows row0 + 4 ty + i (i < 4) and components c0 + CB tx + q (q < CB) by the 16 x 16 threads of the workgroup; -inf at a
// component >= ce.  q_ic is ONE chain over j in ascending order, d = x - mu, e = d d, q = fma(e, p, q): the value does not depend on CB,
// on the tile or on the part (a staged zero beyond dim adds fma(0, 0, q) = q).  Starts with a barrier; none at its end.
template <int CB>
__device__ __forceinline__ void gm_tile_t(const GmArgs& a, GmLds<CB>& L, const double* __restrict__ mu, const double* __restrict__ prec,
                                          const double* __restrict__ lc, long long row0, int nrow, int c0, int ce, double t[4][CB])
{
    constexpr int TC = 16 * CB;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, dim = a.dim;
    double acc[4][CB];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < CB; ++q) acc[i][q] = 0.0;
    for (int j0 = 0; j0 < dim; j0 += kDK) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + 256 * u, rl = idx >> 3, jj = 4 * (idx & 7), col = j0 + jj;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rl < nrow && col < dim) v = *reinterpret_cast<const float4*>(a.x + (row0 + rl) * dim + col);
            L.xs[jj][rl] = (double)v.x; L.xs[jj + 1][rl] = (double)v.y; L.xs[jj + 2][rl] = (double)v.z; L.xs[jj + 3][rl] = (double)v.w;
        }
#pragma unroll
        for (int u = 0; u < TC * kDK / 256; ++u) {
            const int idx = tid + 256 * u, cl = idx >> 5, jj = idx & 31, c = c0 + cl;
            const bool on = c < ce && j0 + jj < dim;
            L.ms[jj][cl] = on ? mu[(size_t)c * dim + j0 + jj] : 0.0;
            L.qs[jj][cl] = on ? prec[(size_t)c * dim + j0 + jj] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < kDK; ++j) {
            double xa[4], ma[CB], pa[CB];
#pragma unroll
            for (int i = 0; i < 4; ++i) xa[i] = L.xs[j][ty * 4 + i];
#pragma unroll
            for (int q = 0; q < CB; ++q) { ma[q] = L.ms[j][tx * CB + q]; pa[q] = L.qs[j][tx * CB + q]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < CB; ++q) { const double d = xa[i] - ma[q]; const double e = d * d; acc[i][q] = fma(e, pa[q], acc[i][q]); }
        }
    }
#pragma unroll
    for (int q = 0; q < CB; ++q) {
        const int c = c0 + tx * CB + q;
        const double l = c < ce ? lc[c] : 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i][q] = c < ce ? fma(-0.5, acc[i][q], l) : -INFINITY;
    }
}

// ---------------------------------------------------------------- E-step
// sel: the one restart *a.best (the E-step after the loop, and avae_gmm_score's), whether or not it has stopped
__global__ __launch_bounds__(256) void gm_e_kernel(GmArgs a, int sel)
{
    __shared__ GmLds<4> L;
    const int r = sel ? *a.best : blockIdx.z;
    if (!sel && a.st[r].done) return;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, N = a.N, k = a.k;
    const long long row0 = (long long)blockIdx.x * a.p.tile;
    const int nrow = (int)std::min<long long>(a.p.tile, N - row0);
    long long cbl; int ce;
    part_range(blockIdx.y, a.p.chunk, k, cbl, ce);
    const int cb = (int)cbl;
    const double* mu = a.MU + (size_t)r * k * a.dim;
    const double* prec = a.PREC + (size_t)r * k * a.dim;
    const double* lc = a.LC + (size_t)r * k;
    double m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, s[4] = {0.0, 0.0, 0.0, 0.0};
    ArgMaxFirst best[4];
    for (int c0 = cb; c0 < ce; c0 += 64) {
        double t[4][4];
        gm_tile_t<4>(a, L, mu, prec, lc, row0, nrow, c0, ce, t);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = c0 + tx * 4 + q;
            if (c < ce) {
#pragma unroll
                for (int i = 0; i < 4; ++i) { lse_take(m[i], s[i], t[i][q]); best[i].take(t[i][q], c); }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // the 16 threads of a row: a butterfly whose pairing is fixed; thread tx = 0 holds what is written
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
            const double om = __shfl_xor(m[i], o, 64), os = __shfl_xor(s[i], o, 64);
            lse_join(m[i], s[i], om, os);
            best[i].merge(ArgMaxFirst{__shfl_xor(best[i].v, o, 64), __shfl_xor(best[i].i, o, 64)});
        }
        const int rl = ty * 4 + i;
        if (tx == 0 && rl < nrow) {
            const size_t o = ((size_t)r * a.p.parts + blockIdx.y) * N + row0 + rl;
            a.pm[o] = m[i]; a.ps[o] = s[i]; a.pt[o] = best[i].v; a.pi[o] = best[i].i;
        }
    }
}

// a row's parts in ascending order -> lse_i = m + log s; without sel the sum over the block's 256 rows (block_sum), with it logp and
// label = the first maximum of t_ic (a row without a number takes component 0)
__global__ __launch_bounds__(256) void gm_merge_kernel(GmArgs a, int sel, double* __restrict__ logp, int32_t* __restrict__ label)
{
    __shared__ double sh[4];
    const int r = sel ? *a.best : blockIdx.y;
    if (!sel && a.st[r].done) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    double v = 0.0;
    if (i < a.N) {
        double m = -INFINITY, s = 0.0;
        ArgMaxFirst b;
        for (int p = 0; p < a.p.parts; ++p) {
            const size_t o = ((size_t)r * a.p.parts + p) * a.N + i;
            lse_join(m, s, a.pm[o], a.ps[o]);
            b.merge(ArgMaxFirst{a.pt[o], a.pi[o]});
        }
        v = m + log(s);
        a.lse[(size_t)r * a.N + i] = v;
        if (sel) {
            if (logp) logp[i] = v;
            if (label) label[i] = b.i == 0x7fffffff ? 0 : b.i;
        }
    }
    if (!sel) {
        v = block_sum<4>(v, sh);
        if (threadIdx.x == 0) a.bpart[(size_t)r * a.p.blks + blockIdx.x] = v;
    }
}

// the responsibilities of restart *a.best: t_ic again, r_ic = exp(t_ic - lse_i); grid = (row tiles) x (blocks of 64 components)
__global__ __launch_bounds__(256) void gm_resp_kernel(GmArgs a, double* __restrict__ resp)
{
    __shared__ GmLds<4> L;
    const int r = *a.best, tx = threadIdx.x & 15, ty = threadIdx.x >> 4, k = a.k;
    const long long row0 = (long long)blockIdx.x * a.p.tile;
    const int nrow = (int)std::min<long long>(a.p.tile, a.N - row0);
    const int c0 = blockIdx.y * 64;
    double t[4][4];
    gm_tile_t<4>(a, L, a.MU + (size_t)r * k * a.dim, a.PREC + (size_t)r * k * a.dim, a.LC + (size_t)r * k, row0, nrow, c0, k, t);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rl = ty * 4 + i;
        if (rl >= nrow) continue;
        const double l = a.lse[(size_t)r * a.N + row0 + rl];
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int c = c0 + tx * 4 + q; if (c < k) resp[(size_t)(row0 + rl) * k + c] = exp(t[i][q] - l); }
    }
}

// ---------------------------------------------------------------- M-step
// VMAX: dim <= 64 VMAX.  ONEHOT (the start from labels): r_ic = 1 where label_in[r, i] = c, else 0
template <int VMAX, bool ONEHOT>
__global__ __launch_bounds__(256) void gm_m_kernel(GmArgs a, const int32_t* __restrict__ label_in)
{
    __shared__ GmLds<1> L;
    __shared__ double rs[kGmTile][kGmMB];
    const int r = blockIdx.z;
    if (!ONEHOT && a.st[r].done) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tx = tid & 15, ty = tid >> 4, N = a.N, k = a.k, dim = a.dim;
    const int c0 = blockIdx.y * kGmMB, ce = std::min(c0 + kGmMB, k);
    const long long s0 = (long long)blockIdx.x * a.p.slice, s1 = std::min<long long>(s0 + a.p.slice, N);
    double a1[4][VMAX], a2[4][VMAX], an[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < VMAX; ++v) { a1[u][v] = 0.0; a2[u][v] = 0.0; }
    for (long long row0 = s0; row0 < s1; row0 += a.p.tile) {
        const int nrow = (int)std::min<long long>(a.p.tile, s1 - row0);
        if (ONEHOT) {
            __syncthreads();
            for (int idx = tid; idx < kGmTile * kGmMB; idx += 256) {
                const int rl = idx >> 4, c = c0 + (idx & 15);
                rs[rl][idx & 15] = (rl < nrow && c < ce && label_in[(size_t)r * N + row0 + rl] == c) ? 1.0 : 0.0;
            }
        } else {
            double t[4][1];
            gm_tile_t<1>(a, L, a.MU + (size_t)r * k * dim, a.PREC + (size_t)r * k * dim, a.LC + (size_t)r * k, row0, nrow, c0, ce, t);
            // (every thread has passed the tile's first barrier, so none still reads the previous tile's rs)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rl = ty * 4 + i;
                rs[rl][tx] = (rl < nrow && c0 + tx < ce) ? exp(t[i][0] - a.lse[(size_t)r * N + row0 + rl]) : 0.0;
            }
        }
        __syncthreads();
        // the next row's elements are loaded while this row's are added (a column >= dim holds 0 and is never written)
        float xn[VMAX];
#pragma unroll
        for (int v = 0; v < VMAX; ++v) { const int j = lane + 64 * v; xn[v] = j < dim ? a.x[row0 * dim + j] : 0.f; }
        for (int rl = 0; rl < nrow; ++rl) {
            double rr[4];
            float xc[VMAX];
#pragma unroll
            for (int u = 0; u < 4; ++u) { rr[u] = rs[rl][4 * wave + u]; an[u] += rr[u]; }
#pragma unroll
            for (int v = 0; v < VMAX; ++v) xc[v] = xn[v];
            if (rl + 1 < nrow) {
                const float* xr = a.x + (row0 + rl + 1) * dim;
#pragma unroll
                for (int v = 0; v < VMAX; ++v) { const int j = lane + 64 * v; xn[v] = j < dim ? xr[j] : 0.f; }
            }
#pragma unroll
            for (int v = 0; v < VMAX; ++v) {
                const double x = (double)xc[v], x2 = x * x;
#pragma unroll
                for (int u = 0; u < 4; ++u) { a1[u][v] = fma(rr[u], x, a1[u][v]); a2[u][v] = fma(rr[u], x2, a2[u][v]); }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = c0 + 4 * wave + u;
        if (c >= ce) continue;
        double* out = a.mpart + (((size_t)r * a.p.slices + blockIdx.x) * k + c) * (size_t)(2 * dim + 1);
        if (lane == 0) out[0] = an[u];
#pragma unroll
        for (int v = 0; v < VMAX; ++v) { const int j = lane + 64 * v; if (j < dim) { out[1 + j] = a1[u][v]; out[1 + dim + j] = a2[u][v]; } }
    }
}

// what the E-step takes from the variances of component c of restart r, by the workgroup of 256 (thread t owns columns t, t + 256 ..):
// COV, PREC = 1 / cov, HLD = half the sum of log cov (own columns ascending, then block_sum), bad = a variance is <= 0 or not finite
__device__ __forceinline__ void gm_derive(const GmArgs& a, int r, int c, const double cov[4], double* sh)
{
    const size_t base = ((size_t)r * a.k + c) * a.dim;
    double hl = 0.0; int bad = 0;
    for (int u = 0; u < 4; ++u) {
        const int j = threadIdx.x + 256 * u;
        if (j < a.dim) {
            a.COV[base + j] = cov[u]; a.PREC[base + j] = 1.0 / cov[u];
            hl += log(cov[u]);
            bad |= !(cov[u] > 0.0) || !(cov[u] < INFINITY);
        }
    }
    hl = block_sum<4>(hl, sh);
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) { a.HLD[(size_t)r * a.k + c] = 0.5 * hl; a.bad[(size_t)r * a.k + c] = bad ? 1 : 0; }
}

// one workgroup per (component, restart): the slices' partials in ascending order, then sklearn's one-pass moments
__global__ __launch_bounds__(256) void gm_params_kernel(GmArgs a, int start)
{
    __shared__ double cv[1024];
    __shared__ double sh[4];
    __shared__ double sph;
    const int r = blockIdx.y, c = blockIdx.x, k = a.k, dim = a.dim;
    if (!start && a.st[r].done) return;
    const size_t w = (size_t)(2 * dim + 1);
    const double* part = a.mpart + ((size_t)r * a.p.slices * k + c) * w;
    double n = 0.0;
    for (int s = 0; s < a.p.slices; ++s) n += part[(size_t)s * k * w];
    const double nc = n + kTenEps;
    double cov[4] = {1.0, 1.0, 1.0, 1.0};
    for (int u = 0; u < 4; ++u) {
        const int j = threadIdx.x + 256 * u;
        if (j >= dim) continue;
        double s1 = 0.0, s2 = 0.0;
        for (int s = 0; s < a.p.slices; ++s) { s1 += part[(size_t)s * k * w + 1 + j]; s2 += part[(size_t)s * k * w + 1 + dim + j]; }
        const double mu = s1 / nc, av = s2 / nc, sq = mu * mu;
        cov[u] = j < a.dreal ? (av - sq) + a.reg : 1.0;       // a padding column (option gmm_pad) has variance 1 whatever it holds
        a.MU[((size_t)r * k + c) * dim + j] = mu;
        cv[j] = cov[u];
    }
    if (a.spherical) {
        __syncthreads();
        if (threadIdx.x == 0) { double s = 0.0; for (int j = 0; j < a.dreal; ++j) s += cv[j]; sph = s / (double)a.dreal; }
        __syncthreads();
        for (int u = 0; u < 4; ++u) if (threadIdx.x + 256 * u < a.dreal) cov[u] = sph;
    }
    gm_derive(a, r, c, cov, sh);
    if (threadIdx.x == 0) a.NC[(size_t)r * k + c] = nc;
}

// the given parameters of (component, restart) into the workspace
__global__ __launch_bounds__(256) void gm_load_kernel(GmArgs a, const double* __restrict__ w, const double* __restrict__ mu, const double* __restrict__ cov)
{
    __shared__ double sh[4];
    const int r = blockIdx.y, c = blockIdx.x;
    const size_t base = ((size_t)r * a.k + c) * a.dim;
    double cv[4] = {1.0, 1.0, 1.0, 1.0};
    for (int u = 0; u < 4; ++u) {
        const int j = threadIdx.x + 256 * u;
        if (j < a.dim) { a.MU[base + j] = mu[base + j]; cv[u] = j < a.dreal ? cov[base + j] : 1.0; }
    }
    gm_derive(a, r, c, cv, sh);
    if (threadIdx.x == 0) a.W[(size_t)r * a.k + c] = w[(size_t)r * a.k + c];
}

// one workgroup per restart.  it >= 0: iteration it's bound = the blocks' partials (thread t adds blocks t, t + 256 .., then block_sum)
// / N; after an M-step (norm) the weights n_c / N divided by their sum in ascending c; the constants of t_ic from the weights as they
// are stored; then the stop.  it = -1: the start (check: a bad variance ends the restart as degenerate)
__global__ __launch_bounds__(256) void gm_decide_kernel(GmArgs a, int it, int norm, int check)
{
    __shared__ double sh[4];
    __shared__ double tot;
    const int r = blockIdx.x, k = a.k;
    GmState& s = a.st[r];
    if (it >= 0 && s.done) return;
    double lower = 0.0;
    if (it >= 0) {
        double v = 0.0;
        for (int b = threadIdx.x; b < a.p.blks; b += 256) v += a.bpart[(size_t)r * a.p.blks + b];
        lower = block_sum<4>(v, sh) / (double)a.N;
    }
    int bad = 0;
    for (int c = threadIdx.x; c < k; c += 256) bad |= a.bad[(size_t)r * k + c];
    bad = __syncthreads_or(bad);
    double* W = a.W + (size_t)r * k;
    if (norm) {
        if (threadIdx.x == 0) { double t = 0.0; for (int c = 0; c < k; ++c) t += a.NC[(size_t)r * k + c] / (double)a.N; tot = t; }
        __syncthreads();
        for (int c = threadIdx.x; c < k; c += 256) W[c] = (a.NC[(size_t)r * k + c] / (double)a.N) / tot;
    }
    for (int c = threadIdx.x; c < k; c += 256) a.LC[(size_t)r * k + c] = (log(W[c]) - a.HLD[(size_t)r * k + c]) - 0.5 * (double)a.dreal * kLog2Pi;
    if (threadIdx.x != 0) return;
    if (it < 0) {
        s.prev = -INFINITY; s.lower = -INFINITY;
        if (check && bad) { s.done = 1; s.how = 2; }
        return;
    }
    const double change = lower - s.prev;
    s.prev = lower; s.lower = lower; s.iters = it + 1;
    if (a.trace) a.trace[(size_t)r * a.max_iter + it] = lower;
    if (bad || !(fabs(lower) < INFINITY)) { s.done = 1; s.how = 2; s.lower = -INFINITY; }
    else if (fabs(change) < a.tol) { s.done = 1; s.how = 0; }
    else if (it + 1 == a.max_iter) { s.done = 1; s.how = 1; }
}

// ---------------------------------------------------------------- the end of the call
// the first restart with the largest bound among those that are not degenerate; restart 0 if all are
__global__ void gm_pick_kernel(GmArgs a, int32_t* stat, double* lower, int32_t* stat_all)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int best = -1;
    for (int r = 0; r < a.R; ++r) {
        GmState& s = a.st[r];
        if (!s.done) { s.done = 1; s.how = 1; }              // max_iter = 0
        lower[r] = s.lower;
        if (s.how != 2 && (best < 0 || s.lower > a.st[best].lower)) best = r;
        if (stat_all) { stat_all[4 * r] = s.iters; stat_all[4 * r + 1] = s.how; stat_all[4 * r + 2] = 0; stat_all[4 * r + 3] = 0; }
    }
    if (best < 0) best = 0;
    *a.best = best;
    stat[0] = best; stat[1] = a.st[best].iters; stat[2] = a.st[best].how; stat[3] = 0;
}

__global__ __launch_bounds__(256) void gm_copy_kernel(GmArgs a, double* weights, double* means, double* covars, double* weights_all, double* means_all,
                                                      double* covars_all)
{
    const int best = *a.best;
    const size_t step = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x, k = (size_t)a.k, kd = k * a.dim;
    for (size_t i = t0; i < k; i += step) weights[i] = a.W[best * k + i];
    for (size_t i = t0; i < kd; i += step) { means[i] = a.MU[best * kd + i]; covars[i] = a.COV[best * kd + i]; }
    if (weights_all) {
        for (size_t i = t0; i < a.R * k; i += step) weights_all[i] = a.W[i];
        for (size_t i = t0; i < a.R * kd; i += step) { means_all[i] = a.MU[i]; covars_all[i] = a.COV[i]; }
    }
}

__global__ __launch_bounds__(256) void gm_fill_kernel(double* p, size_t n, double v)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = v;
}

template <bool ONEHOT>
void gm_m_launch(hipStream_t st, const GmArgs& a, const int32_t* label_in)
{
    const dim3 g(a.p.slices, (a.k + kGmMB - 1) / kGmMB, a.R);
    const int vm = (a.dim + 63) / 64;
    if (vm <= 1) gm_m_kernel<1, ONEHOT><<<g, 256, 0, st>>>(a, label_in);
    else if (vm <= 2) gm_m_kernel<2, ONEHOT><<<g, 256, 0, st>>>(a, label_in);
    else if (vm <= 4) gm_m_kernel<4, ONEHOT><<<g, 256, 0, st>>>(a, label_in);
    else if (vm <= 8) gm_m_kernel<8, ONEHOT><<<g, 256, 0, st>>>(a, label_in);
    else gm_m_kernel<16, ONEHOT><<<g, 256, 0, st>>>(a, label_in);
}

}  // namespace

GmPlan gm_plan(int N, int k, int R, int chunk_opt)
{
    GmPlan p{};
    p.tile = chunk_opt > 0 ? std::min(chunk_opt, kGmTile) : kGmTile;
    p.tiles = (N + p.tile - 1) / p.tile;
    // component parts only where the row tiles alone leave the chip idle
    const long long wgs = (long long)p.tiles * R;
    const RowParts cp = row_parts(k, chunk_opt > 0 ? 1 : 64, (int)std::min<long long>(kGmMaxParts, (1024 + wgs - 1) / wgs), kGmMaxParts, chunk_opt);
    p.parts = cp.parts; p.chunk = cp.chunk;
    // row slices of the M-step: about 2048 workgroups, at most 64 slices (the partials are slices x k x (2 dim + 1) doubles per restart)
    if (chunk_opt > 0) p.slice = chunk_opt;
    else {
        const long long cblocks = (long long)((k + kGmMB - 1) / kGmMB) * R;
        const long long want = std::max<long long>(1, std::min<long long>(64, (2048 + cblocks - 1) / cblocks));
        p.slice = (int)((((N + want - 1) / want + kGmTile - 1) / kGmTile) * kGmTile);
    }
    if ((N + p.slice - 1) / p.slice > kGmMaxSlices) p.slice = (((N + kGmMaxSlices - 1) / kGmMaxSlices + p.tile - 1) / p.tile) * p.tile;
    p.slices = (N + p.slice - 1) / p.slice;
    p.blks = (N + 255) / 256;
    return p;
}

hipError_t gm_load(hipStream_t st, const GmArgs& a, const double* w, const double* mu, const double* cov, int check)
{
    gm_load_kernel<<<dim3(a.k, a.R), 256, 0, st>>>(a, w, mu, cov);
    gm_decide_kernel<<<a.R, 256, 0, st>>>(a, -1, 0, check);
    return hipGetLastError();
}

hipError_t gm_start_labels(hipStream_t st, const GmArgs& a, const int32_t* label_in)
{
    gm_m_launch<true>(st, a, label_in);
    gm_params_kernel<<<dim3(a.k, a.R), 256, 0, st>>>(a, 1);
    gm_decide_kernel<<<a.R, 256, 0, st>>>(a, -1, 1, 1);
    return hipGetLastError();
}

hipError_t gm_iteration(hipStream_t st, const GmArgs& a, int it)
{
    if (it == 0 && a.trace) {
        const size_t n = (size_t)a.R * a.max_iter;
        gm_fill_kernel<<<(unsigned)std::min<size_t>(1024, (n + 255) / 256), 256, 0, st>>>(a.trace, n, -INFINITY);
    }
    gm_e_kernel<<<dim3(a.p.tiles, a.p.parts, a.R), 256, 0, st>>>(a, 0);
    gm_merge_kernel<<<dim3(a.p.blks, a.R), 256, 0, st>>>(a, 0, nullptr, nullptr);
    gm_m_launch<false>(st, a, nullptr);
    gm_params_kernel<<<dim3(a.k, a.R), 256, 0, st>>>(a, 0);
    gm_decide_kernel<<<a.R, 256, 0, st>>>(a, it, 1, 1);
    return hipGetLastError();
}

hipError_t gm_pick(hipStream_t st, const GmArgs& a, int32_t* stat, double* lower, int32_t* stat_all)
{
    gm_pick_kernel<<<1, 64, 0, st>>>(a, stat, lower, stat_all);
    return hipGetLastError();
}

hipError_t gm_final(hipStream_t st, const GmArgs& a, double* logp, int32_t* label, double* resp)
{
    gm_e_kernel<<<dim3(a.p.tiles, a.p.parts, 1), 256, 0, st>>>(a, 1);
    gm_merge_kernel<<<dim3(a.p.blks, 1), 256, 0, st>>>(a, 1, logp, label);
    if (resp) gm_resp_kernel<<<dim3(a.p.tiles, (a.k + 63) / 64), 256, 0, st>>>(a, resp);
    return hipGetLastError();
}

hipError_t gm_copy(hipStream_t st, const GmArgs& a, double* weights, double* means, double* covars, double* weights_all, double* means_all,
                   double* covars_all)
{
    const size_t most = (size_t)(weights_all ? a.R : 1) * a.k * a.dim;
    gm_copy_kernel<<<(unsigned)std::min<size_t>(2048, (most + 255) / 256), 256, 0, st>>>(a, weights, means, covars, weights_all, means_all, covars_all);
    return hipGetLastError();
}

}  // namespace avae
