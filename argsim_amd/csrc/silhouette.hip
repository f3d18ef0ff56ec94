// silhouette.hip -- cluster-quality scores of latent rows for L labelings of the same N rows: the silhouette of every row, its mean, the
// Calinski-Harabasz and the Davies-Bouldin index (contract: include/argsim_vae.h, avae_silhouette).  Every value is a
// double; the rows are fp32 and, for the cosine, divided by their double norm where they are loaded.
//
//   sil_pass     grid = row tiles, one launch per pass of labelings.  A workgroup owns TI rows i and walks ALL N columns k in ascending
//                tiles of 64: 32 elements of the rows and of the columns are staged in LDS as doubles (the next stage's loads in flight), 256 threads hold the TI x 64 pair
//                sums in registers, a pair's sum runs over the elements in ascending order whatever TI is.  The distances go to LDS; then
//                every (row i, labeling l) has ONE owner thread, which walks the tile's columns in ascending k and adds d(i, k) into
//                bins[l][i][label_l[k]] in LDS: no atomics, S_i(c) is summed in ascending k for every plan.  The (N, N) distances are
//                formed once per pass and never reach memory, nor do the bins.  After the last tile the owner turns its bin row into a, b,
//                nearest and s.
//   sil_score    one workgroup per labeling: the mean of s (thread t the rows t, t + 256 .., then block_sum) and the clusters' means --
//                256 rows at a time in LDS, thread t owns the clusters c = t mod 256 and adds their rows in ascending order
//   sil_msum     member sums for CH / DB: a workgroup per (4 columns, labeling) with the clusters' four sums in LDS, 256 rows at a time,
//                thread (t mod 4, t / 4) owns column t mod 4 of the clusters c = t / 4 mod 64: ascending rows
//   sil_mean     sums -> means, the mean of the labelled rows (the clusters' sums in ascending order)
//   sil_rowdev   one wave per (row, labeling): |X_i - m_c|^2 and its root
//   sil_within   per labeling: S_c, trW, trB;  sil_db: per (cluster, labeling) max R;  sil_index: CH and DB
// Reduction orders are fixed by the shape; the only atomics are the integer member counts, which commute.
#include "kernels.h"
#include "reduce_dev.h"
#include "rows_dev.h"

#include <algorithm>

namespace avae {

namespace {

constexpr int TJ = kSilTJ, DK = kSilDK;

__device__ __forceinline__ int valid_label(int c, int K) { return (c >= 0 && c < K) ? c : -1; }

__global__ __launch_bounds__(256) void sil_rownorm_kernel(const float* __restrict__ x, int N, int dim, double* __restrict__ rn)
{
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const double v = wave_row_norm(x, row, dim);
    if ((threadIdx.x & 63) == 0) rn[row] = v;
}

__global__ __launch_bounds__(256) void sil_count_kernel(SilArgs a)
{
    const int l = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    const int c = valid_label(a.label[(size_t)l * a.N + i], a.meta[l]);
    if (c >= 0) atomicAdd(&a.cnt[a.meta[a.L + l] + c], 1);
}

// ---------------------------------------------------------------- the pair pass
// labelings [l0, l0 + nl); tj <= 64 columns per tile (the option caps it).  Dynamic LDS, laid out as sil_staging counts it.
template <int TI, bool COS>
__global__ __launch_bounds__(256) void sil_pass_kernel(SilArgs a, int l0, int nl, int tj)
{
    constexpr int NTY = TI < 16 ? TI : 16, RI = TI / NTY, NTX = 256 / NTY, CJ = TJ / NTX;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x, ty = tid / NTX, tx = tid % NTX;
    const int N = a.N, dim = a.dim, L = a.L;
    const int cbase = a.meta[L + l0], cols = a.meta[L + l0 + nl] - cbase;
    double* bins = smem;
    double* D = bins + (size_t)TI * cols;
    double* xi = D + TI * TJ;
    double* xj = xi + DK * TI;
    double* rni = xj + DK * TJ;
    double* rnj = rni + TI;
    int* labj = reinterpret_cast<int*>(rnj + TJ);
    int* labi = labj + nl * TJ;
    int* sK = labi + nl * TI;
    int* sOff = sK + kSilMaxL;
    const int row0 = blockIdx.x * TI;
    const int nrow = min(TI, N - row0);

    for (int l = tid; l < nl; l += 256) { sK[l] = a.meta[l0 + l]; sOff[l] = (a.meta[L + l0 + l] - cbase) * TI; }
    for (int q = tid; q < TI * cols; q += 256) bins[q] = 0.0;
    for (int q = tid; q < nl * TI; q += 256) {
        const int l = q / TI, i = q % TI;
        labi[q] = i < nrow ? valid_label(a.label[(size_t)(l0 + l) * N + row0 + i], a.meta[l0 + l]) : -1;
    }
    if (tid < TI) rni[tid] = tid < nrow ? (a.rnorm ? a.rnorm[row0 + tid] : -1.0) : 0.0;
    __syncthreads();

    // what this thread stages: per stage of DK elements two float4 of the columns (tile row cr[u], elements ce[u] ..) and, where TI
    // reaches that far, of the rows.  The loads of the next stage -- of the next tile's first, at a tile's last -- are issued before the
    // pair sums of this one and stay in flight behind them (and behind the binning)
    int cr[2], ce[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) { const int idx = tid + 256 * u; cr[u] = idx / (DK / 4); ce[u] = 4 * (idx % (DK / 4)); }
    float4 pi[2], pj[2];
    auto fetch = [&](int col0, int j0) {
        const int ncol = min(tj, N - col0);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int col = j0 + ce[u];
            pi[u] = make_float4(0.f, 0.f, 0.f, 0.f); pj[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (cr[u] < nrow && col < dim) pi[u] = *reinterpret_cast<const float4*>(a.x + (size_t)(row0 + cr[u]) * dim + col);
            if (cr[u] < ncol && col < dim) pj[u] = *reinterpret_cast<const float4*>(a.x + (size_t)(col0 + cr[u]) * dim + col);
        }
    };
    fetch(0, 0);
    for (int col0 = 0; col0 < N; col0 += tj) {
        const int ncol = min(tj, N - col0);
        for (int q = tid; q < nl * TJ; q += 256) {
            const int l = q / TJ, k = q % TJ;
            labj[q] = k < ncol ? valid_label(a.label[(size_t)(l0 + l) * N + col0 + k], sK[l]) : -1;
        }
        if (tid < TJ) rnj[tid] = tid < ncol ? (a.rnorm ? a.rnorm[col0 + tid] : -1.0) : 0.0;
        double acc[RI][CJ];
#pragma unroll
        for (int i = 0; i < RI; ++i)
#pragma unroll
            for (int j = 0; j < CJ; ++j) acc[i][j] = 0.0;
        for (int j0 = 0; j0 < dim; j0 += DK) {
            __syncthreads();                                    // the stage is free (and, the first time, labj and rnj are written)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int rl = cr[u], e0 = ce[u];
                const bool in = j0 + e0 < dim;
                if (rl < TI) stage_row4(xi, TI, e0, rl, pi[u], rni[rl], in && rl < nrow);
                stage_row4(xj, TJ, e0, rl, pj[u], rnj[rl], in && rl < ncol);
            }
            __syncthreads();
            if (j0 + DK < dim) fetch(col0, j0 + DK);
            else if (col0 + tj < N) fetch(col0 + tj, 0);
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
                    for (int q = 0; q < CJ; ++q) {
                        if (COS) acc[i][q] = fma(xa[i], ca[q], acc[i][q]);
                        else { const double d = xa[i] - ca[q]; acc[i][q] = fma(d, d, acc[i][q]); }
                    }
            }
        }
#pragma unroll
        for (int i = 0; i < RI; ++i)
#pragma unroll
            for (int q = 0; q < CJ; ++q) {
                double d = acc[i][q];
                if (COS) d = fmin(fmax(1.0 - d, 0.0), 2.0);
                else if (a.metric == 0) d = sqrt(d);
                D[(ty * RI + i) * TJ + tx * CJ + q] = d;
            }
        __syncthreads();
        // the owner of (i, l) = pair q adds the tile's columns in ascending k; four pairs of a thread side by side (their bins are disjoint),
        // labels and distances read four columns at a time (the columns behind ncol carry the label -1)
        for (int q0 = tid; q0 < nl * TI; q0 += 4 * 256) {
            double* bp[4]; const int* lj[4]; const double* dr[4]; int self[4]; bool on[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = q0 + 256 * u;
                on[u] = q < nl * TI && labi[q] >= 0;
                const int l = on[u] ? q / TI : 0, i = on[u] ? q % TI : 0;
                bp[u] = bins + sOff[l] + i * sK[l]; lj[u] = labj + l * TJ; dr[u] = D + i * TJ; self[u] = on[u] ? row0 + i - col0 : -1;
            }
            for (int k0 = 0; k0 < ncol; k0 += 4) {
                int4 c4[4]; double2 da[4], db[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    c4[u] = on[u] ? *reinterpret_cast<const int4*>(lj[u] + k0) : make_int4(-1, -1, -1, -1);
                    da[u] = *reinterpret_cast<const double2*>(dr[u] + k0); db[u] = *reinterpret_cast<const double2*>(dr[u] + k0 + 2);
                }
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    int c[4]; double v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        c[u] = kk == 0 ? c4[u].x : kk == 1 ? c4[u].y : kk == 2 ? c4[u].z : c4[u].w;
                        if (k0 + kk == self[u]) c[u] = -1;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const double d = kk == 0 ? da[u].x : kk == 1 ? da[u].y : kk == 2 ? db[u].x : db[u].y;
                        v[u] = c[u] >= 0 ? bp[u][c[u]] + d : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) if (c[u] >= 0) bp[u][c[u]] = v[u];
                }
            }
        }
        __syncthreads();                                        // labj and D are free for the next tile
    }

    // the owner's bin row -> a, b, nearest, s
    for (int q = tid; q < nl * TI; q += 256) {
        const int l = q / TI, i = q % TI;
        if (i >= nrow) continue;
        const int ci = labi[q], K = sK[l];
        double av = 0.0, bv = 0.0, sv = 0.0; int near = -1;
        if (ci >= 0) {
            const double* b = bins + sOff[l] + i * K;
            const int* cn = a.cnt + a.meta[L + l0 + l];
            const int nown = cn[ci];
            double best = INFINITY;
            for (int c = 0; c < K; ++c) {
                const int n = cn[c];
                if (c == ci || n == 0) continue;
                const double m = b[c] / (double)n;
                if (m < best) { best = m; near = c; }
            }
            if (nown > 1) av = b[ci] / (double)(nown - 1);
            if (near >= 0) bv = best;
            const double mx = fmax(av, bv);
            if (nown > 1 && near >= 0 && mx > 0.0) sv = (bv - av) / mx;
        }
        const size_t o = (size_t)(l0 + l) * N + row0 + i;
        a.s[o] = sv;
        if (a.ab) { a.ab[2 * o] = av; a.ab[2 * o + 1] = bv; }
        if (a.nearest) a.nearest[o] = near;
    }
}

// ---------------------------------------------------------------- per-row values binned by label
// vals (N) of labeling l into bins (K doubles of LDS, zeroed here), the rows in ascending order per cluster: 256 rows at a time, thread t
// owns the clusters c = t mod 256.  Returns the thread's own sum over the rows t, t + 256 ..  Unlabelled rows count as 0.
__device__ __forceinline__ double bin_rows(const int32_t* __restrict__ lab, const double* __restrict__ vals, int N, int K,
                                           double* __restrict__ bins, int* __restrict__ sl, double* __restrict__ sv)
{
    const int tid = threadIdx.x;
    for (int c = tid; c < K; c += 256) bins[c] = 0.0;
    double own = 0.0;
    for (int base = 0; base < N; base += 256) {
        const int i = base + tid;
        int c = -1; double v = 0.0;
        if (i < N) { c = valid_label(lab[i], K); if (c >= 0) v = vals[i]; }
        __syncthreads();
        sl[tid] = c; sv[tid] = v;
        own += v;
        __syncthreads();
        // eight labels per step (the rows behind N carry -1): the reads do not wait for one another, the adds keep the rows' order
        for (int q0 = 0; q0 < 256 && base + q0 < N; q0 += 8) {
            const int4 ca = *reinterpret_cast<const int4*>(sl + q0), cb = *reinterpret_cast<const int4*>(sl + q0 + 4);
            const int cc[8] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
#pragma unroll
            for (int u = 0; u < 8; ++u) if (cc[u] >= 0 && (cc[u] & 255) == tid) bins[cc[u]] += sv[q0 + u];
        }
    }
    __syncthreads();
    return own;
}

// the labelled rows of labeling l: thread t the clusters t, t + 256 .., an integer sum
__device__ __forceinline__ int labelled_rows(const int* cn, int K, int* shi)
{
    int n = 0;
    for (int c = threadIdx.x; c < K; c += 256) n += cn[c];
    n = wave_sum(n);
    if ((threadIdx.x & 63) == 0) shi[threadIdx.x >> 6] = n;
    __syncthreads();
    n = shi[0] + shi[1] + shi[2] + shi[3];
    __syncthreads();
    return n;
}

__global__ __launch_bounds__(256) void sil_score_kernel(SilArgs a, double* score, int32_t* count, double* cluster_mean)
{
    __shared__ double bins[kSilMaxK];
    __shared__ double sv[256];
    __shared__ __attribute__((aligned(16))) int sl[256];
    __shared__ double sh[4];
    __shared__ int shi[4];
    const int l = blockIdx.x, K = a.meta[l];
    const int* cn = a.cnt + a.meta[a.L + l];
    const double own = bin_rows(a.label + (size_t)l * a.N, a.s + (size_t)l * a.N, a.N, K, bins, sl, sv);
    const double tot = block_sum<4>(own, sh);
    const int nlab = labelled_rows(cn, K, shi);
    if (threadIdx.x == 0) score[l] = nlab > 0 ? tot / (double)nlab : 0.0;
    for (int c = threadIdx.x; c < a.Kmax; c += 256) {
        const int n = c < K ? cn[c] : 0;
        if (count) count[(size_t)l * a.Kmax + c] = n;
        if (cluster_mean) cluster_mean[(size_t)l * a.Kmax + c] = n > 0 ? bins[c] / (double)n : 0.0;
    }
}

// ---------------------------------------------------------------- CH and DB
__global__ __launch_bounds__(256) void sil_msum_kernel(SilArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];      // K x 4 sums
    __shared__ double sv[256 * 4];
    __shared__ __attribute__((aligned(16))) int sl[256];
    const int l = blockIdx.y, c4 = 4 * blockIdx.x, tid = threadIdx.x, K = a.meta[l], N = a.N;
    const int col = tid & 3, cls = tid >> 2;
    const int32_t* lab = a.label + (size_t)l * N;
    for (int q = tid; q < 4 * K; q += 256) smem[q] = 0.0;
    for (int base = 0; base < N; base += 256) {
        const int i = base + tid;
        int c = -1;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        if (i < N) c = valid_label(lab[i], K);
        if (c >= 0) {
            const float4 f = *reinterpret_cast<const float4*>(a.x + (size_t)i * a.dim + c4);
            const double rn = a.rnorm ? a.rnorm[i] : -1.0;
            v[0] = row_value(f.x, rn); v[1] = row_value(f.y, rn); v[2] = row_value(f.z, rn); v[3] = row_value(f.w, rn);
        }
        __syncthreads();
        sl[tid] = c;
        for (int u = 0; u < 4; ++u) sv[4 * tid + u] = v[u];
        __syncthreads();
        for (int q0 = 0; q0 < 256 && base + q0 < N; q0 += 8) {      // eight labels per step, as in bin_rows
            const int4 ca = *reinterpret_cast<const int4*>(sl + q0), cb = *reinterpret_cast<const int4*>(sl + q0 + 4);
            const int cc[8] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
#pragma unroll
            for (int u = 0; u < 8; ++u) if (cc[u] >= 0 && (cc[u] & 63) == cls) smem[4 * cc[u] + col] += sv[4 * (q0 + u) + col];
        }
    }
    __syncthreads();
    double* out = a.msum + (size_t)a.meta[a.L + l] * a.dim;
    for (int q = tid; q < 4 * K; q += 256) out[(size_t)(q >> 2) * a.dim + c4 + (q & 3)] = smem[q];
}

// thread t the columns t, t + 256 ..: the clusters' sums in ascending order -> the mean of the labelled rows; a sum -> the cluster's mean
__global__ __launch_bounds__(256) void sil_mean_kernel(SilArgs a)
{
    const int l = blockIdx.x, K = a.meta[l], dim = a.dim;
    const int* cn = a.cnt + a.meta[a.L + l];
    double* ms = a.msum + (size_t)a.meta[a.L + l] * dim;
    for (int j = threadIdx.x; j < dim; j += 256) {
        double tot = 0.0; int nlab = 0;
        for (int c = 0; c < K; ++c) {
            const int n = cn[c];
            if (n == 0) continue;
            const double v = ms[(size_t)c * dim + j];
            tot += v; nlab += n;
            ms[(size_t)c * dim + j] = v / (double)n;
        }
        a.gmean[(size_t)l * dim + j] = nlab > 0 ? tot / (double)nlab : 0.0;
    }
}

// one wave per row: lane q the elements 4 q .., 256 + 4 q .. in index order, then the butterfly
__global__ __launch_bounds__(256) void sil_rowdev_kernel(SilArgs a)
{
    const int l = blockIdx.y, lane = threadIdx.x & 63, dim = a.dim;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.N) return;
    const int c = valid_label(a.label[(size_t)l * a.N + i], a.meta[l]);
    double s = 0.0;
    if (c >= 0) {
        const double* m = a.msum + (size_t)(a.meta[a.L + l] + c) * dim;
        const double rn = a.rnorm ? a.rnorm[i] : -1.0;
        for (int j = lane * 4; j < dim; j += 256) {
            const float4 f = *reinterpret_cast<const float4*>(a.x + (size_t)i * dim + j);
            double d;
            d = row_value(f.x, rn) - m[j]; s = fma(d, d, s); d = row_value(f.y, rn) - m[j + 1]; s = fma(d, d, s);
            d = row_value(f.z, rn) - m[j + 2]; s = fma(d, d, s); d = row_value(f.w, rn) - m[j + 3]; s = fma(d, d, s);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    }
    if (lane == 0) { a.e[(size_t)l * a.N + i] = s; a.r[(size_t)l * a.N + i] = sqrt(s); }
}

__global__ __launch_bounds__(256) void sil_within_kernel(SilArgs a)
{
    __shared__ double bins[kSilMaxK];
    __shared__ double sv[256];
    __shared__ __attribute__((aligned(16))) int sl[256];
    __shared__ double sh[4];
    __shared__ int shi[4];
    const int l = blockIdx.x, K = a.meta[l], dim = a.dim, N = a.N, off = a.meta[a.L + l];
    const int* cn = a.cnt + off;
    bin_rows(a.label + (size_t)l * N, a.r + (size_t)l * N, N, K, bins, sl, sv);
    for (int c = threadIdx.x; c < K; c += 256) a.Sc[off + c] = cn[c] > 0 ? bins[c] / (double)cn[c] : 0.0;
    double w = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) w += a.e[(size_t)l * N + i];      // (0 for an unlabelled row)
    w = block_sum<4>(w, sh);
    double b = 0.0; int ne = 0;
    const double* gm = a.gmean + (size_t)l * dim;
    for (int c = threadIdx.x; c < K; c += 256) {
        if (cn[c] == 0) continue;
        const double* m = a.msum + (size_t)(off + c) * dim;
        double d2 = 0.0;
        for (int j = 0; j < dim; ++j) { const double d = m[j] - gm[j]; d2 = fma(d, d, d2); }
        b += (double)cn[c] * d2; ++ne;
    }
    b = block_sum<4>(b, sh);
    const int nlab = labelled_rows(cn, K, shi);
    ne = wave_sum(ne);
    if ((threadIdx.x & 63) == 0) shi[threadIdx.x >> 6] = ne;
    __syncthreads();
    if (threadIdx.x == 0) {
        double* t = a.tr + 4 * l;
        t[0] = w; t[1] = b; t[2] = (double)(shi[0] + shi[1] + shi[2] + shi[3]); t[3] = (double)nlab;
    }
}

// one workgroup per (cluster c, labeling): the largest R_cc' over the non-empty c' != c, thread t the clusters t, t + 256 ..
__global__ __launch_bounds__(256) void sil_db_kernel(SilArgs a)
{
    __shared__ double mc[1024];
    __shared__ double sh[4];
    const int l = blockIdx.y, c = blockIdx.x, K = a.meta[l], dim = a.dim, off = a.meta[a.L + l];
    if (c >= K || a.cnt[off + c] == 0) return;
    for (int j = threadIdx.x; j < dim; j += 256) mc[j] = a.msum[(size_t)(off + c) * dim + j];
    __syncthreads();
    const double sc = a.Sc[off + c];
    double best = 0.0;
    for (int o = threadIdx.x; o < K; o += 256) {
        if (o == c || a.cnt[off + o] == 0) continue;
        const double* m = a.msum + (size_t)(off + o) * dim;
        double d2 = 0.0;
        for (int j = 0; j < dim; ++j) { const double d = mc[j] - m[j]; d2 = fma(d, d, d2); }
        const double M = sqrt(d2);
        const double R = M > 0.0 ? (sc + a.Sc[off + o]) / M : 0.0;
        best = fmax(best, R);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = fmax(best, __shfl_xor(best, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) a.dbp[off + c] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}

__global__ __launch_bounds__(256) void sil_index_kernel(SilArgs a, double* index)
{
    __shared__ double sh[4];
    const int l = blockIdx.x, K = a.meta[l], off = a.meta[a.L + l];
    double v = 0.0;
    for (int c = threadIdx.x; c < K; c += 256) if (a.cnt[off + c] > 0) v += a.dbp[off + c];
    v = block_sum<4>(v, sh);
    if (threadIdx.x == 0) {
        const double* t = a.tr + 4 * l;
        const double trW = t[0], trB = t[1], ke = t[2], ne = t[3];
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        double ch = nan;
        if (ke >= 2.0 && ne > ke) ch = trW == 0.0 ? 1.0 : (trB / (ke - 1.0)) / (trW / (ne - ke));
        index[2 * l] = ch;
        index[2 * l + 1] = ke >= 2.0 ? v / ke : nan;
    }
}

template <int TI>
hipError_t launch_pass(hipStream_t st, const SilArgs& a, int tiles, int l0, int nl, int tj, size_t lds)
{
    auto go = [&](auto kernel) {
        if (lds > 65536) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kSilLds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kernel, dim3(tiles), dim3(256), lds, st, a, l0, nl, tj);
        return hipGetLastError();
    };
    return a.metric == 1 ? go(sil_pass_kernel<TI, true>) : go(sil_pass_kernel<TI, false>);
}

int allowed_ti(int cap)
{
    int ti = 4;
    while (ti < 64 && 2 * ti <= cap) ti *= 2;
    return ti;
}

}  // namespace

size_t sil_staging(int TI, int nl)
{
    return 8 * ((size_t)TI * TJ + (size_t)DK * TI + DK * TJ + TI + TJ) + 4 * ((size_t)nl * TJ + (size_t)nl * TI + 2 * kSilMaxL);
}

// The passes at TI rows: labelings are taken in order while their bins and the staging fit the LDS (and, with the option, the bin columns
// stay within it; a labeling alone is always taken).  -> the number of passes, 0 where a labeling does not fit on its own
static int sil_passes(int TI, int L, const int32_t* K, int chunk_opt, SilPlan* p)
{
    int np = 0, l = 0;
    while (l < L) {
        long long cols = 0; int nl = 0;
        while (l + nl < L) {
            const long long c2 = cols + K[l + nl];
            if ((size_t)TI * c2 * 8 + sil_staging(TI, nl + 1) > (size_t)kSilLds) break;
            if (chunk_opt > 0 && nl > 0 && c2 > chunk_opt) break;
            cols = c2; ++nl;
        }
        if (nl == 0) return 0;
        if (p) { p->begin[np] = l; p->bytes[np] = (int)((size_t)TI * cols * 8 + sil_staging(TI, nl)); }
        ++np; l += nl;
    }
    if (p) { p->begin[np] = L; p->npass = np; }
    return np;
}

// the largest TI in {4 .. 64} (within the option's cap) that needs no more passes than TI = 4 does; then, unless the option gave the cap,
// smaller while there are fewer row tiles than CUs.  dim does not enter: the rows are staged 32 elements at a time.
SilPlan sil_plan(int N, int dim, int L, const int32_t* K, int chunk_opt, int cus)
{
    (void)dim;
    SilPlan p{};
    p.TJ = chunk_opt > 0 ? std::min(chunk_opt, TJ) : TJ;
    const int least = sil_passes(4, L, K, chunk_opt, nullptr);
    int ti = chunk_opt > 0 ? allowed_ti(chunk_opt) : 64;
    while (ti > 4 && sil_passes(ti, L, K, chunk_opt, nullptr) != least) ti /= 2;
    while (chunk_opt <= 0 && ti > 4 && (N + ti - 1) / ti < cus) ti /= 2;
    p.TI = ti;
    sil_passes(ti, L, K, chunk_opt, &p);
    return p;
}

hipError_t sil_prepare(hipStream_t st, const SilArgs& a)
{
    if (a.rnorm) sil_rownorm_kernel<<<(a.N + 3) / 4, 256, 0, st>>>(a.x, a.N, a.dim, const_cast<double*>(a.rnorm));
    sil_count_kernel<<<dim3((a.N + 255) / 256, a.L), 256, 0, st>>>(a);
    return hipGetLastError();
}

hipError_t sil_pairs(hipStream_t st, const SilArgs& a, const SilPlan& p)
{
    const int tiles = (a.N + p.TI - 1) / p.TI;
    for (int q = 0; q < p.npass; ++q) {
        const int l0 = p.begin[q], nl = p.begin[q + 1] - l0;
        hipError_t e = hipErrorInvalidValue;
        switch (p.TI) {
            case 4: e = launch_pass<4>(st, a, tiles, l0, nl, p.TJ, (size_t)p.bytes[q]); break;
            case 8: e = launch_pass<8>(st, a, tiles, l0, nl, p.TJ, (size_t)p.bytes[q]); break;
            case 16: e = launch_pass<16>(st, a, tiles, l0, nl, p.TJ, (size_t)p.bytes[q]); break;
            case 32: e = launch_pass<32>(st, a, tiles, l0, nl, p.TJ, (size_t)p.bytes[q]); break;
            case 64: e = launch_pass<64>(st, a, tiles, l0, nl, p.TJ, (size_t)p.bytes[q]); break;
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t sil_scores(hipStream_t st, const SilArgs& a, double* score, int32_t* count, double* cluster_mean)
{
    sil_score_kernel<<<a.L, 256, 0, st>>>(a, score, count, cluster_mean);
    return hipGetLastError();
}

hipError_t sil_indices(hipStream_t st, const SilArgs& a, double* index)
{
    const size_t lds = (size_t)a.Kmax * 4 * sizeof(double);
    if (lds > 65536 - 10240) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sil_msum_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(sil_msum_kernel, dim3(a.dim / 4, a.L), dim3(256), lds, st, a);
    sil_mean_kernel<<<a.L, 256, 0, st>>>(a);
    sil_rowdev_kernel<<<dim3((a.N + 3) / 4, a.L), 256, 0, st>>>(a);
    sil_within_kernel<<<a.L, 256, 0, st>>>(a);
    sil_db_kernel<<<dim3(a.Kmax, a.L), 256, 0, st>>>(a);
    sil_index_kernel<<<a.L, 256, 0, st>>>(a, index);
    return hipGetLastError();
}

}  // namespace avae
