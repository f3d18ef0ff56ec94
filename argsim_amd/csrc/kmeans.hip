// kmeans.hip -- k-means of latent rows: greedy k-means++ seeding, Lloyd iterations with the relocation of empty clusters, R restarts
// side by side (contract: include/argsim_vae.h, avae_kmeans).  Every value a decision or an output depends on is a
// double; the rows are fp32 and, for the cosine, divided by their double norm where they are loaded.
//
//   km_dist      grid = (row tiles) x (centre parts) x (restarts).  64 rows x 64 centres per stage, 16 x 16 threads with 4 x 4 pairs
//                each: 32 columns of the rows and of the centres are staged in LDS as doubles, a pair's sum of (x - c)^2 runs over the
//                columns in ascending order.  A row keeps its running first minimum (distance, centre) over the part's centres: the
//                (N, k) panel never reaches memory.  The seeding runs the same loop with 16 candidates per stage and writes every
//                distance.
//   km_merge     the parts' minima of a row in ascending part order -> label, distance, "a label changed", the row blocks' histograms
//   km_scan      one workgroup per restart: counts, the clusters' first sorted positions, and for empty clusters the rows with the
//                largest distances
//   km_place     the stable counting sort: rows by (label, row)
//   km_slices    member sums of the sorted rows, `slice` positions per workgroup, one partial per (slice, cluster)
//   km_centres   one workgroup per (cluster, restart): the slices' partials in ascending order, the relocations, the centre, its shift
//   km_decide    the shift's sum and the stop decision
// Reduction orders are fixed by the plan alone (km_plan): no float atomics; the integer atomics (histogram, flags) commute.  The same
// arguments give the same bits.
#include "kernels.h"
#include "reduce_dev.h"
#include "row_parts.h"
#include "rows_dev.h"

#include <algorithm>

namespace avae {

namespace {

constexpr int kDK = 32;            // columns per LDS stage

// the norm of row i, or -1 where the rows are taken as they are
__device__ __forceinline__ double row_norm(const KmArgs& a, long long i) { return a.rnorm ? a.rnorm[i] : -1.0; }

// exclusive prefix of one value per thread in thread order, and the total: a shuffle scan per wave, then the waves before this one in
// ascending order.  sh: NW values; ends in a barrier
template <class T, int NW>
__device__ __forceinline__ T block_excl_scan(T v, T* sh, T* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const T u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
    const T prev = __shfl_up(inc, 1, 64);
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    T base = 0, tot = 0;
    for (int w = 0; w < NW; ++w) { if (w == wave) base = tot; tot += sh[w]; }
    __syncthreads();
    *total = tot;
    return lane ? base + prev : base;
}

__device__ __forceinline__ int block_min_int(int v, int* sh, int nw)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = sh[0];
    for (int w = 1; w < nw; ++w) s = min(s, sh[w]);
    __syncthreads();
    return s;
}

// one wave per row: its norm (rows_dev.h)
__global__ __launch_bounds__(256) void km_rownorm_kernel(const float* __restrict__ x, int N, int dim, double* __restrict__ rn)
{
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const double v = wave_row_norm(x, row, dim);
    if ((threadIdx.x & 63) == 0) rn[row] = v;
}

// column sums over a run of rows: mode 0 of the values, mode 1 of their squared deviation from mean; thread t owns columns t, t + 256 ..
__global__ __launch_bounds__(256) void km_colpart_kernel(KmArgs a, int rows, int mode)
{
    const long long r0 = (long long)blockIdx.x * rows, r1 = std::min<long long>(r0 + rows, a.N);
    double acc[4] = {0.0, 0.0, 0.0, 0.0}, mu[4] = {0.0, 0.0, 0.0, 0.0};
    for (int u = 0; u < 4; ++u) { const int c = threadIdx.x + 256 * u; if (mode && c < a.dim) mu[u] = a.mean[c]; }
    for (long long i = r0; i < r1; ++i) {
        const double rn = row_norm(a, i);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = threadIdx.x + 256 * u;
            if (c < a.dim) { const double v = row_value(a.x[i * a.dim + c], rn) - mu[u]; acc[u] += mode ? v * v : v; }
        }
    }
    for (int u = 0; u < 4; ++u) { const int c = threadIdx.x + 256 * u; if (c < a.dim) a.vpart[(size_t)blockIdx.x * a.dim + c] = acc[u]; }
}

// one workgroup, thread c owns column c: the blocks' partials in ascending order; mode 0 -> mean, mode 1 -> tol_abs of every restart
__global__ __launch_bounds__(1024) void km_colreduce_kernel(KmArgs a, int blocks, int mode, double tol)
{
    __shared__ double sh[16];
    const int c = threadIdx.x;
    double s = 0.0;
    if (c < a.dim) for (int b = 0; b < blocks; ++b) s += a.vpart[(size_t)b * a.dim + c];
    s /= (double)a.N;
    if (!mode) { if (c < a.dim) a.mean[c] = s; return; }
    const double tot = block_sum<16>(c < a.dim ? s : 0.0, sh);
    if (c < a.R) a.st[c].tol_abs = tol * (tot / (double)a.dim);
}

// ---------------------------------------------------------------- distances
// MODE 0: the first minimum over the part's centres of every row of the tile -> pd, pi.  `last`: the assignment after the loop, for the
// restarts that did not stop as converged.  MODE 1 (seeding): the distance of every row to each of nc <= 16 candidates -> D.
template <int CB, int MODE>
__global__ __launch_bounds__(256) void km_dist_kernel(KmArgs a, const double* __restrict__ cen, int nc, long long cstride, int last)
{
    constexpr int TC = 16 * CB;
    __shared__ __attribute__((aligned(16))) double xs[kDK][kKmTile];
    __shared__ __attribute__((aligned(16))) double cs[kDK][TC];
    const int r = blockIdx.z;
    if (MODE == 0 && (last ? a.st[r].how == 0 : a.st[r].stop_at != 0)) return;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int N = a.N, dim = a.dim;
    const long long row0 = (long long)blockIdx.x * a.p.tile;
    const int nrow = (int)std::min<long long>(a.p.tile, N - row0);
    int cb = 0, ce = nc;
    if (MODE == 0) { long long b; part_range(blockIdx.y, a.p.chunk, nc, b, ce); cb = (int)b; }
    const double* __restrict__ cr = cen + (size_t)r * cstride;

    // what this thread stages of the rows: two float4 per stage, rows sx[u], column unit sq[u]
    double rn[2];
    for (int u = 0; u < 2; ++u) { const int rl = (tid + 256 * u) >> 3; rn[u] = rl < nrow ? row_norm(a, row0 + rl) : 0.0; }

    ArgMinFirst best[4];
    for (int c0 = cb; c0 < ce; c0 += TC) {
        double acc[4][CB];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < CB; ++j) acc[i][j] = 0.0;
        for (int j0 = 0; j0 < dim; j0 += kDK) {
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int idx = tid + 256 * u, rl = idx >> 3, col = j0 + 4 * (idx & 7);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                const bool on = rl < nrow && col < dim;
                if (on) v = *reinterpret_cast<const float4*>(a.x + (row0 + rl) * dim + col);
                const int jj = 4 * (idx & 7);
                xs[jj][rl] = on ? row_value(v.x, rn[u]) : 0.0; xs[jj + 1][rl] = on ? row_value(v.y, rn[u]) : 0.0;
                xs[jj + 2][rl] = on ? row_value(v.z, rn[u]) : 0.0; xs[jj + 3][rl] = on ? row_value(v.w, rn[u]) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < TC * kDK / 256; ++u) {
                const int idx = tid + 256 * u, cl = idx >> 5, jj = idx & 31, c = c0 + cl;
                cs[jj][cl] = (c < ce && j0 + jj < dim) ? cr[(size_t)c * dim + j0 + jj] : 0.0;
            }
            __syncthreads();
#pragma unroll 4
            for (int j = 0; j < kDK; ++j) {
                double xa[4], ca[CB];
#pragma unroll
                for (int i = 0; i < 4; ++i) xa[i] = xs[j][ty * 4 + i];
#pragma unroll
                for (int i = 0; i < CB; ++i) ca[i] = cs[j][tx * CB + i];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int q = 0; q < CB; ++q) { const double d = xa[i] - ca[q]; acc[i][q] = fma(d, d, acc[i][q]); }
            }
        }
        if (MODE == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < CB; ++q) { const int c = c0 + tx * CB + q; if (c < ce) best[i].take(acc[i][q], c); }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rl = ty * 4 + i;
                if (rl < nrow && tx < nc) a.D[((size_t)r * a.T + tx) * N + row0 + rl] = acc[i][0];
            }
        }
    }
    if (MODE == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            best[i].wave_merge<16>();
            const int rl = ty * 4 + i;
            if (tx == 0 && rl < nrow) {
                const size_t o = ((size_t)r * a.p.parts + blockIdx.y) * N + row0 + rl;
                a.pd[o] = best[i].v; a.pi[o] = best[i].i;
            }
        }
    }
}

// a row's minima over the parts in ascending part order (strict <: the first minimum); a row without a number takes cluster 0
__global__ __launch_bounds__(256) void km_merge_kernel(KmArgs a, int last)
{
    const int r = blockIdx.y;
    if (last ? a.st[r].how == 0 : a.st[r].stop_at != 0) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int diff = 0;
    if (i < a.N) {
        ArgMinFirst m;
        for (int p = 0; p < a.p.parts; ++p) { const size_t o = ((size_t)r * a.p.parts + p) * a.N + i; m.take(a.pd[o], a.pi[o]); }
        const int l = m.i == 0x7fffffff ? 0 : m.i;
        const size_t o = (size_t)r * a.N + i;
        diff = a.lab[o] != l;
        a.lab[o] = l; a.dist[o] = m.v;
        if (!last) atomicAdd(&a.hist[((size_t)r * a.p.blks + (int)(i / a.p.blk)) * a.k + l], 1);
    }
    if (!last && __any(diff) && (threadIdx.x & 63) == 0) atomicOr(&a.st[r].changed, 1);
}

// one workgroup of 1024 per restart, thread t owns clusters 4 t .. 4 t + 3: the counts (the histograms are left zero for the next
// iteration), the clusters' first sorted positions, the list of empty clusters, and for the e-th of them the row with the e-th largest
// distance to its own centre (ties: the smaller row): one sweep over the rows per empty cluster
__global__ __launch_bounds__(1024) void km_scan_kernel(KmArgs a)
{
    __shared__ int shi[16];
    __shared__ double shv[16];
    const int r = blockIdx.x, t = threadIdx.x, k = a.k;
    KmState& s = a.st[r];
    if (s.stop_at != 0) return;
    int cnt[4], mine = 0, emp = 0;
    for (int u = 0; u < 4; ++u) {
        const int c = 4 * t + u;
        int run = 0;
        if (c < k)
            for (int b = 0; b < a.p.blks; ++b) {
                const size_t o = ((size_t)r * a.p.blks + b) * k + c;
                const int h = a.hist[o];
                a.off[o] = run; a.hist[o] = 0; run += h;
            }
        cnt[u] = run; mine += run; emp += (c < k && run == 0) ? 1 : 0;
    }
    int total, nempty;
    int pos = block_excl_scan<int, 16>(mine, shi, &total);
    int e = block_excl_scan<int, 16>(emp, shi, &nempty);
    int* start = a.start + (size_t)r * (k + 1);
    int* rel = a.rel + (size_t)r * k * 3;
    for (int u = 0; u < 4; ++u) {
        const int c = 4 * t + u;
        if (c >= k) break;
        start[c] = pos; pos += cnt[u];
        if (cnt[u] == 0) { rel[3 * e + 2] = c; ++e; }
    }
    if (t == 0) { start[k] = total; s.nempty = nempty; s.reloc += nempty; }
    if (nempty == 0) return;
    const double* dist = a.dist + (size_t)r * a.N;
    double pv = -INFINITY; int pr = -1;                   // the previous pick as (-distance, row): the next one comes strictly after it
    for (int q = 0; q < nempty; ++q) {
        ArgMinFirst m;
        for (int i = t; i < a.N; i += 1024) {
            const double v = -dist[i];
            if (v > pv || (v == pv && i > pr)) m.merge(ArgMinFirst{v, i});
        }
        m.wave_merge();
        m.block_merge<16>(shv, shi);
        const bool none = m.i == 0x7fffffff;
        if (t == 0) { rel[3 * q] = none ? -1 : m.i; rel[3 * q + 1] = none ? 0 : a.lab[(size_t)r * a.N + m.i]; }
        if (none) { for (int z = q + 1 + t; z < nempty; z += 1024) rel[3 * z] = -1; break; }
        pv = m.v; pr = m.i;
    }
}

// the stable counting sort, one workgroup per row block: 256 rows at a time in ascending order; a row's rank among the rows of its label
// in this step comes from a sweep over the step's labels in LDS
__global__ __launch_bounds__(256) void km_place_kernel(KmArgs a)
{
    __shared__ int sl[256];
    __shared__ int pos[kKmMaxK];                            // where the block's next row of a cluster goes
    const int r = blockIdx.y, b = blockIdx.x, t = threadIdx.x, k = a.k;
    if (a.st[r].stop_at != 0) return;
    const long long r0 = (long long)b * a.p.blk, r1 = std::min<long long>(r0 + a.p.blk, a.N);
    const int* start = a.start + (size_t)r * (k + 1);
    const int* off = a.off + ((size_t)r * a.p.blks + b) * k;
    int* order = a.order + (size_t)r * a.N;
    for (int c = t; c < k; c += 256) pos[c] = start[c] + off[c];
    for (long long base = r0; base < r1; base += 256) {
        const long long i = base + t;
        const int l = i < r1 ? a.lab[(size_t)r * a.N + i] : -1;
        sl[t] = l;
        __syncthreads();                                    // (the first one also covers pos)
        int before = 0, same = 0;
        for (int q = 0; q < 256; ++q) { const int m = sl[q] == l; same += m; before += (q < t) ? m : 0; }
        const int at = l >= 0 ? pos[l] : 0;
        __syncthreads();
        if (l >= 0) {
            order[at + before] = (int)i;
            if (before == same - 1) pos[l] = at + same;     // the label's last row of this step
        }
    }
}

// member sums.  Workgroup s owns the sorted positions [s slice, (s + 1) slice) and walks the clusters that have rows there; the partial of
// (s, c) goes to slot s + c (unique: along the walk s or c grows).  Thread = (row group g, column unit q): group g adds positions
// lo + g, lo + g + G .. in that order, then the groups' sums are added in ascending g
__global__ __launch_bounds__(256) void km_slices_kernel(KmArgs a)
{
    __shared__ double red[256 * 4];
    const int r = blockIdx.y, s = blockIdx.x, t = threadIdx.x, k = a.k, dim = a.dim;
    if (a.st[r].stop_at != 0) return;
    const int nq = dim >> 2;
    int nqp = 1; while (nqp < nq) nqp <<= 1;
    const int G = 256 / nqp, g = t / nqp, q = t % nqp;
    const int* start = a.start + (size_t)r * (k + 1);
    const int* order = a.order + (size_t)r * a.N;
    const int pb = (int)std::min<long long>((long long)s * a.p.slice, a.N), pe = (int)std::min<long long>((long long)pb + a.p.slice, a.N);
    int lo = 0, hi = k;                                     // the last cluster with start <= pb
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (start[mid] <= pb) lo = mid; else hi = mid; }
    for (int c = lo; c < k && start[c] < pe; ++c) {
        const int p0 = max(start[c], pb), p1 = min(start[c + 1], pe);
        if (p1 <= p0) continue;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        if (q < nq)
            for (int p = p0 + g; p < p1; p += G) {
                const long long row = order[p];
                const double rn = row_norm(a, row);
                const float4 v = *reinterpret_cast<const float4*>(a.x + row * dim + 4 * q);
                acc[0] += row_value(v.x, rn); acc[1] += row_value(v.y, rn); acc[2] += row_value(v.z, rn); acc[3] += row_value(v.w, rn);
            }
        for (int u = 0; u < 4; ++u) red[(g * nqp + q) * 4 + u] = acc[u];
        __syncthreads();
        if (g == 0 && q < nq) {
            const int ng = min(G, p1 - p0);
            for (int gg = 1; gg < ng; ++gg)
                for (int u = 0; u < 4; ++u) acc[u] += red[(gg * nqp + q) * 4 + u];
            double* out = a.psum + ((size_t)r * (a.p.slices + k) + s + c) * dim + 4 * q;
            for (int u = 0; u < 4; ++u) out[u] = acc[u];
        }
        __syncthreads();
    }
}

// one workgroup per (cluster, restart), thread q owns columns 4 q .. 4 q + 3: the partials of the cluster's slices in ascending order;
// the relocations in their order (the row leaves its cluster's sum and count; the empty cluster becomes that row); sum / count; for
// the cosine the centre divided by its norm; the squared shift against the old centre, which is then overwritten
__global__ __launch_bounds__(256) void km_centres_kernel(KmArgs a)
{
    __shared__ double sh[4];
    const int r = blockIdx.y, c = blockIdx.x, q = threadIdx.x, k = a.k, dim = a.dim;
    const KmState& s = a.st[r];
    if (s.stop_at != 0) return;
    const bool on = 4 * q < dim;
    const int* start = a.start + (size_t)r * (k + 1);
    int cnt = start[c + 1] - start[c];
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    if (cnt > 0 && on) {
        const int s0 = start[c] / a.p.slice, s1 = (start[c + 1] - 1) / a.p.slice;
        for (int sl = s0; sl <= s1; ++sl) {
            const double* in = a.psum + ((size_t)r * (a.p.slices + k) + sl + c) * dim + 4 * q;
            for (int u = 0; u < 4; ++u) sum[u] += in[u];
        }
    }
    const int* rel = a.rel + (size_t)r * k * 3;
    for (int e = 0; e < s.nempty; ++e) {
        const int row = rel[3 * e], from = rel[3 * e + 1], to = rel[3 * e + 2];
        if (row < 0 || (from != c && to != c)) continue;
        double xv[4] = {0.0, 0.0, 0.0, 0.0};
        if (on) {
            const double rn = row_norm(a, row);
            const float4 v = *reinterpret_cast<const float4*>(a.x + (size_t)row * dim + 4 * q);
            xv[0] = row_value(v.x, rn); xv[1] = row_value(v.y, rn); xv[2] = row_value(v.z, rn); xv[3] = row_value(v.w, rn);
        }
        if (from == c) { for (int u = 0; u < 4; ++u) sum[u] -= xv[u]; --cnt; }
        if (to == c) { for (int u = 0; u < 4; ++u) sum[u] = xv[u]; cnt = 1; }
    }
    if (cnt > 0) for (int u = 0; u < 4; ++u) sum[u] /= (double)cnt;
    if (a.rnorm) {
        const double n2 = block_sum<4>(sum[0] * sum[0] + sum[1] * sum[1] + sum[2] * sum[2] + sum[3] * sum[3], sh);
        const double nr = sqrt(n2);
        if (nr > 0.0) for (int u = 0; u < 4; ++u) sum[u] /= nr;
    }
    double* cen = a.C + ((size_t)r * k + c) * dim + 4 * q;
    double d2 = 0.0;
    if (on) for (int u = 0; u < 4; ++u) { const double d = sum[u] - cen[u]; d2 += d * d; cen[u] = sum[u]; }
    d2 = block_sum<4>(d2, sh);
    if (q == 0) a.shiftp[(size_t)r * k + c] = d2;
}

// one workgroup per restart: the shift as the sum over the centres (thread t adds centres t, t + 256 .., then block_sum) and the stop
__global__ __launch_bounds__(256) void km_decide_kernel(KmArgs a, int it)
{
    __shared__ double sh[4];
    const int r = blockIdx.x;
    KmState& s = a.st[r];
    if (s.stop_at != 0) return;
    double v = 0.0;
    for (int c = threadIdx.x; c < a.k; c += 256) v += a.shiftp[(size_t)r * a.k + c];
    const double shift = block_sum<4>(v, sh);
    if (threadIdx.x == 0) {
        int how = -1;
        if (!s.changed) how = 0;
        else if (shift <= s.tol_abs) how = 1;
        else if (it + 1 == a.max_iter) how = 2;
        s.changed = 0;
        if (how >= 0) { s.how = how; s.stop_at = it + 1; }
    }
}

// ---------------------------------------------------------------- the end of the call
// inertia partials: one workgroup per row tile, wave w the tile's rows w, w + 4 .. (lane l the columns 4 l .., 256 + 4 l .., then the
// butterfly), the rows' sums added in that order, then the waves ascending
__global__ __launch_bounds__(256) void km_inertia_kernel(KmArgs a)
{
    __shared__ double sh[4];
    const int r = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, dim = a.dim;
    const long long row0 = (long long)blockIdx.x * a.p.tile;
    const int nrow = (int)std::min<long long>(a.p.tile, a.N - row0);
    double tot = 0.0;
    for (int rl = wave; rl < nrow; rl += 4) {
        const long long i = row0 + rl;
        const double rn = row_norm(a, i);
        const double* cen = a.C + ((size_t)r * a.k + a.lab[(size_t)r * a.N + i]) * dim;
        double sacc = 0.0;
        for (int c = lane * 4; c < dim; c += 256) {
            const float4 v = *reinterpret_cast<const float4*>(a.x + i * dim + c);
            double d;
            d = row_value(v.x, rn) - cen[c]; sacc = fma(d, d, sacc); d = row_value(v.y, rn) - cen[c + 1]; sacc = fma(d, d, sacc);
            d = row_value(v.z, rn) - cen[c + 2]; sacc = fma(d, d, sacc); d = row_value(v.w, rn) - cen[c + 3]; sacc = fma(d, d, sacc);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sacc += __shfl_xor(sacc, o, 64);
        tot += sacc;
    }
    if (lane == 0) sh[wave] = tot;
    __syncthreads();
    if (threadIdx.x == 0) a.ipart[(size_t)r * a.p.tiles + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// one workgroup: every restart's inertia (thread t adds tiles t, t + 1024 .., then block_sum), the first smallest, the statistics
__global__ __launch_bounds__(1024) void km_best_kernel(KmArgs a, int32_t* stat, double* inertia, int32_t* stat_all)
{
    __shared__ double sh[16];
    __shared__ double ine[kKmMaxInit];
    for (int r = 0; r < a.R; ++r) {
        double v = 0.0;
        for (int t = threadIdx.x; t < a.p.tiles; t += 1024) v += a.ipart[(size_t)r * a.p.tiles + t];
        v = block_sum<16>(v, sh);
        if (threadIdx.x == 0) ine[r] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int best = 0;
        for (int r = 0; r < a.R; ++r) {
            inertia[r] = ine[r];
            if (ine[r] < ine[best]) best = r;
            if (stat_all) { stat_all[4 * r] = a.st[r].stop_at; stat_all[4 * r + 1] = a.st[r].how; stat_all[4 * r + 2] = a.st[r].reloc; stat_all[4 * r + 3] = 0; }
        }
        *a.best = best;
        stat[0] = best; stat[1] = a.st[best].stop_at; stat[2] = a.st[best].how; stat[3] = a.st[best].reloc;
    }
}

__global__ __launch_bounds__(256) void km_copy_kernel(KmArgs a, int32_t* label, float* centers, int32_t* label_all, double* centers_all)
{
    const int best = *a.best;
    const size_t step = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x, kd = (size_t)a.k * a.dim;
    for (size_t i = t0; i < (size_t)a.N; i += step) label[i] = a.lab[(size_t)best * a.N + i];
    for (size_t i = t0; i < kd; i += step) centers[i] = (float)a.C[best * kd + i];
    if (label_all) for (size_t i = t0; i < (size_t)a.R * a.N; i += step) label_all[i] = a.lab[i];
    if (centers_all) for (size_t i = t0; i < a.R * kd; i += step) centers_all[i] = a.C[i];
}

__global__ __launch_bounds__(256) void km_load_kernel(const float* __restrict__ in, double* __restrict__ C, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) C[i] = (double)in[i];
}

// ---------------------------------------------------------------- seeding
__device__ __forceinline__ uint64_t seed_index(int r, int c, int t) { return ((((uint64_t)r << 20) + (uint64_t)c) << 20) + (uint64_t)t; }

// row `row` as doubles into dst (dim), by the whole workgroup
__device__ __forceinline__ void copy_row(const KmArgs& a, int row, double* dst)
{
    const double rn = row_norm(a, row);
    for (int j = threadIdx.x; j < a.dim; j += blockDim.x) dst[j] = row_value(a.x[(size_t)row * a.dim + j], rn);
}

// centre 0 of restart r: row floor(u N), as the only candidate of round 0
__global__ __launch_bounds__(256) void km_seed_first_kernel(KmArgs a)
{
    const int r = blockIdx.x;
    const double u = (double)uniform01(a.seed, 7, seed_index(r, 0, 0));
    const int row = min((int)floor(u * (double)a.N), a.N - 1);
    copy_row(a, row, a.candC + (size_t)r * a.T * a.dim);
    copy_row(a, row, a.C + (size_t)r * a.k * a.dim);
    if (threadIdx.x == 0) { a.st[r].chosen = 0; a.cand[r * a.T] = row; }
}

// per candidate the potential's partial over a scan tile: thread t the rows 4 t .. 4 t + 3 of the tile in order, then block_sum
__global__ __launch_bounds__(256) void km_seed_pot_kernel(KmArgs a)
{
    __shared__ double sh[4];
    const int r = blockIdx.y, N = a.N;
    const long long r0 = (long long)blockIdx.x * a.p.scan;
    const int nrow = (int)std::min<long long>(a.p.scan, N - r0);
    for (int t = 0; t < a.T; ++t) {
        double v = 0.0;
        for (int u = 0; u < 4; ++u) {
            const int rl = 4 * threadIdx.x + u;
            if (rl < nrow) v += fmin(a.closest[(size_t)r * N + r0 + rl], a.D[((size_t)r * a.T + t) * N + r0 + rl]);
        }
        v = block_sum<4>(v, sh);
        if (threadIdx.x == 0) a.ppart[((size_t)r * a.T + t) * a.p.scans + blockIdx.x] = v;
    }
}

// one workgroup per restart: each candidate's potential (thread t adds tiles t, t + 1024 .., then block_sum), the first smallest, and
// that candidate as centre c
__global__ __launch_bounds__(1024) void km_seed_pick_kernel(KmArgs a, int c)
{
    __shared__ double sh[16];
    __shared__ int pick;
    const int r = blockIdx.x;
    double bestv = INFINITY; int best = 0;
    for (int t = 0; t < a.T; ++t) {
        double v = 0.0;
        for (int q = threadIdx.x; q < a.p.scans; q += 1024) v += a.ppart[((size_t)r * a.T + t) * a.p.scans + q];
        v = block_sum<16>(v, sh);
        if (v < bestv) { bestv = v; best = t; }
    }
    if (threadIdx.x == 0) { a.st[r].chosen = best; pick = best; }
    __syncthreads();
    const double* src = a.candC + ((size_t)r * a.T + pick) * a.dim;
    double* dst = a.C + ((size_t)r * a.k + c) * a.dim;
    for (int j = threadIdx.x; j < a.dim; j += 1024) dst[j] = src[j];
}

// closest <- the chosen candidate's distance (first), or the smaller of the two; the scan tile's sum as in km_seed_pot
__global__ __launch_bounds__(256) void km_seed_update_kernel(KmArgs a, int first)
{
    __shared__ double sh[4];
    const int r = blockIdx.y, N = a.N;
    const long long r0 = (long long)blockIdx.x * a.p.scan;
    const int nrow = (int)std::min<long long>(a.p.scan, N - r0);
    const double* d = a.D + ((size_t)r * a.T + a.st[r].chosen) * N;
    double v = 0.0;
    for (int u = 0; u < 4; ++u) {
        const int rl = 4 * threadIdx.x + u;
        if (rl < nrow) {
            const size_t o = (size_t)r * N + r0 + rl;
            const double nv = first ? d[r0 + rl] : fmin(a.closest[o], d[r0 + rl]);
            a.closest[o] = nv; v += nv;
        }
    }
    v = block_sum<4>(v, sh);
    if (threadIdx.x == 0) a.tsum[(size_t)r * a.p.scans + blockIdx.x] = v;
}

// one workgroup of 1024 per restart: the candidates of centre c.  The tiles' sums are scanned (thread t owns tiles 4 t .. 4 t + 3); a
// candidate is the first row whose inclusive cumulative sum -- the tiles before its own, then the rows of its tile in order -- reaches
// u total; it is clipped to the tile's last row, and to N - 1
__global__ __launch_bounds__(1024) void km_seed_search_kernel(KmArgs a, int c)
{
    __shared__ double shv[16];
    __shared__ int shi[16];
    const int r = blockIdx.x, t = threadIdx.x, N = a.N, scans = a.p.scans;
    const double* ts = a.tsum + (size_t)r * scans;
    double tv[4], mine = 0.0;
    for (int u = 0; u < 4; ++u) { const int q = 4 * t + u; tv[u] = q < scans ? ts[q] : 0.0; mine += tv[u]; }
    double total;
    const double before = block_excl_scan<double, 16>(mine, shv, &total);
    if (t == 0) a.st[r].total = total;
    for (int tr = 0; tr < a.T; ++tr) {
        const double thr = (double)uniform01(a.seed, 7, seed_index(r, c, tr)) * total;
        int tile = 0x7fffffff; double run = before, tb = 0.0;
        for (int u = 0; u < 4; ++u) {
            const int q = 4 * t + u;
            if (q < scans && tile == 0x7fffffff && run + tv[u] >= thr) { tile = q; tb = run; }
            run += tv[u];
        }
        const int first = block_min_int(tile, shi, 16);
        const int tl = first == 0x7fffffff ? scans - 1 : first;
        // the sum in front of the tile: its owner's
        if (t == tl / 4) { double rr = before; for (int u = 0; u < (tl & 3); ++u) rr += tv[u]; shv[0] = rr; }
        __syncthreads();
        tb = shv[0];
        __syncthreads();
        const long long r0 = (long long)tl * a.p.scan;
        const int nrow = (int)std::min<long long>(a.p.scan, N - r0);
        const double v = t < nrow ? a.closest[(size_t)r * N + r0 + t] : 0.0;
        double dummy;
        const double ex = block_excl_scan<double, 16>(v, shv, &dummy);
        const int hit = (t < nrow && tb + (ex + v) >= thr) ? t : 0x7fffffff;
        const int rl = block_min_int(hit, shi, 16);
        const int row = (int)std::min<long long>(r0 + (rl == 0x7fffffff ? nrow - 1 : rl), N - 1);
        if (t == 0) a.cand[r * a.T + tr] = row;
        copy_row(a, row, a.candC + ((size_t)r * a.T + tr) * a.dim);
    }
}

}  // namespace

KmPlan km_plan(int N, int k, int R, int chunk_opt)
{
    KmPlan p{};
    p.tile = chunk_opt > 0 ? std::min(chunk_opt, kKmTile) : kKmTile;
    p.tiles = (N + p.tile - 1) / p.tile;
    // centre parts only where the row tiles alone leave the chip idle
    const long long wgs = (long long)p.tiles * R;
    const RowParts cp = row_parts(k, chunk_opt > 0 ? 1 : 64, (int)std::min<long long>(kKmMaxParts, (1024 + wgs - 1) / wgs), kKmMaxParts, chunk_opt);
    p.parts = cp.parts; p.chunk = cp.chunk;
    p.slice = chunk_opt > 0 ? chunk_opt : (N <= (1 << 16) ? 256 : 1024);
    p.slices = (N + p.slice - 1) / p.slice;
    const RowParts bp = row_parts(N, chunk_opt > 0 ? 1 : 256, kKmMaxBlocks, kKmMaxBlocks, chunk_opt);
    p.blk = bp.chunk; p.blks = bp.parts;
    p.scan = chunk_opt > 0 ? std::min(chunk_opt, kKmScanRows) : kKmScanRows;
    if ((N + p.scan - 1) / p.scan > 4096) p.scan = kKmScanRows;
    p.scans = (N + p.scan - 1) / p.scan;
    return p;
}

hipError_t km_prepare(hipStream_t st, const KmArgs& a, double tol)
{
    if (a.rnorm) km_rownorm_kernel<<<(a.N + 3) / 4, 256, 0, st>>>(a.x, a.N, a.dim, const_cast<double*>(a.rnorm));
    if (tol > 0.0) {
        const int blocks = std::min(kKmMaxBlocks, (a.N + 255) / 256), rows = (a.N + blocks - 1) / blocks, nb = (a.N + rows - 1) / rows;
        for (int mode = 0; mode < 2; ++mode) {
            km_colpart_kernel<<<nb, 256, 0, st>>>(a, rows, mode);
            km_colreduce_kernel<<<1, 1024, 0, st>>>(a, nb, mode, tol);
        }
    }
    return hipGetLastError();
}

hipError_t km_load(hipStream_t st, const KmArgs& a, const float* centers_in)
{
    const size_t n = (size_t)a.R * a.k * a.dim;
    km_load_kernel<<<(unsigned)std::min<size_t>(2048, (n + 255) / 256), 256, 0, st>>>(centers_in, a.C, n);
    return hipGetLastError();
}

hipError_t km_seed(hipStream_t st, const KmArgs& a)
{
    const dim3 gd(a.p.tiles, 1, a.R), gs(a.p.scans, a.R);
    km_seed_first_kernel<<<a.R, 256, 0, st>>>(a);
    km_dist_kernel<1, 1><<<gd, 256, 0, st>>>(a, a.candC, 1, (long long)a.T * a.dim, 0);
    km_seed_update_kernel<<<gs, 256, 0, st>>>(a, 1);
    for (int c = 1; c < a.k; ++c) {
        km_seed_search_kernel<<<a.R, 1024, 0, st>>>(a, c);
        km_dist_kernel<1, 1><<<gd, 256, 0, st>>>(a, a.candC, a.T, (long long)a.T * a.dim, 0);
        km_seed_pot_kernel<<<gs, 256, 0, st>>>(a);
        km_seed_pick_kernel<<<a.R, 1024, 0, st>>>(a, c);
        if (c + 1 < a.k) km_seed_update_kernel<<<gs, 256, 0, st>>>(a, 0);
    }
    return hipGetLastError();
}

static void km_assign(hipStream_t st, const KmArgs& a, int last)
{
    km_dist_kernel<4, 0><<<dim3(a.p.tiles, a.p.parts, a.R), 256, 0, st>>>(a, a.C, a.k, (long long)a.k * a.dim, last);
    km_merge_kernel<<<dim3((a.N + 255) / 256, a.R), 256, 0, st>>>(a, last);
}

hipError_t km_iteration(hipStream_t st, const KmArgs& a, int it)
{
    km_assign(st, a, 0);
    km_scan_kernel<<<a.R, 1024, 0, st>>>(a);
    km_place_kernel<<<dim3(a.p.blks, a.R), 256, 0, st>>>(a);
    km_slices_kernel<<<dim3(a.p.slices, a.R), 256, 0, st>>>(a);
    km_centres_kernel<<<dim3(a.k, a.R), 256, 0, st>>>(a);
    km_decide_kernel<<<a.R, 256, 0, st>>>(a, it);
    return hipGetLastError();
}

hipError_t km_finish(hipStream_t st, const KmArgs& a, int32_t* label, float* centers, int32_t* stat, double* inertia, int32_t* label_all,
                     double* centers_all, int32_t* stat_all)
{
    km_assign(st, a, 1);
    km_inertia_kernel<<<dim3(a.p.tiles, a.R), 256, 0, st>>>(a);
    km_best_kernel<<<1, 1024, 0, st>>>(a, stat, inertia, stat_all);
    const size_t most = std::max((size_t)a.R * a.N, (size_t)a.R * a.k * a.dim);
    km_copy_kernel<<<(unsigned)std::min<size_t>(2048, (most + 255) / 256), 256, 0, st>>>(a, label, centers, label_all, centers_all);
    return hipGetLastError();
}

}  // namespace avae
