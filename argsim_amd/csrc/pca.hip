// pca.hip -- principal components of latent rows (contract: include/argsim_vae.h, avae_pca_fit / avae_pca_transform).
// Everything is double arithmetic on fp32 rows; no float atomics; every sum has an order fixed by the plan.
//
//   pca_msum     grid = row chunks.  Thread t owns columns 4 t .. 4 t + 3 and adds its chunk's rows in ascending order.
//   pca_mean     mean[j] = (the chunks' sums in ascending chunk order) / N
//   pca_cov      grid = (tile pairs on or above the diagonal, row chunks).  16 rows of the two 64-column tiles are staged in LDS as
//                centred doubles (x - mean; columns behind dreal are 0), the next stage's loads in flight; 256 threads hold 4 x 4 sums
//                each and add the rows in ascending order.  The partial tile goes to workspace.
//   pca_cmerge   C[i][j] = C[j][i] = (the chunks' partial sums in ascending chunk order) / (N - 1), i <= j
//   pca_init     V = I; thr = 2^-52 ||C||_F / dreal (one workgroup, a fixed tree)
//   the solve    two-sided cyclic Jacobi in round-robin rounds.  A round's rotations are read off the matrix as it stands at the start
//                of the round (pca_rot), and every element of J^T A J and of V J is formed from at most four source elements by
//                pca_elem / pca_vrow -- the SAME two functions in both forms, compiled without contraction, so both give the same bits.
//     resident   (dreal <= 128) one workgroup of 1024 threads keeps A in LDS, forms the next A's triangle from it into a staging matrix (global, L2-resident), copies
//                it back behind a barrier, and rotates the rows of V^T in global memory (a pair's two rows by the same thread): every round and
//                sweep of the solve in ONE launch.  The stop is a count in LDS.
//     launched   one launch per round over 16 x 16 tiles of A and of V^T, out of place into the other buffer of a pair: the launch order
//                is the only barrier.  A one-thread launch per sweep decides the stop; launches behind it return at once.
//   pca_finish   a wave per eigenvector: its place in the descending order (ties: the smaller position first), its sign (the entry of
//                largest magnitude, the first of equals, positive), var clipped at 0, the row of comp; the first wave writes stat.
//   pca_transform  a workgroup owns up to 16 rows and 64 components; 32 columns of the rows (centred) and of the components are staged in
//                LDS as doubles; a thread adds its sums over the columns in ascending order and rounds once.
#include "kernels.h"
#include "reduce_dev.h"

#include <algorithm>

namespace avae {

namespace {

constexpr int T = kPcaT, DK = kPcaDK;

// ---------------------------------------------------------------- mean
__global__ __launch_bounds__(256) void pca_msum_kernel(PcaArgs a, int rows)
{
    const int t = threadIdx.x;
    if (4 * t >= a.dim) return;
    const long long r0 = (long long)blockIdx.x * rows, r1 = min(r0 + rows, (long long)a.N);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (long long r = r0; r < r1; ++r) {
        const float4 v = *reinterpret_cast<const float4*>(a.x + (size_t)r * a.dim + 4 * t);
        s0 += (double)v.x; s1 += (double)v.y; s2 += (double)v.z; s3 += (double)v.w;
    }
    double* o = a.msum + (size_t)blockIdx.x * a.dim + 4 * t;
    o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
}

__global__ __launch_bounds__(256) void pca_mean_kernel(PcaArgs a, int chunks)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.dreal) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += a.msum[(size_t)c * a.dim + j];
    a.mean[j] = s / (double)a.N;
}

// ---------------------------------------------------------------- covariance
// pair q of the upper triangle of tiles x tiles, row by row -> (ta, tb), ta <= tb
__device__ __forceinline__ void tile_pair(int q, int tiles, int& ta, int& tb)
{
    ta = 0;
    while (q >= tiles - ta) { q -= tiles - ta; ++ta; }
    tb = ta + q;
}

__global__ __launch_bounds__(256) void pca_cov_kernel(PcaArgs a, int tiles, int rows)
{
    __shared__ __attribute__((aligned(16))) double xa[DK * T];
    __shared__ __attribute__((aligned(16))) double xb[DK * T];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    int ta, tb;
    tile_pair(blockIdx.x, tiles, ta, tb);
    const long long r0 = (long long)blockIdx.y * rows, r1 = min(r0 + rows, (long long)a.N);
    // what this thread stages: row sr of a stage, columns sc .. sc + 3 of both tiles
    const int sr = tid >> 4, sc = 4 * (tid & 15);
    const int ca = ta * T + sc, cb = tb * T + sc;
    double ma[4], mb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        ma[e] = ca + e < a.dreal ? a.mean[ca + e] : 0.0;
        mb[e] = cb + e < a.dreal ? a.mean[cb + e] : 0.0;
    }
    float4 pa, pb;
    auto fetch = [&](long long r) {
        pa = make_float4(0.f, 0.f, 0.f, 0.f); pb = pa;
        if (r + sr < r1) {
            if (ca < a.dim) pa = *reinterpret_cast<const float4*>(a.x + (size_t)(r + sr) * a.dim + ca);
            if (cb < a.dim) pb = *reinterpret_cast<const float4*>(a.x + (size_t)(r + sr) * a.dim + cb);
        }
    };
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    if (r0 < r1) fetch(r0);
    for (long long r = r0; r < r1; r += DK) {
        __syncthreads();
        const bool live = r + sr < r1;                          // rows behind the chunk and columns behind dreal are staged as 0
        const float fa[4] = {pa.x, pa.y, pa.z, pa.w}, fb[4] = {pb.x, pb.y, pb.z, pb.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xa[sr * T + sc + e] = live && ca + e < a.dreal ? (double)fa[e] - ma[e] : 0.0;
            xb[sr * T + sc + e] = live && cb + e < a.dreal ? (double)fb[e] - mb[e] : 0.0;
        }
        __syncthreads();
        if (r + DK < r1) fetch(r + DK);
#pragma unroll 4
        for (int k = 0; k < DK; ++k) {
            double va[4], vb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { va[i] = xa[k * T + 4 * ty + i]; vb[i] = xb[k * T + 4 * tx + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(va[i], vb[j], acc[i][j]);
        }
    }
    double* o = a.part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (T * T);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[(4 * ty + i) * T + 4 * tx + j] = acc[i][j];
}

__global__ __launch_bounds__(256) void pca_cmerge_kernel(PcaArgs a, int tiles, int chunks)
{
    int ta, tb;
    tile_pair(blockIdx.x, tiles, ta, tb);
    const int e = blockIdx.y * 256 + threadIdx.x;               // element of the 64 x 64 tile
    const int i = ta * T + e / T, j = tb * T + e % T, n = a.dreal;
    if (i >= n || j >= n || i > j) return;
    const size_t stride = (size_t)gridDim.x * (T * T);
    const double* p = a.part + (size_t)blockIdx.x * (T * T) + e;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += p[(size_t)c * stride];
    s /= (double)(a.N - 1);
    a.A[0][(size_t)i * n + j] = s;
    a.A[0][(size_t)j * n + i] = s;
}

// ---------------------------------------------------------------- the solve
// V^T = I (every workgroup its share); workgroup 0: thr from the Frobenius norm, thread t the elements t, t + 256, .. then a fixed tree
__global__ __launch_bounds__(256) void pca_init_kernel(PcaArgs a)
{
    __shared__ double sh[256];
    const int n = a.dreal;
    const size_t nn = (size_t)n * n;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < nn; e += (size_t)gridDim.x * 256)
        a.Vt[0][e] = (e / n == e % n) ? 1.0 : 0.0;
    if (blockIdx.x != 0) return;
    double s = 0.0;
    for (size_t e = threadIdx.x; e < nn; e += 256) { const double v = a.A[0][e]; s += v * v; }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.st->thr = 0x1p-52 * sqrt(sh[0]) / (double)n;
}

// column idx in round r: the other column of its pair (ps; idx itself where there is no rotation), whether the pair rotates, and
// J[idx][idx] = w, J[ps][idx] = u, the change dd of the diagonal entry.  Pairs: with m = n rounded up to even, column m - 1 meets column
// r and every other column j meets (2 r - j) mod (m - 1); a partner >= n is the bye.
struct Rot { double w, u, dd; int ps, rot; };

__device__ __forceinline__ Rot pca_rot(const double* A, int n, int r, int idx, double thr)
{
    Rot o{1.0, 0.0, 0.0, idx, 0};
    if (idx >= n) return o;
    const int m = n + (n & 1);
    int p;
    if (idx == m - 1) p = r;
    else {
        p = (2 * r - idx) % (m - 1);
        if (p < 0) p += m - 1;
        if (p == idx) p = m - 1;
    }
    if (p >= n) return o;
    const int lo = min(idx, p), hi = max(idx, p);
    const double apq = A[(size_t)lo * n + hi];
    if (!(fabs(apq) > thr)) return o;
    const double app = A[(size_t)lo * n + lo], aqq = A[(size_t)hi * n + hi];
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
    const double c = 1.0 / sqrt(1.0 + t * t);
    const double s = t * c;
    o.w = c; o.ps = p; o.rot = 1;
    if (idx == lo) { o.u = -s; o.dd = -(t * apq); }
    else { o.u = s; o.dd = t * apq; }
    return o;
}

// element (lo, hi), lo <= hi, of J^T A J; ra / rb are the rotations of columns lo / hi.  A is symmetric bit for bit and stays so:
// both (i, j) and (j, i) are formed as (min, max)
__device__ __forceinline__ double pca_elem(const double* A, int n, int lo, int hi, const Rot& ra, const Rot& rb)
{
    const double* row = A + (size_t)lo * n;
    if (lo == hi) return ra.rot ? row[lo] + ra.dd : row[lo];
    if (!ra.rot && !rb.rot) return row[hi];
    if (ra.rot && ra.ps == hi) return 0.0;
    const double b0 = rb.rot ? row[hi] * rb.w + row[rb.ps] * rb.u : row[hi];
    if (!ra.rot) return b0;
    const double* prow = A + (size_t)ra.ps * n;
    const double b1 = rb.rot ? prow[hi] * rb.w + prow[rb.ps] * rb.u : prow[hi];
    return ra.w * b0 + ra.u * b1;
}

// element c of row j of (V J)^T
__device__ __forceinline__ double pca_vrow(double v, double vp, const Rot& r) { return r.w * v + r.u * vp; }

// launched form, round r of a sweep: blockIdx.z == 0 a 16 x 16 tile of A, == 1 of V^T
__global__ __launch_bounds__(256) void pca_round_kernel(PcaArgs a, int r, int from)
{
    if (a.st->done) return;
    __shared__ Rot rot[32];
    const int n = a.dreal, tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
    const double* A = a.A[from];
    if (tid < 32) {
        const int idx = tid < 16 ? i0 + tid : j0 + tid - 16;
        const Rot o = pca_rot(A, n, r, idx, a.st->thr);
        rot[tid] = o;
        if (blockIdx.z == 1 && blockIdx.x == 0 && tid < 16 && o.rot && idx < o.ps) atomicAdd(&a.st->rot_sweep, 1);     // each pair once
    }
    __syncthreads();
    const int i = i0 + ty, j = j0 + tx;
    if (i >= n || j >= n) return;
    if (blockIdx.z == 0) {
        const bool up = i <= j;
        a.A[from ^ 1][(size_t)i * n + j] = pca_elem(A, n, up ? i : j, up ? j : i, rot[up ? ty : 16 + tx], rot[up ? 16 + tx : ty]);
    } else {
        const double* V = a.Vt[from];
        const Rot o = rot[ty];
        const double v = V[(size_t)i * n + j];
        a.Vt[from ^ 1][(size_t)i * n + j] = o.rot ? pca_vrow(v, V[(size_t)o.ps * n + j], o) : v;
    }
}

__global__ void pca_sweep_kernel(PcaArgs a, int max_sweeps)
{
    PcaState* st = a.st;
    if (st->done) return;
    st->sweeps += 1;
    st->rotations += st->rot_sweep;
    if (st->rot_sweep == 0) { st->converged = 1; st->done = 1; }
    if (st->sweeps >= max_sweeps) st->done = 1;
    st->rot_sweep = 0;
}

constexpr int kResThreads = 1024;
// resident form: dynamic LDS = A (n n doubles), w, u, dd (n doubles each), ps, rot (n ints each), then (i << 8 | j) of the n (n + 1) / 2
// elements on or above the diagonal.  A round's new elements are formed from A in LDS into the staging matrix a.A[1] (global, 128 KB at
// most: it stays in L2), both sides of the diagonal from one value, and copied back behind a barrier
__global__ __launch_bounds__(kResThreads) void pca_resident_kernel(PcaArgs a, int max_sweeps)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ int cnt;
    const int n = a.dreal, tid = threadIdx.x, nn = n * n, tri = n * (n + 1) / 2;
    double* A = sm;
    double *rw = A + nn, *ru = rw + n, *rd = ru + n;
    int *rp = reinterpret_cast<int*>(rd + n), *rr = rp + n;
    unsigned short* tab = reinterpret_cast<unsigned short*>(rr + n);
    for (int t = tid; t < tri; t += kResThreads) {
        int e = t, i = 0;
        while (e >= n - i) { e -= n - i; ++i; }
        tab[t] = (unsigned short)(i << 8 | (i + e));
    }
    for (int e = tid; e < nn; e += kResThreads) A[e] = a.A[0][e];
    const double thr = a.st->thr;
    const int m = n + (n & 1), R = m - 1;
    double* V = a.Vt[0];
    double* S = a.A[1];
    int sweeps = 0, rotations = 0, converged = 0;
    auto get = [&](int idx) { return Rot{rw[idx], ru[idx], rd[idx], rp[idx], rr[idx]}; };
    while (sweeps < max_sweeps && !converged) {
        if (tid == 0) cnt = 0;
        for (int r = 0; r < R; ++r) {
            __syncthreads();                                    // A of the round before is in place
            if (tid < n) {
                const Rot o = pca_rot(A, n, r, tid, thr);
                rw[tid] = o.w; ru[tid] = o.u; rd[tid] = o.dd; rp[tid] = o.ps; rr[tid] = o.rot;
                if (o.rot && tid < o.ps) atomicAdd(&cnt, 1);
            }
            __syncthreads();
#pragma unroll 3
            for (int t = tid; t < tri; t += kResThreads) {
                const int lo = tab[t] >> 8, hi = tab[t] & 255;
                const double v = pca_elem(A, n, lo, hi, get(lo), get(hi));
                S[lo * n + hi] = v; S[hi * n + lo] = v;
            }
            // the rows of V^T: a pair's two rows, column c, by one thread
            for (int e = tid; e < (m / 2) * n; e += kResThreads) {
                const int k = e / n, c = e % n;
                const int p = k == 0 ? r : (r + k) % (m - 1);
                if (p >= n || !rr[p]) continue;
                const int q = rp[p];
                const double vp = V[(size_t)p * n + c], vq = V[(size_t)q * n + c];
                V[(size_t)p * n + c] = pca_vrow(vp, vq, get(p));
                V[(size_t)q * n + c] = pca_vrow(vq, vp, get(q));
            }
            __syncthreads();                                    // every read of the old A is done, the new one is in S
            for (int e = tid; e < nn; e += kResThreads) A[e] = S[e];
        }
        __syncthreads();
        const int c = cnt;
        __syncthreads();
        ++sweeps; rotations += c; converged = c == 0;
    }
    for (int e = tid; e < nn; e += kResThreads) a.A[0][e] = A[e];
    if (tid == 0) { a.st->sweeps = sweeps; a.st->rotations = rotations; a.st->converged = converged; a.st->done = 1; }
}

// ---------------------------------------------------------------- order, clip, sign, copy-out
__global__ __launch_bounds__(256) void pca_finish_kernel(PcaArgs a, int launched, int R, double* var, double* comp, int32_t* stat)
{
    const int n = a.dreal, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int b = launched ? (int)(((long long)a.st->sweeps * R) & 1) : 0;
    const double* A = a.A[b];
    const double* v = a.Vt[b] + (size_t)i * n;
    const double di = A[(size_t)i * n + i], thr = a.st->thr;
    int before = 0, big = 0;
    for (int j = lane; j < n; j += 64) {
        const double dj = A[(size_t)j * n + j];
        before += dj > di || (dj == di && j < i);
        big += (dj > 0.0 ? dj : 0.0) > thr;
    }
    before = wave_sum(before); big = wave_sum(big);
    double best = -1.0; int at = 0x7fffffff;                    // the entry of largest magnitude, the first of equals
    for (int j = lane; j < n; j += 64) {
        const double m = fabs(v[j]);
        if (m > best) { best = m; at = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(at, o, 64);
        if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
    const double sg = (at < n && v[at] < 0.0) ? -1.0 : 1.0;
    before = min(before, n - 1);
    for (int j = lane; j < n; j += 64) comp[(size_t)before * a.dim + j] = sg * v[j];
    if (lane == 0) var[before] = di > 0.0 ? di : 0.0;
    if (i == 0 && lane == 0) {
        stat[0] = a.st->sweeps; stat[1] = a.st->converged; stat[2] = a.st->rotations & 0x7fffffff; stat[3] = big;
        stat[4] = 0; stat[5] = 0; stat[6] = 0; stat[7] = 0;
    }
}

// ---------------------------------------------------------------- projection
constexpr int TC = 64, TJ = 32;

__global__ __launch_bounds__(256) void pca_transform_kernel(const float* __restrict__ x, int n, int dim, const double* __restrict__ mean,
                                                            const double* __restrict__ comp, const double* __restrict__ scale, int k,
                                                            float* __restrict__ y, int trows)
{
    __shared__ double cs[TC * (TJ + 1)];
    __shared__ double xs[16 * TJ];
    const int tid = threadIdx.x, ry = tid >> 6, c = tid & 63;
    const long long r0 = (long long)blockIdx.x * trows;
    const int nrow = (int)min((long long)trows, n - r0), c0 = blockIdx.y * TC;
    const int rt = trows / 4;                                   // rows of a thread: ry, ry + 4, ..
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < dim; j0 += TJ) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < TC * TJ / 256; ++q) {
            const int idx = tid + 256 * q, cc = idx / TJ, jj = idx % TJ;
            cs[cc * (TJ + 1) + jj] = (c0 + cc < k && j0 + jj < dim) ? comp[(size_t)(c0 + cc) * dim + j0 + jj] : 0.0;
        }
        if (tid < 16 * TJ / 4) {
            const int row = tid / (TJ / 4), j4 = 4 * (tid % (TJ / 4));
            double d[4] = {0.0, 0.0, 0.0, 0.0};
            if (row < nrow && j0 + j4 < dim) {
                const float4 v = *reinterpret_cast<const float4*>(x + (size_t)(r0 + row) * dim + j0 + j4);
                const double* mu = mean + j0 + j4;
                d[0] = (double)v.x - mu[0]; d[1] = (double)v.y - mu[1]; d[2] = (double)v.z - mu[2]; d[3] = (double)v.w - mu[3];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) xs[row * TJ + j4 + e] = d[e];
        }
        __syncthreads();
#pragma unroll 8
        for (int jj = 0; jj < TJ; ++jj) {
            const double cv = cs[c * (TJ + 1) + jj];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < rt) acc[q] = fma(xs[(ry + 4 * q) * TJ + jj], cv, acc[q]);
        }
    }
    if (c0 + c >= k) return;
    const double sc = scale ? scale[c0 + c] : 1.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = ry + 4 * q;
        if (q < rt && row < nrow) y[(size_t)(r0 + row) * k + c0 + c] = (float)(scale ? sc * acc[q] : acc[q]);
    }
}

}  // namespace

size_t pca_resident_lds(int dreal) { return 8 * ((size_t)dreal * dreal + 3 * (size_t)dreal) + 4 * 2 * (size_t)dreal + 2 * ((size_t)dreal * (dreal + 1) / 2); }

// Tiles of 64 columns; the pairs on or above the diagonal.  The rows are cut into chunks so that pairs x chunks gives about four
// workgroups per CU, a chunk a multiple of 16 rows and at least 64; the chunks are capped so that the partial tiles stay within 2^25
// doubles (and 1024 chunks).  chunk_opt > 0 (option pca_chunk, a test aid) caps the rows of a chunk and the rows of a transform tile.
// form: form_opt, or the resident solve wherever dreal allows it.
PcaPlan pca_plan(int N, int dim, int pad, int chunk_opt, int form_opt, int cus)
{
    PcaPlan p{};
    p.dreal = dim - pad;
    p.tiles = (p.dreal + T - 1) / T;
    p.pairs = p.tiles * (p.tiles + 1) / 2;
    const long long want = std::max(1LL, (4LL * std::max(cus, 1) + p.pairs - 1) / p.pairs);
    long long rows = (N + want - 1) / want;
    rows = std::max(64LL, (rows + DK - 1) / DK * DK);
    if (chunk_opt > 0) rows = std::min(rows, (long long)chunk_opt);
    const long long maxchunks = std::min(1024LL, std::max(1LL, (1LL << 25) / ((long long)p.pairs * T * T)));
    rows = std::max(rows, (N + maxchunks - 1) / maxchunks);
    p.rows = (int)rows;
    p.chunks = (int)((N + rows - 1) / rows);
    p.form = form_opt ? form_opt : (p.dreal <= kPcaResident ? 1 : 2);
    p.rounds = p.dreal + (p.dreal & 1) - 1;
    p.sweeps = kPcaSweeps;
    p.lds = p.form == 1 ? (int)pca_resident_lds(p.dreal) : (int)(32 * sizeof(Rot));
    p.trows = 16;
    if (chunk_opt > 0) p.trows = chunk_opt >= 16 ? 16 : chunk_opt >= 8 ? 8 : 4;
    // mean 2, covariance 2, init 1, finish 1, and the solve
    p.launches = 6 + (p.form == 1 ? 1 : p.sweeps * (p.rounds + 1));
    return p;
}

hipError_t pca_cov(hipStream_t st, const PcaArgs& a, const PcaPlan& p)
{
    pca_msum_kernel<<<p.chunks, 256, 0, st>>>(a, p.rows);
    pca_mean_kernel<<<(a.dreal + 255) / 256, 256, 0, st>>>(a, p.chunks);
    pca_cov_kernel<<<dim3(p.pairs, p.chunks), 256, 0, st>>>(a, p.tiles, p.rows);
    pca_cmerge_kernel<<<dim3(p.pairs, T * T / 256), 256, 0, st>>>(a, p.tiles, p.chunks);
    return hipGetLastError();
}

hipError_t pca_solve(hipStream_t st, const PcaArgs& a, const PcaPlan& p, int max_sweeps)
{
    const int n = a.dreal;
    pca_init_kernel<<<std::min(1024, (n * n + 255) / 256), 256, 0, st>>>(a);
    if (p.form == 1) {
        const size_t lds = pca_resident_lds(n);
        if (lds > 48 * 1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pca_resident_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(pca_resident_kernel, dim3(1), dim3(kResThreads), lds, st, a, max_sweeps);
        return hipGetLastError();
    }
    // every round of every sweep is enqueued; a launch behind the stop returns at once.  Never a synchronisation
    const int nt = (n + 15) / 16;
    int from = 0;
    for (int s = 0; s < max_sweeps; ++s) {
        for (int r = 0; r < p.rounds; ++r, from ^= 1) pca_round_kernel<<<dim3(nt, nt, 2), 256, 0, st>>>(a, r, from);
        pca_sweep_kernel<<<1, 1, 0, st>>>(a, max_sweeps);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t pca_finish(hipStream_t st, const PcaArgs& a, const PcaPlan& p, double* var, double* comp, int32_t* stat)
{
    pca_finish_kernel<<<(a.dreal + 3) / 4, 256, 0, st>>>(a, p.form == 2, p.rounds, var, comp, stat);
    return hipGetLastError();
}

hipError_t pca_transform(hipStream_t st, const float* x, int n, int dim, const double* mean, const double* comp, const double* scale, int k,
                         float* y, int trows)
{
    const dim3 grid((unsigned)(((long long)n + trows - 1) / trows), (k + TC - 1) / TC);
    pca_transform_kernel<<<grid, 256, 0, st>>>(x, n, dim, mean, comp, scale, k, y, trows);
    return hipGetLastError();
}

}  // namespace avae
