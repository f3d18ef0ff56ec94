// ward.hip -- Ward agglomerative clustering of latent rows, G independent groups per call (contract: include/argsim_vae.h, avae_ward /
// avae_ward_cut; host loop: clustering.cpp).
//
// Per group (WardGroup, workspace): D (n, n) fp32 of which the entries [i][j], i < j, hold the stored pair values; S (n, dim) double
// sums of member rows; cnt (n) member counts, 0 = retired; nn (n) the nearest-neighbour cache of slot i over alive j > i as ONE
// 64-bit word  key(value) << 32 | i << 16 | j  (kNone: no alive j > i), so that the smallest word is the smallest value, then the
// lowest i, then the lowest j; st (4) the last merge (a, b), which the launch-per-merge form hands from launch to launch.
//
//   pair value   ONE wave per pair, whatever the kernel: lane l owns dims 256 c + 4 l .. + 3 of chunk c (c < 4), forms the centroids
//                sum / count in double, chains fma(d, d, acc) over its <= 16 differences in that order, and the 64 chains meet in a
//                fixed xor butterfly (32, 16, .. 1).  Times |A||B| / (|A| + |B|) in double, ONE rounding to fp32.  (ward_value)
//   init         ward_init_kernel copies the rows into S; ward_pairs_kernel: one wave per row strip i, the row held in registers,
//                all j > i read as float4 straight from x (a count of 1 divides nothing: the same bits as from S), nn[i] on the way.
//   one merge    ward_pick: the row of the previous merge's slot a is rescanned and the argmin over the caches taken in the same
//                workgroup reduction; ward_apply records the merge, adds sums and counts, retires b.  ward_update_rows / ward_update_row (one wave per
//                alive k): Delta(a, k) from the sums -> D; rows k < a fold the new value into their cache, a row whose cached
//                neighbour was a or b is rescanned in full; nothing relies on reducibility.
//   forms        ward_tree_kernel: one workgroup per group runs every merge of the group in one launch (workgroup barriers only).
//                ward_pick_kernel + ward_update_kernel: two launches per merge, grid = (groups, row tiles); a finished group returns
//                at once.  Both call the SAME device functions; the argmin is an exact integer minimum, so neither the workgroup
//                size nor the tile changes a bit.
// No kernel waits on another workgroup; every loop is bounded by n_g (or dim) at launch.  No float atomics.
#include "kernels.h"

#include <algorithm>

namespace avae {

namespace {

typedef unsigned long long u64;
constexpr u64 kNone = ~0ull;
constexpr int kUpdRows = 16;         // rows k per workgroup of ward_update_kernel (4 waves)

// order key of a stored value: ascending with the value, a NaN above everything (+inf included)
__device__ inline unsigned ward_key(float v)
{
    if (v != v) return 0xffffffffu;
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float ward_unkey(unsigned k)
{
    if (k == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return (k & 0x80000000u) ? __uint_as_float(k & 0x7fffffffu) : __uint_as_float(~k);
}
__device__ inline u64 ward_word(float v, int i, int j) { return ((u64)ward_key(v) << 32) | ((u64)(unsigned)i << 16) | (u64)(unsigned)j; }
__device__ inline u64 umin64(u64 a, u64 b) { return a < b ? a : b; }
__device__ inline u64 wave_min(u64 v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = umin64(v, __shfl_xor(v, m, 64));
    return v;
}

// the lane's share of a cluster's centroid: sum / count in double (a count of 1 divides nothing); 0 beyond dim
template <class T>
__device__ inline void ward_centroid(const T* row, int cnt, int dim, int lane, double (&c)[16])
{
    const double den = (double)cnt;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        const int d = ch * 256 + lane * 4;
        double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
        if (d < dim) {
            if constexpr (sizeof(T) == 4) {
                const float4 q = *reinterpret_cast<const float4*>(row + d);
                v0 = q.x; v1 = q.y; v2 = q.z; v3 = q.w;
            } else {
                const double2 p = *reinterpret_cast<const double2*>(row + d), q = *reinterpret_cast<const double2*>(row + d + 2);
                v0 = p.x; v1 = p.y; v2 = q.x; v3 = q.y;
            }
            if (cnt != 1) { v0 /= den; v1 /= den; v2 /= den; v3 /= den; }
        }
        c[ch * 4] = v0; c[ch * 4 + 1] = v1; c[ch * 4 + 2] = v2; c[ch * 4 + 3] = v3;
    }
}

// Delta(A, B) = |A||B| / (|A| + |B|) |c_A - c_B|^2 by one wave, every lane returns it.  The chunks beyond dim add exact zeros.
__device__ inline float ward_value(const double (&ca)[16], int na, const double (&cb)[16], int nb, int dim)
{
    double acc = 0.0;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        if (ch * 256 < dim) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const double d = ca[ch * 4 + e] - cb[ch * 4 + e]; acc = fma(d, d, acc); }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    const double f = (double)na * (double)nb / ((double)na + (double)nb);
    return (float)(f * acc);
}

// a wave's scan of row i: the nearest alive j > i (lowest j on ties), or kNone.  skip: a column whose stored value the caller holds
// in a register (it is being rewritten by this very wave) and folds in itself.
__device__ inline u64 ward_row_scan(const WardGroup& g, int i, int skip, int lane)
{
    u64 best = kNone;
    const float* row = g.D + (size_t)i * g.n;
    for (int j = i + 1 + lane; j < g.n; j += 64)
        if (j != skip && g.cnt[j] > 0) best = umin64(best, ward_word(row[j], i, j));
    return wave_min(best);
}

// (pick) by the whole workgroup: rescans the row of `prev`, the slot the previous merge went into (-1: none), and returns the smallest
// cache word over the alive slots.  s_red: 64 words of LDS.
__device__ inline u64 ward_pick(const WardGroup& g, int prev, u64* s_red)
{
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    u64 ra = kNone, best = kNone;
    if (prev >= 0) {
        const float* row = g.D + (size_t)prev * g.n;
        for (int j = prev + 1 + tid; j < g.n; j += nt)
            if (g.cnt[j] > 0) ra = umin64(ra, ward_word(row[j], prev, j));
    }
    for (int i = tid; i < g.n; i += nt)
        if (i != prev && g.cnt[i] > 0) best = umin64(best, g.nn[i]);
    ra = wave_min(ra); best = wave_min(best);
    if (lane == 0) { s_red[wave] = ra; s_red[32 + wave] = best; }
    __syncthreads();
    ra = kNone; best = kNone;
    for (int w = 0; w < nw; ++w) { ra = umin64(ra, s_red[w]); best = umin64(best, s_red[32 + w]); }
    if (tid == 0 && prev >= 0) g.nn[prev] = ra;
    __syncthreads();
    return umin64(best, ra);
}

// records merge t = (a, b) of the group, adds b's sums and count to a's and retires b (whole workgroup)
__device__ inline void ward_apply(const WardGroup& g, int dim, int t, int a, int b, float val, int32_t* pair, float* delta, int32_t* size)
{
    const int na = g.cnt[a], nb = g.cnt[b];
    double* sa = g.S + (size_t)a * dim;
    const double* sb = g.S + (size_t)b * dim;
    for (int d = threadIdx.x; d < dim; d += blockDim.x) sa[d] += sb[d];
    __syncthreads();                                  // every thread has read the two counts
    if (threadIdx.x == 0) {
        const size_t m = (size_t)g.mrg + t;
        pair[2 * m] = a; pair[2 * m + 1] = b; delta[m] = val;
        if (size) size[m] = na + nb;
        g.cnt[a] = na + nb; g.cnt[b] = 0;
        g.st[0] = a; g.st[1] = b;
    }
    __syncthreads();
}

// (update) by one wave, for the alive slot k != a after the merge (a, b) whose new centroid the wave holds in ca; nk = cnt[k], cur = nn[k]
__device__ inline void ward_update_row(const WardGroup& g, int dim, int a, int b, int k, int nk, u64 cur, const double (&ca)[16], int na, int lane)
{
    double ck[16];
    ward_centroid(g.S + (size_t)k * dim, nk, dim, lane, ck);
    const float v = ward_value(ca, na, ck, nk, dim);
    if (lane == 0) g.D[k < a ? (size_t)k * g.n + a : (size_t)a * g.n + k] = v;
    if (k > b) return;                                // rows behind b hold neither a nor b
    const int cj = (int)(cur & 0xffffu);
    u64 nw;
    if (k < a) {
        const u64 mine = ward_word(v, k, a);
        nw = (cur != kNone && (cj == a || cj == b)) ? umin64(ward_row_scan(g, k, a, lane), mine) : umin64(cur, mine);
    } else {                                          // a < k < b: the row holds b only
        if (cur == kNone || cj != b) return;
        nw = ward_row_scan(g, k, -1, lane);
    }
    if (lane == 0 && nw != cur) g.nn[k] = nw;
}

// a wave's share of the update: the slots first, first + step, .. below limit.  64 of them at a time: every lane fetches one slot's
// count and cache word, and the wave then walks the alive ones only (retired slots cost no round trip of their own).  Nothing else
// writes cnt in this phase, and nn[k] is written by the wave that owns k alone.
__device__ inline void ward_update_rows(const WardGroup& g, int dim, int a, int b, int first, int step, int limit, const double (&ca)[16], int na, int lane)
{
    for (int k0 = first; k0 < limit; k0 += 64 * step) {
        const int kl = k0 + lane * step;
        const bool in = kl < limit;
        const int cl = in ? g.cnt[kl] : 0;
        const u64 wl = in ? g.nn[kl] : kNone;
        u64 todo = __ballot(cl > 0 && kl != a);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            ward_update_row(g, dim, a, b, k0 + l * step, __shfl(cl, l, 64), __shfl(wl, l, 64), ca, na, lane);
        }
    }
}

// a cache word that names no pair of the group cannot come out of a correct cache; it is refused rather than followed
__device__ inline bool ward_unpack(u64 w, int n, int* a, int* b)
{
    *a = (int)((w >> 16) & 0xffffu); *b = (int)(w & 0xffffu);
    return w != kNone && *a < *b && *b < n;
}

// grid = (groups, strips)
__global__ __launch_bounds__(256) void ward_init_kernel(const WardGroup* gs, const float* x, int dim)
{
    const WardGroup g = gs[blockIdx.x];
    const size_t total = (size_t)g.n * dim, step = (size_t)gridDim.y * 256, first = (size_t)blockIdx.y * 256 + threadIdx.x;
    const float* src = x + (size_t)g.off * dim;
    for (size_t e = first; e < total; e += step) g.S[e] = (double)src[e];
    for (size_t i = first; i < (size_t)g.n; i += step) { g.cnt[i] = 1; g.nn[i] = kNone; }
    if (blockIdx.y == 0 && threadIdx.x < 4) g.st[threadIdx.x] = -1;
}

// grid = (groups, strips): wave w of a group's strips takes the rows w, w + waves, ..
__global__ __launch_bounds__(256) void ward_pairs_kernel(const WardGroup* gs, const float* x, int dim)
{
    const WardGroup g = gs[blockIdx.x];
    const int lane = threadIdx.x & 63, stride = gridDim.y * 4;
    const float* src = x + (size_t)g.off * dim;
    for (int i = blockIdx.y * 4 + (threadIdx.x >> 6); i < g.n - 1; i += stride) {
        double ci[16], cj[16];
        ward_centroid(src + (size_t)i * dim, 1, dim, lane, ci);
        float* row = g.D + (size_t)i * g.n;
        u64 best = kNone;
        float keep = 0.f;
        for (int j = i + 1; j < g.n; ++j) {
            ward_centroid(src + (size_t)j * dim, 1, dim, lane, cj);
            const float v = ward_value(ci, 1, cj, 1, dim);
            best = umin64(best, ward_word(v, i, j));
            const int q = (j - i - 1) & 63;           // 64 values of the strip leave in one store
            if (lane == q) keep = v;
            if (q == 63 || j == g.n - 1) { if (lane <= q) row[j - q + lane] = keep; }
        }
        if (lane == 0) g.nn[i] = best;
    }
}

// one-workgroup form: every merge of group blockIdx.x in this launch
__global__ __launch_bounds__(1024) void ward_tree_kernel(const WardGroup* gs, int dim, int32_t* pair, float* delta, int32_t* size)
{
    __shared__ u64 s_red[64];
    const WardGroup g = gs[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int prev = -1;
    for (int t = 0; t < g.n - 1; ++t) {
        const u64 best = ward_pick(g, prev, s_red);
        int a, b;
        if (!ward_unpack(best, g.n, &a, &b)) return;
        ward_apply(g, dim, t, a, b, ward_unkey((unsigned)(best >> 32)), pair, delta, size);
        const int na = g.cnt[a];
        double ca[16];
        ward_centroid(g.S + (size_t)a * dim, na, dim, lane, ca);
        ward_update_rows(g, dim, a, b, wave, nw, g.n, ca, na, lane);
        __syncthreads();
        prev = a;
    }
}

// launch-per-merge form, first launch of round t: grid = groups
__global__ __launch_bounds__(1024) void ward_pick_kernel(const WardGroup* gs, int dim, int t, int32_t* pair, float* delta, int32_t* size)
{
    __shared__ u64 s_red[64];
    const WardGroup g = gs[blockIdx.x];
    if (t >= g.n - 1) return;
    const int prev = g.st[0];
    const u64 best = ward_pick(g, prev, s_red);       // (its barriers stand between the read of st[0] and ward_apply's write)
    int a, b;
    if (!ward_unpack(best, g.n, &a, &b)) { if (threadIdx.x == 0) { g.st[0] = -1; g.st[1] = -1; } return; }
    ward_apply(g, dim, t, a, b, ward_unkey((unsigned)(best >> 32)), pair, delta, size);
}

// second launch of round t: grid = (groups, tiles of kUpdRows rows)
__global__ __launch_bounds__(256) void ward_update_kernel(const WardGroup* gs, int dim, int t)
{
    const WardGroup g = gs[blockIdx.x];
    const int k0 = blockIdx.y * kUpdRows;
    if (t >= g.n - 1 || k0 >= g.n) return;
    const int a = g.st[0], b = g.st[1], lane = threadIdx.x & 63;
    if (a < 0 || b <= a || b >= g.n) return;
    const int na = g.cnt[a], k1 = k0 + kUpdRows < g.n ? k0 + kUpdRows : g.n;
    double ca[16];
    ward_centroid(g.S + (size_t)a * dim, na, dim, lane, ca);
    ward_update_rows(g, dim, a, b, k0 + (threadIdx.x >> 6), 4, k1, ca, na, lane);
}

// ---- cut: grid = (groups, tiles of 256 rows)
__global__ __launch_bounds__(256) void ward_cut_kernel(const WardCutGroup* gs, const int32_t* pair, int32_t* p, int32_t* label, int phase)
{
    const WardCutGroup g = gs[blockIdx.x];
    const int i = blockIdx.y * 256 + threadIdx.x;
    if (phase == 0) {                                 // every slot its own parent
        if (i < g.n) p[(size_t)g.off + i] = i;
    } else if (phase == 1) {                          // the first m merges: p[b] = a (every b is retired once: no two writers)
        if (i < g.m) {
            const int a = pair[2 * ((size_t)g.mrg + i)], b = pair[2 * ((size_t)g.mrg + i) + 1];
            if (a >= 0 && a < b && b < g.n) p[(size_t)g.off + b] = a;
        }
    } else if (i < g.n) {                             // slots only decrease: at most n steps
        int r = i;
        for (int s = 0; s < g.n; ++s) {
            const int q = p[(size_t)g.off + r];
            if (q == r) break;
            r = q;
        }
        label[(size_t)g.off + i] = r;
    }
}

// pick and the one-workgroup form: 16 waves whatever the group (the update walks one slot per wave at a time)
inline int ward_threads(int) { return 1024; }

}  // namespace

hipError_t ward_init(hipStream_t st, const WardGroup* gs, int G, int nmax, const float* x, int dim)
{
    const size_t cells = (size_t)nmax * dim;
    const int strips = (int)std::min<size_t>(1024, (cells + 255) / 256);
    hipLaunchKernelGGL(ward_init_kernel, dim3(G, strips), dim3(256), 0, st, gs, x, dim);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ward_pairs_kernel, dim3(G, std::min(1024, (nmax + 3) / 4)), dim3(256), 0, st, gs, x, dim);
    return hipGetLastError();
}

hipError_t ward_tree(hipStream_t st, const WardGroup* gs, int G, int nmax, int dim, int32_t* pair, float* delta, int32_t* size)
{
    hipLaunchKernelGGL(ward_tree_kernel, dim3(G), dim3(ward_threads(nmax)), 0, st, gs, dim, pair, delta, size);
    return hipGetLastError();
}

hipError_t ward_round(hipStream_t st, const WardGroup* gs, int G, int nmax, int dim, int t, int32_t* pair, float* delta, int32_t* size)
{
    hipLaunchKernelGGL(ward_pick_kernel, dim3(G), dim3(ward_threads(nmax)), 0, st, gs, dim, t, pair, delta, size);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ward_update_kernel, dim3(G, (nmax + kUpdRows - 1) / kUpdRows), dim3(256), 0, st, gs, dim, t);
    return hipGetLastError();
}

hipError_t ward_cut(hipStream_t st, const WardCutGroup* gs, int G, int nmax, const int32_t* pair, int32_t* p, int32_t* label)
{
    for (int phase = 0; phase < 3; ++phase) {
        hipLaunchKernelGGL(ward_cut_kernel, dim3(G, (nmax + 255) / 256), dim3(256), 0, st, gs, pair, p, label, phase);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace avae
