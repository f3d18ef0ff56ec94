// score.hip -- the kernels of the importance-weighted sentence likelihood (include/argsim_vae.h, avae_score / avae_score_z):
// the K latent draws of every row with their latent term, the replication of the target ids over the draws, the per-row
// sums of the compacted per-token cross-entropy and the log-mean-exp over the draws.  Every reduction runs in a fixed
// order (a thread's own terms in index order, a wave's by shuffles, a workgroup's through LDS): no float atomics, the
// same inputs give the same bits.
#include <algorithm>
#include "kernels.h"
#include "reduce_dev.h"
#include "sample_dev.h"

namespace avae {

constexpr uint64_t kScoreStream = 4;      // of the counter generator (sample_dev.h: normal01)

// ---------------------------------------------------------------- draw
// One workgroup per (k, r): z = mu[r] + exp(lv[r] / 2) eps[k, r] into the row the pair has in the decoder batches
// (ScoreDraw::rc: rows r are cut into blocks of rc, a block's k draws lie behind each other, draw-major), eps echoed,
// lat[k, r] = 1/2 sum_j (z^2 - eps^2 - lv).
__global__ __launch_bounds__(256) void score_draw_kernel(ScoreDraw a)
{
    __shared__ float sh[4];
    const int r = blockIdx.x % a.B, kk = blockIdx.x / a.B, tid = threadIdx.x;
    const int r0 = r / a.rc * a.rc, rcb = min(a.rc, a.B - r0);
    const size_t zrow = (size_t)r0 * a.k + (size_t)kk * rcb + (r - r0), nat = (size_t)kk * a.B + r;
    const uint64_t base = (((uint64_t)(unsigned)r << 20) + (uint64_t)(unsigned)kk) << 20;
    float part = 0.f; int bad = 0;
    for (int j = tid; j < a.R; j += 256) {
        const float mu = a.mu[(size_t)r * a.R + j], lv = a.lv[(size_t)r * a.R + j];
        const float e = a.eps_in ? a.eps_in[nat * a.R + j] : normal01(a.seed, kScoreStream, base + (uint64_t)j);
        bad |= !isfinite(e);
        const float z = mu + expf(0.5f * lv) * e;
        a.z[zrow * a.R + j] = z;
        if (a.eps_out) a.eps_out[nat * a.R + j] = e;
        part += z * z - e * e - lv;
    }
    if (bad) *a.err = 1;
    part = wave_sum(part);
    if ((tid & 63) == 0) sh[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) a.lat[nat] = 0.5f * (((sh[0] + sh[1]) + sh[2]) + sh[3]);
}
hipError_t score_draw(hipStream_t st, const ScoreDraw& a)
{
    hipLaunchKernelGGL(score_draw_kernel, dim3((unsigned)a.k * a.B), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------- target replication
// dst (n, S) row j = src row (j % rc): the ids of a block of rc rows under each of its draws
__global__ __launch_bounds__(256) void tile_ids_kernel(int32_t* __restrict__ dst, const int32_t* __restrict__ src, int n, int rc, int S)
{
    const size_t total = (size_t)n * S;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int j = (int)(i / S), s = (int)(i - (size_t)j * S);
        dst[i] = src[(size_t)(j % rc) * S + s];
    }
}
hipError_t tile_ids(hipStream_t st, int32_t* dst, const int32_t* src, int n, int rc, int S)
{
    const size_t total = (size_t)n * S;
    hipLaunchKernelGGL(tile_ids_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 1024)), dim3(256), 0, st, dst, src, n, rc, S);
    return hipGetLastError();
}
// the shared first-layer projection of a decoder batch of n = kc x rc rows: ids0 (T, rc) = the lead ids of the block's rows
// (the first rc rows of every step), tokrow (T, n) = the row of (t, j) in the projection over ids0
__global__ __launch_bounds__(256) void lead_rows_kernel(const int32_t* __restrict__ lead, int T, int n, int rc, int32_t* __restrict__ ids0, int32_t* __restrict__ tokrow)
{
    const int total = T * n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int t = i / n, j = i - t * n, rr = j % rc;
        tokrow[i] = t * rc + rr;
        if (j < rc) ids0[t * rc + j] = lead[i];
    }
}
hipError_t lead_rows(hipStream_t st, const int32_t* lead, int T, int n, int rc, int32_t* ids0, int32_t* tokrow)
{
    hipLaunchKernelGGL(lead_rows_kernel, dim3(std::min((T * n + 255) / 256, 1024)), dim3(256), 0, st, lead, T, n, rc, ids0, tokrow);
    return hipGetLastError();
}

// ---------------------------------------------------------------- per-row sums of the compacted cross-entropy
// One wave per row j of a decoder batch of n rows: rank[t * n + j] is the compact row of position (t, j) in the per-token
// array (time-major tf.boolean_mask order, prep_ids) or -1; lane l takes t = l, l + 64, .. in order.
__global__ __launch_bounds__(256) void score_rows_kernel(ScoreRows a)
{
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= a.n) return;
    float s = 0.f; int cnt = 0;
    for (int t = lane; t < a.T; t += 64) {
        const int c = a.rank[(size_t)t * a.n + j];
        if (c >= 0) { s += a.loss[c]; ++cnt; }
    }
    s = wave_sum(s);
    cnt = wave_sum(cnt);
    if (lane == 0) {
        const int kk = a.k0 + j / a.rc, r = a.r0 + j % a.rc;
        a.logpx[(size_t)kk * a.B + r] = -s;
        if (kk == 0 && a.ntok) a.ntok[r] = cnt;
    }
}
hipError_t score_rows(hipStream_t st, const ScoreRows& a)
{
    hipLaunchKernelGGL(score_rows_kernel, dim3((a.n + 3) / 4), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------- log-mean-exp over the draws
// One wave per row r: logw[k, r] = logpx[k, r] - lat[k, r]; bound[r] = max_k logw + log sum_k exp(logw - max) - log k
// (logw is around -600 at the production geometry: its exponential is 0 in fp32, the differences to the maximum are not).
__global__ __launch_bounds__(256) void score_bound_kernel(const float* __restrict__ logpx, const float* __restrict__ lat, int k, int B,
                                                          float* __restrict__ logw, float* __restrict__ bound)
{
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= B) return;
    float m = -INFINITY;
    for (int kk = lane; kk < k; kk += 64) {
        const size_t i = (size_t)kk * B + r;
        const float w = logpx[i] - lat[i];
        if (logw) logw[i] = w;
        m = fmaxf(m, w);
    }
    m = wave_max(m);
    float s = 0.f;
    for (int kk = lane; kk < k; kk += 64) {
        const size_t i = (size_t)kk * B + r;
        const float w = logpx[i] - lat[i];
        s += w == m ? 1.f : expf(w - m);
    }
    s = wave_sum(s);
    if (lane == 0) bound[r] = m + logf(s) - logf((float)k);
}
hipError_t score_bound(hipStream_t st, const float* logpx, const float* lat, int k, int B, float* logw, float* bound)
{
    hipLaunchKernelGGL(score_bound_kernel, dim3((B + 3) / 4), dim3(256), 0, st, logpx, lat, k, B, logw, bound);
    return hipGetLastError();
}

}  // namespace avae
