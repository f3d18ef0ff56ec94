// beam.hip -- beam-search decoding on the launch-per-token path (contract: include/argsim_vae.h, avae_decode_beam).
//
// The n sentences of a group carry `width` hypotheses each; hypothesis (r, w) is decoder batch row r * width + w.  Per token:
//   beam_rows    one workgroup per ROW: the row's log-sum-exp, then the `width` best of its V candidates cum + logp under
//                (score descending, token ascending) -- a radix select of the width-th largest score key (sample_dev.h, the
//                sampler's top-k) and, where more keys tie at that threshold than are needed, a second select over the tied
//                TOKENS.  No row can place more than `width` candidates in its sentence's next beam, so the sentence-level
//                selection only ever sees width x width candidates; the V-wide work is spread over one workgroup per row.
//                A finished row offers itself: (cum, eos).
//   beam_select  one workgroup per SENTENCE: merges the sorted lists of its rows under (score descending, parent slot
//                ascending, token ascending), writes the lattice entry of the step, the new cum / finished / length of
//                every slot and adds the slots still alive to the step's counter.
//   beam_gather  the GRU state of every new slot from its parent's row, straight out of the per-layer outputs of the
//                decoder into the other ping-pong buffer (the copy a greedy step makes, with an index).
// After the loop beam_backtrack ranks a sentence's final slots by cum / len^alpha and walks the lattice back per slot.
// Reductions run in a fixed order (a thread's terms in index order, a wave by shuffles, the workgroup through LDS); the
// only atomics are integer ones (LDS histograms, list slots, the live-slot counter): the same arguments give the same bits.
#include "kernels.h"
#include "reduce_dev.h"
#include "sample_dev.h"

#include <algorithm>

namespace avae {

namespace {

constexpr int kBeamMax = 32;

// candidate order inside one row: larger key, then smaller token
__device__ __forceinline__ bool row_better(unsigned ka, int ta, unsigned kb, int tb) { return ka > kb || (ka == kb && ta < tb); }

__global__ __launch_bounds__(256) void beam_rows_kernel(const float* __restrict__ logits, int V, int W, const float* __restrict__ cum_in,
                                                        const int32_t* __restrict__ fin_in, int eos,
                                                        float* __restrict__ cand_sc, int32_t* __restrict__ cand_tok, int32_t* __restrict__ cand_cnt)
{
    __shared__ unsigned s_sel[258];
    __shared__ float s_m[4], s_s[4];
    __shared__ unsigned s_key[kBeamMax]; __shared__ int s_tok[kBeamMax]; __shared__ float s_sc[kBeamMax];
    __shared__ int s_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.x;
    const float cum = cum_in ? cum_in[row] : 0.f;
    if (fin_in && fin_in[row]) {                                   // (uniform over the workgroup)
        if (tid == 0) { cand_cnt[row] = 1; cand_sc[(size_t)row * W] = cum; cand_tok[(size_t)row * W] = eos; }
        return;
    }
    const float* x = logits + (size_t)row * V;
    float m = -INFINITY, s = 0.f;
    for (int c = tid; c < V; c += 256) { const float l = x[c]; if (l == l) lse_add(m, s, l); }
    lse_wave_merge(m, s);
    if (tid == 0) s_n = 0;
    if (lane == 0) { s_m[wave] = m; s_s[wave] = s; }
    __syncthreads();
    m = s_m[0]; s = s_s[0];
    for (int w = 1; w < 4; ++w) lse_merge(m, s, s_m[w], s_s[w]);  // every thread in the same order: the same bits
    const float ls = logf(s);
    const bool by_logit = W == 1;                                  // width 1: the first maximum of l itself, as the greedy loop takes it
    auto score = [&](float l) { return cum + ((l == m ? 0.f : l - m) - ls); };
    auto key_of = [&](float l) { return order_key(by_logit ? l : score(l)); };
    unsigned need, ties;                                           // keys equal to thr among the W largest, and how many there are
    const unsigned thr = kth_largest_key([&](auto f) { for (int c = tid; c < V; c += 256) f(key_of(x[c])); }, (unsigned)W, s_sel, &need, &ties);
    int tok_max = 0x7fffffff;                                      // ties at the threshold: the `need` smallest tokens
    if (ties > need)
        tok_max = (int)~kth_largest_key([&](auto f) { for (int c = tid; c < V; c += 256) if (key_of(x[c]) == thr) f(~(unsigned)c); }, need, s_sel);
    for (int c = tid; c < V; c += 256) {
        const float l = x[c];
        const unsigned k = key_of(l);
        if (k > thr || (k == thr && c <= tok_max)) {
            const int slot = atomicAdd(&s_n, 1);
            if (slot < kBeamMax) { s_key[slot] = k; s_tok[slot] = c; s_sc[slot] = score(l); }
        }
    }
    __syncthreads();
    const int n = min(s_n, W);                                     // (= W: V >= W keys, exactly W pass the two thresholds)
    if (tid < n) {
        int rank = 0;
        for (int i = 0; i < n; ++i) rank += row_better(s_key[i], s_tok[i], s_key[tid], s_tok[tid]) ? 1 : 0;
        cand_sc[(size_t)row * W + rank] = s_sc[tid]; cand_tok[(size_t)row * W + rank] = s_tok[tid];
    }
    if (tid == 0) cand_cnt[row] = n;
}

__global__ __launch_bounds__(256) void beam_select_kernel(int Win, int W, const float* __restrict__ cand_sc, const int32_t* __restrict__ cand_tok,
                                                          const int32_t* __restrict__ cand_cnt, const int32_t* __restrict__ fin_in,
                                                          const int32_t* __restrict__ len_in, int eos,
                                                          int32_t* __restrict__ lat_parent, int32_t* __restrict__ lat_token, float* __restrict__ lat_cum,
                                                          float* __restrict__ cum_out, int32_t* __restrict__ fin_out, int32_t* __restrict__ len_out,
                                                          int32_t* __restrict__ live)
{
    __shared__ unsigned s_key[kBeamMax * kBeamMax];
    __shared__ int s_cnt[kBeamMax];
    const int tid = threadIdx.x, r = blockIdx.x, total = Win * W;
    const size_t in0 = (size_t)r * Win, out0 = (size_t)r * W;
    if (tid < Win) s_cnt[tid] = cand_cnt[in0 + tid];
    for (int i = tid; i < total; i += 256) s_key[i] = order_key(cand_sc[in0 * W + i]);
    __syncthreads();
    int alive = 0;
    for (int idx = tid; idx < total; idx += 256) {
        const int p = idx / W, i = idx - p * W;
        if (i >= s_cnt[p]) continue;
        const unsigned k = s_key[idx];
        int rank = i;                                              // the row's list is sorted: i of its own are better
        for (int q = 0; q < Win && rank < W; ++q) {
            if (q == p) continue;
            const int nq = s_cnt[q];
            for (int j = 0; j < nq && rank < W; ++j) {             // equal scores: the lower parent slot first, whatever the token
                const unsigned kq = s_key[q * W + j];
                if (kq > k || (kq == k && q < p)) ++rank; else break;
            }
        }
        if (rank >= W) continue;
        const int tok = cand_tok[in0 * W + idx];
        const int pf = fin_in ? fin_in[in0 + p] : 0, pl = len_in ? len_in[in0 + p] : 0;
        const int f = (pf || tok == eos) ? 1 : 0;
        lat_parent[out0 + rank] = p; lat_token[out0 + rank] = tok; lat_cum[out0 + rank] = cand_sc[in0 * W + idx];
        cum_out[out0 + rank] = cand_sc[in0 * W + idx]; fin_out[out0 + rank] = f; len_out[out0 + rank] = pf ? pl : pl + 1;
        alive += 1 - f;
    }
    if (alive) atomicAdd(live, alive);
}

struct GatherSrc { const float* hd[8]; };
__global__ __launch_bounds__(128) void beam_gather_kernel(GatherSrc src, int Win, int W, int D4, size_t layer_stride4,
                                                          const int32_t* __restrict__ parent, float4* __restrict__ state_out)
{
    const int row = blockIdx.x, l = blockIdx.y, r = row / W;
    const float4* from = reinterpret_cast<const float4*>(src.hd[l]) + ((size_t)r * Win + parent[row]) * D4;
    float4* to = state_out + (size_t)l * layer_stride4 + (size_t)row * D4;
    for (int i = threadIdx.x; i < D4; i += 128) to[i] = from[i];
}

// one wave per (sentence, final slot)
__global__ __launch_bounds__(64) void beam_backtrack_kernel(int W, int rows, int n_run, int steps, int eos,
                                                            const int32_t* __restrict__ lat_parent, const int32_t* __restrict__ lat_token,
                                                            const float* __restrict__ cum, const int32_t* __restrict__ len,
                                                            const float* __restrict__ lenpow,
                                                            int32_t* __restrict__ out_ids, float* __restrict__ score_out, float* __restrict__ cum_out,
                                                            int32_t* __restrict__ len_out)
{
    const int lane = threadIdx.x, r = blockIdx.x / W, j = blockIdx.x - r * W;
    const size_t s0 = (size_t)r * W;
    float sc = 0.f; unsigned key = 0;
    if (lane < W) {
        const float c = cum[s0 + lane];
        sc = lenpow ? __fdiv_rn(c, lenpow[len[s0 + lane]]) : c;
        key = order_key(sc);
    }
    const unsigned kj = __shfl(key, j, 64);
    const float scj = __shfl(sc, j, 64);
    const unsigned long long better = __ballot(lane < W && (key > kj || (key == kj && lane < j)));
    const int rank = __popcll(better);
    int32_t* out = out_ids + (s0 + rank) * (size_t)steps;
    if (lane == 0) {
        int slot = j;
        for (int t = n_run - 1; t >= 0; --t) {
            const size_t at = (size_t)t * rows + s0 + slot;
            out[t] = lat_token[at];
            slot = lat_parent[at];
        }
        if (score_out) score_out[s0 + rank] = scj;
        if (cum_out) cum_out[s0 + rank] = cum[s0 + j];
        if (len_out) len_out[s0 + rank] = len[s0 + j];
    }
    for (int t = n_run + lane; t < steps; t += 64) out[t] = eos;
}

// the group's lattice (steps run, n, W) into the caller's (steps, b, W) arrays; beyond the steps run: the frozen entry
__global__ __launch_bounds__(256) void beam_lattice_out_kernel(int W, int rows, int n_run, int steps, int eos, size_t out_step, const int32_t* __restrict__ lat_parent,
                                                               const int32_t* __restrict__ lat_token, const float* __restrict__ lat_cum,
                                                               const float* __restrict__ cum, int32_t* __restrict__ o_parent,
                                                               int32_t* __restrict__ o_token, float* __restrict__ o_cum)
{
    const size_t total = (size_t)steps * rows;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t t = i / rows, e = i - t * rows, o = t * out_step + e;
        const bool ran = (int)t < n_run;
        if (o_parent) o_parent[o] = ran ? lat_parent[i] : (int)(e % W);
        if (o_token) o_token[o] = ran ? lat_token[i] : eos;
        if (o_cum) o_cum[o] = ran ? lat_cum[i] : cum[e];
    }
}

}  // namespace

hipError_t beam_rows(hipStream_t st, const float* logits, int rows, int V, int W, const float* cum, const int32_t* fin, int eos,
                     float* cand_sc, int32_t* cand_tok, int32_t* cand_cnt)
{
    if (rows < 1 || W < 1 || W > kBeamMax || W > V) return hipErrorInvalidValue;
    hipLaunchKernelGGL(beam_rows_kernel, dim3(rows), dim3(256), 0, st, logits, V, W, cum, fin, eos, cand_sc, cand_tok, cand_cnt);
    return hipGetLastError();
}

hipError_t beam_select(hipStream_t st, const BeamStep& a)
{
    if (a.n < 1 || a.W < 1 || a.W > kBeamMax || a.Win < 1 || a.Win > a.W) return hipErrorInvalidValue;
    hipLaunchKernelGGL(beam_select_kernel, dim3(a.n), dim3(256), 0, st, a.Win, a.W, a.cand_sc, a.cand_tok, a.cand_cnt, a.fin_in, a.len_in, a.eos,
                       a.lat_parent, a.lat_token, a.lat_cum, a.cum_out, a.fin_out, a.len_out, a.live);
    return hipGetLastError();
}

hipError_t beam_gather(hipStream_t st, const float* const* hd, int L, int n, int Win, int W, int D, const int32_t* parent, float* state_out)
{
    if (L < 1 || L > 8 || (D & 3) || n < 1) return hipErrorInvalidValue;
    GatherSrc src{};
    for (int l = 0; l < L; ++l) src.hd[l] = hd[l];
    hipLaunchKernelGGL(beam_gather_kernel, dim3(n * W, L), dim3(128), 0, st, src, Win, W, D / 4, (size_t)n * W * (D / 4), parent,
                       reinterpret_cast<float4*>(state_out));
    return hipGetLastError();
}

hipError_t beam_backtrack(hipStream_t st, const BeamEnd& a)
{
    if (a.n < 1 || a.W < 1 || a.W > kBeamMax || a.n_run < 1 || a.n_run > a.steps) return hipErrorInvalidValue;
    const int rows = a.n * a.W;
    hipLaunchKernelGGL(beam_backtrack_kernel, dim3(rows), dim3(64), 0, st, a.W, rows, a.n_run, a.steps, a.eos, a.lat_parent, a.lat_token, a.cum, a.len,
                       a.lenpow, a.out_ids, a.score_out, a.cum_out, a.len_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !(a.o_parent || a.o_token || a.o_cum)) return e;
    const size_t total = (size_t)a.steps * rows;
    hipLaunchKernelGGL(beam_lattice_out_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, st, a.W, rows, a.n_run, a.steps,
                       a.eos, a.out_step, a.lat_parent, a.lat_token, a.lat_cum, a.cum, a.o_parent, a.o_token, a.o_cum);
    return hipGetLastError();
}

}  // namespace avae
