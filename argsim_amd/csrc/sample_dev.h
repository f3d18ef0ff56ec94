// sample_dev.h -- device helpers shared by the samplers (decode.hip: the persistent launch; ops.hip: sample_rows, sample_rows_p),
// beam.hip and score.hip: the counter RNG (mixer, uniform, normal) and the Gumbel noise of stream 3, order-preserving keys with a
// workgroup radix select of the k-th largest and one by probability mass (the nucleus), the running (max, sum exp) pair of a
// log-sum-exp, the tie rule cand_better, and the samplers' pick: struct Pick (candidate + log-sum-exp with its wave and workgroup
// merges) and pick_kept, the final pass over a kept set.  The generic reductions are in reduce_dev.h, which includes this file.
// The contract is in include/argsim_vae.h (avae_decode_sample, avae_decode_sample_p); both samplers and the float64 references of
// tests/sampling_ref.py and tests/nucleus_ref.py implement exactly it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace avae {

__device__ __forceinline__ uint64_t mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

// the generator itself: value = f(seed, stream, index).  Streams: 1 word dropout, 2 epsilon (ops.hip), 3 Gumbel (below),
// 4 the draws of the importance-weighted score (score.hip), 5 the perturbation of the affinity-propagation similarities (affinity.hip),
// 6 the random start of the t-SNE embedding (tsne.hip), 7 the k-means++ draws (kmeans.hip), 8 the keys of the generated relabelings of
// the two-sample test (mmd.hip; the 64-bit keys themselves, not uniform01)
__device__ __forceinline__ float uniform01(uint64_t seed, uint64_t stream, uint64_t idx)
{
    uint64_t r = mix64(mix64(seed ^ (stream * 0xD6E8FEB86659FD93ULL)) + idx);
    return (float)((r >> 40) + 0.5) * (1.0f / 16777216.0f);      // (0,1)
}
__device__ __forceinline__ float normal01(uint64_t seed, uint64_t stream, uint64_t idx)
{
    float u1 = uniform01(seed, stream, 2 * idx), u2 = uniform01(seed, stream, 2 * idx + 1);
    return sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// stream 3 of the generator (1: word dropout, 2: epsilon).  key = sample_key(seed) once per call / thread;
// index = ((row << 20) + step) << 20 + v: a row's draws depend on neither the batch size nor the step cap.
__device__ __forceinline__ uint64_t sample_key(uint64_t seed) { return mix64(seed ^ (3ULL * 0xD6E8FEB86659FD93ULL)); }
__device__ __forceinline__ uint64_t sample_base(int row, int step) { return (((uint64_t)(unsigned)row << 20) + (uint64_t)(unsigned)step) << 20; }
// g = -log(-log u), u = (23 random bits + 0.5) 2^-23: exact in fp32 and strictly inside (0, 1), so g is finite (the
// 24-bit form of uniform01 rounds to 1.0 for its top values: k + 0.5 is no fp32 number above 2^23)
__device__ __forceinline__ float gumbel(uint64_t key, uint64_t base, int v)
{
    const uint64_t x = mix64(key + base + (uint64_t)(unsigned)v);
    const float u = ((float)(unsigned)(x >> 41) + 0.5f) * (1.0f / 8388608.0f);
    return -logf(-logf(u));
}

// fp32 -> uint key with the same order (larger float, larger key; -0 and +0 share one key, as they compare equal); a NaN
// gets key 0, below -inf: it is never kept before a number and never selected
__device__ __forceinline__ unsigned order_key(float x)
{
    if (x != x) return 0u;
    if (x == 0.f) x = 0.f;
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the k-th largest key (1 <= k <= number of keys) over the whole workgroup by a radix select, 4 passes of 8 bits from
// the top: a 256-bin histogram in LDS of the keys that match the prefix found so far, then the bin in which the count
// from the top reaches k.  each(f) calls f(key) for every key of THIS thread; sh: 258 words of LDS.  Every thread of
// the workgroup must call it (barriers inside); all return the same key.  need / ties (optional, both or neither): how many keys
// EQUAL to the result are among the k largest, and how many keys equal it (beam.hip breaks that tie by token); with them the call
// ends in a barrier, so that sh is free again at once.
template <class Each>
__device__ __forceinline__ unsigned kth_largest_key(Each each, unsigned k, unsigned* sh, unsigned* need = nullptr, unsigned* ties = nullptr)
{
    const int tid = threadIdx.x, nth = blockDim.x;
    unsigned prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < 256; i += nth) sh[i] = 0;
        __syncthreads();
        each([&](unsigned key) { if ((key & mask) == prefix) atomicAdd(&sh[(key >> shift) & 255u], 1u); });
        __syncthreads();
        if (tid < 64) {                         // lane i owns bins 4 i .. 4 i + 3; suffix sums run from the top bin down
            const unsigned c0 = sh[4 * tid], c1 = sh[4 * tid + 1], c2 = sh[4 * tid + 2], c3 = sh[4 * tid + 3];
            unsigned suf = c0 + c1 + c2 + c3;
            for (int o = 1; o < 64; o <<= 1) { const unsigned v = __shfl_down(suf, o, 64); if (tid + o < 64) suf += v; }
            unsigned above = suf - (c0 + c1 + c2 + c3);       // keys in bins above this lane's
            if (above < k && k <= suf) {                       // exactly one lane: the count crosses k inside its bins
                int bin = 4 * tid + 3;
                if (above + c3 < k) { above += c3; bin = 4 * tid + 2;
                    if (above + c2 < k) { above += c2; bin = 4 * tid + 1;
                        if (above + c1 < k) { above += c1; bin = 4 * tid; } } }
                sh[256] = (unsigned)bin; sh[257] = k - above;
            }
        }
        __syncthreads();
        prefix |= sh[256] << shift; mask |= 255u << shift; k = sh[257];
    }
    if (need) { *need = k; *ties = sh[prefix & 255u]; __syncthreads(); }      // (the last pass' histogram: keys that share the top 24 bits, by their low 8)
    return prefix;
}

// nucleus (top-p) sampling, contract in include/argsim_vae.h (avae_decode_sample_p): the fixed-point weight of a token whose
// scaled logit is x under the kept set's maximum m: floor(exp(x - m) 2^40), the maximum itself exactly 2^40 without an
// exponential (the lse_add convention: +inf weighs 2^40 and everything beside it 0).  Integer weights sum to the same
// total in any order: the mass select below is bit-reproducible without a fixed reduction tree.
__device__ __forceinline__ unsigned long long mass_weight(float x, float m)
{
    return x == m ? (1ULL << 40) : (unsigned long long)(expf(x - m) * 1099511627776.f);
}

// the sibling of kth_largest_key that selects by MASS: the largest key with (sum of the weights of the keys >= it) >= need,
// need = ceil(top_p W) clamped to [1, W], W = the sum of all weights.  The same 4 passes of 8 bits from the top; the 256
// bins hold 64-bit weight sums (64-bit integer LDS atomics), the 64-lane suffix scan runs over them, and the pass ends in
// the bin in which the running mass crosses need, less the mass above that bin.  each(f) calls f(key, weight) for every
// member of THIS thread (the caller leaves out what is not in the set: NaN, below the top-k threshold); sh: 260 x 8 bytes
// of LDS.  Every thread of the workgroup must call it; all return the same key and *nkept = how many members have a key
// >= it (0 for an empty set, whose key is 0).  Ends in a barrier: sh is free again at once.
template <class Each>
__device__ __forceinline__ unsigned mass_threshold_key(Each each, float top_p, unsigned long long* sh, unsigned* nkept)
{
    const int tid = threadIdx.x, nth = blockDim.x;
    unsigned prefix = 0, mask = 0;
    unsigned long long need = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < 256; i += nth) sh[i] = 0;
        if (tid == 0) sh[258] = 0;
        __syncthreads();
        each([&](unsigned key, unsigned long long w) { if (w != 0 && (key & mask) == prefix) atomicAdd(&sh[(key >> shift) & 255u], w); });
        __syncthreads();
        if (tid < 64) {                         // lane i owns bins 4 i .. 4 i + 3; suffix sums run from the top bin down
            const unsigned long long c0 = sh[4 * tid], c1 = sh[4 * tid + 1], c2 = sh[4 * tid + 2], c3 = sh[4 * tid + 3];
            unsigned long long suf = c0 + c1 + c2 + c3;
            for (int o = 1; o < 64; o <<= 1) { const unsigned long long v = __shfl_down(suf, o, 64); if (tid + o < 64) suf += v; }
            if (shift == 24) {                  // lane 0's suffix is the whole mass W
                const unsigned long long W = __shfl(suf, 0, 64);
                const double dn = ceil((double)top_p * (double)W);
                need = !(dn >= 1.0) ? 1ULL : (dn >= (double)W ? W : (unsigned long long)dn);
                if (W == 0) { need = 0; if (tid == 0) { sh[256] = 0; sh[257] = 0; } }      // nothing in the set: key 0, nobody crosses
            }
            unsigned long long above = suf - (c0 + c1 + c2 + c3);       // mass in bins above this lane's
            if (above < need && need <= suf) {                            // exactly one lane: the mass crosses need inside its bins
                int bin = 4 * tid + 3;
                if (above + c3 < need) { above += c3; bin = 4 * tid + 2;
                    if (above + c2 < need) { above += c2; bin = 4 * tid + 1;
                        if (above + c1 < need) { above += c1; bin = 4 * tid; } } }
                sh[256] = (unsigned long long)bin; sh[257] = need - above;
            }
        }
        __syncthreads();
        prefix |= (unsigned)sh[256] << shift; mask |= 255u << shift; need = sh[257];
    }
    unsigned cnt = 0;
    each([&](unsigned key, unsigned long long) { cnt += key >= prefix ? 1u : 0u; });
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0 && cnt) atomicAdd(reinterpret_cast<unsigned*>(&sh[258]), cnt);      // (sh[258] was zeroed before the last pass' barriers)
    __syncthreads();
    *nkept = *reinterpret_cast<unsigned*>(&sh[258]);
    __syncthreads();
    return prefix;
}

// running log-sum-exp as (m, s): sum = s exp(m).  Equal values add 1 without an exponential, so a +inf logit gives
// (inf, count) and not NaN; a NaN x is skipped by the caller.
__device__ __forceinline__ void lse_add(float& m, float& s, float x)
{
    if (x == m) s += 1.f;
    else if (x > m) { s = s * expf(m - x) + 1.f; m = x; }       // m = -inf at the start: s = 0 * 0 + 1
    else s += expf(x - m);
}
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2)
{
    if (s2 == 0.f) return;
    if (s == 0.f) { m = m2; s = s2; return; }
    if (m2 == m) s += s2;
    else if (m2 > m) { s = s * expf(m - m2) + s2; m = m2; }
    else s += s2 * expf(m2 - m);
}
// log-softmax value of x under (m, s)
__device__ __forceinline__ float lse_logp(float x, float m, float s) { return (x == m ? 0.f : x - m) - logf(s); }

// candidate (score, id) merge: larger score, then smaller id (the first maximum).  THE tie rule of every row kernel: pred is the
// first maximum, beam search at width 1 equals greedy, top_p 0 equals avae_decode_sample bit for bit.  ArgFirst (reduce_dev.h) and
// Pick below merge through it and nothing else spells it out.
__device__ __forceinline__ bool cand_better(float sc, int id, float best, int besti) { return sc > best || (sc == best && id < besti); }

// what a sampler keeps per thread, wave and workgroup: the best candidate (score, id) with its scaled logit bx = l inv_t, and the
// running log-sum-exp (m, s) of the scaled logits of the whole kept set -- the token and its log-probability
struct Pick {
    float best = -INFINITY, bx = 0.f, m = -INFINITY, s = 0.f; int besti = 0x7fffffff;
    // a thread's own scan in ascending id order: strict >, so the first maximum stays and a NaN score never enters
    __device__ __forceinline__ void take(float sc, int id, float xs)
    {
        if (sc > best) { best = sc; besti = id; bx = xs; }
        lse_add(m, s, xs);
    }
    __device__ __forceinline__ void merge(const Pick& o)
    {
        if (cand_better(o.best, o.besti, best, besti)) { best = o.best; besti = o.besti; bx = o.bx; }
        lse_merge(m, s, o.m, o.s);
    }
    // butterfly over aligned groups of W lanes (64: the wave; 8: decode mode 1, whose lanes 8.. hold the neutral element), in every lane
    template <int W = 64>
    __device__ __forceinline__ void wave_merge()
    {
#pragma unroll
        for (int o = W / 2; o > 0; o >>= 1)
            merge(Pick{__shfl_xor(best, o, 64), __shfl_xor(bx, o, 64), __shfl_xor(m, o, 64), __shfl_xor(s, o, 64), __shfl_xor(besti, o, 64)});
    }
    // over the NW waves of the workgroup, after wave_merge(): lane 0 of wave w stores its record at sh[5 w .. 5 w + 4] (5 NW words of
    // LDS), ONE barrier, then thread 0 merges waves 1 .. NW-1 into its own in that order (a sequential LSE merge: the order is part of
    // the result's bits).  Every thread must call it; the result is valid on thread 0.  No barrier before the stores and none after the
    // sweep: the caller keeps sh free on both sides.
    template <int NW>
    __device__ __forceinline__ void block_merge(float* sh)
    {
        if ((threadIdx.x & 63) == 0) {
            float* r = sh + 5 * (threadIdx.x >> 6);
            r[0] = best; r[1] = bx; r[2] = m; r[3] = s; r[4] = __int_as_float(besti);
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int w = 1; w < NW; ++w) { const float* r = sh + 5 * w; merge(Pick{r[0], r[1], r[2], r[3], __float_as_int(r[4])}); }
    }
    __device__ __forceinline__ bool none() const { return besti == 0x7fffffff; }      // nothing above -inf was offered
    __device__ __forceinline__ int token() const { return none() ? 0 : besti; }
    __device__ __forceinline__ float logp() const { return lse_logp(bx, m, s); }
};

// the samplers' final pass over a kept set: each(f) calls f(id, l) for every logit of THIS thread that is a number, in ascending id;
// kept = order_key(l) >= thr; score = l inv_t + Gumbel noise of (key, base, id), without noise l itself.  Returns the thread's Pick.
template <class Each>
__device__ __forceinline__ Pick pick_kept(Each each, unsigned thr, float inv_t, bool noise, uint64_t key, uint64_t base)
{
    Pick p;
    each([=, &p](int id, float l) {
        if (order_key(l) < thr) return;
        const float xs = l * inv_t;
        p.take(noise ? xs + gumbel(key, base, id) : l, id, xs);
    });
    return p;
}

}  // namespace avae
