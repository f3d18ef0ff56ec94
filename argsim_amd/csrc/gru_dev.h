// gru_dev.h -- device-side helpers shared by the GRU kernel files (gru.hip, gru_reg.hip, gru_team.hip, gru_rs.hip): fragment loads with the in-band
// "not yet written" check, buffer-instruction wrappers, bounded spins, the same-XCD rendezvous, the tiled exchange index maps,
// team barriers, the team-kernel workgroup map, the forward and backward cell, and the shared part of the team kernels' scaffold.
// Internal; not part of the C ABI.
#pragma once
#include <type_traits>
#include "kernels.h"
#include "mfma_tile.h"      // the vector typedefs and pack_bf16

namespace avae {

// 16-bit exchange (bf16 mode, backward team kernels): the exchanged operand itself is stored as bf16, eight k per 16-byte
// chunk -- element (pos, row, k) at halfword
//     X[(((pos * B/16 + row/16) * K/8 + k/8) * 16 + row%16) * 8 + k%8]
// -- so one load instruction of a wave still reads 1 KB of contiguous memory and IS the v_mfma_f32_16x16x32_bf16 A operand
// (half the bytes through the texture addresser, no conversion, the whole K range of a wave in flight at once).  "Not
// yet written" is the halfword 0xFFFF (the launcher's fill); a stored value with that pattern (a NaN) becomes 0x7FC0.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned xch16_index(int pos, int row, int k, int B, int K)
{
    return ((((unsigned)pos * (unsigned)(B >> 4) + (unsigned)(row >> 4)) * (unsigned)(K >> 3) + (unsigned)(k >> 3)) * 16u + (unsigned)(row & 15)) * 8u + (unsigned)(k & 7);
}
__device__ __forceinline__ unsigned short bf16_not_sentinel(float v)
{
    const unsigned short h = (unsigned short)(pack_bf16(v, 0.f) & 0xffffu);
    return h == 0xffffu ? (unsigned short)0x7fc0u : h;
}
__device__ __forceinline__ unsigned pk_max_u16(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ bool any_half_sentinel(unsigned mx) { return (mx & 0xffffu) == 0xffffu || (mx >> 16) == 0xffffu; }
// bf16-operand mode in the register-form kernels: the operand keeps its fp32 register but carries a bf16 value (products of
// two such values are exact in fp32, so these kernels and the team kernels' bf16 MFMA differ only in summation order)
__device__ __forceinline__ float opnd(float x, bool bf) { return bf ? __uint_as_float(pack_bf16(0.f, x)) : x; }

constexpr unsigned kSentinel = 0xFFFFFFFFu;
#ifdef AVAE_DIAG
constexpr bool kDiagBuild = true;
#else
constexpr bool kDiagBuild = false;
#endif

// An exchanged value must never alias the "not yet written" pattern: a NaN that reaches the gate math with every
// payload bit set (e.g. from a poisoned parameter) would otherwise make every consumer spin until its 2 s bound.
// Such a value is stored as the canonical quiet NaN instead: still a NaN, never the sentinel.
__device__ __forceinline__ float not_sentinel(float v)
{
    return __float_as_uint(v) == kSentinel ? __uint_as_float(0x7FC00000u) : v;
}
__device__ __forceinline__ int pos_map(int p, int len, int reverse) { return (reverse && p < len) ? (len - 1 - p) : p; }
// sigmoid / tanh on v_exp_f32 + v_rcp_f32 (each <= 1 ulp): absolute error ~1e-7, far inside the
// fp32 parity tolerances, at a fraction of the libm cost that sat on the per-step critical path
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) { return __builtin_fmaf(2.f, __builtin_amdgcn_rcpf(1.f + __expf(-2.f * x)), -1.f); }
// One cell update, shared by every forward kernel form.  Which multiply-adds are fused is written out: left to the
// compiler's contraction the choice followed the surrounding code, and two forms of the same step (the team kernels and
// the one-launch-per-step kernels the tests compare them with) differed in the last bit.
struct GruCellOut { float r, u, n, h; };
__device__ __forceinline__ GruCellOut gru_cell(float gi_r, float gi_u, float gi_n, float gh_r, float gh_u, float gh_n, float hprev)
{
    GruCellOut c;
    c.r = sigmoidf_(gi_r + gh_r);
    c.u = sigmoidf_(gi_u + gh_u);
    c.n = tanhf_(__builtin_fmaf(c.r, gh_n, gi_n));
    float t = (1.f - c.u) * c.n;
    asm volatile("" : "+v"(t));                   // a product of its own, not a candidate for fusion with the sum below
    c.h = __builtin_fmaf(c.u, hprev, t);
    return c;
}

// The gate derivatives of one cell, shared by every backward kernel form:
//   dn = dH (1-u)(1-n^2)   du = dH (h_prev - n) u (1-u)   dr = dn hn r (1-r)     dgi = [dr, du, dn]   dgh = [dr, du, dn r]
// The two products left to the caller -- dn r, and dH u, what the step before inherits through the update gate -- are formed where
// they are stored: computed up here they moved in the instruction stream of every kernel.
struct GruCellGrad { float dr, du, dn; };
__device__ __forceinline__ GruCellGrad gru_cell_bwd(float dH, float r, float u, float n, float hn, float hprev)
{
    GruCellGrad g;
    g.dn = dH * (1.f - u) * (1.f - n * n);
    g.du = dH * (hprev - n) * u * (1.f - u);
    g.dr = g.dn * hn * r * (1.f - r);
    return g;
}

// k offset (inside one wave's contiguous K range) of MFMA step ks for lane quarter kh
template <int NKS>
__device__ __forceinline__ int kperm(int ks, int kh)
{
    if (NKS % 4 == 0) return 16 * (ks >> 2) + 4 * kh + (ks & 3);
    return 4 * ks + kh;
}

// diagnostic phase stamps: 100 MHz real-time counter deltas summed per workgroup into the caller's ph[] / tprev.  `on` is a
// template flag (the production instantiation then carries no stamp code at all) or a run-time flag of a diagnostic instantiation.
#define GRU_STAMP(on, i) do { if (on) { unsigned long long t_ = __builtin_amdgcn_s_memrealtime(); ph[i] += t_ - tprev; tprev = t_; } } while (0)

__device__ __forceinline__ u32x4 load16_sc1(__amdgpu_buffer_rsrc_t rsrc, unsigned byte_off)
{
    return __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)byte_off, 0, 16);     // aux 16 = sc1
}
// Buffer forms of the gate-phase accesses: 32-bit byte offsets against a wave-uniform descriptor.  On the texture
// addresser a buffer instruction costs about half of the global (64-bit address per lane) form of the same access
// (scripts/micro/ta_cost.hip: x4 store of 4 rows x 256 B 43 vs 83 cycles, dword store 31 vs 63).
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x3 __attribute__((ext_vector_type(3)));
__device__ __forceinline__ float bload1(__amdgpu_buffer_rsrc_t rs, unsigned off) { return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)off, 0, 0)); }
__device__ __forceinline__ float4 bload4(__amdgpu_buffer_rsrc_t rs, unsigned off)
{
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ void bstore1(float v, __amdgpu_buffer_rsrc_t rs, unsigned off) { __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, (int)off, 0, 0); }
__device__ __forceinline__ void bstore1_sc1(float v, __amdgpu_buffer_rsrc_t rs, unsigned off) { __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, (int)off, 0, 16); }
__device__ __forceinline__ void bstore3(float x, float y, float z, __amdgpu_buffer_rsrc_t rs, unsigned off)
{
    const u32x3 v = {__float_as_uint(x), __float_as_uint(y), __float_as_uint(z)};
    __builtin_amdgcn_raw_buffer_store_b96(v, rs, (int)off, 0, 0);
}
__device__ __forceinline__ void bstore4(float x, float y, float z, float w, __amdgpu_buffer_rsrc_t rs, unsigned off)
{
    const u32x4 v = {__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), __float_as_uint(w)};
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, (int)off, 0, 0);
}
__device__ __forceinline__ unsigned load4_sc1(const float* p)
{
    return __hip_atomic_load(reinterpret_cast<const unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store4_sc1(float* p, float v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const float* p)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, -1, 0x00020000);
}

// bounded spin bookkeeping shared by the data polls: returns true when the wave must give up
struct SpinGuard {
    unsigned long long t0 = 0; unsigned n = 0;
    __device__ __forceinline__ bool expired(int* err)
    {
        __builtin_amdgcn_s_sleep(4);
        if ((++n & 31u) != 0) return false;
        if (t0 == 0) t0 = __builtin_amdgcn_s_memrealtime();
        if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return true;
        if (__builtin_amdgcn_s_memrealtime() - t0 > 200000000ULL) {   // 2 s at 100 MHz
            __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return true;
        }
        return false;
    }
};

// The loads of a fragment are ISSUED (no wait) and the fragment is verified later, at its
// first use.  Written so that hipcc's waitcnt insertion stays counted on the fast path: younger fragments
// issued in straight-line code before the check stay in flight (vmcnt(N)); only the rare re-load loop,
// which consumes what it loads inside the loop, waits for everything.
template <int NQ>
__device__ __forceinline__ void frag_issue(u32x4 (&v)[NQ], __amdgpu_buffer_rsrc_t rs, unsigned off)
{
#pragma unroll
    for (int q = 0; q < NQ; ++q) v[q] = load16_sc1(rs, off + 64u * q);
}
// the same with a run-time (wave-uniform) distance between the pieces: it travels in the scalar offset operand
template <int NQ>
__device__ __forceinline__ void frag_issue(u32x4 (&v)[NQ], __amdgpu_buffer_rsrc_t rs, unsigned off, unsigned qstride)
{
#pragma unroll
    for (int q = 0; q < NQ; ++q) v[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, (int)(qstride * q), 16);
}
template <int NQ>
__device__ __forceinline__ bool frag_bad(const u32x4 (&v)[NQ])
{
    unsigned mx = 0u;                     // the sentinel is the largest unsigned value: one running maximum
#pragma unroll
    for (int q = 0; q < NQ; ++q) mx = max(max(mx, max(v[q].x, v[q].y)), max(v[q].z, v[q].w));
    return __any(mx == kSentinel);
}
// verify `v`; on sentinels re-load it until complete (bounded)
template <int NQ>
__device__ __forceinline__ void frag_ensure(u32x4 (&v)[NQ], __amdgpu_buffer_rsrc_t rs, unsigned off, int* err)
{
    if (frag_bad<NQ>(v)) {
        SpinGuard sg;
        do { frag_issue<NQ>(v, rs, off); } while (frag_bad<NQ>(v) && !sg.expired(err));
    }
}
template <int NQ>
__device__ __forceinline__ void frag_ensure(u32x4 (&v)[NQ], __amdgpu_buffer_rsrc_t rs, unsigned off, int* err, unsigned qstride)
{
    if (frag_bad<NQ>(v)) {
        SpinGuard sg;
        do { frag_issue<NQ>(v, rs, off, qstride); } while (frag_bad<NQ>(v) && !sg.expired(err));
    }
}
// the same for a 16-bit exchange: "not yet written" is the halfword 0xFFFF (one running v_pk_max_u16)
template <int NQ>
__device__ __forceinline__ bool frag_bad16(const u32x4 (&v)[NQ])
{
    unsigned mx = 0u;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const unsigned a = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(unsigned short __attribute__((ext_vector_type(2))), v[q].x), __builtin_bit_cast(unsigned short __attribute__((ext_vector_type(2))), v[q].y)));
        const unsigned b = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(unsigned short __attribute__((ext_vector_type(2))), v[q].z), __builtin_bit_cast(unsigned short __attribute__((ext_vector_type(2))), v[q].w)));
        const unsigned c = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(unsigned short __attribute__((ext_vector_type(2))), a), __builtin_bit_cast(unsigned short __attribute__((ext_vector_type(2))), b)));
        mx = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(unsigned short __attribute__((ext_vector_type(2))), mx), __builtin_bit_cast(unsigned short __attribute__((ext_vector_type(2))), c)));
    }
    return __any((mx & 0xffffu) == 0xffffu || (mx >> 16) == 0xffffu);
}
template <int NQ>
__device__ __forceinline__ void frag_ensure16(u32x4 (&v)[NQ], __amdgpu_buffer_rsrc_t rs, unsigned off, int* err, unsigned qstride)
{
    if (frag_bad16<NQ>(v)) {
        SpinGuard sg;
        do { frag_issue<NQ>(v, rs, off, qstride); } while (frag_bad16<NQ>(v) && !sg.expired(err));
    }
}

// Hand-counted form of the same pipeline for the D = 512 backward pass.  hipcc's waitcnt insertion falls
// back to vmcnt(0) around the re-load branches of frag_ensure, which serialises every piece behind a
// full L2 round trip; these loads are invisible to it (inline asm), are waited for by explicit counted
// s_waitcnt statements that name the destination registers, and are fully retired before the code leaves
// the block that issued them (cdna_hip_programming.md section 5.7 forms (ii)/(iii)).
typedef int i32x4 __attribute__((ext_vector_type(4)));
// the buffer descriptor of a whole address space behind p, as the inline-asm loads take it
__device__ __forceinline__ i32x4 make_srd(const float* p)
{
    const unsigned long long pa = (unsigned long long)p;
    return (i32x4){(int)(unsigned)(pa & 0xffffffffULL), (int)(unsigned)((pa >> 32) & 0xffffULL), -1, 0x00020000};
}
template <int OFF>
__device__ __forceinline__ void asm_issue6(u32x4 (&v)[6], unsigned voff, i32x4 srd)
{
    asm volatile("buffer_load_dwordx4 %0, %6, %7, 0 offen offset:%c8 sc1\n\t"
                 "buffer_load_dwordx4 %1, %6, %7, 0 offen offset:%c9 sc1\n\t"
                 "buffer_load_dwordx4 %2, %6, %7, 0 offen offset:%c10 sc1\n\t"
                 "buffer_load_dwordx4 %3, %6, %7, 0 offen offset:%c11 sc1\n\t"
                 "buffer_load_dwordx4 %4, %6, %7, 0 offen offset:%c12 sc1\n\t"
                 "buffer_load_dwordx4 %5, %6, %7, 0 offen offset:%c13 sc1"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5])
                 : "v"(voff), "s"(srd), "i"(OFF), "i"(OFF + 64), "i"(OFF + 128), "i"(OFF + 192), "i"(OFF + 256), "i"(OFF + 320)
                 : "memory");
}
// the same six loads from the tiled exchange: 1 KB between consecutive 16-float groups (soffset carries what the 12-bit
// immediate cannot)
__device__ __forceinline__ void asm_issue6x(u32x4 (&v)[6], unsigned voff, i32x4 srd, int soff0, int soff1)
{
    asm volatile("buffer_load_dwordx4 %0, %6, %7, %8 offen offset:0 sc1\n\t"
                 "buffer_load_dwordx4 %1, %6, %7, %8 offen offset:1024 sc1\n\t"
                 "buffer_load_dwordx4 %2, %6, %7, %8 offen offset:2048 sc1\n\t"
                 "buffer_load_dwordx4 %3, %6, %7, %8 offen offset:3072 sc1\n\t"
                 "buffer_load_dwordx4 %4, %6, %7, %9 offen offset:0 sc1\n\t"
                 "buffer_load_dwordx4 %5, %6, %7, %9 offen offset:1024 sc1"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5])
                 : "v"(voff), "s"(srd), "s"(soff0), "s"(soff1)
                 : "memory");
}
template <int N>
__device__ __forceinline__ void asm_wait6(u32x4 (&v)[6])
{
    asm volatile("s_waitcnt vmcnt(%c6)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]) : "i"(N) : "memory");
}

// scalar-element variant for the small test dimensions (wave K range not a multiple of 16)
template <int N, int NKS>
__device__ __forceinline__ void load_frag_scalar(float* dst, const float* base, int ks0, int kh, bool poll, int* err)
{
    SpinGuard sg;
    for (;;) {
        unsigned v[N]; bool bad = false;
#pragma unroll
        for (int i = 0; i < N; ++i) { v[i] = load4_sc1(base + kperm<NKS>(ks0 + i, kh)); bad |= v[i] == kSentinel; }
        if (!poll || !__any(bad) || sg.expired(err)) {
#pragma unroll
            for (int i = 0; i < N; ++i) dst[i] = __uint_as_float(v[i]);
            return;
        }
    }
}

// Same-XCD detection (speed only): every workgroup of a group publishes the id of the XCD it runs
// on with the placement-independent sc1 protocol; if all HT ids agree the group's per-step stores
// may stay in that XCD's L2 (plain stores) instead of being written through to the memory side.
// All members read the same HT words, so they all take the same decision.
// first half of the rendezvous, for kernels that have work to do before they need the answer (the team kernels copy their
// weight slice to LDS in between: ~6 us per launch during which the other workgroups' publications arrive)
__device__ __forceinline__ void xcd_publish(unsigned* ctr2, unsigned* ids, int ht)
{
    if (threadIdx.x == 0) {
        const unsigned my = __builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xfu;     // HW_REG_XCC_ID
        __hip_atomic_store(ids + ht, my + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(ctr2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
__device__ __forceinline__ bool group_same_xcd(unsigned* ctr2, unsigned* ids, int ht, int HT, int* err, int force_slow, bool published = false)
{
    __shared__ int s_fast;
    if (threadIdx.x < 64) {          // the first wave: lane 0 publishes and waits, then lane i reads id i (one round trip, not HT)
        const unsigned my = __builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xfu;     // HW_REG_XCC_ID
        bool ok = true;
        if (threadIdx.x == 0) {
            if (!published) {
            __hip_atomic_store(ids + ht, my + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_fetch_add(ctr2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            SpinGuard sg;
            while (__hip_atomic_load(ctr2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)HT)
                if (sg.expired(err)) { ok = false; break; }
        }
        ok = __all(ok);
        bool same = true;
        for (int i = threadIdx.x; i < HT; i += 64)
            same = same && __hip_atomic_load(ids + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == my + 1u;
        same = __all(same) && ok && !force_slow;
        if (threadIdx.x == 0) s_fast = same ? 1 : 0;
    }
    __syncthreads();
    return s_fast != 0;
}

// blockIdx -> (job, group, hidden tile).  Under round-robin dispatch blocks b and b + grid/2 share a
// CU (2 workgroups per CU): the map gives them DIFFERENT chains (the other direction, or another batch
// group) so one's MFMA phase can overlap the other's exchange latency, keeps blockIdx % 8 = group % 8
// (a group's workgroups on one XCD), and reports which half a block is in so that half can be
// staggered by part of a step.  Any placement is correct; this is speed only.
__device__ __forceinline__ bool wg_map(const GruArgs& a, int HT, int* jb, int* g, int* ht)
{
    const int per_job = a.G * HT, bid = blockIdx.x;
    // alt = which of two interleaved sets a block belongs to: blocks b and b+8 (consecutive blocks of one
    // XCD, which the dispatcher was observed to place on the same CU) get different chains
    const int alt = (bid >> 3) & 1, idx = ((bid >> 4) << 3) | (bid & 7);
    if (a.njobs == 2 && (per_job & 7) == 0) {                       // the two encoder directions
        *jb = alt; *g = idx % a.G; *ht = idx / a.G;
        return alt != 0;
    }
    if (a.njobs == 1 && a.G == 16) {                                // one decoder layer: groups g and g+8
        *jb = 0; *g = (bid & 7) + 8 * alt; *ht = bid >> 4;
        return alt != 0;
    }
    *jb = bid / per_job;
    const int rem = bid - *jb * per_job;
    *g = rem % a.G; *ht = rem / a.G;
    return false;
}

// ---- tiled exchange (team kernels).  The MFMA A operand puts 16 different batch rows in 16 adjacent lanes.  Read from
// a row-major (pos, row, k) buffer, every lane of a 16-byte load touches another cache line (rows are 2-6 KB apart) and
// the CU's texture addresser spends ~64 cycles per load instruction: TA_BUSY was 93 % of the backward kernel and 48 %
// of the forward (gpurun_out/pp1_p5), the real limiter of the step.  The exchanged operand therefore lives in a
// scratch buffer in fragment order -- element (pos, row, k) at
//     X[(((pos * B/16 + row/16) * K/4 + k/4) * 16 + row%16) * 4 + k%4]
// -- so that one load instruction of a wave reads 1 KB of contiguous memory (lane (n, kh): 16 bytes at n*16 + kh*256).
// The row-major hs / dgh the GEMMs consume are written beside it with plain stores and are no longer polled.
// (float index; a job's buffer is below 2^32 bytes -- team_geometry checks -- so 32-bit arithmetic is exact)
__device__ __forceinline__ unsigned xch_index(int pos, int row, int k, int B, int K)
{
    return ((((unsigned)pos * (unsigned)(B >> 4) + (unsigned)(row >> 4)) * (unsigned)(K >> 2) + (unsigned)(k >> 2)) * 16u + (unsigned)(row & 15)) * 4u + (unsigned)(k & 3);
}
// byte offset of lane (n, kh)'s 16 bytes of chunk kc0 + kh, rows row0 .. row0+15 (row0 % 16 == 0) at position pos
__device__ __forceinline__ unsigned xch_lane_offset(int pos, int row0, int kc0, int n, int kh, int B, int K)
{
    return ((((unsigned)pos * (unsigned)(B >> 4) + (unsigned)(row0 >> 4)) * (unsigned)(K >> 2) + (unsigned)(kc0 + kh)) * 16u + (unsigned)n) * 16u;
}

// ---- exchange ring (fp32 team kernels with one row block per workgroup; GruPlan::ring = kGruRing slots).  A consumer of iteration q
// reads only what iteration q - 1 produced, so the scratch need not be as long as the sequence: the value a team produces in its
// iteration q (its running step count -- NOT pos_map(...), which differs per row in a reversed ragged job; producer and consumer of a
// value agree on the iteration) lives in slot q % 4, the layout inside a slot as above with `pos` = the slot.  Data stays the flag
// (sentinel, probe, running-max check, bounded spins: all unchanged); the launcher arms min(S, 4) slots and the producers re-arm
// them: in iteration p, behind the team barrier that follows the MFMA pass, ONE wave of the team stores the sentinel over the
// workgroup's own slice (its 16 or 48 columns x the team's 16 rows: 1 or 3 KB, contiguous) of slot (p + 2) % 4, the slot that held
// iteration p - 2, unless the row block has no iteration p + 2 that stores.
//   Dead: at that barrier every wave of this team holds its whole operand of iteration p, i.e. the iteration p - 1 values of all 32
// producers; a producer stores those only behind its own team barrier of iteration p - 1, where all its waves' loads of iteration
// p - 2 have returned.  Nobody reads slot (p - 2) % 4 any more.
//   Armed in time: the slot next takes data in iteration p + 2 and is polled from p + 3 on.  The re-arming wave waits for its operand
// loads of iteration p + 1 -- vmcnt counts stores too and retires in issue order, so the re-arm is acknowledged by L2 by then --
// before the team barrier of p + 1, behind which the gate threads store the iteration p + 1 values; a consumer that has seen those
// (it cannot poll the slot earlier) therefore sees the re-arm, and this workgroup's own data stores of p + 2 come after it.  With 3
// slots the re-armed slot would take data one iteration later, ordered against nothing but a new vmcnt(0) on the gate path.
// N16 stores of 16 bytes per lane, 1 KB apart, from chunk kc0 of the team's rows at row0; sc1 off the same-XCD fast path like the data.
template <int N16>
__device__ __forceinline__ void xch_rearm(__amdgpu_buffer_rsrc_t rs, int slot, int row0, int kc0, int lane, int B, int K, bool fast)
{
    const unsigned off = ((((unsigned)slot * (unsigned)(B >> 4) + (unsigned)(row0 >> 4)) * (unsigned)(K >> 2) + (unsigned)kc0) * 16u + (unsigned)lane) * 16u;
    const u32x4 s4 = {kSentinel, kSentinel, kSentinel, kSentinel};
    if (fast) {
#pragma unroll
        for (int i = 0; i < N16; ++i) __builtin_amdgcn_raw_buffer_store_b128(s4, rs, (int)(off + 1024u * i), 0, 0);
    } else {
#pragma unroll
        for (int i = 0; i < N16; ++i) __builtin_amdgcn_raw_buffer_store_b128(s4, rs, (int)(off + 1024u * i), 0, 16);
    }
}

__device__ __forceinline__ void team_barrier(unsigned* word, unsigned target)
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                       // this wave's LDS traffic is done
    if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < target) __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}


// blockIdx -> (chain group, hidden tile): the grid is C x 32 workgroups, C <= 8 chain groups.  A chain group is a job
// plus the 64-row blocks slot, slot + cpj, ... of that job (cpj = chain groups per job); the 32 workgroups of a chain
// group exchange with each other and share blockIdx % C (one XCD under round-robin dispatch when C = 8; speed only).
struct TeamMap { int cid, ht, jb, slot, cpj, nrb; };
__device__ __forceinline__ TeamMap team_map(const GruArgs& a, int rows_per_block)
{
    TeamMap m;
    const int C = gridDim.x / 32;
    m.cid = blockIdx.x % C; m.ht = blockIdx.x / C;
    m.cpj = C / a.njobs;
    m.jb = m.cid / m.cpj; m.slot = m.cid % m.cpj;
    m.nrb = ((a.Bx > a.B ? a.Bx : a.B) / rows_per_block) / m.cpj;
    return m;
}

// Padding skipped (GruArgs::slens / perm, optional): slens[slot] = the steps row `slot` really has (its length; decoder: + 1),
// perm[slot] = the batch row that sits in that slot -- rows sorted by length and dealt over the workgroups by the caller
// (ops.hip row_order), so that a team's 16 rows are of similar length.  A team runs a row block for
//     nst = max over its 16 rows of slens (made non-increasing over a workgroup's row blocks by a suffix maximum)
// steps instead of S; the positions behind them -- padding in both time orientations -- are zero-filled in the row-major
// outputs (hs / hp forward, dgi / dgh backward: the GEMMs that sum over all rows must meet finite zeros there, as they did
// when the steps were computed) and never touch the exchange.  All 32 workgroups of a chain group read the same slens, so
// they agree on every team's step count; any perm is correct, a sorted one is fast.  The exchange scratch is indexed by
// slot, every external array by perm[slot].
__device__ __forceinline__ int team_steps(const int* slens, int row0, int lane)
{
    int v = slens[row0 + (lane & 15)];
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v = max(v, __shfl_xor(v, o, 64));
    return __builtin_amdgcn_readfirstlane(v);
}

// ---- the scaffold the three 1024-thread team kernels share (gru_fwd_team_kernel, gru_bwd_team_kernel, gru_bwd_rs_kernel).
// hipcc optimises a helper on its own before it inlines it, and these hand-scheduled kernels then come out with other code (commuted
// scalar adds, selects for branches, another order of the loop-edge copies).  What is shared here is what left every kernel's
// instructions as they were; the step counts per row block, the per-row-block registers, the zero fill behind a row block's steps and
// the bias-gradient epilogue did not, in any spelling tried, and stay written out in the kernels.

// wave -> (team, K-split index; reduce-scatter form: wave of the team), as constants the kernels apply themselves:
//     team = (wave >> team_shift) & team_mask,   wk = (wave & wk_mask) + wk_mul * (wave >> wk_shift)
// Waves w and w + 4 share a SIMD; a team's K-split partners meet at a barrier every step.  Which SIMDs a team sits on is a 1-3 % effect
// since the operand loads stopped saturating the texture addresser; the mapping per form is the best of {one SIMD, a SIMD pair, all
// four} measured in-process (scripts/ab_classes.py).  CMP = the compact layout, i.e. a ragged batch: teams run
// out of steps at different times and the ones still running should have every SIMD -- the pipelined forms at 1024 x 64 RAGGED:
// 32.97 -> 30.37 ms with all four, FULL 59.06 -> 59.88.  The reduce-scatter kernel's waves split N, not K, and always sit on all four.
enum class TeamKernel { fwd, bwd, rs };
struct WaveSplit { int team_shift, team_mask, wk_mask, wk_mul, wk_shift; };
constexpr WaveSplit team_wave_split(TeamKernel k, int T, bool pipe, bool cmp)
{
    const bool packed = k != TeamKernel::rs && pipe && !cmp;
    if (T == 4 && packed) return {0, 3, 0, 1, 2};         // one SIMD:       team = wave & 3,        wk = wave >> 2
    if (T == 4) return {2, 3, 3, 0, 0};                   // all four SIMDs: team = wave >> 2,       wk = wave & 3   (forward, RAGGED 10.56 -> 10.43 ms; FULL unchanged)
    if (packed) return {1, 1, 1, 2, 2};                   // a SIMD pair:    team = (wave >> 1) & 1, wk = (wave & 1) + 2 * (wave >> 2)
    // T = 2 on all four SIMDs: a team whose partner has run out of steps (ragged batches) has the whole CU -- forward, RAGGED 256 x 64
    // 10.76 -> 10.54 ms, FULL 16.50 -> 16.45
    if (k == TeamKernel::fwd) return {2, 1, 3, 4, 3};     //                 team = (wave >> 2) & 1, wk = (wave & 3) + 4 * (wave >> 3)
    return {3, 1, 7, 0, 0};                               //                 team = wave >> 3,       wk = wave & 7
}
// one consistent arbitration order on all four SIMDs: a team's K-split partners sit on different SIMDs and meet at the team
// barrier, so if every SIMD serves the teams in the same order the partners finish together (otherwise the barrier pays the
// arbitration skew, measured at 2-3 us per step)
__device__ __forceinline__ void team_set_priority(int team)
{
    const int tq = __builtin_amdgcn_readfirstlane(team);
    if (tq == 0) __builtin_amdgcn_s_setprio(3);
    else if (tq == 1) __builtin_amdgcn_s_setprio(2);
    else if (tq == 2) __builtin_amdgcn_s_setprio(1);
}
// PIPE forms: the item after (p, r) -- the next row block that still has step p, else row block 0 of the next step (FWD: p + 1; the
// backward runs downwards and its tail item p = -1 exists for every row block).  nst_of(r): steps of row block r.
struct NextItem { int r, p; };
template <bool FWD, class N>
__device__ __forceinline__ NextItem team_next_item(N&& nst_of, int nrb, int p, int r)
{
    const bool same_p = r + 1 < nrb && ((!FWD && p < 0) || p < nst_of(r + 1));
    return {same_p ? r + 1 : 0, same_p ? p : (FWD ? p + 1 : p - 1)};
}

// ---- host side: residency check and launch of the 1024-thread team kernels
// Residency.  The persistent kernels exchange data between workgroups inside one launch, so every workgroup of the
// grid must be resident at once.  A plain launch checks nothing (and the occupancy API is advisory), so the grid is
// compared here with (workgroups per CU the occupancy query admits) x (CU count) once per kernel and launch shape,
// and an oversize grid is refused with hipErrorCooperativeLaunchTooLarge instead of being left to the 2 s spin
// bound.  The kernels used need one (1024-thread team kernels) or two (256-thread kernels, <= 80 SGPRs... 102 SGPRs:
// the hardware admits >= 6 such blocks) workgroups per CU, far from the edge where the API over-reports by one.
template <class K>
static hipError_t resident(K kernel, int threads, int dyn_lds, int grid)
{
    struct Entry { const void* k; int threads, lds, cap; };
    static Entry cache[32]; static int ncache = 0;
    const void* kp = reinterpret_cast<const void*>(kernel);
    for (int i = 0; i < ncache; ++i)
        if (cache[i].k == kp && cache[i].threads == threads && cache[i].lds == dyn_lds)
            return grid <= cache[i].cap ? hipSuccess : hipErrorCooperativeLaunchTooLarge;
    int per_cu = 0, dev = 0, cus = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, (size_t)dyn_lds);
    if (e == hipSuccess) e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    const int cap = per_cu * cus;
    if (ncache < 32) cache[ncache++] = Entry{kp, threads, dyn_lds, cap};
    return grid <= cap ? hipSuccess : hipErrorCooperativeLaunchTooLarge;
}

template <class K>
static hipError_t launch_team(hipStream_t st, K kernel, const GruArgs& a, int lds_bytes, int C)
{
    static const void* attr_done[64]; static int nattr = 0;
    const void* kp = reinterpret_cast<const void*>(kernel);
    bool seen = false;
    for (int i = 0; i < nattr; ++i) seen |= attr_done[i] == kp;
    if (!seen) {
        hipError_t e = hipFuncSetAttribute(kp, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        if (e != hipSuccess) return e;
        if (nattr < 64) attr_done[nattr++] = kp;
    }
    const int grid = C * 32;
    hipError_t e = resident(kernel, 1024, lds_bytes, grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(1024), lds_bytes, st, a);
    return hipGetLastError();
}

// the team-kernel instantiation of a runtime T in {2, 4} and runtime flags (pipe, bf16, cmp, ...): f(T, FLAG...) called with
// std::integral_constant arguments, so each combination names its template arguments once
template <class F>
static hipError_t with_flags(F&& f) { return f(); }
template <class F, class... Bs>
static hipError_t with_flags(F&& f, bool b, Bs... rest)
{
    return b ? with_flags([&](auto... c) { return f(std::true_type{}, c...); }, rest...)
             : with_flags([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}
template <class F, class... Bs>
static hipError_t team_dispatch(int T, F&& f, Bs... flags)
{
    return T == 4 ? with_flags([&](auto... c) { return f(std::integral_constant<int, 4>{}, c...); }, flags...)
                  : with_flags([&](auto... c) { return f(std::integral_constant<int, 2>{}, c...); }, flags...);
}

}  // namespace avae
