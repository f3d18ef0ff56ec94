// gru.hip -- the recurrent part of cuDNN-style (reset-after) GRU layers, forward and BPTT,
// as persistent kernels for gfx950.
//
// Replaces tf.contrib.cudnn_rnn.CudnnGRU (reference src/model.py:15,120-121,160):
//   r = s(gi_r + R_r h + bR_r)   u = s(gi_u + R_u h + bR_u)
//   n = tanh(gi_n + r * (R_n h + bR_n))          h' = (1-u) n + u h
// gi = W x + bW is hoisted out of the time loop (one MFMA GEMM, gemm_f32.hip).
//
// Decomposition.  One workgroup (4 waves) owns 16 hidden units (x3 gates) of one job
// (= one layer-direction) for one batch group.  Its 48xD slice of R lives in REGISTERS for
// the whole launch, already in v_mfma_f32_16x16x4_f32 B-operand order (3*D/16 VGPRs per lane);
// (rows in "G16" order c' = (unit/16)*48 + (unit%16)*3 + gate, see kernels.h); the four waves split K, partial sums meet in LDS, then 256 threads do the gate math.
// Per step a workgroup reads only its group's h_{t-1} rows (A operand) and writes its
// 16-column slice of h_t.
//
// Exchange between the workgroups of a group ("the data is the flag", MI355X_MICROARCH.md
// R2 granules with an in-band tag): the launcher fills the exchanged buffer (hs forward, dgh
// backward) with a sentinel bit pattern that the arithmetic never produces (0xFFFFFFFF, a NaN with
// every payload bit set; h is bounded by 1 and hardware NaNs are canonical).  Each 4-byte element
// is written exactly once per launch by ONE store; a consumer wave loads its A fragment with
// L1-bypassing (sc1) loads and simply re-loads it until no dword carries the sentinel.  There is no
// counter, no fence, no store drain and no workgroup barrier on the hand-off.  Stores are
// write-through (sc1) unless all workgroups of the group were dispatched to one XCD, in which case
// that XCD's L2 is the coherence point and plain stores suffice (detected at run time with the
// placement-independent protocol; speed only).  Every spin is bounded; on time-out the error word
// is set and every wait falls through, so the grid always drains.
#include <algorithm>
#include "kernels.h"
#include "gru_dev.h"
#include <type_traits>

namespace avae {

// ------------------------------------------------------------------------------ forward
// Per step and workgroup: (1) issue the loads that do not depend on the exchange (gi);
// (2) load the A operand = the group's h_{p-1} rows, re-loading until complete; (3) MFMAs;
// (4) K-split partial sums and the workgroup's own h_{p-1} slice meet in LDS (the only barrier of
// the step); (5) gate math; (6) store h_p (the exchanged data) first, then the saved gates.
template <int KS, bool STAMPS>   // D = 16*KS
__global__ __launch_bounds__(256, 2) void gru_fwd_kernel(GruArgs a)
{
    constexpr int D = 16 * KS, HT = KS;
    constexpr int WK = 4 * KS;                                  // K range per wave
    __shared__ __attribute__((aligned(16))) float part[2][2][4][3][256];   // [buf][chunk][wave][gate][lane*4+reg]
    __shared__ __attribute__((aligned(16))) float hps[2][2][16][16];       // [buf][chunk][row][unit] own h_{p-1} slice

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, kh = lane >> 4;
    int jb, g, ht;
    const bool second_half = wg_map(a, HT, &jb, &g, &ht);
    const GruJob& J = a.job[jb];
    const int B = a.B;
    const int row_beg = g * a.rows_per_group;
    const int row_end = min(B, row_beg + a.rows_per_group);
    const int ab = STAMPS ? a.ablate : 0;                      // timing experiments exist in the diagnostic instantiation only
    const bool one_sc = row_end - row_beg <= 32;               // single super-chunk: lengths stay in registers

    // weights -> registers, MFMA B-operand order: B[k][n] = R'[ht*48 + gate*16 + n][k]
    const bool bf = a.bf16 != 0;                                // bf16-operand mode: both operands of h R' carry bf16 values
    float w[3][KS];
#pragma unroll
    for (int gate = 0; gate < 3; ++gate) {
        const float* rp = J.R + (size_t)(ht * 48 + n * 3 + gate) * D + wave * WK;
        if (KS % 4 == 0) {
#pragma unroll
            for (int q = 0; q < KS / 4; ++q) {
                float4 v = *reinterpret_cast<const float4*>(rp + 16 * q + 4 * kh);
                w[gate][4 * q + 0] = v.x; w[gate][4 * q + 1] = v.y; w[gate][4 * q + 2] = v.z; w[gate][4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) w[gate][ks] = rp[kperm<KS>(ks, kh)];
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) w[gate][ks] = opnd(w[gate][ks], bf);
    }
    const int gn = tid & 15, gr = tid >> 4;        // gate-phase item: unit gn, row gr (+16 per chunk)
    const int j = ht * 16 + gn;
    float bR[3];
#pragma unroll
    for (int gate = 0; gate < 3; ++gate) bR[gate] = J.bR[ht * 48 + gn * 3 + gate];
    // which wave / register group holds this workgroup's own 16 columns of h_{p-1}
    const int own_wave = (KS % 4 == 0) ? (ht * 16) / WK : -1;
    const int own_q = (KS % 4 == 0) ? ((ht * 16) % WK) / 16 : 0;
    // sequence lengths of the rows this thread touches (A rows: lane&15, gate rows: tid>>4)
    int len_a[2] = {0, 0}, len_g[2] = {0, 0};
    if (J.reverse) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            len_a[c] = a.lens[min(row_beg + 16 * c + n, B - 1)];
            len_g[c] = a.lens[min(row_beg + 16 * c + gr, B - 1)];
        }
    }

    const __amdgpu_buffer_rsrc_t rs_hs = make_rsrc(J.hs), rs_h0 = make_rsrc(J.h0 ? J.h0 : J.hs);
    bool fast = false;
    if (a.p_end - a.p_begin > 1 && !(ab & 16))
        fast = group_same_xcd(a.counters + 64 + jb * a.G + g, a.counters + 128 + (jb * a.G + g) * HT, ht, HT, a.err, a.force_slow);
    if (second_half && a.p_end - a.p_begin > 1) for (int i = 0; i < a.stagger; ++i) __builtin_amdgcn_s_sleep(32);   // stagger x ~1 us
    int buf = 0;
    unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = __builtin_amdgcn_s_memrealtime();
    for (int p = a.p_begin; p < a.p_end; ++p) {
        const bool poll = p > a.p_begin && !(ab & 16);
        for (int rb = row_beg; rb < row_end; rb += 32, buf ^= 1) {
            AVAE_STAMP(7);
            // (1) exchange-independent loads of the gate phase
            float gi[2][3]; int gpos[2]; bool gok[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int row = rb + 16 * c + gr;
                gok[c] = row < row_end;
                gpos[c] = 0;
                gi[c][0] = gi[c][1] = gi[c][2] = 0.f;
                if (gok[c]) {
                    const int len = J.reverse ? (one_sc ? len_g[c] : a.lens[row]) : 0;
                    gpos[c] = pos_map(p, len, J.reverse);
                    if (!(ab & 2)) {
                        const float* gp = J.gi + ((size_t)gpos[c] * B + row) * a.ldg + ht * 48 + gn * 3;
                        gi[c][0] = gp[0]; gi[c][1] = gp[1]; gi[c][2] = gp[2];
                    }
                }
            }
            AVAE_STAMP(0);
            // (2) A operand = h_{p-1} of the group's rows, this wave's K quarter.  Both chunks' loads are issued
            // back to back; chunk 0 is verified and multiplied while chunk 1 is still landing.
            const bool c1 = rb + 16 < row_end;                       // second chunk present (uniform)
            constexpr int NQ = (KS % 4 == 0) ? KS / 4 : 1;
            u32x4 ra[2][NQ];
            float as[2][KS];                                         // scalar path (small test dims only)
            unsigned aoff[2] = {0, 0};
            const bool have = !(ab & 1) && (p > 0 || J.h0 != nullptr);
            const __amdgpu_buffer_rsrc_t rs = (p == 0) ? rs_h0 : rs_hs;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (c == 1 && !c1) break;
                const int row = min(rb + 16 * c + n, B - 1);         // clamped: rows >= B are never stored
                if (p == 0) aoff[c] = (unsigned)((size_t)row * D * 4);
                else {
                    const int len = J.reverse ? (one_sc ? len_a[c] : a.lens[row]) : 0;
                    aoff[c] = (unsigned)((((size_t)pos_map(p - 1, len, J.reverse) * B + row) * a.ldh) * 4);
                }
                aoff[c] += (wave * WK + 4 * kh) * 4;
                if constexpr (KS % 4 == 0) {
                    if (have) frag_issue<NQ>(ra[c], rs, aoff[c]);
                    else {
#pragma unroll
                        for (int q = 0; q < NQ; ++q) ra[c][q] = (u32x4){0u, 0u, 0u, 0u};
                    }
                }
            }
            AVAE_STAMP(1);
            // (3) verify + MFMAs, chunk by chunk
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (c == 1 && !c1) break;
                if constexpr (KS % 4 == 0) {
                    if (poll && have) frag_ensure<NQ>(ra[c], rs, aoff[c], a.err);
                } else {
                    if (have) load_frag_scalar<KS, KS>(as[c], ((p == 0) ? J.h0 : J.hs) + aoff[c] / 4 - 4 * kh, 0, kh, poll, a.err);
                    else {
#pragma unroll
                        for (int ks = 0; ks < KS; ++ks) as[c][ks] = 0.f;
                    }
                }
                auto aval = [&](int ks) -> float {
                    if constexpr (KS % 4 == 0) return __uint_as_float(ra[c][ks >> 2][ks & 3]);
                    else return as[c][ks];
                };
                f32x4 acc[3];
#pragma unroll
                for (int gate = 0; gate < 3; ++gate) acc[gate] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (!(ab & 1)) {
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                        for (int gate = 0; gate < 3; ++gate)
                            acc[gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(opnd(aval(ks), bf), w[gate][ks], acc[gate], 0, 0, 0);
                }
#pragma unroll
                for (int gate = 0; gate < 3; ++gate)
                    *reinterpret_cast<f32x4*>(&part[buf][c][wave][gate][lane * 4]) = acc[gate];
                // (4) own h_{p-1} slice -> LDS: lane (kh*16 + r) holds h[r][k = wave*WK + 16q + 4kh + e]
                if constexpr (KS % 4 == 0) {
                    if (wave == own_wave) {
#pragma unroll
                        for (int q = 0; q < NQ; ++q)
                            if (q == own_q) *reinterpret_cast<u32x4*>(&hps[buf][c][n][4 * kh]) = ra[c][q];
                    }
                } else {
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        int k = wave * WK + kperm<KS>(ks, kh) - ht * 16;
                        if (k >= 0 && k < 16) hps[buf][c][n][k] = as[c][ks];
                    }
                }
            }
            AVAE_STAMP(2);
            __syncthreads();
            AVAE_STAMP(3);
            // (5) gate math: 32 rows x 16 units, two items per thread
            float o_r[2], o_u[2], o_n[2], o_hn[2], o_hp[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (!gok[c]) continue;
                const int row = rb + 16 * c + gr;
                const int pidx = ((gr >> 2) * 16 + gn) * 4 + (gr & 3);
                float gh[3];
#pragma unroll
                for (int gate = 0; gate < 3; ++gate)
                    gh[gate] = bR[gate] + ((part[buf][c][0][gate][pidx] + part[buf][c][1][gate][pidx]) +
                                           (part[buf][c][2][gate][pidx] + part[buf][c][3][gate][pidx]));
                const float hprev = hps[buf][c][gr][gn];
                float r, u, nn, hnew;
                if (ab & 8) { r = 0.5f + 0.1f * (gi[c][0] + gh[0]); u = 0.5f + 0.1f * (gi[c][1] + gh[1]); nn = 0.1f * (gi[c][2] + r * gh[2]); hnew = (1.f - u) * nn + u * hprev; }
                else { const GruCellOut cell = gru_cell(gi[c][0], gi[c][1], gi[c][2], gh[0], gh[1], gh[2], hprev); r = cell.r; u = cell.u; nn = cell.n; hnew = cell.h; }
                // (6) exchanged store first
                float* hdst = J.hs + ((size_t)gpos[c] * B + row) * a.ldh + j;
                if (fast) *hdst = not_sentinel(hnew); else store4_sc1(hdst, not_sentinel(hnew));
                o_r[c] = r; o_u[c] = u; o_n[c] = nn; o_hn[c] = gh[2]; o_hp[c] = hprev;
            }
            AVAE_STAMP(4);
            // stores nobody in this launch waits for
            if (!(ab & 4)) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    if (!gok[c]) continue;
                    const size_t rix = (size_t)gpos[c] * B + (rb + 16 * c + gr);
                    if (J.sv) {
                        *reinterpret_cast<float4*>(J.sv + (rix * HT + ht) * 64 + gn * 4) = make_float4(o_r[c], o_u[c], o_n[c], o_hn[c]);
                    }
                    if (J.hp) J.hp[rix * D + j] = o_hp[c];
                }
            }
            AVAE_STAMP(6);
        }
    }
    if (STAMPS && tid == 0 && a.stamps) {
        for (int i = 0; i < 8; ++i) atomicAdd(a.stamps + i, ph[i]);
        atomicAdd(a.stamps + 8, (unsigned long long)(a.p_end - a.p_begin));
        atomicAdd(a.stamps + 9, (unsigned long long)(fast ? 1 : 0));
        atomicAdd(a.stamps + 10, 1ULL);
    }
}

// ------------------------------------------------------------------------------ forward, D = 512, 32 rows per group
// Software-pipelined form of the same algorithm for the benchmark geometry (two full 16-row chunks per
// workgroup).  Work item = (step, chunk).  The A-operand loads of item i+1 are issued (inline asm, hand
// counted) right after item i's own fragment has been verified, and land while item i runs its MFMAs, LDS
// reduction and gate math: chunk 1 of a step only needs step p-1 data, and chunk 0 of step p+1 needs what every
// workgroup stored one whole item earlier, so the exchange latency leaves the critical path.  A fragment that
// still carries a sentinel is re-loaded in place until complete (same protocol, same bounds).
template <int OFF>
__device__ __forceinline__ void asm_issue8(u32x4 (&v)[8], unsigned voff, i32x4 srd)
{
    asm volatile("buffer_load_dwordx4 %0, %8, %9, 0 offen offset:%c10 sc1\n\t"
                 "buffer_load_dwordx4 %1, %8, %9, 0 offen offset:%c11 sc1\n\t"
                 "buffer_load_dwordx4 %2, %8, %9, 0 offen offset:%c12 sc1\n\t"
                 "buffer_load_dwordx4 %3, %8, %9, 0 offen offset:%c13 sc1\n\t"
                 "buffer_load_dwordx4 %4, %8, %9, 0 offen offset:%c14 sc1\n\t"
                 "buffer_load_dwordx4 %5, %8, %9, 0 offen offset:%c15 sc1\n\t"
                 "buffer_load_dwordx4 %6, %8, %9, 0 offen offset:%c16 sc1\n\t"
                 "buffer_load_dwordx4 %7, %8, %9, 0 offen offset:%c17 sc1"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
                 : "v"(voff), "s"(srd), "i"(OFF), "i"(OFF + 64), "i"(OFF + 128), "i"(OFF + 192), "i"(OFF + 256), "i"(OFF + 320),
                   "i"(OFF + 384), "i"(OFF + 448)
                 : "memory");
}
__device__ __forceinline__ void asm_wait8_all(u32x4 (&v)[8])
{
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]) :: "memory");
}
__device__ __forceinline__ i32x4 make_srd(const float* p)
{
    const unsigned long long pa = (unsigned long long)p;
    return (i32x4){(int)(unsigned)(pa & 0xffffffffULL), (int)(unsigned)((pa >> 32) & 0xffffULL), -1, 0x00020000};
}

__global__ __launch_bounds__(256, 2) void gru_fwd_item_kernel(GruArgs a)
{
    constexpr int KS = 32, D = 512, HT = 32, WK = 128;
    __shared__ __attribute__((aligned(16))) float part[2][4][3][256];   // [item parity][wave][gate][lane*4+reg]
    __shared__ __attribute__((aligned(16))) float hps[2][16][16];       // [item parity][row][unit] own h_{p-1} slice

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, kh = lane >> 4;
    int jb, g, ht;
    const bool second_half = wg_map(a, HT, &jb, &g, &ht);
    const GruJob& J = a.job[jb];
    const int B = a.B;
    const int row_beg = g * 32;

    const bool bf = a.bf16 != 0;                                // bf16-operand mode (see gru_fwd_kernel)
    float w[3][KS];
#pragma unroll
    for (int gate = 0; gate < 3; ++gate) {
        const float* rp = J.R + (size_t)(ht * 48 + n * 3 + gate) * D + wave * WK;
#pragma unroll
        for (int q = 0; q < KS / 4; ++q) {
            float4 v = *reinterpret_cast<const float4*>(rp + 16 * q + 4 * kh);
            w[gate][4 * q + 0] = opnd(v.x, bf); w[gate][4 * q + 1] = opnd(v.y, bf); w[gate][4 * q + 2] = opnd(v.z, bf); w[gate][4 * q + 3] = opnd(v.w, bf);
        }
    }
    const int gn = tid & 15, gr = tid >> 4;
    const int j = ht * 16 + gn;
    float bR[3];
#pragma unroll
    for (int gate = 0; gate < 3; ++gate) bR[gate] = J.bR[ht * 48 + gn * 3 + gate];
    const int own_wave = (ht * 16) / WK, own_q = ((ht * 16) % WK) / 16;
    int len_a[2] = {0, 0}, len_g[2] = {0, 0};
    if (J.reverse) {
#pragma unroll
        for (int c = 0; c < 2; ++c) { len_a[c] = a.lens[row_beg + 16 * c + n]; len_g[c] = a.lens[row_beg + 16 * c + gr]; }
    }
    const i32x4 srd_hs = make_srd(J.hs), srd_h0 = make_srd(J.h0 ? J.h0 : J.hs);
    const bool fast = group_same_xcd(a.counters + 64 + jb * a.G + g, a.counters + 128 + (jb * a.G + g) * HT, ht, HT, a.err, a.force_slow);
    if (second_half) for (int i = 0; i < a.stagger; ++i) __builtin_amdgcn_s_sleep(32);   // stagger x ~1 us

    const int total = 2 * (a.p_end - a.p_begin);
    // byte offset of this lane's first 16-byte piece of the A fragment of item `it`; have == false: zeros
    auto item_off = [&](int it, bool* have, bool* from_h0) -> unsigned {
        const int p = a.p_begin + (it >> 1), c = it & 1;
        const int row = row_beg + 16 * c + n;
        *from_h0 = p == 0;
        *have = p > 0 || J.h0 != nullptr;
        if (p == 0) return (unsigned)((size_t)row * D * 4) + (wave * WK + 4 * kh) * 4;
        return (unsigned)((((size_t)pos_map(p - 1, len_a[c], J.reverse) * B + row) * a.ldh) * 4) + (wave * WK + 4 * kh) * 4;
    };
    u32x4 ra[2][8];
    {
        bool have, h0;
        const unsigned off = item_off(0, &have, &h0);
        if (have) asm_issue8<0>(ra[0], off, h0 ? srd_h0 : srd_hs);
        else {
#pragma unroll
            for (int q = 0; q < 8; ++q) ra[0][q] = (u32x4){0u, 0u, 0u, 0u};
        }
    }
    auto item = [&](int p, auto c_tag) __attribute__((always_inline)) {
        constexpr int c = decltype(c_tag)::value, buf = c;              // two items per step: parity == chunk
        const int it = 2 * (p - a.p_begin) + c;
        u32x4 (&cur)[8] = ra[c];
        // (1) this item's fragment: everything issued so far must have landed; verify, re-load if needed
        {
            bool have, h0;
            const unsigned off = item_off(it, &have, &h0);
            if (have) {
                asm_wait8_all(cur);
                if (p > a.p_begin) {
                    SpinGuard sg;
                    for (;;) {
                        unsigned mx = 0u;
#pragma unroll
                        for (int q = 0; q < 8; ++q) mx = max(max(mx, max(cur[q].x, cur[q].y)), max(cur[q].z, cur[q].w));
                        if (!__any(mx == kSentinel) || sg.expired(a.err)) break;
                        asm_issue8<0>(cur, off, srd_hs);
                        asm_wait8_all(cur);
                    }
                }
            }
        }
        // (2) the next item's fragment goes in flight now
        if (it + 1 < total) {
            bool have, h0;
            const unsigned off = item_off(it + 1, &have, &h0);
            if (have) asm_issue8<0>(ra[c ^ 1], off, h0 ? srd_h0 : srd_hs);
            else {
#pragma unroll
                for (int q = 0; q < 8; ++q) ra[c ^ 1][q] = (u32x4){0u, 0u, 0u, 0u};
            }
        }
        // (3) exchange-independent loads of the gate phase (land behind the MFMAs)
        const int grow = row_beg + 16 * c + gr;
        const int gpos = pos_map(p, len_g[c], J.reverse);
        const float* gp = J.gi + ((size_t)gpos * B + grow) * a.ldg + ht * 48 + gn * 3;
        const float gi0 = gp[0], gi1 = gp[1], gi2 = gp[2];
        // (4) MFMAs
        f32x4 acc[3];
#pragma unroll
        for (int gate = 0; gate < 3; ++gate) acc[gate] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int gate = 0; gate < 3; ++gate)
                acc[gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(opnd(__uint_as_float(cur[ks >> 2][ks & 3]), bf), w[gate][ks], acc[gate], 0, 0, 0);
#pragma unroll
        for (int gate = 0; gate < 3; ++gate)
            *reinterpret_cast<f32x4*>(&part[buf][wave][gate][lane * 4]) = acc[gate];
        if (wave == own_wave) {
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q == own_q) *reinterpret_cast<u32x4*>(&hps[buf][n][4 * kh]) = cur[q];
        }
        __syncthreads();
        // (5) gate math: 16 rows x 16 units, one element per thread; exchanged store first
        {
            const int pidx = ((gr >> 2) * 16 + gn) * 4 + (gr & 3);
            float gh[3];
#pragma unroll
            for (int gate = 0; gate < 3; ++gate)
                gh[gate] = bR[gate] + ((part[buf][0][gate][pidx] + part[buf][1][gate][pidx]) + (part[buf][2][gate][pidx] + part[buf][3][gate][pidx]));
            const float hprev = hps[buf][gr][gn];
            const GruCellOut cell = gru_cell(gi0, gi1, gi2, gh[0], gh[1], gh[2], hprev);
            const float r = cell.r, u = cell.u, nn = cell.n, hnew = cell.h;
            const size_t rix = (size_t)gpos * B + grow;
            float* hdst = J.hs + rix * a.ldh + j;
            if (fast) *hdst = not_sentinel(hnew); else store4_sc1(hdst, not_sentinel(hnew));
            if (J.sv) *reinterpret_cast<float4*>(J.sv + (rix * HT + ht) * 64 + gn * 4) = make_float4(r, u, nn, gh[2]);
            if (J.hp) J.hp[rix * D + j] = hprev;
        }
    };
    for (int p = a.p_begin; p < a.p_end; ++p) {
        item(p, std::integral_constant<int, 0>{});
        item(p, std::integral_constant<int, 1>{});
    }
}

// ------------------------------------------------------------------------------ forward, D = 512, four teams per CU
// The register-resident form above tops out at two chains per CU (96 weight registers per lane allow only
// 2 waves per SIMD) and the matrix pipe sits ~50 % idle while those two chains wait on their exchange.
// Here ONE workgroup of 16 waves owns a (job, 16-unit slice) pair: its 48 x 512 weight slice lives in LDS
// (96 KB, already in MFMA B-fragment order, one ds_read_b128 per gate and four MFMA steps) and is shared by
// FOUR teams of 4 waves; every team runs an independent 16-row chain (its own A fragment, K split over its 4
// waves, partial sums and gate math inside the team).  4 waves per SIMD = four chains to fill the matrix
// pipe.  Teams synchronise through two monotonic LDS counters per team (LDS atomics + LDS polling; never
// s_barrier, which would put the four chains in lock step).  Exchange between workgroups: the same in-band
// sentinel protocol as above.

// PIPE (several row blocks per workgroup): the A fragment of an item is put in flight behind the MFMAs of the item
// before it (another chain, stored an item ago) and only verified at its own item; !PIPE (one row block: the next
// item depends on this one's own stores): polled and loaded at the top of the item.  Two instantiations so that each
// has ONE load site inside the loop -- with two, the register allocator parks the prefetched fragment in other
// registers and copies it at the loop edge, which waits for the loads exactly where they were meant to overlap.
// T teams of KS = 16 / T waves: T = 4 (64 rows per workgroup, K split over 4 waves) where a job fills the chip with 64-row
// blocks, T = 2 (32 rows, K split over 8 waves: half the MFMAs and half the operand bytes per wave and step on the
// latency chain) where it does not, e.g. one decoder layer at B = 256.
// BF (bf16-operand mode, compute_dtype 1): the recurrent product h R' rounds both operands to bf16 like every other
// contraction of that mode -- weights packed as bf16 in LDS (48 KB), v_mfma_f32_16x16x32_bf16 with fp32 accumulation (12
// MFMAs of 16 cycles per wave and item instead of 96 of 32).  The exchange is 16-bit as in the backward (xch16_index: a
// loaded 16-byte piece is the MFMA operand; half the bytes and half the load instructions through the texture addresser),
// with one extra position in front: slot 0 holds h0 (or zeros), written by the launcher (gru_prepare16_kernel), so step 0
// reads its operand like any other step; h_t lands in slot pos + 1.  The state h itself stays fp32: every gate thread keeps
// the h_{t-1} of its (row, unit) in a register (one per row block) instead of picking it out of the exchanged operand; the
// gate math and everything saved stay fp32.
constexpr int kFwdTeamLdsBytes = (96 * 256 + 48 * 256 + 4 * 256) * 4 + 128;      // dynamic LDS of gru_fwd_team_kernel: Wl | part | hps | sync
template <bool DIAG, bool PIPE, int T, bool BF = false, bool CMP = false, bool RING = false>      // CMP: compact external arrays / phantom rows (GruArgs::rowmap, Bx); RING: exchange ring (GruPlan::ring)
__global__ __launch_bounds__(1024, 4) void gru_fwd_team_kernel(GruArgs a)
{
    static_assert(!RING || (!PIPE && !BF && !DIAG), "the exchange ring: fp32, one row block per workgroup");
    const int ab = DIAG ? a.ablate : 0;                     // timing experiments / stamps: diagnostic instantiation only
    constexpr int D = 512, HT = 32, KS = 16 / T, WK = D / KS, NQ = WK / 16, RB = 16 * T;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Wl = lds;                                        // [wk KS][gate 3][q NQ][lane 64][4]    96 KB
    float* part = Wl + 96 * 256;                            // [team T][wk KS][gate 3][256]         48 KB
    float* hps = part + 48 * 256;                           // [team T][16][16]
    unsigned* sync = reinterpret_cast<unsigned*>(hps + T * 256);      // [team T] barrier counters, [team T] exchange-ready epochs

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // wave -> (team, K-split index).  Waves w and w + 4 share a SIMD; a team's K-split partners meet at a barrier every
    // step.  Which SIMDs a team sits on is a 1-3 % effect since the operand loads stopped saturating the texture
    // addresser; the mapping per form is the best of {one SIMD, a SIMD pair, all four} measured in-process
    // (gpurun_out/ab16.log, scripts/ab_classes.py).
    int team, wk;
    // (CMP = the compact layout, i.e. a ragged batch: teams run out of steps at different times and the ones still running should
    //  have every SIMD -- the pipelined forms at 1024 x 64 RAGGED: 32.97 -> 30.37 ms with all four, FULL 59.06 -> 59.88)
    if (T == 4 && PIPE && !CMP) { team = wave & 3; wk = wave >> 2; }                                           // one SIMD
    else if (T == 4)         { team = wave >> 2; wk = wave & 3; }                                              // all four SIMDs (RAGGED 10.56 -> 10.43 ms; FULL unchanged)
    else if (PIPE && !CMP)   { team = (wave >> 1) & 1; wk = (wave & 1) + 2 * (wave >> 2); }                   // a SIMD pair
    else                     { team = (wave >> 2) & 1; wk = (wave & 3) + 4 * (wave >> 3); }                   // all four SIMDs: a team whose partner has run out of steps
                                                                                                               // (ragged batches) has the whole CU: RAGGED 256 x 64 10.76 -> 10.54 ms, FULL 16.50 -> 16.45
    const int n = lane & 15, kh = lane >> 4;
    const TeamMap tm = team_map(a, RB);
    const int cid = tm.cid, ht = tm.ht;
    const GruJob& J = a.job[tm.jb];
    const int Bs = a.B;                           // rows per position of every external array (Bs < B: slots whose perm entry is >= Bs are phantom rows)
    const int B = (CMP && a.Bx > Bs) ? a.Bx : Bs; // rows of the launch geometry: the exchange scratch and everything indexed by slot
    xcd_publish(a.counters + 64 + cid, a.counters + 128 + cid * HT, ht);      // (collected after the weights are in LDS)

    // weights -> LDS in B-fragment order: block (wk', gate, q): lane (n, kh) holds R'[ht*48 + n*3 + gate][wk'*128 + 16q + 4kh ..+3]
    if constexpr (BF) {   // block (wk', gate, q2): lane (n, kh) holds the 8 bf16 R'[ht*48 + n*3 + gate][wk'*WK + 32 q2 + 8 kh + e], e = 0..7
        for (int blk = wave; blk < 48; blk += 16) {
            const int wq = blk / (3 * (NQ / 2)), gate = (blk / (NQ / 2)) % 3, q2 = blk % (NQ / 2);
            const float* rp = J.R + (size_t)(ht * 48 + n * 3 + gate) * D + wq * WK + 32 * q2 + 8 * kh;
            const float4 v0 = *reinterpret_cast<const float4*>(rp), v1 = *reinterpret_cast<const float4*>(rp + 4);
            const u32x4 pk = {pack_bf16(v0.x, v0.y), pack_bf16(v0.z, v0.w), pack_bf16(v1.x, v1.y), pack_bf16(v1.z, v1.w)};
            *reinterpret_cast<u32x4*>(Wl + (size_t)blk * 256 + lane * 4) = pk;
        }
    } else
    for (int blk = wave; blk < 96; blk += 16) {
        const int wq = blk / (3 * NQ), gate = (blk / NQ) % 3, q = blk % NQ;
        const float4 v = *reinterpret_cast<const float4*>(J.R + (size_t)(ht * 48 + n * 3 + gate) * D + wq * WK + 16 * q + 4 * kh);
        *reinterpret_cast<float4*>(Wl + (size_t)blk * 256 + lane * 4) = v;
    }
    if (tid < 2 * T) sync[tid] = 0u;
    const int tt = wk * 64 + lane;                          // thread inside the team; its first 256 threads do the gate math
    const bool gate_thread = tt < 256;
    const int gn = tt & 15, gr = (tt >> 4) & 15;
    const int j = ht * 16 + gn;
    float bR[3];
#pragma unroll
    for (int gate = 0; gate < 3; ++gate) bR[gate] = J.bR[ht * 48 + gn * 3 + gate];
    const int own_wk = (ht * 16) / WK, own_q = ((ht * 16) % WK) / 16;
    const float* __restrict__ p_gi = J.gi;                  // read only, under no other name: its loads need not wait for this item's stores
    const int32_t* __restrict__ p_girows = J.gi_rows;
    float* __restrict__ p_svw = J.sv;                       // written only, under no other name: later loads need not wait for them
    float* __restrict__ p_hpw = J.hp;
    float* __restrict__ p_hsw = J.hs;
    // this job's exchange buffer (tiled, sentinel-filled; BF: S + 1 positions of 16-bit values)
    // exchange ring (gru_dev.h): the value of iteration p (= the step: team launches begin at step 0) in slot p % kGruRing of min(S, kGruRing)
    constexpr bool ring = RING;
    float* const xh = BF ? a.xbuf + (size_t)tm.jb * (a.S + 1) * B * D / 2 : a.xbuf + (size_t)tm.jb * (ring ? min(a.S, kGruRing) : a.S) * B * D;
    const __amdgpu_buffer_rsrc_t rs_hs = make_rsrc(xh), rs_h0 = make_rsrc(J.h0 ? J.h0 : xh);
    const __amdgpu_buffer_rsrc_t rs_gi = make_rsrc(p_gi), rs_hsw = make_rsrc(p_hsw);
    const __amdgpu_buffer_rsrc_t rs_svw = make_rsrc(p_svw ? p_svw : p_hsw), rs_hpw = make_rsrc(p_hpw ? p_hpw : p_hsw);
    // bf16 mode: the row-major h / h_prev copies as bf16 INSTEAD of fp32 where the caller gave 16-bit arrays (the next layer's
    // GEMM operand and the dR GEMM's operand as they stand: no conversion pass, half the bytes)
    unsigned short* __restrict__ p_hs16 = BF ? J.hs16 : nullptr;
    unsigned short* __restrict__ p_hp16 = BF ? J.hp16 : nullptr;
    const __amdgpu_buffer_rsrc_t rs_hs16 = make_rsrc(reinterpret_cast<const float*>(p_hs16 ? p_hs16 : reinterpret_cast<unsigned short*>(p_hsw)));
    const __amdgpu_buffer_rsrc_t rs_hp16 = make_rsrc(reinterpret_cast<const float*>(p_hp16 ? p_hp16 : reinterpret_cast<unsigned short*>(p_hsw)));
    auto to_bf16 = [](float v) -> unsigned short { return (unsigned short)(pack_bf16(v, 0.f) & 0xffffu); };
    const bool fast = group_same_xcd(a.counters + 64 + cid, a.counters + 128 + cid * HT, ht, HT, a.err, a.force_slow, true);   // has a __syncthreads
    float* tpart = part + team * (KS * 3 * 256);
    float* thps = hps + team * 256;
    unsigned* tsync = sync + team;
    unsigned* ready = sync + T + team;
    unsigned epoch = 0;
    // de-phase the four chains: identical chains started together stay in lock step and collide on the matrix
    // pipe; an initial offset of a fraction of a step per team persists (equal periods)
    // one consistent arbitration order on all four SIMDs: a team's K-split partners sit on different SIMDs and
    // meet at the team barrier, so if every SIMD serves the teams in the same order the partners finish together
    // (otherwise the barrier pays the arbitration skew, measured at 2-3 us per step)
    if (ab & 256) { } else {
        const int tq = __builtin_amdgcn_readfirstlane(team);
        if (tq == 0) __builtin_amdgcn_s_setprio(3);
        else if (tq == 1) __builtin_amdgcn_s_setprio(2);
        else if (tq == 2) __builtin_amdgcn_s_setprio(1);
    }

    const bool stamp = (ab & 128) != 0;                        // diagnostic phase stamps (never in timed runs)
    unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = __builtin_amdgcn_s_memrealtime();
#define TSTAMP(i) do { if (stamp) { unsigned long long t_ = __builtin_amdgcn_s_memrealtime(); ph[i] += t_ - tprev; tprev = t_; } } while (0)
    // Work item = (step p, row block r).  With more than one row block per workgroup a team's next item belongs to
    // another chain, whose operands every producer stored a whole item ago: the exchange latency of one chain hides
    // behind the MFMAs of the others (software pipelining over the row blocks; time is then linear in rows at the
    // matrix-pipe rate instead of at the chain latency).
    unsigned it = 0;                                          // items done so far (monotonic; LDS epochs derive from it)
    constexpr int NQA = BF ? NQ / 2 : NQ;                    // 16-byte pieces of the A fragment per lane
    u32x4 ra[NQA];
    float hc = 0.f, hc0 = 0.f, hc1 = 0.f, hc2 = 0.f, hc3 = 0.f;      // BF: this thread's h_{t-1} (!PIPE: one row block; PIPE: per row block)
    // byte offset of this lane's first 16-byte piece: step 0 reads the row-major h0 (pieces 64 B apart), later steps
    // the tiled exchange (pieces 1 KB apart); BF: always the exchange, whose slot 0 holds h0
    const int* const lens_by_slot = a.slens ? a.slens : a.lens;      // (rows permuted: lengths by slot)
    const int* const perm = a.perm;                                  // slot -> batch row of every external array (nullptr: identity)
    auto a_offset = [&](int p, int row0, int len_a) -> unsigned {
        if constexpr (BF) return xch_lane_offset(p == 0 ? 0 : pos_map(p - 1, len_a, J.reverse) + 1, row0, wk * (WK / 8), n, kh, B, D / 2);
        if (p == 0) return (unsigned)((size_t)(CMP ? min(perm ? perm[row0 + n] : row0 + n, Bs - 1) : (perm ? perm[row0 + n] : row0 + n)) * D * 4) + (wk * WK + 4 * kh) * 4;      // (row-major h0: an external array; a phantom row reads the last real one's)
        return xch_lane_offset(ring ? ((p - 1) & (kGruRing - 1)) : pos_map(p - 1, len_a, J.reverse), row0, wk * (WK / 4), n, kh, B, D);
    };
    auto q_stride = [&](int p) -> unsigned { return (p == 0 && !BF) ? 64u : 1024u; };
    auto next_frag = [&](int p2, int r2, int len2) __attribute__((always_inline)) {   // PIPE: issue (or zero) the fragment of item (p2, r2)
        if (BF || p2 > 0 || J.h0 != nullptr) {
            const int row2 = (tm.slot + r2 * tm.cpj) * RB + team * 16;
            frag_issue<NQA>(ra, (p2 == 0 && !BF) ? rs_h0 : rs_hs, a_offset(p2, row2, len2), q_stride(p2));
        } else {
#pragma unroll
            for (int q = 0; q < NQA; ++q) ra[q] = (u32x4){0u, 0u, 0u, 0u};
        }
    };
    // sequence lengths of the rows this lane touches in the current item (A rows: n, gate rows: tid's row)
    int len_a = J.reverse ? lens_by_slot[tm.slot * RB + team * 16 + n] : 0, len_g = J.reverse ? lens_by_slot[tm.slot * RB + team * 16 + gr] : 0;
    const int len_p0 = J.reverse ? lens_by_slot[tm.slot * RB + team * 16 + 15] : 0;      // the probe's row (last of the team's 16)
    // steps of this team's row blocks (padding skipped, see team_steps): non-increasing over r
    int nst0 = a.p_end, nst1 = a.p_end, nst2 = a.p_end, nst3 = a.p_end;
    if (a.slens) {
        nst3 = tm.nrb > 3 ? min(a.p_end, team_steps(a.slens, (tm.slot + 3 * tm.cpj) * RB + team * 16, lane)) : 0;
        nst2 = tm.nrb > 2 ? max(nst3, min(a.p_end, team_steps(a.slens, (tm.slot + 2 * tm.cpj) * RB + team * 16, lane))) : 0;
        nst1 = tm.nrb > 1 ? max(nst2, min(a.p_end, team_steps(a.slens, (tm.slot + 1 * tm.cpj) * RB + team * 16, lane))) : 0;
        nst0 = max(nst1, min(a.p_end, team_steps(a.slens, tm.slot * RB + team * 16, lane)));
    }
    auto nst_of = [&](int r) -> int { return r == 0 ? nst0 : (r == 1 ? nst1 : (r == 2 ? nst2 : nst3)); };
    const int p_stop = nst0;                                    // (= a.p_end without slens)
    int ge_cur = tm.slot * RB + team * 16 + gr;                 // batch row of this thread's gate row in the current item
    if (perm) ge_cur = perm[ge_cur];
    const int* const rowmap = CMP ? a.rowmap : nullptr;       // (pos * B + row) -> row of the COMPACT external arrays, -1 for a padding position (nullptr: padded layout)
    if (a.slens && gate_thread && !rowmap) {
        // positions behind a row block's steps: zeros in the row-major outputs (the GEMMs over all rows read them)
        for (int r = 0; r < tm.nrb; ++r) {
            const int gs = (tm.slot + r * tm.cpj) * RB + team * 16 + gr, ge = perm ? perm[gs] : gs;
            for (int p = nst_of(r); p < a.p_end; ++p) {
                const unsigned rix = (unsigned)p * (unsigned)Bs + (unsigned)ge;
                if (BF && p_hs16) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)0, rs_hs16, (int)((rix * (unsigned)a.ldh + j) * 2u), 0, 0);
                else bstore1(0.f, rs_hsw, (rix * (unsigned)a.ldh + j) * 4u);
                if (BF && p_hp16) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)0, rs_hp16, (int)((rix * D + j) * 2u), 0, 0);
                else if (p_hpw) bstore1(0.f, rs_hpw, (rix * D + j) * 4u);
            }
        }
    }
    if constexpr (PIPE) { if (a.p_begin < p_stop) next_frag(a.p_begin, 0, len_a); }
    for (int p = a.p_begin; p < p_stop; ++p) {
      for (int r = 0; r < tm.nrb && p < nst_of(r); ++r, ++it) {
        TSTAMP(5);
        const int row0 = (tm.slot + r * tm.cpj) * RB + team * 16;     // this team's 16 rows of row block r
        const bool poll = p > a.p_begin && !(ab & 16);            // ablate 16: timing experiment, wrong results
        // (1) exchange-independent loads of the gate phase
        const int grow = row0 + gr;                               // slot (exchange index); ge_cur: the batch row (external arrays)
        const int gpos = pos_map(p, len_g, J.reverse);
        const unsigned prix = (unsigned)gpos * (unsigned)Bs + (unsigned)ge_cur;     // (byte offsets below 2^32: team_geometry checks)
        // compact layout: every external array but a table-fed layer's row index is addressed by the row's place among the REAL
        // positions; a padding position of a row shorter than its team's longest -- and every position of a phantom row -- takes
        // part in the exchange only
        const int crow = (rowmap && gate_thread) ? (ge_cur < Bs ? rowmap[prix] : -1) : (int)prix;
        const bool real = !CMP || crow >= 0;
        const unsigned rix = (unsigned)crow;
        float gi0 = 0.f, gi1 = 0.f, gi2 = 0.f, h0_own = 0.f;
        if (gate_thread && real) {
            const unsigned grix = p_girows ? (unsigned)p_girows[prix] : rix;         // (table-fed layer: the row of the per-id projection)
            const u32x3 g3 = __builtin_amdgcn_raw_buffer_load_b96(rs_gi, (int)((grix * (unsigned)a.ldg + ht * 48 + gn * 3) * 4u), 0, 0);
            gi0 = __uint_as_float(g3.x); gi1 = __uint_as_float(g3.y); gi2 = __uint_as_float(g3.z);
            if constexpr (BF) { if (p == 0 && J.h0 != nullptr) h0_own = bload1(rs_h0, ((unsigned)ge_cur * D + j) * 4u); }
        }
        // PIPE: the item after this one (its row lengths are fetched now, long before they are needed)
        const bool same_p = r + 1 < tm.nrb && p < nst_of(r + 1);
        const int r2 = same_p ? r + 1 : 0, p2 = same_p ? p : p + 1;
        int len2 = len_a, len2g = len_g, ge2 = ge_cur;
        if constexpr (PIPE) {
            if (p2 < p_stop) {
                const int row2 = (tm.slot + r2 * tm.cpj) * RB + team * 16;
                if (J.reverse) { len2 = lens_by_slot[row2 + n]; len2g = lens_by_slot[row2 + gr]; }
                ge2 = perm ? perm[row2 + gr] : row2 + gr;
            }
        }
        // (2) A operand: this wave's K quarter of the team's 16 rows
        const bool have = BF || p > 0 || J.h0 != nullptr;
        if (have) {
            const unsigned aoff = a_offset(p, row0, len_a);
            const __amdgpu_buffer_rsrc_t rs = (p == 0 && !BF) ? rs_h0 : rs_hs;
            if constexpr (!PIPE) {
                // GruArgs::spec (few rows alive per step: the step is the latency of one chain, the texture addresser is idle): the
                // fragment is loaded at once, WITHOUT the probe's round trip in front of it; complete -> the step goes on one L2
                // round trip earlier.  A wave whose fragment still carries a sentinel takes the polling path below.
                bool got = false;
                if (poll && a.spec) {
                    frag_issue<NQA>(ra, rs, aoff, q_stride(p));
                    if constexpr (BF) got = !frag_bad16<NQA>(ra); else got = !frag_bad<NQA>(ra);
                }
                if (poll) {
                    // ONE wave per team polls the exchange and releases its three K-split partners through an LDS
                    // word: four independent polls would leave the partners up to a poll period (~1 us) apart and
                    // the team barrier pays that skew.  The probe (lane l reads the last element producer l&31
                    // stores for these 16 rows: one 256-byte request per poll) is a start signal only; every wave
                    // still verifies its own fragment dword by dword below.
                    if (wk == 0) {
                        if (!got) {
                        const int prow = row0 + 15;
                        const int plen = len_p0;                     // (!PIPE: one row block, fetched once before the loop)
                        const float* pp = BF ? xh + (xch16_index(pos_map(p - 1, plen, J.reverse) + 1, prow, (lane & 31) * 16 + 15, B, D) >> 1)      // (the high half of its dword)
                                             : xh + xch_index(ring ? ((p - 1) & (kGruRing - 1)) : pos_map(p - 1, plen, J.reverse), prow, (lane & 31) * 16 + 15, B, D);
                        SpinGuard sg;
                        while (__any(BF ? (load4_sc1(pp) >> 16) == 0xffffu : load4_sc1(pp) == kSentinel) && !sg.expired(a.err)) { }
                        }
                        if (lane == 0) __hip_atomic_store(ready, it + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    } else if (!got) {
                        while (__hip_atomic_load(ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < it + 1u) __builtin_amdgcn_s_sleep(1);
                    }
                }
                if (!got) frag_issue<NQA>(ra, rs, aoff, q_stride(p));
            }
            if (poll) { if constexpr (BF) frag_ensure16<NQA>(ra, rs, aoff, a.err, q_stride(p)); else frag_ensure<NQA>(ra, rs, aoff, a.err, q_stride(p)); }
        } else if constexpr (!PIPE) {
#pragma unroll
            for (int q = 0; q < NQA; ++q) ra[q] = (u32x4){0u, 0u, 0u, 0u};
        }
        TSTAMP(0);
        // (3) MFMAs, B fragments from LDS
        f32x4 acc[3];
#pragma unroll
        for (int gate = 0; gate < 3; ++gate) acc[gate] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if constexpr (BF) {
#pragma unroll
            for (int q2 = 0; q2 < NQ / 2; ++q2) {
                const bf16x8 a8 = __builtin_bit_cast(bf16x8, ra[q2]);       // a loaded 16-byte piece is the operand as it stands
#pragma unroll
                for (int gate = 0; gate < 3; ++gate) {
                    const bf16x8 b8 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(Wl + (size_t)((wk * 3 + gate) * (NQ / 2) + q2) * 256 + lane * 4));
                    acc[gate] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a8, b8, acc[gate], 0, 0, 0);
                }
            }
        } else
        {   // B fragments one q ahead of their MFMAs (see the backward)
            f32x4 bn[3];
#pragma unroll
            for (int gate = 0; gate < 3; ++gate)
                bn[gate] = *reinterpret_cast<const f32x4*>(Wl + (size_t)((wk * 3 + gate) * NQ + 0) * 256 + lane * 4);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                f32x4 b[3];
#pragma unroll
                for (int gate = 0; gate < 3; ++gate) b[gate] = bn[gate];
                if (q + 1 < NQ) {
#pragma unroll
                    for (int gate = 0; gate < 3; ++gate)
                        bn[gate] = *reinterpret_cast<const f32x4*>(Wl + (size_t)((wk * 3 + gate) * NQ + q + 1) * 256 + lane * 4);
                }
                __builtin_amdgcn_sched_barrier(0);              // (the scheduler otherwise sinks the reads back to their use)
#pragma unroll
                for (int e = 0; e < 4; ++e)            // gates interleaved: consecutive MFMAs hit different accumulators
#pragma unroll
                    for (int gate = 0; gate < 3; ++gate)
                        acc[gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ra[q][e]), b[gate][e], acc[gate], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        TSTAMP(1);
        // every wave of the team has finished READING the previous item's partial sums (second team barrier
        // of that item, taken here so that it costs nothing), then publish this item's
        if (it > 0) { epoch += KS; team_barrier(tsync, epoch); }
        TSTAMP(6);
#pragma unroll
        for (int gate = 0; gate < 3; ++gate)
            *reinterpret_cast<f32x4*>(tpart + (wk * 3 + gate) * 256 + lane * 4) = acc[gate];
        if constexpr (!BF) {
            if (wk == own_wk) {
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    if (q == own_q) *reinterpret_cast<u32x4*>(thps + n * 16 + 4 * kh) = ra[q];
            }
        }
        // (3b) PIPE: the NEXT item is another chain, whose operand every producer stored an item ago.  Its loads go in
        // flight now, into the registers the MFMAs have just released, and land behind the team barrier and the gate
        // math (unverified here: the sentinel check of (2) still decides).
        if constexpr (PIPE) {
            // (every load issued so far is retired HERE, on purpose: hipcc's waitcnt insertion merges the two sides of
            //  the branch below conservatively and would otherwise wait for the new fragment at the first use of gi)
            asm volatile("" :: "v"(gi0), "v"(gi1), "v"(gi2), "v"(h0_own), "v"(len2), "v"(len2g), "v"(ge2));
            __builtin_amdgcn_sched_barrier(0);
            if (p2 < p_stop) next_frag(p2, r2, len2);
            __builtin_amdgcn_sched_barrier(0);
        }
        TSTAMP(7);
        epoch += KS; team_barrier(tsync, epoch);
        TSTAMP(2);
        // (4) gate math: the team's 256 threads, one element each; exchanged store first
        if (gate_thread) {
            const int pidx = ((gr >> 2) * 16 + gn) * 4 + (gr & 3);
            float gh[3];
#pragma unroll
            for (int gate = 0; gate < 3; ++gate) {
                float s4[4] = {0.f, 0.f, 0.f, 0.f};          // K-split partial sums, the order of the 4-wave form: ((0+1)+(2+3))
#pragma unroll
                for (int k = 0; k < KS; ++k) s4[k & 3] += tpart[(k * 3 + gate) * 256 + pidx];
                gh[gate] = bR[gate] + ((s4[0] + s4[1]) + (s4[2] + s4[3]));
            }
            float hprev;
            if constexpr (BF) {     // the fp32 state of this (row, unit): in a register since the step before (step 0: h0 or zero)
                if (p == 0) hprev = h0_own;
                else if constexpr (PIPE) hprev = r == 0 ? hc0 : (r == 1 ? hc1 : (r == 2 ? hc2 : hc3));
                else hprev = hc;
            } else hprev = thps[gr * 16 + gn];
            const GruCellOut cell = gru_cell(gi0, gi1, gi2, gh[0], gh[1], gh[2], hprev);
            const float r_ = cell.r, u = cell.u, nn = cell.n, hnew = cell.h;
            if constexpr (BF) {      // exchanged store first: bf16, slot gpos + 1
                const unsigned xo = xch16_index(gpos + 1, grow, j, B, D) * 2u;
                if (fast) __builtin_amdgcn_raw_buffer_store_b16(bf16_not_sentinel(hnew), rs_hs, (int)xo, 0, 0);
                else __builtin_amdgcn_raw_buffer_store_b16(bf16_not_sentinel(hnew), rs_hs, (int)xo, 0, 16);
                if constexpr (PIPE) { if (r == 0) hc0 = hnew; else if (r == 1) hc1 = hnew; else if (r == 2) hc2 = hnew; else hc3 = hnew; }
                else hc = hnew;
            } else {
                const unsigned xo = xch_index(ring ? (p & (kGruRing - 1)) : gpos, grow, j, B, D) * 4u;      // exchanged store first
                if (fast) bstore1(not_sentinel(hnew), rs_hs, xo); else bstore1_sc1(not_sentinel(hnew), rs_hs, xo);
            }
            if (real) {
            if (BF && p_hs16) __builtin_amdgcn_raw_buffer_store_b16(to_bf16(hnew), rs_hs16, (int)((rix * (unsigned)a.ldh + j) * 2u), 0, 0);
            else bstore1(hnew, rs_hsw, (rix * (unsigned)a.ldh + j) * 4u);       // the row-major copy the GEMMs and the next layer read
            if (p_svw) {
                if (BF && a.sv16) {     // saved gates as bf16 (same index in halfwords): half the bytes here and in the BPTT's reads
                    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                    const u32x2 s2 = {pack_bf16(r_, u), pack_bf16(nn, gh[2])};
                    __builtin_amdgcn_raw_buffer_store_b64(s2, rs_svw, (int)(((rix * HT + ht) * 64 + gn * 4) * 2u), 0, 0);
                } else bstore4(r_, u, nn, gh[2], rs_svw, ((rix * HT + ht) * 64 + gn * 4) * 4u);
            }
            if (BF && p_hp16) __builtin_amdgcn_raw_buffer_store_b16(to_bf16(hprev), rs_hp16, (int)((rix * D + j) * 2u), 0, 0);
            else if (p_hpw) bstore1(hprev, rs_hpw, (rix * D + j) * 4u);
            }
        }
        // exchange ring: the slot that held iteration p - 2 is dead behind the team barrier above; the team's last K-split wave (T = 2: one
        // that sits out the gate math) re-arms this workgroup's slice of it for iteration p + 2 (gru_dev.h xch_rearm).  The first two
        // re-arms would hit slots the launcher armed.
        if constexpr (RING) {
            if (wk == KS - 1 && p >= 2 && p + 2 < p_stop) xch_rearm<1>(rs_hs, (p + 2) & (kGruRing - 1), row0, ht * 4, lane, B, D, fast);
        }
        len_a = len2; len_g = len2g; ge_cur = ge2;
        TSTAMP(3);
      }
    }
    if (stamp && tt == 0 && a.stamps) {
        for (int i = 0; i < 8; ++i) atomicAdd(a.stamps + i, ph[i]);
        atomicAdd(a.stamps + 8, (unsigned long long)(a.p_end - a.p_begin));
        atomicAdd(a.stamps + 10, 1ULL);
    }
#undef TSTAMP
}

// ------------------------------------------------------------------------------ backward
// step p (descending):  dH_p = dh_out[p] + dH_{p+1} u_{p+1} + dgh_{p+1} R'
//   dn = dH (1-u)(1-n^2)   du = dH (h_{p-1} - n) u (1-u)   dr = dn hn r (1-r)
//   dgi = [dr,du,dn]   dgh = [dr,du,dn r]
// dgh is the exchanged buffer (sentinel-filled by the launcher).  The bias gradients (column sums
// of dgi / dgh over all rows and steps) are accumulated in registers across the whole launch and
// leave through one LDS reduction + 96 float atomics.
template <int KS, bool STAMPS>
__global__ __launch_bounds__(256, 2) void gru_bwd_kernel(GruArgs a)
{
    constexpr int D = 16 * KS, HT = KS, NKS = 3 * KS;   // wave K range = 3D/4 = 12*KS floats
    __shared__ __attribute__((aligned(16))) float part[2][2][4][256];
    __shared__ float red[4][16];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, kh = lane >> 4;
    int jb, g, ht;
    const bool second_half = wg_map(a, HT, &jb, &g, &ht);
    const GruJob& J = a.job[jb];
    const int B = a.B, S = a.S;
    const int row_beg = g * a.rows_per_group;
    const int row_end = min(B, row_beg + a.rows_per_group);
    const int ab = STAMPS ? a.ablate : 0;
    const bool one_sc = row_end - row_beg <= 32;

    // B operand: B[k = c'][n] = R'[c'][ht*16 + n]
    const bool bf = a.bf16 != 0;                                // bf16-operand mode (see gru_fwd_kernel)
    float w[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
        w[ks] = opnd(J.R[(size_t)(wave * 12 * KS + kperm<NKS>(ks, kh)) * D + ht * 16 + n], bf);

    const int gn = tid & 15, gr = tid >> 4;
    const int j = ht * 16 + gn;
    int len_a[2] = {0, 0}, len_g[2] = {0, 0};
    if (J.reverse) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            len_a[c] = a.lens[min(row_beg + 16 * c + n, B - 1)];
            len_g[c] = a.lens[min(row_beg + 16 * c + gr, B - 1)];
        }
    }
    const bool want_dh0 = (J.dh0 != nullptr) && a.p_begin == 0;
    const int p_last = want_dh0 ? -1 : a.p_begin;       // p == -1: only dh0 = carry + dgh_0 R'
    const __amdgpu_buffer_rsrc_t rs_dgh = make_rsrc(J.dgh);
    float sb_r = 0.f, sb_u = 0.f, sb_n = 0.f, sb_nr = 0.f;   // bias-gradient partial sums
    bool fast = false;
    if (a.p_end - 1 > p_last && !(ab & 16))
        fast = group_same_xcd(a.counters + 64 + jb * a.G + g, a.counters + 128 + (jb * a.G + g) * HT, ht, HT, a.err, a.force_slow);
    if (second_half && a.p_end - 1 > p_last) for (int i = 0; i < a.stagger; ++i) __builtin_amdgcn_s_sleep(32);   // stagger x ~1 us
    int buf = 0, done = 0;
    unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = __builtin_amdgcn_s_memrealtime();
    for (int p = a.p_end - 1; p >= p_last; --p, ++done) {
        const bool have_next = (p + 1 < S);
        const bool poll = done > 0 && !(ab & 16);
        for (int rb = row_beg; rb < row_end; rb += 32, buf ^= 1) {
            AVAE_STAMP(7);
            // (1) exchange-independent loads of the gate phase
            float s_r[2], s_u[2], s_n[2], s_hn[2], s_hp[2], s_do[2]; int rix[2]; bool gok[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int row = rb + 16 * c + gr;
                gok[c] = row < row_end && p >= 0;
                rix[c] = 0; s_r[c] = s_u[c] = s_n[c] = s_hn[c] = s_hp[c] = s_do[c] = 0.f;
                if (gok[c]) {
                    const int len = J.reverse ? (one_sc ? len_g[c] : a.lens[row]) : 0;
                    rix[c] = pos_map(p, len, J.reverse) * B + row;
                    if (!(ab & 2)) {
                        const float4 sv = *reinterpret_cast<const float4*>(J.sv + ((size_t)rix[c] * HT + ht) * 64 + gn * 4);
                        s_r[c] = sv.x; s_u[c] = sv.y; s_n[c] = sv.z; s_hn[c] = sv.w;
                        s_hp[c] = J.hp[(size_t)rix[c] * D + j];
                        if (J.dh_out) s_do[c] = J.dh_out[(size_t)rix[c] * a.ldh + j];
                    }
                }
            }
            AVAE_STAMP(0);
            const bool c1 = rb + 16 < row_end;
            // (2)+(3) A operand = dgh_{p+1} rows (K = 3D, this wave's quarter) streamed in pieces through a ring
            // of NB register buffers: the loads of piece st+NB-1 are issued BEFORE piece st is verified, so
            // NB-1 pieces are always in flight behind the MFMAs of the current one (counted waits on the fast
            // path; a piece that still carries sentinels is re-loaded in place until complete).
            constexpr int NH = (NKS % 16 == 0) ? 4 : ((NKS % 8 == 0) ? 2 : 1);   // pieces per chunk
            constexpr int HK = NKS / NH;                                          // MFMA steps per piece
            constexpr int PQ = (NKS % 4 == 0) ? HK / 4 : 1;                       // 16-byte loads per piece and lane
            constexpr int NB = 3;
            u32x4 hv[NB][PQ];
            float hs_[HK];                                                        // scalar path (small test dims)
            auto piece_off = [&](int c, int hf) -> unsigned {
                const int row = min(rb + 16 * c + n, B - 1);
                const int len = J.reverse ? (one_sc ? len_a[c] : a.lens[row]) : 0;
                const int pos1 = pos_map(p + 1, len, J.reverse);
                return (unsigned)((((size_t)pos1 * B + row) * a.ldg + wave * 12 * KS + hf * 4 * HK) * 4);
            };
            const bool do_mm = have_next && !(ab & 1);
            const int nstage = (c1 ? 2 : 1) * NH;                     // (chunk, piece) stages, uniform
            f32x4 acc[4];
            // D = 512 fast form.  (a) A one-instruction probe -- lane l reads the last element producer l&31
            // stores for chunk l>>5 -- is polled until no sentinel is left: a HEURISTIC start signal (the stores
            // of one producer are unordered).  (b) The whole A operand then streams through the register ring
            // in straight-line code with hand-counted waits, so two pieces stay in flight behind the MFMAs of
            // the current one, while every loaded dword is also compared with the sentinel.  (c) If any lane of
            // the wave saw one, the partial sums are discarded and the pass repeats (bounded).  Correctness
            // rests on (b)+(c) only.
            if constexpr (KS == 32) {
                if (!do_mm) {
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                        if (c == 0 || c1) *reinterpret_cast<f32x4*>(&part[buf][c][wave][lane * 4]) = (f32x4){0.f, 0.f, 0.f, 0.f};
                } else {
                    const unsigned long long pa = (unsigned long long)J.dgh;
                    const i32x4 srd = {(int)(unsigned)(pa & 0xffffffffULL), (int)(unsigned)((pa >> 32) & 0xffffULL), -1, 0x00020000};
                    const unsigned voff0 = piece_off(0, 0) + 16 * kh, voff1 = c1 ? piece_off(1, 0) + 16 * kh : voff0;
                    auto pass = [&](auto nst_tag) __attribute__((always_inline)) -> bool {
                        constexpr int NST = decltype(nst_tag)::value;       // 4 (one chunk) or 8 (two chunks)
                        unsigned mx = 0u;
                        asm_issue6<0>(hv[0], voff0, srd);
                        asm_issue6<384>(hv[1], voff0, srd);
#pragma unroll
                        for (int st = 0; st < NST; ++st) {
                            const int c = st / NH, hf = st % NH;
                            if (st + 2 < NST) {
                                const unsigned vo = ((st + 2) / NH) ? voff1 : voff0;
                                if ((st + 2) % NH == 0) asm_issue6<0>(hv[(st + 2) % NB], vo, srd);
                                if ((st + 2) % NH == 1) asm_issue6<384>(hv[(st + 2) % NB], vo, srd);
                                if ((st + 2) % NH == 2) asm_issue6<768>(hv[(st + 2) % NB], vo, srd);
                                if ((st + 2) % NH == 3) asm_issue6<1152>(hv[(st + 2) % NB], vo, srd);
                            }
                            if (st + 2 < NST) asm_wait6<12>(hv[st % NB]);
                            else if (st + 1 < NST) asm_wait6<6>(hv[st % NB]);
                            else asm_wait6<0>(hv[st % NB]);
                            if (hf == 0) {
#pragma unroll
                                for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
                            }
                            // sentinel = the largest unsigned value: keep a running maximum of every loaded dword
                            // (pinned here so that the ring registers die before their buffer is re-loaded)
#pragma unroll
                            for (int q = 0; q < PQ; ++q)
                                mx = max(max(mx, max(hv[st % NB][q].x, hv[st % NB][q].y)), max(hv[st % NB][q].z, hv[st % NB][q].w));
                            asm volatile("" : "+v"(mx));
#pragma unroll
                            for (int ks = 0; ks < HK; ++ks)
                                acc[ks & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(opnd(__uint_as_float(hv[st % NB][ks >> 2][ks & 3]), bf),
                                                                                   w[ks + hf * HK], acc[ks & 3], 0, 0, 0);
                            if (hf == NH - 1) {
                                f32x4 s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
                                *reinterpret_cast<f32x4*>(&part[buf][c][wave][lane * 4]) = s;
                            }
                        }
                        return __any(mx == kSentinel);
                    };
                    SpinGuard sg;
                    for (;;) {
                        if (poll) {
                            const int pc = c1 ? (lane >> 5) : 0, prow = min(min(rb + 16 * pc + 15, row_end - 1), B - 1);
                            const int plen = J.reverse ? a.lens[prow] : 0;
                            const float* pp = J.dgh + ((size_t)pos_map(p + 1, plen, J.reverse) * B + prow) * a.ldg + (lane & 31) * 48 + 47;
                            while (__any(load4_sc1(pp) == kSentinel) && !sg.expired(a.err)) { }
                        }
                        const bool bad = c1 ? pass(std::integral_constant<int, 2 * NH>{}) : pass(std::integral_constant<int, NH>{});
                        if (!poll || !bad || sg.expired(a.err)) break;
                    }
                }
            } else {
            if constexpr (NKS % 4 == 0) {
                if (do_mm) {
#pragma unroll
                    for (int s0 = 0; s0 < NB - 1; ++s0)
                        if (s0 < nstage) frag_issue<PQ>(hv[s0], rs_dgh, piece_off(s0 / NH, s0 % NH) + 16 * kh);
                }
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
#pragma unroll
                for (int hf = 0; hf < NH; ++hf) {
                    const int st = c * NH + hf;                     // compile-time after unrolling
                    if (st < nstage) {
                        if (hf == 0) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
                        }
                        if (do_mm) {
                            if constexpr (NKS % 4 == 0) {
                                if (st + NB - 1 < nstage)
                                    frag_issue<PQ>(hv[(st + NB - 1) % NB], rs_dgh, piece_off((st + NB - 1) / NH, (st + NB - 1) % NH) + 16 * kh);
                                if (poll) frag_ensure<PQ>(hv[st % NB], rs_dgh, piece_off(c, hf) + 16 * kh, a.err);
#pragma unroll
                                for (int ks = 0; ks < HK; ++ks)
                                    acc[ks & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(opnd(__uint_as_float(hv[st % NB][ks >> 2][ks & 3]), bf),
                                                                                       w[ks + hf * HK], acc[ks & 3], 0, 0, 0);
                            } else {
                                load_frag_scalar<HK, NKS>(hs_, J.dgh + piece_off(c, 0) / 4, hf * HK, kh, poll, a.err);
#pragma unroll
                                for (int ks = 0; ks < HK; ++ks)
                                    acc[ks & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(opnd(hs_[ks], bf), w[ks + hf * HK], acc[ks & 3], 0, 0, 0);
                            }
                        }
                        if (hf == NH - 1) {
                            f32x4 s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
                            *reinterpret_cast<f32x4*>(&part[buf][c][wave][lane * 4]) = s;
                        }
                    }
                }
            }
            }   // KS != 32: compiler-tracked form
            AVAE_STAMP(2);
            __syncthreads();
            AVAE_STAMP(3);
            float o_dr[2], o_du[2], o_dn[2], o_car[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int row = rb + 16 * c + gr;
                if (row >= row_end) continue;
                const int pidx = ((gr >> 2) * 16 + gn) * 4 + (gr & 3);
                float carried = (part[buf][c][0][pidx] + part[buf][c][1][pidx]) + (part[buf][c][2][pidx] + part[buf][c][3][pidx]);
                float* carryp = J.carry + (size_t)row * D + j;
                if (have_next) carried += *carryp;
                if (p < 0) { J.dh0[(size_t)row * D + j] = carried; continue; }
                const float dH = carried + s_do[c];
                const float r = s_r[c], u = s_u[c], nn = s_n[c];
                const float dn = dH * (1.f - u) * (1.f - nn * nn);
                const float du = dH * (s_hp[c] - nn) * u * (1.f - u);
                const float dr = dn * s_hn[c] * r * (1.f - r);
                float* dgh = J.dgh + (size_t)rix[c] * a.ldg + ht * 48 + gn * 3;
                const float x0 = not_sentinel(dr), x1 = not_sentinel(du), x2 = not_sentinel(dn * r);
                if (fast) { dgh[0] = x0; dgh[1] = x1; dgh[2] = x2; }                              // exchanged
                else { store4_sc1(dgh, x0); store4_sc1(dgh + 1, x1); store4_sc1(dgh + 2, x2); }
                o_dr[c] = dr; o_du[c] = du; o_dn[c] = dn; o_car[c] = dH * u;
                sb_r += dr; sb_u += du; sb_n += dn; sb_nr += dn * r;
            }
            AVAE_STAMP(4);
            if (p >= 0) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int row = rb + 16 * c + gr;
                    if (row >= row_end) continue;
                    J.carry[(size_t)row * D + j] = o_car[c];
                    if (!(ab & 4)) {
                        float* dgi = J.dgi + (size_t)rix[c] * a.ldg + ht * 48 + gn * 3;
                        dgi[0] = o_dr[c]; dgi[1] = o_du[c]; dgi[2] = o_dn[c];
                    }
                }
            }
            AVAE_STAMP(6);
        }
    }
    if (STAMPS && tid == 0 && a.stamps) {
        for (int i = 0; i < 8; ++i) atomicAdd(a.stamps + 16 + i, ph[i]);
        atomicAdd(a.stamps + 16 + 8, (unsigned long long)(a.p_end - a.p_begin));
        atomicAdd(a.stamps + 16 + 9, (unsigned long long)(fast ? 1 : 0));
        atomicAdd(a.stamps + 16 + 10, 1ULL);
    }
    // bias gradients: reduce the 16 row-lanes of the workgroup, then one atomic per (gate, unit)
    if (J.dbW || J.dbR) {
        if (tid < 64) red[tid >> 4][tid & 15] = 0.f;
        __syncthreads();
        atomicAdd(&red[0][gn], sb_r); atomicAdd(&red[1][gn], sb_u); atomicAdd(&red[2][gn], sb_n); atomicAdd(&red[3][gn], sb_nr);
        __syncthreads();
        if (tid < 48) {
            const int gate = tid >> 4, u = tid & 15;
            if (J.dbW) atomicAdd(J.dbW + ht * 48 + u * 3 + gate, red[gate][u]);
            if (J.dbR) atomicAdd(J.dbR + ht * 48 + u * 3 + gate, red[gate == 2 ? 3 : gate][u]);
        }
    }
}

// ------------------------------------------------------------------------------ backward, D = 512, four teams per CU
// The LDS-weight form of the backward step (the forward's gru_fwd_team_kernel is its model): ONE workgroup of 16
// waves owns a (job, 16-unit slice) and one or more 64-row blocks; its 1536 x 16 slice of R' (the B operand of
// dH_prev = dgh R) lives in LDS in MFMA B-fragment order (96 KB, one ds_read_b128 per four MFMA steps) and is shared by
// FOUR teams of 4 waves; every team runs independent 16-row chains (one per row block, interleaved item by item as in
// the forward).  A operand: the hand-counted sc1 piece stream with a running-max sentinel check and a one-instruction
// probe of the register-form D = 512 path above, with a ring of NB 24-register pieces (128-register budget at 4 waves
// per SIMD) whose first NB pieces are in flight before the MFMAs start.  A job with dh0 (decoder layers) gets the
// tail item p = -1: dh0 = carry + dgh_0 R.  Teams synchronise through monotonic LDS counters, never s_barrier.
constexpr int kBwdTeamLdsBytes = (4 * 24 * 256 + 16 * 256 + 64) * 4 + 64;      // dynamic LDS of gru_bwd_team_kernel: Wl | part | red | sync
template <int NB, bool PIPE, int T, bool DIAG = false, bool BF = false, bool CMP = false, bool RING = false>   // CMP: compact external arrays / phantom rows (GruArgs::rowmap, Bx); PIPE: several row blocks per workgroup; T teams of 16 / T waves; BF: bf16 operands (see the forward); RING: exchange ring (GruPlan::ring)
__global__ __launch_bounds__(1024, 4) void gru_bwd_team_kernel(GruArgs a)
{
    static_assert(!RING || (!PIPE && !BF && !DIAG), "the exchange ring: fp32, one row block per workgroup");
    // diagnostic phase stamps (DIAG instantiation only): [0] top loads [1] probe + first pieces [2] operand stream + MFMAs
    // [3] barrier 1 [4] partial write + prefetch [5] barrier 2 [6] gate derivatives + stores
    unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = DIAG ? __builtin_amdgcn_s_memrealtime() : 0ULL;
#define BSTAMP(i) do { if constexpr (DIAG) { unsigned long long t_ = __builtin_amdgcn_s_memrealtime(); ph[i] += t_ - tprev; tprev = t_; } } while (0)
    // KPL = k values per load instruction (1 KB of the tiled exchange): 16 floats, or 32 bf16 in the 16-bit exchange of BF
    constexpr int D = 512, HT = 32, PQ = 6, KS = 16 / T, WKB = 3 * D / KS, KPL = BF ? 32 : 16, NH = WKB / (PQ * KPL), KB4 = 96 / KS, RB = 16 * T;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Wl = lds;                                        // [wk KS][ks4 KB4][lane 64][4]    96 KB (BF: [wk][WKB/32][lane][8 bf16], 48 KB)
    float* part = Wl + 96 * 256;                            // [team T][wk KS][256]            16 KB
    float* red = part + 16 * 256;                           // [4][16] bias-gradient sums
    unsigned* sync = reinterpret_cast<unsigned*>(red + 64); // [team 4]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // wave -> (team, K-split index).  Waves w and w + 4 share a SIMD; a team's K-split partners meet at a barrier every
    // step.  Which SIMDs a team sits on is a 1-3 % effect since the operand loads stopped saturating the texture
    // addresser; the mapping per form is the best of {one SIMD, a SIMD pair, all four} measured in-process
    // (gpurun_out/ab16.log, scripts/ab_classes.py).
    int team, wk;
    if (T == 4 && PIPE && !CMP) { team = wave & 3; wk = wave >> 2; }                                           // one SIMD
    else if (T == 4)         { team = wave >> 2; wk = wave & 3; }                                              // all four SIMDs
    else if (PIPE && !CMP)   { team = (wave >> 1) & 1; wk = (wave & 1) + 2 * (wave >> 2); }                   // a SIMD pair (CMP: all four, see the forward)
    else                     { team = wave >> 3; wk = wave & 7; }                                              // all four SIMDs
    const int n = lane & 15, kh = lane >> 4;
    const TeamMap tm = team_map(a, RB);
    const int cid = tm.cid, ht = tm.ht;
    const GruJob& J = a.job[tm.jb];
    const int Bs = a.B, S = a.S;                           // Bs: rows per position of the external arrays
    const int B = (CMP && a.Bx > Bs) ? a.Bx : Bs;          // rows of the launch geometry (exchange scratch, slots)
    xcd_publish(a.counters + 64 + cid, a.counters + 128 + cid * HT, ht);      // (collected after the weights are in LDS)

    // weights -> LDS: block (wq, ks4): lane (n, kh) holds w[4 ks4 + e] = R'[wq*384 + 16 ks4 + 4 kh + e][ht*16 + n], e = 0..3
    // the exchanged operand is in gate-major order inside a producer's 48 columns (kx = tile*48 + gate*16 + unit, so
    // that a producer wave's store of one gate covers whole 16-byte groups); R' rows are in unit-major order
    auto r_row = [&](int kx) -> const float* { const int rem = kx % 48; return J.R + (size_t)((kx - rem) + (rem & 15) * 3 + (rem >> 4)) * D + ht * 16 + n; };
    if constexpr (BF) {   // block (wq, kp): lane (n, kh) holds the 8 bf16 R'[wq*WKB + 32 kp + 8 kh + e][ht*16 + n], e = 0..7
        for (int blk = wave; blk < 48; blk += 16) {
            const int wq = blk / (KB4 / 2), kp = blk % (KB4 / 2);
            const float* r0 = r_row(wq * WKB + 32 * kp + 8 * kh);          // (8 consecutive kx stay inside one 16-unit gate group)
            const u32x4 pk = {pack_bf16(r0[0], r0[3 * D]), pack_bf16(r0[6 * D], r0[9 * D]), pack_bf16(r0[12 * D], r0[15 * D]), pack_bf16(r0[18 * D], r0[21 * D])};
            *reinterpret_cast<u32x4*>(Wl + (size_t)blk * 256 + lane * 4) = pk;
        }
    } else
    for (int blk = wave; blk < 96; blk += 16) {
        const int wq = blk / KB4, ks4 = blk % KB4;
        const float* rp = r_row(wq * WKB + 16 * ks4 + 4 * kh);
        *reinterpret_cast<float4*>(Wl + (size_t)blk * 256 + lane * 4) = make_float4(rp[0], rp[3 * D], rp[6 * D], rp[9 * D]);
    }
    if (tid < 2 * T) sync[tid] = 0u;
    if (tid < 64) red[tid] = 0.f;
    const int tt = wk * 64 + lane, gn = tt & 15, gr = (tt >> 4) & 15;
    const bool gate_thread = tt < 256;                        // the team's first 256 threads own one (row, unit) each
    const int j = ht * 16 + gn;
    unsigned long long tp0 = 0, tp1 = 0;
    if constexpr (DIAG) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); tp0 = __builtin_amdgcn_s_memrealtime(); }
    const bool fast = group_same_xcd(a.counters + 64 + cid, a.counters + 128 + cid * HT, ht, HT, a.err, a.force_slow, true);   // has a __syncthreads
    if constexpr (DIAG) {
        tp1 = __builtin_amdgcn_s_memrealtime();
        if (tt == 0 && a.stamps && ((a.ablate & 256) ? T == 2 : T == 4)) {
            atomicAdd(a.stamps + 16 + 11, tp0 - tprev);     // weights -> LDS
            atomicAdd(a.stamps + 16 + 12, tp1 - tp0);       // same-XCD rendezvous
        }
    }
    float* tpart = part + team * (KS * 256);
    unsigned* tsync = sync + team;
    unsigned* ready = sync + T + team;                        // exchange-ready epoch (one polling wave per team, see the forward)
    unsigned epoch = 0;
    {
        const int tq = __builtin_amdgcn_readfirstlane(team);      // one arbitration order on all four SIMDs (see the forward)
        if (tq == 0) __builtin_amdgcn_s_setprio(3);
        else if (tq == 1) __builtin_amdgcn_s_setprio(2);
        else if (tq == 2) __builtin_amdgcn_s_setprio(1);
    }
    // The saved activations are only read and dgi is only written here, never through another name: saying so lets the
    // compiler issue the next item's loads without first waiting for this item's stores (without it every item paid
    // two to three exposed memory round trips: hipcc orders any load behind any earlier store it cannot prove
    // disjoint with s_waitcnt vmcnt(0)).
    const float* __restrict__ p_sv = J.sv;
    const float* __restrict__ p_hp = J.hp;
    const float* __restrict__ p_do = J.dh_out;
    float* __restrict__ p_dgi = J.dgi;
    float* __restrict__ p_dghw = J.dgh;
    unsigned short* __restrict__ p_dgi16 = BF ? J.dgi16 : nullptr;      // BF: the gate gradients as bf16 row-major INSTEAD of fp32
    unsigned short* __restrict__ p_dgh16 = BF ? J.dgh16 : nullptr;      // (the bf16 GEMMs' operands as they stand: no conversion pass)
    float* p_dh0 = J.dh0;
    float* p_carry = J.carry;
    const int* p_lens = a.slens ? a.slens : a.lens;           // (rows permuted: lengths by slot)
    const int* const perm = a.perm;                           // slot -> batch row of every external array (nullptr: identity)
    int* p_err = a.err;
    const int j_rev = J.reverse, ldg = a.ldg, ldh = a.ldh;
    // exchange ring (gru_dev.h): the value of iteration `done` (steps run downwards; the count runs up) in slot done % kGruRing of min(S, kGruRing)
    constexpr bool ring = RING;
    float* const xg = a.xbuf + (size_t)tm.jb * (ring ? min(S, kGruRing) : S) * B * (3 * D) / (BF ? 2 : 1);       // this job's exchange buffer (tiled, sentinel-filled)
    const unsigned long long pa = (unsigned long long)xg;
    const i32x4 srd = {(int)(unsigned)(pa & 0xffffffffULL), (int)(unsigned)((pa >> 32) & 0xffffULL), -1, 0x00020000};
    float sb_r = 0.f, sb_u = 0.f, sb_n = 0.f, sb_nr = 0.f;
    const bool want_dh0 = (p_dh0 != nullptr) && a.p_begin == 0;
    const int p_last = want_dh0 ? -1 : a.p_begin;             // p == -1: only dh0 = carry + dgh_0 R'
    int done = 0;
    unsigned it = 0;
    float carry_reg = 0.f;                                    // !PIPE: dH_{p+1} u_{p+1} of this thread's (row, unit)
    float carry_r0 = 0.f, carry_r1 = 0.f, carry_r2 = 0.f, carry_r3 = 0.f;      // PIPE: the same, per row block
    u32x4 hv[NB][PQ];                                         // ring of A-operand pieces
    const __amdgpu_buffer_rsrc_t rs_dgh = make_rsrc(xg);
    const __amdgpu_buffer_rsrc_t rs_sv = make_rsrc(p_sv), rs_hp = make_rsrc(p_hp), rs_do = make_rsrc(p_do ? p_do : p_hp);
    const unsigned short* __restrict__ p_hp16 = BF ? J.hp16 : nullptr;      // h_prev as the forward's bf16 team kernel wrote it
    const __amdgpu_buffer_rsrc_t rs_hp16 = make_rsrc(reinterpret_cast<const float*>(p_hp16 ? p_hp16 : reinterpret_cast<const unsigned short*>(p_hp)));
    const __amdgpu_buffer_rsrc_t rs_dgi = make_rsrc(p_dgi), rs_dghw = make_rsrc(p_dghw);
    const __amdgpu_buffer_rsrc_t rs_dgi16 = make_rsrc(reinterpret_cast<const float*>(p_dgi16 ? p_dgi16 : reinterpret_cast<unsigned short*>(p_dgi)));
    const __amdgpu_buffer_rsrc_t rs_dgh16 = make_rsrc(reinterpret_cast<const float*>(p_dgh16 ? p_dgh16 : reinterpret_cast<unsigned short*>(p_dghw)));
    auto a_offset = [&](int p, int row0, int len_a) -> unsigned {      // byte offset of this lane's first piece of dgh_{p+1}
        if constexpr (BF) return xch_lane_offset(pos_map(p + 1, len_a, j_rev), row0, wk * (WKB / 8), n, kh, B, 3 * D / 2);
        return xch_lane_offset(ring ? ((done - 1) & (kGruRing - 1)) : pos_map(p + 1, len_a, j_rev), row0, wk * (WKB / 4), n, kh, B, 3 * D);
    };
    auto issue_piece = [&](int piece, u32x4 (&dst)[PQ], unsigned vo) __attribute__((always_inline)) {
        asm_issue6x(dst, vo, srd, 6144 * piece, 6144 * piece + 4096);       // a piece = 96 floats (BF: 192 bf16) of K = 24 chunks of 256 B
    };
    // the first NB pieces go in flight BEFORE the item's MFMAs, the rest behind the MFMAs of the piece whose
    // registers they reuse
    auto head = [&](unsigned vo) __attribute__((always_inline)) {
#pragma unroll
        for (int s0 = 0; s0 < NB && s0 < NH; ++s0) issue_piece(s0, hv[s0], vo);
    };
    // PIPE: the first NB pieces of item (p2, r2) as compiler-visible loads (not the inline-asm form): they stay pending
    // across the barrier, the gate math and the loop edge, so the compiler itself must keep their destination
    // registers intact and wait for them before the pass touches hv; beside the asm loads its counted waits can only
    // over-wait
    // steps of this team's row blocks (padding skipped, see team_steps): non-increasing over r
    int nst0 = a.p_end, nst1 = a.p_end, nst2 = a.p_end, nst3 = a.p_end;
    if (a.slens) {
        nst3 = tm.nrb > 3 ? min(a.p_end, team_steps(a.slens, (tm.slot + 3 * tm.cpj) * RB + team * 16, lane)) : 0;
        nst2 = tm.nrb > 2 ? max(nst3, min(a.p_end, team_steps(a.slens, (tm.slot + 2 * tm.cpj) * RB + team * 16, lane))) : 0;
        nst1 = tm.nrb > 1 ? max(nst2, min(a.p_end, team_steps(a.slens, (tm.slot + 1 * tm.cpj) * RB + team * 16, lane))) : 0;
        nst0 = max(nst1, min(a.p_end, team_steps(a.slens, tm.slot * RB + team * 16, lane)));
    }
    auto nst_of = [&](int r) -> int { return r == 0 ? nst0 : (r == 1 ? nst1 : (r == 2 ? nst2 : nst3)); };
    auto next_head = [&](int p2, int r2, int len2) __attribute__((always_inline)) {
        if (p2 + 1 < nst_of(r2)) {
            const int row2 = (tm.slot + r2 * tm.cpj) * RB + team * 16;
            const unsigned vo2 = a_offset(p2, row2, len2);
#pragma unroll
            for (int s0 = 0; s0 < NB && s0 < NH; ++s0)
#pragma unroll
                for (int q = 0; q < PQ; ++q) hv[s0][q] = load16_sc1(rs_dgh, vo2 + 6144u * s0 + 1024u * q);
        }
    };
    int len_a = j_rev ? p_lens[tm.slot * RB + team * 16 + n] : 0, len_g = j_rev ? p_lens[tm.slot * RB + team * 16 + gr] : 0;
    const int len_p0 = j_rev ? p_lens[tm.slot * RB + team * 16 + 15] : 0;      // the probe's row (last of the team's 16)
    int ge_cur = tm.slot * RB + team * 16 + gr;                 // batch row of this thread's gate row in the current item
    if (perm) ge_cur = perm[ge_cur];
    const int* const rowmap = CMP ? a.rowmap : nullptr;       // compact layout of the external arrays (see the forward); J.dgi_by_pos: dgi keeps the padded layout
    const bool dgi_by_pos = rowmap != nullptr && J.dgi_by_pos != 0;
    if (a.slens && gate_thread && (!rowmap || dgi_by_pos)) {
        // positions behind a row block's steps: zero gate gradients (the weight-gradient GEMMs sum over every row)
        for (int r = 0; r < tm.nrb; ++r) {
            const int gs = (tm.slot + r * tm.cpj) * RB + team * 16 + gr, ge = perm ? perm[gs] : gs;
            if (CMP && ge >= Bs) continue;                         // (a phantom row: no external row)
            for (int p = nst_of(r); p < a.p_end; ++p) {
                const unsigned orow = (((unsigned)p * (unsigned)Bs + (unsigned)ge) * (unsigned)ldg + ht * 48 + gn * 3) * 4u;
                if (BF && p_dgh16 != nullptr) {          // (dgh as bf16; dgi as bf16 too, or fp32 for a table-fed layer: summed by id first)
                    if ((gn & 1) == 0) {
                        const u32x3 z3 = {0u, 0u, 0u};
                        if (!rowmap) __builtin_amdgcn_raw_buffer_store_b96(z3, rs_dgh16, (int)(orow >> 1), 0, 0);
                        if (p_dgi16 != nullptr) __builtin_amdgcn_raw_buffer_store_b96(z3, rs_dgi16, (int)(orow >> 1), 0, 0);
                    }
                    if (p_dgi16 == nullptr) bstore3(0.f, 0.f, 0.f, rs_dgi, orow);
                } else { if (!rowmap) bstore3(0.f, 0.f, 0.f, rs_dghw, orow); bstore3(0.f, 0.f, 0.f, rs_dgi, orow); }
            }
        }
    }
    const int p_first = nst0 - 1;                               // (= a.p_end - 1 without slens)
    if constexpr (PIPE) next_head(p_first, 0, len_a);
    for (int p = p_first; p >= p_last; --p, ++done) {
      for (int r = 0; r < tm.nrb && (p < 0 || p < nst_of(r)); ++r, ++it) {
        const int row0 = (tm.slot + r * tm.cpj) * RB + team * 16;
        // (the compiler would otherwise keep a dozen loop-invariant 64-bit per-lane addresses alive across the MFMA
        //  phase and spill them at 128 VGPRs; hidden behind an empty asm the lane's unit / row are re-derived per item)
        int gn_l = gn, gr_l = gr, ln_l = lane;
        asm volatile("" : "+v"(gn_l), "+v"(gr_l), "+v"(ln_l));
        const int grow = row0 + gr_l, j_l = ht * 16 + gn_l;       // grow: slot (exchange, carry scratch); ge_cur: the batch row
        const bool have_next = p + 1 < nst_of(r);
        const bool poll = done > 0 && !(DIAG && (a.ablate & 16));      // ablate 16 (diagnostic build): no waiting, wrong results
        // PIPE: the item after this one (its row lengths are fetched now, long before they are needed)
        const bool same_p = r + 1 < tm.nrb && (p < 0 || p < nst_of(r + 1));
        const int r2 = same_p ? r + 1 : 0, p2 = same_p ? p : p - 1;
        int len2 = len_a, len2g = len_g, ge2 = ge_cur;
        if constexpr (PIPE) {
            if (p2 >= p_last) {
                const int row2 = (tm.slot + r2 * tm.cpj) * RB + team * 16;
                if (j_rev) { len2 = p_lens[row2 + n]; len2g = p_lens[row2 + gr]; }
                ge2 = perm ? perm[row2 + gr] : row2 + gr;
            }
        }
        BSTAMP(7);
        // (1) exchange-independent loads of the gate phase
        const int gpos = pos_map(p < 0 ? 0 : p, len_g, j_rev);
        const unsigned prix = (unsigned)gpos * (unsigned)Bs + (unsigned)ge_cur;     // (byte offsets below 2^32: team_geometry checks)
        const bool inb = !CMP || ge_cur < Bs;                     // (false: a phantom row of a launch geometry wider than the batch)
        const int crow = (rowmap && gate_thread && p >= 0) ? (inb ? rowmap[prix] : -1) : (int)prix;
        const bool real = !CMP || crow >= 0;                             // (a padding position: zero inputs, zero gradients, exchange only)
        const unsigned rix = (unsigned)crow;
        float4 sv = make_float4(0.f, 0.f, 0.f, 0.f); float s_hp = 0.f, s_do = 0.f;
        if (p >= 0 && gate_thread && real) {
            if (BF && a.sv16) {
                typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                const u32x2 s2 = __builtin_amdgcn_raw_buffer_load_b64(rs_sv, (int)(((rix * HT + ht) * 64 + gn_l * 4) * 2u), 0, 0);
                sv = make_float4(__uint_as_float(s2.x << 16), __uint_as_float(s2.x & 0xffff0000u), __uint_as_float(s2.y << 16), __uint_as_float(s2.y & 0xffff0000u));
            } else
            sv = bload4(rs_sv, ((rix * HT + ht) * 64 + gn_l * 4) * 4u);
            if (BF && p_hp16) s_hp = __uint_as_float((unsigned)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rs_hp16, (int)((rix * D + j_l) * 2u), 0, 0) << 16);
            else s_hp = bload1(rs_hp, (rix * D + j_l) * 4u);
            s_do = p_do ? bload1(rs_do, (rix * (unsigned)ldh + j_l) * 4u) : 0.f;
        }
        // dH_{p+1} u_{p+1} of this (row, unit): written by this same thread one step ago
        // (PIPE: fetched here, ahead of the next item's operand loads -- memory returns in order, so a load issued
        //  behind them would wait for them)
        // One row block (!PIPE): the same thread owns the same (row, unit) at every step, so the carry lives in a register
        // for the whole launch (memory only at its ends).
        float* carryp = p_carry + (size_t)grow * D + j_l;
        float s_carry = 0.f;
        if constexpr (PIPE) {       // up to four row blocks: one register each, selected by the (uniform) block index
            if (done == 0 && have_next && gate_thread) { const float c0 = *carryp; if (r == 0) carry_r0 = c0; else if (r == 1) carry_r1 = c0; else if (r == 2) carry_r2 = c0; else carry_r3 = c0; }
            s_carry = r == 0 ? carry_r0 : (r == 1 ? carry_r1 : (r == 2 ? carry_r2 : carry_r3));
        }
        else { if (done == 0 && have_next && gate_thread) carry_reg = *carryp; }
        BSTAMP(0);
        // (2)+(3) A operand = dgh_{p+1} of the team's 16 rows, this wave's K quarter, in four 96-float pieces
        f32x4 sum = {0.f, 0.f, 0.f, 0.f};
        if (have_next) {
            const unsigned voff = a_offset(p, row0, len_a);
            f32x4 acc[2];
            auto pass = [&]() __attribute__((always_inline)) -> bool {
                unsigned mx = 0u;
                // B fragments one step ahead of their MFMAs: read right before use, every ds_read_b128 was followed by a
                // full lgkmcnt(0) wait and a lone wave's matrix pipe idled ~100 cycles per four MFMAs
                auto ldsB = [&](int st_, int q_) __attribute__((always_inline)) {
                    return *reinterpret_cast<const f32x4*>(Wl + (size_t)((wk * KB4 + st_ * 6 + q_) * 64 + lane) * 4);
                };
                f32x4 bq = {0.f, 0.f, 0.f, 0.f};
                if constexpr (!BF) bq = ldsB(0, 0);
#pragma unroll
                for (int st = 0; st < NH; ++st) {
                    const int issued = (NB + st < NH) ? NB + st : NH;                       // pieces issued so far
                    const int younger = issued - 1 - st;                                    // still allowed in flight
                    if (younger == 2) asm_wait6<12>(hv[st % NB]);
                    else if (younger == 1) asm_wait6<6>(hv[st % NB]);
                    else asm_wait6<0>(hv[st % NB]);
                    if (st == 0) { acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
                    for (int q = 0; q < PQ; ++q) {
                        if constexpr (BF) mx = pk_max_u16(pk_max_u16(mx, pk_max_u16(hv[st % NB][q].x, hv[st % NB][q].y)), pk_max_u16(hv[st % NB][q].z, hv[st % NB][q].w));
                        else mx = max(max(mx, max(hv[st % NB][q].x, hv[st % NB][q].y)), max(hv[st % NB][q].z, hv[st % NB][q].w));
                    }
                    asm volatile("" : "+v"(mx));
                    if constexpr (BF) {
#pragma unroll
                        for (int q = 0; q < PQ; ++q) {          // a loaded 16-byte piece is the MFMA operand as it stands
                            const bf16x8 b8 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(Wl + (size_t)((wk * (KB4 / 2) + st * PQ + q) * 64 + lane) * 4));
                            acc[q & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, hv[st % NB][q]), b8, acc[q & 1], 0, 0, 0);
                        }
                    } else
#pragma unroll
                    for (int q = 0; q < PQ; ++q) {
                        const f32x4 b = bq;
                        if (q + 1 < PQ) bq = ldsB(st, q + 1); else if (st + 1 < NH) bq = ldsB(st + 1, 0);
                        __builtin_amdgcn_sched_barrier(0);          // (the scheduler otherwise sinks the read back to its use)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[e & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(hv[st % NB][q][e]), b[e], acc[e & 1], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if (st + NB < NH) issue_piece(st + NB, hv[st % NB], voff);
                }
                sum = acc[0] + acc[1];
                if constexpr (BF) return __any(any_half_sentinel(mx));
                return __any(mx == kSentinel);
            };
            auto probe = [&](SpinGuard& sg) __attribute__((always_inline)) {
                // start signal (heuristic): lane l reads the last element producer l&31 stores for the team's last row
                const int len_p = PIPE ? (j_rev ? p_lens[row0 + 15] : 0) : len_p0;      // (one row block: fetched once, before the loop)
                const float* pp = BF ? xg + (xch16_index(pos_map(p + 1, len_p, j_rev), row0 + 15, (ln_l & 31) * 48 + 47, B, 3 * D) >> 1)      // (the high half of its dword)
                                     : xg + xch_index(ring ? ((done - 1) & (kGruRing - 1)) : pos_map(p + 1, len_p, j_rev), row0 + 15, (ln_l & 31) * 48 + 47, B, 3 * D);
                for (;;) {
                    unsigned v = 0u;
                    if (ln_l < 32) v = load4_sc1(pp);              // 32 cache lines per poll: half the wave stays out of it
                    if (!__any(BF ? (v >> 16) == 0xffffu : v == kSentinel) || sg.expired(p_err)) break;
                }
            };
            SpinGuard sg;
            if constexpr (!PIPE) {
                if (poll) {     // ONE wave per team polls (a poll costs ~180 texture-addresser cycles) and releases its partners through LDS
                    if (wk == 0) {
                        probe(sg);
                        if (lane == 0) __hip_atomic_store(ready, it + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    } else {
                        while (__hip_atomic_load(ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < it + 1u) __builtin_amdgcn_s_sleep(1);
                    }
                }
                head(voff);
            }
            BSTAMP(1);
            for (;;) {
                const bool bad = pass();
                if (!poll || !bad || sg.expired(p_err)) break;
                probe(sg);
                head(voff);
            }
        }
        // PIPE: the next item is another chain whose dgh every producer stored an item ago: its first NB pieces go in
        // flight now, behind the team barrier and the gate math (the pass still checks every dword)
        if constexpr (PIPE) {
            // (the loads of the gate phase are retired HERE, on purpose: see the forward)
            asm volatile("" :: "v"(sv.x), "v"(sv.y), "v"(sv.z), "v"(sv.w), "v"(s_hp), "v"(s_do), "v"(s_carry), "v"(len2), "v"(len2g), "v"(ge2));
            __builtin_amdgcn_sched_barrier(0);
            if (p2 >= p_last) next_head(p2, r2, len2);
            __builtin_amdgcn_sched_barrier(0);
        }
        BSTAMP(2);
        // every wave of the team has finished READING the previous item's partial sums, then publish this item's
        if (it > 0) { epoch += KS; team_barrier(tsync, epoch); }
        BSTAMP(3);
        *reinterpret_cast<f32x4*>(tpart + wk * 256 + lane * 4) = sum;
        BSTAMP(4);
        epoch += KS; team_barrier(tsync, epoch);
        BSTAMP(5);
        // (4) gate derivatives: the team's 256 threads, one (row, unit) each; exchanged stores first
        if (gate_thread) {
            const int pidx = ((gr >> 2) * 16 + gn) * 4 + (gr & 3);
            float s4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < KS; ++k) s4[k & 3] += tpart[k * 256 + pidx];
            float carried = (s4[0] + s4[1]) + (s4[2] + s4[3]);
            if constexpr (PIPE) carried += s_carry;
            else if (have_next) carried += carry_reg;
            if (p < 0) { if (inb) p_dh0[(size_t)ge_cur * D + j_l] = carried; len_a = len2; len_g = len2g; ge_cur = ge2; continue; }
            const float dH = carried + s_do;
            const float r_ = sv.x, u = sv.y, nn = sv.z;
            const float dn = dH * (1.f - u) * (1.f - nn * nn);
            const float du = dH * (s_hp - nn) * u * (1.f - u);
            const float dr = dn * sv.w * r_ * (1.f - r_);
            if constexpr (BF) {   // exchanged stores first: bf16, gate g of this unit 2 chunks = 512 B after gate g - 1
                const unsigned short x0 = bf16_not_sentinel(dr), x1 = bf16_not_sentinel(du), x2 = bf16_not_sentinel(dn * r_);
                const unsigned o0 = xch16_index(gpos, grow, ht * 48 + gn_l, B, 3 * D) * 2u;
                if (fast) {
                    __builtin_amdgcn_raw_buffer_store_b16(x0, rs_dgh, (int)o0, 0, 0); __builtin_amdgcn_raw_buffer_store_b16(x1, rs_dgh, (int)(o0 + 512u), 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b16(x2, rs_dgh, (int)(o0 + 1024u), 0, 0);
                } else {
                    __builtin_amdgcn_raw_buffer_store_b16(x0, rs_dgh, (int)o0, 0, 16); __builtin_amdgcn_raw_buffer_store_b16(x1, rs_dgh, (int)(o0 + 512u), 0, 16);
                    __builtin_amdgcn_raw_buffer_store_b16(x2, rs_dgh, (int)(o0 + 1024u), 0, 16);
                }
            } else {   // exchanged stores first (tiled buffer, gate-major: gate g of this unit sits 4 chunks = 1 KB after gate g - 1)
                const float x0 = not_sentinel(dr), x1 = not_sentinel(du), x2 = not_sentinel(dn * r_);
                const unsigned o0 = xch_index(ring ? (done & (kGruRing - 1)) : gpos, grow, ht * 48 + gn_l, B, 3 * D) * 4u;
                if (fast) { bstore1(x0, rs_dgh, o0); bstore1(x1, rs_dgh, o0 + 1024u); bstore1(x2, rs_dgh, o0 + 2048u); }
                else { bstore1_sc1(x0, rs_dgh, o0); bstore1_sc1(x1, rs_dgh, o0 + 1024u); bstore1_sc1(x2, rs_dgh, o0 + 2048u); }
            }
            const unsigned orow = (rix * (unsigned)ldg + ht * 48 + gn_l * 3) * 4u;
            const unsigned orow_i = dgi_by_pos ? (prix * (unsigned)ldg + ht * 48 + gn_l * 3) * 4u : orow;      // dgi's own row (padded layout kept for a table-fed layer)
            if (BF && p_dgh16 != nullptr) {
                // 16-bit row-major copies (dgi16 absent: a table-fed layer, whose dgi stays fp32 for the sum by id): the even unit's lane takes its odd neighbour's three values (quad-permute DPP: lanes
                // 0,2 read lanes 1,3) and stores the six bf16 of both units as one 12-byte access
                const float dnr = dn * r_;
                const float o_r = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(dr), 0xF5, 0xF, 0xF, false));
                const float o_u = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(du), 0xF5, 0xF, 0xF, false));
                const float o_n = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(dn), 0xF5, 0xF, 0xF, false));
                const float o_nr = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(dnr), 0xF5, 0xF, 0xF, false));
                if ((gn_l & 1) == 0) {
                    const u32x3 vh = {pack_bf16(dr, du), pack_bf16(dnr, o_r), pack_bf16(o_u, o_nr)};
                    const u32x3 vi = {pack_bf16(dr, du), pack_bf16(dn, o_r), pack_bf16(o_u, o_n)};
                    if (real) __builtin_amdgcn_raw_buffer_store_b96(vh, rs_dgh16, (int)(orow >> 1), 0, 0);
                    if (p_dgi16 != nullptr && (real || (dgi_by_pos && inb))) __builtin_amdgcn_raw_buffer_store_b96(vi, rs_dgi16, (int)(orow_i >> 1), 0, 0);
                }
                if (p_dgi16 == nullptr && (real || (dgi_by_pos && inb))) bstore3(dr, du, dn, rs_dgi, orow_i);
                if constexpr (PIPE) { const float c1 = dH * u; if (r == 0) carry_r0 = c1; else if (r == 1) carry_r1 = c1; else if (r == 2) carry_r2 = c1; else carry_r3 = c1; }
                else carry_reg = dH * u;
            } else {
            if (real) bstore3(dr, du, dn * r_, rs_dghw, orow);                 // the row-major copy the weight-gradient GEMM reads
            if constexpr (PIPE) { const float c1 = dH * u; if (r == 0) carry_r0 = c1; else if (r == 1) carry_r1 = c1; else if (r == 2) carry_r2 = c1; else carry_r3 = c1; }
            else carry_reg = dH * u;
            if (real || (dgi_by_pos && inb)) bstore3(dr, du, dn, rs_dgi, orow_i);
            }
            sb_r += dr; sb_u += du; sb_n += dn; sb_nr += dn * r_;
        }
        // exchange ring: the slot that held iteration done - 2 is dead behind the team barrier above; the team's last K-split wave (T = 2: one
        // that sits out the gate math) re-arms this workgroup's slice of it for iteration done + 2, i.e. step p - 2 (gru_dev.h xch_rearm).
        // Issued here, outside the hand-counted piece stream; the next pass's counted waits cover it (it is older than every piece).
        if constexpr (RING) {
            if (wk == KS - 1 && done >= 2 && p >= 2) xch_rearm<3>(rs_dgh, (done + 2) & (kGruRing - 1), row0, ht * 12, lane, B, 3 * D, fast);
        }
        len_a = len2; len_g = len2g; ge_cur = ge2;
        BSTAMP(6);
      }
    }
    if (gate_thread && p_last >= 0 && a.p_end - 1 >= p_last) {      // a later launch over earlier steps continues from memory
        if constexpr (!PIPE) p_carry[(size_t)(tm.slot * RB + team * 16 + gr) * D + j] = carry_reg;
        else
            for (int r = 0; r < tm.nrb; ++r)
                p_carry[(size_t)((tm.slot + r * tm.cpj) * RB + team * 16 + gr) * D + j] = r == 0 ? carry_r0 : (r == 1 ? carry_r1 : (r == 2 ? carry_r2 : carry_r3));
    }
    if constexpr (DIAG) {
        if (tt == 0 && a.stamps && ((a.ablate & 256) ? T == 2 : T == 4)) {      // ablate bit 256: the T = 2 launches instead
            for (int i = 0; i < 8; ++i) atomicAdd(a.stamps + 16 + i, ph[i]);
            atomicAdd(a.stamps + 16 + 8, (unsigned long long)(a.p_end - a.p_begin));
            atomicAdd(a.stamps + 16 + 10, 1ULL);
        }
    }
#undef BSTAMP
    // bias gradients: all rows of the workgroup into LDS, then one atomic per (gate, unit)
    if (J.dbW || J.dbR) {
        atomicAdd(&red[gn], sb_r); atomicAdd(&red[16 + gn], sb_u); atomicAdd(&red[32 + gn], sb_n); atomicAdd(&red[48 + gn], sb_nr);
        __syncthreads();
        if (tid < 48) {
            const int gate = tid >> 4, u = tid & 15;
            if (J.dbW) atomicAdd(J.dbW + ht * 48 + u * 3 + gate, red[gate * 16 + u]);
            if (J.dbR) atomicAdd(J.dbR + ht * 48 + u * 3 + gate, red[(gate == 2 ? 3 : gate) * 16 + u]);
        }
    }
}

// ------------------------------------------------------------------------------ one step from a zero state
// The top encoder layer's backward direction (model.py:119-121,135): the only consumer of that layer's output is the pick at
// position len_b - 1, where the reversed direction has seen exactly ONE token -- its first step, from h = 0.  Every later step
// of that direction is dead in the reference's graph (never reaches z or the loss, zero gradient: dR of that direction is
// exactly zero), so the build runs that one step only: the cell of gru_cell with R h = 0, i.e. gh = bR, for B rows.
// gi (B, 3D) and bR in G16 order; h goes to h_out[b * ldo + j]; sv (B, D/16, 16, 4) keeps r, u, n, hn for the backward.
// A row without a single non-eos id (lens[b] = 0) has no such step: h = 0 and, in the backward, zero gate gradients (the pick
// of ops.hip pick_last_kernel treats such a row the same way in the full form).
__global__ __launch_bounds__(256) void gru_first_step_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ bR, float* __restrict__ h_out,
                                                                 int ldo, float* __restrict__ sv, int B, int D, const int32_t* __restrict__ lens)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * D) return;
    const int b = i / D, j = i - b * D, c = (j >> 4) * 48 + (j & 15) * 3;
    const float* g = gi + (size_t)b * 3 * D + c;
    const bool live = !lens || lens[b] > 0;
    const GruCellOut cell = gru_cell(g[0], g[1], g[2], bR[c], bR[c + 1], bR[c + 2], 0.f);
    h_out[(size_t)b * ldo + j] = live ? cell.h : 0.f;
    if (sv) *reinterpret_cast<float4*>(sv + ((size_t)b * D + j) * 4) = make_float4(cell.r, cell.u, cell.n, bR[c + 2]);
}
hipError_t gru_first_step_fwd(hipStream_t st, const float* gi, const float* bR, float* h_out, int ldo, float* sv, int B, int D, const int32_t* lens)
{
    hipLaunchKernelGGL(gru_first_step_fwd_kernel, dim3((B * D + 255) / 256), dim3(256), 0, st, gi, bR, h_out, ldo, sv, B, D, lens);
    return hipGetLastError();
}
// its BPTT: dH = dh (nothing carried), h_prev = 0 -- the formulas of gru_bwd_team_kernel's gate phase.  dgi = [dr, du, dn],
// dgh = [dr, du, dn r], both (B, 3D) in G16 column order.
__global__ __launch_bounds__(256) void gru_first_step_bwd_kernel(const float* __restrict__ dh, int ldd, const float* __restrict__ sv,
                                                                 float* __restrict__ dgi, float* __restrict__ dgh, int B, int D, const int32_t* __restrict__ lens)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * D) return;
    const int b = i / D, j = i - b * D, c = (j >> 4) * 48 + (j & 15) * 3;
    const float4 s = *reinterpret_cast<const float4*>(sv + ((size_t)b * D + j) * 4);
    const float dH = (!lens || lens[b] > 0) ? dh[(size_t)b * ldd + j] : 0.f;
    const float r_ = s.x, u = s.y, nn = s.z;
    const float dn = dH * (1.f - u) * (1.f - nn * nn);
    const float du = dH * (0.f - nn) * u * (1.f - u);
    const float dr = dn * s.w * r_ * (1.f - r_);
    float* a = dgi + (size_t)b * 3 * D + c; float* g = dgh + (size_t)b * 3 * D + c;
    a[0] = dr; a[1] = du; a[2] = dn;
    g[0] = dr; g[1] = du; g[2] = dn * r_;
}
hipError_t gru_first_step_bwd(hipStream_t st, const float* dh, int ldd, const float* sv, float* dgi, float* dgh, int B, int D, const int32_t* lens)
{
    hipLaunchKernelGGL(gru_first_step_bwd_kernel, dim3((B * D + 255) / 256), dim3(256), 0, st, dh, ldd, sv, dgi, dgh, B, D, lens);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ launchers
constexpr int kGruSyncWords = 64 + 64 + 1536;   // (spare) | detection counters | XCD ids (njobs*G*HT)
bool gru_dim_supported(int D) { return D == 16 || D == 32 || D == 64 || D == 128 || D == 256 || D == 512; }

#ifdef AVAE_DIAG
constexpr bool kDiagBuild = true;
#else
constexpr bool kDiagBuild = false;
#endif
bool gru_diag_build() { return kDiagBuild; }

template <bool FWD, int KSV, bool DIAG>
static hipError_t launch_ks(hipStream_t st, const GruArgs& a, int grid, bool need_resident)
{
    auto kernel = [] { if constexpr (FWD) return gru_fwd_kernel<KSV, DIAG>; else return gru_bwd_kernel<KSV, DIAG>; }();
    if (need_resident) { hipError_t e = resident(kernel, 256, 0, grid); if (e != hipSuccess) return e; }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}
template <bool FWD>
static hipError_t launch(hipStream_t st, const GruArgs& a, int grid, bool need_resident)
{
#ifdef AVAE_DIAG
#define AVAE_GRU_CASE(KSV) case KSV: return a.ablate ? launch_ks<FWD, KSV, true>(st, a, grid, need_resident) : launch_ks<FWD, KSV, false>(st, a, grid, need_resident);
#else
#define AVAE_GRU_CASE(KSV) case KSV: return launch_ks<FWD, KSV, false>(st, a, grid, need_resident);
#endif
    switch (a.D / 16) {
        AVAE_GRU_CASE(1)
        AVAE_GRU_CASE(2)
        AVAE_GRU_CASE(4)
        AVAE_GRU_CASE(8)
        AVAE_GRU_CASE(16)
        AVAE_GRU_CASE(32)
        default: return hipErrorInvalidValue;
    }
#undef AVAE_GRU_CASE
}

static hipError_t check(const GruArgs& a, int* grid)
{
    if (!gru_dim_supported(a.D) || a.njobs < 1 || a.njobs > kMaxGruJobs) return hipErrorInvalidValue;
    if (a.rows_per_group % 16 || a.G * a.rows_per_group < a.B) return hipErrorInvalidValue;
    if (!kDiagBuild && a.ablate) return hipErrorInvalidValue;
    *grid = a.njobs * a.G * (a.D / 16);
    return hipSuccess;
}

// One launch prepares a persistent run: zero the sync words and fill the exchanged buffer with the
// sentinel (a plain kernel: hipMemsetAsync goes through the blit path and costs ~10 us of stream gap).
__global__ __launch_bounds__(256) void gru_prepare_kernel(unsigned* sync_words, int nsync, uint4* buf, size_t n16)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)nsync) sync_words[i] = 0u;
    const uint4 s4 = make_uint4(kSentinel, kSentinel, kSentinel, kSentinel);
    for (; i < n16; i += stride) buf[i] = s4;
}
// bf16 mode, forward team kernels: the 16-bit exchange of every job = slot 0 seeded with h0 (zeros without one), converted
// to bf16 in the tiled order of xch16_index, and S sentinel-filled slots behind it
struct GruH0 { const float* p[kMaxGruJobs]; };
__global__ __launch_bounds__(256) void gru_prepare16_kernel(unsigned* sync_words, int nsync, uint4* buf, size_t n16, size_t chunks_per_job,
                                                            size_t seed_chunks, GruH0 h0s, int D, const int* perm, int ext_rows)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)nsync) sync_words[i] = 0u;
    const uint4 s4 = make_uint4(kSentinel, kSentinel, kSentinel, kSentinel);
    for (; i < n16; i += stride) {
        const size_t job = i / chunks_per_job, c = i - job * chunks_per_job;
        uint4 v = s4;
        if (c < seed_chunks) {              // chunk ((row/16) * D/8 + k/8) * 16 + row%16 of slot 0
            v = make_uint4(0u, 0u, 0u, 0u);
            const float* h0 = h0s.p[job];
            if (h0) {
                const size_t rb = c / ((size_t)(D >> 3) * 16), rem = c - rb * ((size_t)(D >> 3) * 16);
                const size_t k8 = rem >> 4, slot = rb * 16 + (rem & 15), row = perm ? (size_t)perm[slot] : slot;      // (h0 is an external array)
                if (row < (size_t)ext_rows) {
                const float4 a0 = *reinterpret_cast<const float4*>(h0 + row * D + k8 * 8), a1 = *reinterpret_cast<const float4*>(h0 + row * D + k8 * 8 + 4);
                v = make_uint4(pack_bf16(a0.x, a0.y), pack_bf16(a0.z, a0.w), pack_bf16(a1.x, a1.y), pack_bf16(a1.z, a1.w));
                }
            }
        }
        buf[i] = v;
    }
}
static hipError_t fill_sentinel2d(hipStream_t st, float* base, size_t rows, size_t width, size_t ld)
{
    return hipMemset2DAsync(base, ld * sizeof(float), 0xFF, width * sizeof(float), rows, st);
}

// sentinel-fill the exchanged buffer of every job and zero the sync words; jobs that tile whole rows side
// by side (the two encoder directions) are covered by ONE linear fill
static hipError_t prepare_exchange(hipStream_t st, const GruArgs& a, bool fwd, const GruPlan& p)
{
    const bool team = p.form == GruForm::team, bf = team && a.bf16 && !p.diag;      // (bf: the kernel exchanges 16-bit values)
    const size_t Bg = p.Bg;          // (the launch geometry's rows: B but for the team kernels' phantom rows)
    const size_t rows = (size_t)a.S * Bg, width = fwd ? a.D : 3 * (size_t)a.D, ld = fwd ? a.ldh : a.ldg;
    if (bf && fwd) {
        GruH0 h0s{};
        for (int i = 0; i < a.njobs; ++i) h0s.p[i] = a.job[i].h0;
        const size_t chunks_per_job = ((size_t)a.S + 1) * Bg * a.D / 8;
        hipLaunchKernelGGL(gru_prepare16_kernel, dim3(2048), dim3(256), 0, st, a.counters, kGruSyncWords, reinterpret_cast<uint4*>(a.xbuf),
                           (size_t)a.njobs * chunks_per_job, chunks_per_job, Bg * a.D / 8, h0s, a.D, a.perm, a.B);
        return hipGetLastError();
    }
    if (team) {       // team kernels exchange through the tiled scratch buffer: one linear fill over every job's part
        // (exchange ring: min(S, ring) slots per job at the front of the scratch, which the producers re-arm themselves -- a fill of a few MB)
        const size_t slots = p.ring ? (size_t)std::min(a.S, p.ring) : (size_t)a.S;
        size_t n16 = (size_t)a.njobs * slots * Bg * width / 4;             // (bf16 mode, backward: the exchange holds 16-bit values)
        if (bf) n16 /= 2;
        const size_t blocks = (std::max(n16, (size_t)kGruSyncWords) + 255) / 256;
        hipLaunchKernelGGL(gru_prepare_kernel, dim3((unsigned)std::min<size_t>(blocks, 2048)), dim3(256), 0, st, a.counters, kGruSyncWords,
                           reinterpret_cast<uint4*>(a.xbuf), n16);
        return hipGetLastError();
    }
    float* base0 = fwd ? a.job[0].hs : a.job[0].dgh;
    bool side_by_side = (size_t)a.njobs * width == ld && (((uintptr_t)base0) & 15) == 0 && ((rows * ld) & 3) == 0;
    for (int i = 0; i < a.njobs && side_by_side; ++i)
        side_by_side = (fwd ? a.job[i].hs : a.job[i].dgh) == base0 + i * width;
    if (side_by_side) {
        hipLaunchKernelGGL(gru_prepare_kernel, dim3(2048), dim3(256), 0, st, a.counters, kGruSyncWords,
                           reinterpret_cast<uint4*>(base0), rows * ld / 4);
        return hipGetLastError();
    }
    hipError_t e = hipMemsetAsync(a.counters, 0, sizeof(unsigned) * kGruSyncWords, st);
    for (int i = 0; i < a.njobs && e == hipSuccess; ++i)
        e = fill_sentinel2d(st, fwd ? a.job[i].hs : a.job[i].dgh, rows, width, ld);
    return e;
}

// geometry of the LDS-weight team kernels: C <= 8 chain groups x 32 hidden tiles = at most one 1024-thread workgroup
// per CU; a chain group = one job and every (C / njobs)-th block of 16 T rows of it.  T = 4 teams (64-row blocks) where
// that fills the chip, else T = 2 (32-row blocks, K split over 8 waves).  Returns false where neither applies.
// which (T, C) a job count and a row count give (the batch-dependent half of team_geometry)
static bool team_rows(int njobs, int B, int* T, int* C)
{
    for (int t = 4; t >= 2; t >>= 1) {
        const int rb = 16 * t;
        if (B % rb) continue;
        const int nrbj = B / rb, np = njobs * nrbj;
        if (np < 8) continue;                       // would leave CUs idle: try smaller blocks
        if (np == 8) { *T = t; *C = 8; return true; }
        const int cpj = 8 / njobs;
        if (nrbj % cpj || nrbj / cpj > 4) continue;      // (at most four row blocks per workgroup: the backward keeps one carry register per block)
        *T = t; *C = 8;
        return true;
    }
    // Batches too small to fill the chip in either form still run the team kernels, one row block per workgroup on
    // njobs x blocks x 32 CUs -- the forms of the benchmark geometry (4 teams for the encoder's two directions, 2 teams for
    // a decoder layer), which is what lets the B = 64 oracle fixtures of tests/test_gpu_round2.py reach them.
    for (int i = 0; i < 2; ++i) {
        const int t = (njobs == 2) == (i == 0) ? 4 : 2, rb = 16 * t;
        if (B % rb == 0 && njobs * (B / rb) <= 8) { *T = t; *C = njobs * (B / rb); return true; }
    }
    return false;
}
// The smallest row count >= B the team kernels have a geometry for with one job AND with two (0: none within 256 rows -- every
// batch up to 1024 rows has one): a batch of any size runs them with that many slots, the slots beyond B holding phantom rows
// (GruArgs::Bx), which cost one step each.
int gru_team_batch(int B)
{
    int T = 0, C = 0;
    for (int bx = (B + 15) / 16 * 16; bx <= B + 256; bx += 16)
        if (team_rows(1, bx, &T, &C) && team_rows(2, bx, &T, &C)) return bx;
    return 0;
}
static bool team_geometry(const GruArgs& a, bool fwd, int Bg, int* T, int* C)
{
    if (a.D != 512 || a.njobs > 2 || a.p_begin != 0) return false;
    // the tiled exchange scratch: present, 16-byte aligned, large enough, addressable with 32-bit byte offsets per job
    const size_t per_job = (size_t)a.S * Bg * a.D * (fwd ? 1 : 3);
    if (!a.xbuf || (((uintptr_t)a.xbuf) & 15) || a.xbuf_floats < per_job * a.njobs || per_job * 4 >= (1ull << 32)) return false;
    // (the gate phase addresses gi / hs / saved gates / dgi / dgh with 32-bit byte offsets as well)
    const size_t widest = std::max<size_t>((size_t)std::max(a.ldg, a.ldh), (size_t)4 * a.D);
    if ((size_t)a.S * a.B * widest * 4 >= (1ull << 32)) return false;
    return team_rows(a.njobs, Bg, T, C);
}

// The one place that decides the kernel form (kernels.h GruPlan).  The diagnostic build runs its timing experiments with gru_ablate
// bits 16 | 128 | 256 alone on the team kernels as well (the forward with 4 teams only), never in the reduce-scatter form; the forward
// with any of them and the backward with bit 128 on the diagnostic instantiation (fp32 over the padded layout: no 16-bit operands,
// compact layout or phantom rows).
GruPlan gru_plan(const GruArgs& a, bool fwd, bool persistent)
{
    GruPlan p{};
    p.Bg = a.Bx > a.B ? a.Bx : a.B;
    if (!persistent || (fwd && a.p_end - a.p_begin < 2)) { p.form = GruForm::stepwise; return p; }
    const bool ablate_ok = !a.ablate || (kDiagBuild && !(a.ablate & ~(16 | 128 | 256)));
    int T = 0, C = 0;
    if (!(team_geometry(a, fwd, p.Bg, &T, &C) && a.item_pipeline == 2 && ablate_ok && (!fwd || !a.ablate || T == 4))) {
        // benchmark geometry (D = 512, two full 16-row chunks per workgroup): the software-pipelined forward kernel
        const bool item = fwd && a.D == 512 && a.rows_per_group == 32 && a.B % 32 == 0 && a.G * 32 == a.B && !a.ablate && a.item_pipeline;
        p.form = item ? GruForm::item : GruForm::persistent;
        return p;
    }
    // the reduce-scatter BPTT takes a whole-sequence fp32 launch (team_geometry: p_begin = 0) whose scratch holds its ring
    const bool rs = !fwd && a.bwd_rs && !a.bf16 && !a.ablate && a.p_end == a.S && a.xbuf_floats >= gru_bwd_rs_xbuf_floats(a.njobs, p.Bg);
    p.form = rs ? GruForm::team_rs : GruForm::team;
    p.T = T; p.C = C; p.cpj = C / a.njobs;
    p.pipe = a.njobs * (p.Bg / (16 * T)) > C;
    p.diag = kDiagBuild && (fwd ? a.ablate != 0 : (a.ablate & 128) != 0);
    // the exchange ring: the fp32 kernels with one row block per workgroup (the pipelined and the bf16 forms keep one slot per position)
    p.ring = (a.ring && p.form == GruForm::team && !p.pipe && !a.bf16 && !p.diag) ? kGruRing : 0;
    return p;
}

// the operands only some forms honour
static hipError_t check_operands(const GruArgs& a, const GruPlan& p, bool fwd)
{
    const bool team = p.team(), bf = p.full() && a.bf16;      // (16-bit operands: the bf16 team kernels only)
    bool ok = (!a.sv16 || bf) && (!(a.rowmap || a.Bx > a.B) || p.full())      // compact layout / phantom rows: team kernels only,
              && (a.Bx <= a.B || (a.slens && a.perm && a.rowmap));         // and phantom rows exist through the row order and the row map only
    for (int i = 0; i < a.njobs; ++i) {
        const GruJob& j = a.job[i];
        ok = ok && (!j.hp16 || bf) && (fwd ? (!j.hs16 || bf) && (!j.gi_rows || team) : (!(j.dgi16 || j.dgh16) || bf));
    }
    return ok ? hipSuccess : hipErrorInvalidValue;
}

hipError_t gru_forward(hipStream_t st, const GruArgs& a, bool persistent)
{
    int grid; hipError_t e = check(a, &grid); if (e != hipSuccess) return e;
    const GruPlan p = gru_plan(a, true, persistent);
    e = check_operands(a, p, true); if (e != hipSuccess) return e;
    if (p.form == GruForm::stepwise) {
        for (int q = a.p_begin; q < a.p_end; ++q) {
            GruArgs b = a; b.p_begin = q; b.p_end = q + 1;
            e = launch<true>(st, b, grid, false); if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    e = prepare_exchange(st, a, true, p); if (e != hipSuccess) return e;
    switch (p.form) {
    case GruForm::team: {
        // D = 512: independent 16-row teams sharing one LDS-resident weight slice per CU, the row blocks of a workgroup
        // interleaved item by item (team_geometry picks 4 teams x 4 waves or 2 teams x 8 waves)
        return team_dispatch(p.T, [&](auto T, auto PIPE, auto BF, auto CMP, auto RING) {
            if constexpr (RING && (PIPE || BF)) return hipErrorInvalidValue;      // (gru_plan gives these forms no ring)
            else {
            if constexpr (kDiagBuild && T == 4 && !BF && !CMP && !RING) if (p.diag) return launch_team(st, gru_fwd_team_kernel<true, PIPE, 4>, a, kFwdTeamLdsBytes, p.C);
            return launch_team(st, gru_fwd_team_kernel<false, PIPE, T, BF, CMP, RING>, a, kFwdTeamLdsBytes, p.C);
            }
        }, p.pipe, a.bf16 && !p.diag, a.rowmap != nullptr, p.ring != 0);
    }
    case GruForm::item:
        e = resident(gru_fwd_item_kernel, 256, 0, grid); if (e != hipSuccess) return e;
        hipLaunchKernelGGL(gru_fwd_item_kernel, dim3(grid), dim3(256), 0, st, a);
        return hipGetLastError();
    default:
        return launch<true>(st, a, grid, true);
    }
}

hipError_t gru_backward(hipStream_t st, const GruArgs& a, bool persistent)
{
    int grid; hipError_t e = check(a, &grid); if (e != hipSuccess) return e;
    const GruPlan p = gru_plan(a, false, persistent);
    e = check_operands(a, p, false); if (e != hipSuccess) return e;
    switch (p.form) {
    case GruForm::team_rs:
        // reduce-scatter form (gru_rs.hip): the exchange is a two-slot ring of partial dH tiles, filled with 1-bits (the tag the
        // first use of a slot does NOT expect)
        hipLaunchKernelGGL(gru_prepare_kernel, dim3(2048), dim3(256), 0, st, a.counters, kGruSyncWords,
                           reinterpret_cast<uint4*>(a.xbuf), gru_bwd_rs_xbuf_floats(a.njobs, p.Bg) / 4);
        e = hipGetLastError(); if (e != hipSuccess) return e;
        return gru_bwd_rs_launch(st, a, p);
    case GruForm::team: {
        e = prepare_exchange(st, a, false, p); if (e != hipSuccess) return e;
        return team_dispatch(p.T, [&](auto T, auto PIPE, auto BF, auto CMP, auto RING) {
            if constexpr (RING && (PIPE || BF)) return hipErrorInvalidValue;      // (gru_plan gives these forms no ring)
            else {
            if constexpr (kDiagBuild && !BF && !CMP && !RING) if (p.diag) return launch_team(st, gru_bwd_team_kernel<2, PIPE, T, true>, a, kBwdTeamLdsBytes, p.C);
            return launch_team(st, gru_bwd_team_kernel<2, PIPE, T, false, BF, CMP, RING>, a, kBwdTeamLdsBytes, p.C);
            }
        }, p.pipe, a.bf16 && !p.diag, a.rowmap != nullptr, p.ring != 0);
    }
    case GruForm::persistent:
        e = prepare_exchange(st, a, false, p); if (e != hipSuccess) return e;
        return launch<false>(st, a, grid, true);
    default:
        break;
    }
    // one launch per step (descending); the dh0 tail (p = -1) is its own launch
    for (int q = a.p_end - 1; q >= a.p_begin; --q) {
        GruArgs b = a; b.p_begin = q; b.p_end = q + 1;
        for (int i = 0; i < b.njobs; ++i) b.job[i].dh0 = nullptr;
        e = launch<false>(st, b, grid, false); if (e != hipSuccess) return e;
        if (q == 0) {
            bool any = false; for (int i = 0; i < a.njobs; ++i) any |= a.job[i].dh0 != nullptr;
            if (any) {
                GruArgs d = a; d.p_begin = 0; d.p_end = 0;   // loop runs p = -1 only
                e = launch<false>(st, d, grid, false); if (e != hipSuccess) return e;
            }
        }
    }
    return hipSuccess;
}

}  // namespace avae
