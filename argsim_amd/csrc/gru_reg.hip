// gru_reg.hip -- the register-resident forms of the GRU recurrence (gru.hip has the overview and the exchange protocol):
// gru_fwd_kernel / gru_bwd_kernel for D = 16 .. 512, the software-pipelined gru_fwd_item_kernel for D = 512, the two first-step
// kernels, and their launchers.
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
            GRU_STAMP(STAMPS, 7);
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
            GRU_STAMP(STAMPS, 0);
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
            GRU_STAMP(STAMPS, 1);
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
            GRU_STAMP(STAMPS, 2);
            __syncthreads();
            GRU_STAMP(STAMPS, 3);
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
            GRU_STAMP(STAMPS, 4);
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
            GRU_STAMP(STAMPS, 6);
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
            GRU_STAMP(STAMPS, 7);
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
            GRU_STAMP(STAMPS, 0);
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
                    const i32x4 srd = make_srd(J.dgh);
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
            GRU_STAMP(STAMPS, 2);
            __syncthreads();
            GRU_STAMP(STAMPS, 3);
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
                const float r = s_r[c], u = s_u[c];
                const GruCellGrad cg = gru_cell_bwd(dH, r, u, s_n[c], s_hn[c], s_hp[c]);
                const float dr = cg.dr, du = cg.du, dn = cg.dn;
                float* dgh = J.dgh + (size_t)rix[c] * a.ldg + ht * 48 + gn * 3;
                const float x0 = not_sentinel(dr), x1 = not_sentinel(du), x2 = not_sentinel(dn * r);
                if (fast) { dgh[0] = x0; dgh[1] = x1; dgh[2] = x2; }                              // exchanged
                else { store4_sc1(dgh, x0); store4_sc1(dgh + 1, x1); store4_sc1(dgh + 2, x2); }
                o_dr[c] = dr; o_du[c] = du; o_dn[c] = dn; o_car[c] = dH * u;
                sb_r += dr; sb_u += du; sb_n += dn; sb_nr += dn * r;
            }
            GRU_STAMP(STAMPS, 4);
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
            GRU_STAMP(STAMPS, 6);
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
// its BPTT: dH = dh (nothing carried), h_prev = 0 -- gru_cell_bwd.  dgi = [dr, du, dn],
// dgh = [dr, du, dn r], both (B, 3D) in G16 column order.
__global__ __launch_bounds__(256) void gru_first_step_bwd_kernel(const float* __restrict__ dh, int ldd, const float* __restrict__ sv,
                                                                 float* __restrict__ dgi, float* __restrict__ dgh, int B, int D, const int32_t* __restrict__ lens)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * D) return;
    const int b = i / D, j = i - b * D, c = (j >> 4) * 48 + (j & 15) * 3;
    const float4 s = *reinterpret_cast<const float4*>(sv + ((size_t)b * D + j) * 4);
    const float dH = (!lens || lens[b] > 0) ? dh[(size_t)b * ldd + j] : 0.f;
    const GruCellGrad cg = gru_cell_bwd(dH, s.x, s.y, s.z, s.w, 0.f);
    float* a = dgi + (size_t)b * 3 * D + c; float* g = dgh + (size_t)b * 3 * D + c;
    a[0] = cg.dr; a[1] = cg.du; a[2] = cg.dn;
    g[0] = cg.dr; g[1] = cg.du; g[2] = cg.dn * s.x;
}
hipError_t gru_first_step_bwd(hipStream_t st, const float* dh, int ldd, const float* sv, float* dgi, float* dgh, int B, int D, const int32_t* lens)
{
    hipLaunchKernelGGL(gru_first_step_bwd_kernel, dim3((B * D + 255) / 256), dim3(256), 0, st, dh, ldd, sv, dgi, dgh, B, D, lens);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ launchers
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
hipError_t gru_reg_launch(hipStream_t st, const GruArgs& a, bool fwd, int grid, bool need_resident)
{
    return fwd ? launch<true>(st, a, grid, need_resident) : launch<false>(st, a, grid, need_resident);
}
hipError_t gru_fwd_item_launch(hipStream_t st, const GruArgs& a, int grid)
{
    hipError_t e = resident(gru_fwd_item_kernel, 256, 0, grid); if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gru_fwd_item_kernel, dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace avae

