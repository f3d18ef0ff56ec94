// gru_team.hip -- the LDS-weight team forms of the GRU recurrence for D = 512 (gru.hip has the overview and the exchange
// protocol, gru_dev.h the scaffold the team kernels share with gru_rs.hip): gru_fwd_team_kernel, gru_bwd_team_kernel and
// their launch functions.
#include <algorithm>
#include "kernels.h"
#include "gru_dev.h"
#include <type_traits>

namespace avae {

// ------------------------------------------------------------------------------ forward, D = 512, four teams per CU
// The register-resident form (gru_reg.hip) tops out at two chains per CU (96 weight registers per lane allow only
// 2 waves per SIMD) and the matrix pipe sits ~50 % idle while those two chains wait on their exchange.
// Here ONE workgroup of 16 waves owns a (job, 16-unit slice) pair: its 48 x 512 weight slice lives in LDS
// (96 KB, already in MFMA B-fragment order, one ds_read_b128 per gate and four MFMA steps) and is shared by
// FOUR teams of 4 waves; every team runs an independent 16-row chain (its own A fragment, K split over its 4
// waves, partial sums and gate math inside the team).  4 waves per SIMD = four chains to fill the matrix
// pipe.  Teams synchronise through two monotonic LDS counters per team (LDS atomics + LDS polling; never
// s_barrier, which would put the four chains in lock step).  Exchange between workgroups: the same in-band
// sentinel protocol as there.

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
constexpr int kFwdTeamLdsBytes = (96 * 256 + 48 * 256 + 4 * 256) * 4 + 128;      // dynamic LDS of gru_fwd_team_kernel: Wl | part | hps | sync (T = 4; the kernel checks its carve against it)
template <bool DIAG, bool PIPE, int T, bool BF = false, bool CMP = false, bool RING = false>      // CMP: compact external arrays / phantom rows (GruArgs::rowmap, Bx); RING: exchange ring (GruPlan::ring)
__global__ __launch_bounds__(1024, 4) void gru_fwd_team_kernel(GruArgs a)
{
    static_assert(!RING || (!PIPE && !BF && !DIAG), "the exchange ring: fp32, one row block per workgroup");
    const int ab = DIAG ? a.ablate : 0;                     // timing experiments / stamps: diagnostic instantiation only
    constexpr int D = 512, HT = 32, KS = 16 / T, WK = D / KS, NQ = WK / 16, RB = 16 * T;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int oPart = 96 * 256, oHps = oPart + 48 * 256, oSync = oHps + T * 256;      // float offsets into lds[]
    static_assert((oSync + 2 * T) * 4 <= kFwdTeamLdsBytes, "lds[] is carved inside the dynamic LDS the launch asks for");
    float* Wl = lds;                                        // [wk KS][gate 3][q NQ][lane 64][4]    96 KB
    float* part = lds + oPart;                              // [team T][wk KS][gate 3][256]         48 KB
    float* hps = lds + oHps;                                // [team T][16][16]
    unsigned* sync = reinterpret_cast<unsigned*>(lds + oSync);        // [team T] barrier counters, [team T] exchange-ready epochs

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr WaveSplit ws = team_wave_split(TeamKernel::fwd, T, PIPE, CMP);      // (placement: gru_dev.h)
    const int team = (wave >> ws.team_shift) & ws.team_mask, wk = (wave & ws.wk_mask) + ws.wk_mul * (wave >> ws.wk_shift);
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
    if (ab & 256) { } else team_set_priority(team);      // (one arbitration order on all four SIMDs)

    const bool stamp = (ab & 128) != 0;                        // diagnostic phase stamps (never in timed runs)
    unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = __builtin_amdgcn_s_memrealtime();
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
        GRU_STAMP(stamp, 5);
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
        const NextItem nx = team_next_item<true>(nst_of, tm.nrb, p, r);
        const int r2 = nx.r, p2 = nx.p;
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
        GRU_STAMP(stamp, 0);
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
        GRU_STAMP(stamp, 1);
        // every wave of the team has finished READING the previous item's partial sums (second team barrier
        // of that item, taken here so that it costs nothing), then publish this item's
        if (it > 0) { epoch += KS; team_barrier(tsync, epoch); }
        GRU_STAMP(stamp, 6);
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
        GRU_STAMP(stamp, 7);
        epoch += KS; team_barrier(tsync, epoch);
        GRU_STAMP(stamp, 2);
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
        GRU_STAMP(stamp, 3);
      }
    }
    if (stamp && tt == 0 && a.stamps) {
        for (int i = 0; i < 8; ++i) atomicAdd(a.stamps + i, ph[i]);
        atomicAdd(a.stamps + 8, (unsigned long long)(a.p_end - a.p_begin));
        atomicAdd(a.stamps + 10, 1ULL);
    }
}

// ------------------------------------------------------------------------------ backward, D = 512, four teams per CU
// The LDS-weight form of the backward step (the forward's gru_fwd_team_kernel is its model): ONE workgroup of 16
// waves owns a (job, 16-unit slice) and one or more 64-row blocks; its 1536 x 16 slice of R' (the B operand of
// dH_prev = dgh R) lives in LDS in MFMA B-fragment order (96 KB, one ds_read_b128 per four MFMA steps) and is shared by
// FOUR teams of 4 waves; every team runs independent 16-row chains (one per row block, interleaved item by item as in
// the forward).  A operand: the hand-counted sc1 piece stream with a running-max sentinel check and a one-instruction
// probe of the register-form D = 512 path (gru_reg.hip gru_bwd_kernel), with a ring of NB 24-register pieces (128-register budget at 4 waves
// per SIMD) whose first NB pieces are in flight before the MFMAs start.  A job with dh0 (decoder layers) gets the
// tail item p = -1: dh0 = carry + dgh_0 R.  Teams synchronise through monotonic LDS counters, never s_barrier.
constexpr int kBwdTeamLdsBytes = (4 * 24 * 256 + 16 * 256 + 64) * 4 + 64;      // dynamic LDS of gru_bwd_team_kernel: Wl | part | red | sync (the kernel checks its carve against it)
template <int NB, bool PIPE, int T, bool DIAG = false, bool BF = false, bool CMP = false, bool RING = false>   // CMP: compact external arrays / phantom rows (GruArgs::rowmap, Bx); PIPE: several row blocks per workgroup; T teams of 16 / T waves; BF: bf16 operands (see the forward); RING: exchange ring (GruPlan::ring)
__global__ __launch_bounds__(1024, 4) void gru_bwd_team_kernel(GruArgs a)
{
    static_assert(!RING || (!PIPE && !BF && !DIAG), "the exchange ring: fp32, one row block per workgroup");
    // diagnostic phase stamps (DIAG instantiation only): [0] top loads [1] probe + first pieces [2] operand stream + MFMAs
    // [3] barrier 1 [4] partial write + prefetch [5] barrier 2 [6] gate derivatives + stores
    unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = DIAG ? __builtin_amdgcn_s_memrealtime() : 0ULL;
    // KPL = k values per load instruction (1 KB of the tiled exchange): 16 floats, or 32 bf16 in the 16-bit exchange of BF
    constexpr int D = 512, HT = 32, PQ = 6, KS = 16 / T, WKB = 3 * D / KS, KPL = BF ? 32 : 16, NH = WKB / (PQ * KPL), KB4 = 96 / KS, RB = 16 * T;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int oPart = 96 * 256, oRed = oPart + 16 * 256, oSync = oRed + 64;      // float offsets into lds[]
    static_assert((oSync + 2 * T) * 4 <= kBwdTeamLdsBytes, "lds[] is carved inside the dynamic LDS the launch asks for");
    float* Wl = lds;                                        // [wk KS][ks4 KB4][lane 64][4]    96 KB (BF: [wk][WKB/32][lane][8 bf16], 48 KB)
    float* part = lds + oPart;                              // [team T][wk KS][256]            16 KB
    float* red = lds + oRed;                                // [4][16] bias-gradient sums
    unsigned* sync = reinterpret_cast<unsigned*>(lds + oSync);       // [team T] barrier counters, [team T] exchange-ready epochs

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr WaveSplit ws = team_wave_split(TeamKernel::bwd, T, PIPE, CMP);      // (placement: gru_dev.h)
    const int team = (wave >> ws.team_shift) & ws.team_mask, wk = (wave & ws.wk_mask) + ws.wk_mul * (wave >> ws.wk_shift);
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
    team_set_priority(team);
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
    const i32x4 srd = make_srd(xg);
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
        const NextItem nx = team_next_item<false>(nst_of, tm.nrb, p, r);
        const int r2 = nx.r, p2 = nx.p;
        int len2 = len_a, len2g = len_g, ge2 = ge_cur;
        if constexpr (PIPE) {
            if (p2 >= p_last) {
                const int row2 = (tm.slot + r2 * tm.cpj) * RB + team * 16;
                if (j_rev) { len2 = p_lens[row2 + n]; len2g = p_lens[row2 + gr]; }
                ge2 = perm ? perm[row2 + gr] : row2 + gr;
            }
        }
        GRU_STAMP(DIAG, 7);
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
        GRU_STAMP(DIAG, 0);
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
            GRU_STAMP(DIAG, 1);
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
        GRU_STAMP(DIAG, 2);
        // every wave of the team has finished READING the previous item's partial sums, then publish this item's
        if (it > 0) { epoch += KS; team_barrier(tsync, epoch); }
        GRU_STAMP(DIAG, 3);
        *reinterpret_cast<f32x4*>(tpart + wk * 256 + lane * 4) = sum;
        GRU_STAMP(DIAG, 4);
        epoch += KS; team_barrier(tsync, epoch);
        GRU_STAMP(DIAG, 5);
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
            const float r_ = sv.x, u = sv.y;
            const GruCellGrad cg = gru_cell_bwd(dH, r_, u, sv.z, sv.w, s_hp);
            const float dr = cg.dr, du = cg.du, dn = cg.dn;
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
        GRU_STAMP(DIAG, 6);
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

// ------------------------------------------------------------------------------ launchers
// D = 512: independent 16-row teams sharing one LDS-resident weight slice per CU, the row blocks of a workgroup
// interleaved item by item (team_geometry picks 4 teams x 4 waves or 2 teams x 8 waves)
hipError_t gru_fwd_team_launch(hipStream_t st, const GruArgs& a, const GruPlan& p)
{
    return team_dispatch(p.T, [&](auto T, auto PIPE, auto BF, auto CMP, auto RING) {
        if constexpr (RING && (PIPE || BF)) return hipErrorInvalidValue;      // (gru_plan gives these forms no ring)
        else {
        if constexpr (kDiagBuild && T == 4 && !BF && !CMP && !RING) if (p.diag) return launch_team(st, gru_fwd_team_kernel<true, PIPE, 4>, a, kFwdTeamLdsBytes, p.C);
        return launch_team(st, gru_fwd_team_kernel<false, PIPE, T, BF, CMP, RING>, a, kFwdTeamLdsBytes, p.C);
        }
    }, p.pipe, a.bf16 && !p.diag, a.rowmap != nullptr, p.ring != 0);
}
hipError_t gru_bwd_team_launch(hipStream_t st, const GruArgs& a, const GruPlan& p)
{
    return team_dispatch(p.T, [&](auto T, auto PIPE, auto BF, auto CMP, auto RING) {
        if constexpr (RING && (PIPE || BF)) return hipErrorInvalidValue;      // (gru_plan gives these forms no ring)
        else {
        if constexpr (kDiagBuild && !BF && !CMP && !RING) if (p.diag) return launch_team(st, gru_bwd_team_kernel<2, PIPE, T, true>, a, kBwdTeamLdsBytes, p.C);
        return launch_team(st, gru_bwd_team_kernel<2, PIPE, T, false, BF, CMP, RING>, a, kBwdTeamLdsBytes, p.C);
        }
    }, p.pipe, a.bf16 && !p.diag, a.rowmap != nullptr, p.ring != 0);
}

}  // namespace avae

