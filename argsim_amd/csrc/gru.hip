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
//
// This file: the checks, the exchange preparation, the plan (which kernel form a launch takes) and gru_forward / gru_backward.
// The kernels and their launch functions: gru_reg.hip (register-resident forms, the one-step kernels), gru_team.hip (LDS-weight
// team forms, D = 512), gru_rs.hip (reduce-scatter BPTT); what they share: gru_dev.h.
#include <algorithm>
#include "kernels.h"
#include "gru_dev.h"
#include <type_traits>

namespace avae {

// ------------------------------------------------------------------------------ planning and launch
constexpr int kGruSyncWords = 64 + 64 + 1536;   // (spare) | detection counters | XCD ids (njobs*G*HT)
bool gru_dim_supported(int D) { return D == 16 || D == 32 || D == 64 || D == 128 || D == 256 || D == 512; }

bool gru_diag_build() { return kDiagBuild; }

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
        e = hipMemset2DAsync(fwd ? a.job[i].hs : a.job[i].dgh, ld * sizeof(float), 0xFF, width * sizeof(float), rows, st);      // (the sentinel is all 1-bits)
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
            e = gru_reg_launch(st, b, true, grid, false); if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    e = prepare_exchange(st, a, true, p); if (e != hipSuccess) return e;
    switch (p.form) {
    case GruForm::team: return gru_fwd_team_launch(st, a, p);
    case GruForm::item: return gru_fwd_item_launch(st, a, grid);
    default: return gru_reg_launch(st, a, true, grid, true);
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
    case GruForm::team:
        e = prepare_exchange(st, a, false, p); if (e != hipSuccess) return e;
        return gru_bwd_team_launch(st, a, p);
    case GruForm::persistent:
        e = prepare_exchange(st, a, false, p); if (e != hipSuccess) return e;
        return gru_reg_launch(st, a, false, grid, true);
    default:
        break;
    }
    // one launch per step (descending); the dh0 tail (p = -1) is its own launch
    for (int q = a.p_end - 1; q >= a.p_begin; --q) {
        GruArgs b = a; b.p_begin = q; b.p_end = q + 1;
        for (int i = 0; i < b.njobs; ++i) b.job[i].dh0 = nullptr;
        e = gru_reg_launch(st, b, false, grid, false); if (e != hipSuccess) return e;
        if (q == 0) {
            bool any = false; for (int i = 0; i < a.njobs; ++i) any |= a.job[i].dh0 != nullptr;
            if (any) {
                GruArgs d = a; d.p_begin = 0; d.p_end = 0;   // loop runs p = -1 only
                e = gru_reg_launch(st, d, false, grid, false); if (e != hipSuccess) return e;
            }
        }
    }
    return hipSuccess;
}

}  // namespace avae
