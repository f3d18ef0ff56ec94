// gemm_plan.cpp -- launch shaping of every GEMM product for the 256-CU chip, as one pure function (gemm_plan.h).
// model.cpp's gemm() runs the plan: for each launch, clear what the plan asks for, then launch.  Every threshold below is a
// measurement; the comment beside it says which.  tests/test_gemm_plan.py pins the whole function to a recorded table.
#include "gemm_plan.h"

#include <algorithm>
#include <cmath>

namespace avae {

namespace {

GemmPlan one(const GemmShape& s, int thin, int split_k, int accumulate, int zero = kZeroNone, bool dyn = true)
{
    return GemmPlan{1, {{0, s.M, thin, split_k, accumulate, zero, dyn && s.dyn_kind ? 1 : 0}, {0, 0, 0, 0, 0, 0, 0}}};
}

// K-split so that a weight-gradient GEMM (few output tiles, very long K) fills the chip: aim at 768
// co-resident workgroups (3 per CU), every slice at least 4 K-tiles deep
int grad_split(int M, int N, int K)
{
    int tiles = ((M + 127) / 128) * ((N + 127) / 128);
    int s = 768 / tiles;
    int kmax = K / 128; if (kmax < 1) kmax = 1;
    if (s > kmax) s = kmax;
    return s < 1 ? 1 : s;
}

// dW (M x N) += A^T B over K rows into the zero-filled gradient: one slice may store, several add
GemmPlan plan_wgrad(const GemmShape& s)
{
    const int M = s.M, N = s.N, K = s.K;
    if (s.compute_dtype != 0) {
        const int sk = grad_split(M, N, K);
        return one(s, 0, sk, sk > 1 ? 0 : 1);
    }
    // exact-fp32 kernel.  Few output tiles over a very long K: the K split's float atomics (~1.3 TB/s chip-wide, all
    // workgroups at once at the end of one synchronous round) are the overhead, and they scale with tile bytes x
    // slices.  64x64 tiles give four times the tiles, so a quarter of the slices fill the chip (decoder dW/dR pair,
    // the two directions' dR: +6 %); ~1536 workgroups = 6 per CU.  A pair shares them.
    // A small output (decode/out/kernel, latent) uses 32x128 tiles.
    const int np = s.pair ? 2 : 1;
    const int t128 = ((M + 127) / 128) * ((N + 127) / 128);
    int thin = 2, tiles = ((M + 63) / 64) * ((N + 63) / 64) * np, target = 1536;
    if (t128 * np > 96) { thin = 0; tiles = t128 * np; target = 768; }      // enough full tiles: 128x128 (measured: 64x64 loses 3-8 % there)
    if (t128 <= 16) { thin = 1; tiles = ((M + 31) / 32) * ((N + 127) / 128) * np; target = 768; }
    int sk = (target + tiles / 2) / tiles;
    sk = std::max(1, std::min(sk, std::max(1, K / 128)));
    return one(s, thin, sk, 0);
}

}  // namespace

// C = alpha * op(A) op(B) (+bias) with launch shaping for the 256-CU chip (k-contiguous A only):
//  * thin outputs (M <= 512): 32x128 block tiles so that the few rows still spread over many CUs;
//    where float atomics are acceptable (backward) a long K is split over ~768 workgroups instead;
//  * a tile count just above a multiple of 256 (M = 65*256 rows -> 130 row tiles): the rows that make
//    whole rounds of 256 tiles run as one launch and the thin remainder as 32x128 tiles, instead of a
//    few CUs carrying an extra full tile while the rest idle.
// Both forward forms are deterministic (no atomics): z and the per-token losses stay bit-reproducible.
GemmPlan gemm_plan(const GemmShape& s)
{
    const int M = s.M, N = s.N, K = s.K;
    if (s.wgrad) return plan_wgrad(s);
    if (s.thin >= 0) return one(s, s.thin, s.split_k, s.accumulate);       // the caller's own form and split, as they stand
    // mu and lv, two affines of the batch rows in one launch: the skinny form for every batch size (see rows_are_batch below)
    if (s.pair) return one(s, s.skinny ? 3 : (M <= 512 ? 1 : 0), 1, s.accumulate);
    if (s.split_k != 0 || s.a_mc || s.dyn_kind == 2) return one(s, 0, s.split_k ? s.split_k : 1, s.accumulate);
    const int mt = (M + 127) / 128, nt = (N + 127) / 128, tiles = mt * nt;
    const bool plain_out = !s.accumulate && s.ldc == N;       // (a K split adds into the cleared output: whole rows of it)
    // The skinny form (gemm_f32.hip: one 32x32 tile per workgroup, K split over its waves) sums K in another order than the tiled
    // kernels, so WHICH form a forward product takes must not depend on the batch: z and the per-token losses of a row are the
    // same bits in a batch of 16 and of 1024 (test_large_batch_rows_are_independent).  Forward: only the call sites whose rows
    // are the batch rows themselves ask for it (rows_are_batch), for every batch size.  Backward (allow_atomic: the gradients carry
    // float-atomic order anyway): a few rows over a moderate K take it instead of a zero fill + split-K atomics.
    if (s.rows_are_batch && s.skinny && s.compute_dtype != 1 && s.dyn_kind == 0) return one(s, 3, 1, s.accumulate);
    // Ragged batches (compact layout: the host knows roughly how many rows are real): a backward GEMM with a narrow output whose real rows
    // make fewer 128x128 tiles than the chip has CUs (dho = dlogits E over 7.4 k of 16.6 k token rows: 232 tiles, ONE workgroup per CU,
    // 105 TFLOP/s) splits K over ~768 workgroups instead (float atomics into the zero-filled output: the gradients carry that order anyway).
    // The expectation only shapes the launch; rows beyond the device-side count are never touched either way.
    if (s.allow_atomic && s.dyn_split && s.dyn_kind == 1 && plain_out && s.compute_dtype == 0 && K >= 1536 && s.dyn_expect > 0) {
        const int eff_tiles = ((s.dyn_expect + 127) / 128) * nt;
        const int sk = std::min(768 / std::max(eff_tiles, 1), K / 512);
        if (eff_tiles <= 320 && sk >= 2) return one(s, 0, sk, 0, kZeroDynRows);
    }
    const bool prefer_skinny = s.allow_atomic && s.skinny && M <= 512 && K <= 2048 && s.compute_dtype != 1;
    const int thin_form = (s.allow_atomic && s.skinny) ? 3 : 1;       // (3: the skinny form where it applies, else 32x128 tiles)
    if (tiles <= 96) {
        if (s.allow_atomic && plain_out && K >= 512 && !prefer_skinny) {
            const int sk = std::min(768 / tiles, K / 128);
            if (sk >= 2) return one(s, 0, sk, 0, kZeroAll);
        }
        if (M <= 512) return one(s, thin_form, 1, s.accumulate);
    }
    // A GEMM whose row count is only known on the device (the ids present in the batch: about V / 2 of the static bound
    // of V rows) with a narrow output: 128x128 tiles over the rows that exist are fewer than one round of the chip (dE of
    // the table-fed layers: 112 tiles for 768 slots, 49 TFLOP/s).  64x64 tiles: four times the tiles, deterministic.
    if (s.dyn_thin && s.dyn_kind == 1 && s.compute_dtype == 0 && nt <= 4 && tiles <= 512 && K >= 1024) {
        // (backward -- dE of the present ids, K = 3D or 6D: the K range split over 2-4 slices as well, float atomics into the zeroed rows:
        //  3 584 x 512 x 3 072: 113 -> 96 us; fewer present ids, a ragged batch: more)
        const int sk = std::min(4, K / 768);
        if (s.allow_atomic && s.dyn_split && plain_out && sk >= 2) return one(s, 2, sk, 0, kZeroDynRows);
        return one(s, 2, 1, s.accumulate);
    }
    // The forward projection of the present target ids (static bound V rows x 3D: 768 tiles of 128x128, about 40 % of them real): 32x128
    // tiles fill the chip with the rows that exist (78 -> 54 us; the encoder's, 1536 static tiles, is faster on 128x128).  Any tile
    // form keeps a row's K order: the bits of gi do not move.
    if (s.dyn_thin && s.dyn_kind == 1 && s.compute_dtype == 0 && tiles <= 768 && nt > 4 && K <= 512 && !s.accumulate) return one(s, 1, 1, s.accumulate);
    if (tiles > 256 && tiles % 256 != 0) {
        int main_mt = mt;
        while (main_mt > 0 && (main_mt * nt) % 256 != 0) --main_mt;
        const int tail_tiles = (mt - main_mt) * nt;
        const double frac = (double)tiles / 256.0;
        if (main_mt > 0 && tail_tiles < 200 && (std::ceil(frac) - frac) >= 0.3) {
            const int main_rows = main_mt * 128, tail_rows = M - main_rows;
            // rows beyond the device-side row count hold unread garbage either way: the tail keeps the static bound
            GemmPlan p{2, {{0, main_rows, 0, 1, s.accumulate, kZeroNone, s.dyn_kind ? 1 : 0}, {main_rows, tail_rows, thin_form, 1, s.accumulate, kZeroNone, 0}}};
            if (s.allow_atomic && plain_out && K >= 1024 && !(s.skinny && K <= 2048 && s.compute_dtype != 1)) {
                // backward only: a few rows x a long K (dho: 256 rows x K = 8192 took 0.2 ms on 32 thin tiles):
                // K split over ~768 workgroups of full tiles with float atomics instead
                const int sk = std::min(768 / (((tail_rows + 127) / 128) * nt), K / 128);
                if (sk >= 2) p.launch[1] = GemmLaunch{main_rows, tail_rows, 0, sk, 0, kZeroAll, 0};
            }
            return p;
        }
    }
    return one(s, 0, 1, s.accumulate);
}

bool gemm_tn16_shape(int M, int N) { return ((M | N) & 7) == 0 && (long long)M * N >= 1ll << 19; }

// large tiles at one workgroup per CU: a caller's split was sized for 128x128 tiles at three workgroups per CU, so it is
// re-derived -- ~2 rounds of 256 workgroups, at most 16 slices (more: the float atomics dominate), each at least 4 K tiles deep
int gemm_bf16_slices(int split_k, int big_tiles, int K, int bk)
{
    const int s2 = split_k > 1 ? (512 + big_tiles / 2) / big_tiles : 1;
    return std::max(1, std::min(std::min(s2, 16), std::max(1, K / (4 * bk))));
}
bool gemm_bf16_big_fills(int M, int N, int big_tiles, int slices) { return N >= 192 && M >= 192 && big_tiles * slices >= 200; }

}  // namespace avae
