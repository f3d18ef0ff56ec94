// hooks.cpp -- every avae_debug_* entry point: test surface, not product.  Each runs one piece of the library on caller buffers or
// reports a host-side decision, so that tests restate neither.
#include "ctx.h"

using namespace avae;
using namespace avae::host;

extern "C" {

// rows of the launch geometry the GRU team kernels take for a batch of B rows (gru_team_batch: B itself, the next row count with a
// geometry -- the slots beyond B hold phantom rows --, or 0).  Host arithmetic only: callable without a GPU.
int avae_debug_team_batch(int32_t B) { return B > 0 ? gru_team_batch(B) : 0; }
// test hook: gemm_plan() for n shapes.  in: n x 19 int32, GemmShape's fields in their order; out: n x 15 -- the number of launches, then per
// launch row0, rows, thin, split_k, accumulate, zero (GemmZero), dyn (an unused launch: zeros).  Host arithmetic only: callable without a GPU.
int avae_debug_gemm_plan(const int32_t* in, int32_t n, int32_t* out)
{
    if (!in || !out || n < 0) return 1;
    for (int r = 0; r < n; ++r, in += 19, out += 15) {
        const GemmShape s{in[0] != 0, in[1] != 0, in[2], in[3], in[4], in[5], in[6], in[7], in[8], in[9], in[10], in[11] != 0, in[12] != 0,
                          in[13] != 0, in[14] != 0, in[15], in[16] != 0, in[17] != 0, in[18] != 0};
        const GemmPlan p = gemm_plan(s);
        out[0] = p.n;
        for (int i = 0; i < 2; ++i) {
            const GemmLaunch l = i < p.n ? p.launch[i] : GemmLaunch{0, 0, 0, 0, 0, 0, 0};
            const int32_t f[7] = {l.row0, l.rows, l.thin, l.split_k, l.accumulate, l.zero, l.dyn};
            std::copy(f, f + 7, out + 1 + 7 * i);
        }
    }
    return 0;
}
// test hook: one whole product through gemm() -- plan, clears, launches -- on caller buffers, with the handle's options.  flags: 1 allow_atomic,
// 2 rows_are_batch, 4 weight gradient (a_mc = b_nc = 1).  count: the device-side count or null (rows; a weight gradient: depth), expect: what
// the host is to expect of it (0: unknown).  A2 / B2 / C2: the second problem of a pair or null; keep16: GemmCall::keep_a16 or null.
int avae_debug_gemm_call(avae_handle h, int a_mc, int b_nc, const float* A, const float* Bm, float* Cm, const float* bias, int M, int N, int K,
                         int lda, int ldb, int ldc, float alpha, int accumulate, int flags, const int* count, int expect,
                         const float* A2, const float* B2, float* C2, unsigned short* keep16)
{
    if (!h) return 1;
    GemmCall c{A, lda, a_mc != 0, Bm, ldb, b_nc != 0, Cm, ldc, M, N, K};
    c.alpha = alpha; c.bias = bias; c.accumulate = accumulate; c.keep_a16 = keep16;
    c.allow_atomic = (flags & 1) != 0; c.rows_are_batch = (flags & 2) != 0; c.wgrad = (flags & 4) != 0;
    if (c.wgrad) c.depth(count); else c.rows(count);
    const Pair second{A2, B2, C2, nullptr};
    if (A2) c.pair = &second;
    const int* const was_ptr = h->expect_ptr[0]; const int was_val = h->expect_val[0];
    h->expect_ptr[0] = count; h->expect_val[0] = expect;
    const int r = gemm(h, c);
    h->expect_ptr[0] = was_ptr; h->expect_val[0] = was_val;
    return r;
}
// test hook: one product through gemm() in the CALLER's form: thin (GemmArgs::thin, 0..3) and split_k (>= 1) reach the kernels as they stand, and
// the plan adds no clear -- the caller owns what C holds beforehand.  count / dyn_kind (0 none, 1 rows, 2 depth) / expect: the device-side count as in
// avae_debug_gemm_call; A2 / B2 / C2 / bias2: the second problem of a pair or null.  The handle's compute_dtype and options choose the kernel family.
int avae_debug_gemm_forced(avae_handle h, int a_mc, int b_nc, const float* A, const float* Bm, float* Cm, const float* bias, int M, int N, int K,
                           int lda, int ldb, int ldc, float alpha, int accumulate, int thin, int split_k, const int* count, int dyn_kind, int expect,
                           const float* A2, const float* B2, float* C2, const float* bias2)
{
    if (!h) return 1;
    if (thin < 0 || thin > 3 || split_k < 1 || dyn_kind < 0 || dyn_kind > 2 || (dyn_kind != 0) != (count != nullptr))
        return fail(h, "avae_debug_gemm_forced: thin in 0..3, split_k >= 1, dyn_kind in 0..2 with a count exactly where it is not 0");
    GemmCall c{A, lda, a_mc != 0, Bm, ldb, b_nc != 0, Cm, ldc, M, N, K};
    c.alpha = alpha; c.bias = bias; c.accumulate = accumulate;
    if (dyn_kind == 2) c.depth(count); else c.rows(count);
    c.form(thin, split_k);
    const Pair second{A2, B2, C2, bias2};
    if (A2) c.pair = &second;
    const int* const was_ptr = h->expect_ptr[0]; const int was_val = h->expect_val[0];
    h->expect_ptr[0] = count; h->expect_val[0] = expect;
    const int r = gemm(h, c);
    h->expect_ptr[0] = was_ptr; h->expect_val[0] = was_val;
    return r;
}
// test hook: what gemm_f32() launches for a problem (gemm_f32_form): out = tile form (0 128x128, 1 32x128, 2 64x64, 3 skinny, -1 nothing), fast, db,
// persist, grid x, y, z, refused (1: gemm_f32 returns an error instead).  pair: a second problem rides along.  Host arithmetic only: callable
// without a GPU.
int avae_debug_gemm_f32_form(int a_mc, int b_nc, int M, int N, int K, int lda, int ldb, int ldc, int accumulate, int thin, int split_k, int dyn_kind,
                             int expect, int pair, int32_t out[8])
{
    if (!out) return 1;
    alignas(16) static const float other[4] = {0.f, 0.f, 0.f, 0.f};      // (the form looks at whether there is a second problem and how it is aligned)
    const GemmArgs g{nullptr, nullptr, nullptr, nullptr, M, N, K, lda, ldb, ldc, 1.f, accumulate, split_k, nullptr, dyn_kind, expect, thin,
                     pair ? other : nullptr, pair ? other : nullptr, nullptr, nullptr};
    const GemmF32Form f = gemm_f32_form(a_mc != 0, b_nc != 0, g);
    const int32_t v[8] = {f.tile, f.fast, f.db, f.persist, (int32_t)f.gx, (int32_t)f.gy, (int32_t)f.gz, f.err != hipSuccess};
    std::copy(v, v + 8, out);
    return 0;
}
// test hook: what a decoding call runs (decode_route and, through it, decode_mode / decode_plan: the functions decode_loop and the launchers
// themselves decide with).  in = sampled (0: avae_decode_greedy), D, V, L, b, top_k, nucleus (top_p > 0), persistent (the option), G, lds_max -- G or
// lds_max 0: the current device's; out = route (0 one launch, 1 per token by option or batch, 2 per token because the geometry is refused), kMode
// (-1: top-k or nucleus beyond 8192 ids), ok, nu, vp, cache_e, lds_bytes, the G and lds_max planned for.  Host arithmetic only where G and lds_max
// are given: callable without a GPU.
int avae_debug_decode_plan(const int64_t in[10], int64_t out[9])
{
    if (!in || !out) return 1;
    for (int i = 1; i < 5; ++i) if (in[i] < 1 || in[i] > INT32_MAX) return 1;
    if (in[5] < 0 || in[5] > INT32_MAX || in[8] < 0 || in[8] > INT32_MAX || in[9] < 0 || in[9] > INT32_MAX) return 1;
    DecodePlan p;
    const int route = decode_route(in[7] != 0, (int)in[4], in[0] != 0, (int)in[5], in[6] != 0, (int)in[1], (int)in[2], (int)in[3], (int)in[8], (int)in[9], &p);
    if (route < 0) return 1;
    const int64_t v[9] = {route, p.mode, p.ok, p.nu, p.vp, p.cache_e, p.lds_bytes, p.G, p.lds_max};
    std::copy(v, v + 9, out);
    return 0;
}
// test hook: the decoder batches of the last avae_score / avae_score_z (score_plan): out = N, rc, kc, batches that ran the shared
// first-layer projection of the non-table path (lead_rows + GruJob::gi_rows)
int avae_debug_score_plan(avae_handle h, int32_t out[4])
{
    if (!h || !out) return 1;
    for (int i = 0; i < 4; ++i) out[i] = h->score_plan[i];
    return 0;
}
// ids present in the last forward's two id sources (encoder input, decoder input) where those layers were table-fed
// (use_table), else -1: out[0] = src, out[1] = tgt.  Synchronises.
int avae_debug_present_ids(avae_handle h, int32_t out[2])
{
    if (!h || !out) return 1;
    AV_CHECK(hipStreamSynchronize(h->stream));
    out[0] = out[1] = -1;
    if (h->cnt_src) AV_CHECK(hipMemcpy(&out[0], h->cnt_src, sizeof(int), hipMemcpyDeviceToHost));
    if (h->cnt_tgt) AV_CHECK(hipMemcpy(&out[1], h->cnt_tgt, sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}
// test hook: the route the LAST avae_forward_backward took, as the step noted it where it decided (avae_ctx::Route; every value -1 where no
// step has run).  out = source first layer table-fed, target first layer table-fed (use_table), Ws::compact, Ws::compact_d, Ws::Bx, the BPTT
// form taken (rs_pick: 0 gather, 1 reduce-scatter -- with bwd_rs = 2 the automatic choice), the top encoder layer as one-job launches + the
// one-step kernels (top_one_step); then form, T, C, pipe, ring (gru_plan on the arguments that were launched; form -1: no such launch) for the
// encoder's two-direction forward and backward, the top encoder layer's one-job forward and backward, the decoder's forward and backward.
// Reads host memory only: no launch, no synchronisation.
int avae_debug_step_route(avae_handle h, int32_t out[37])
{
    if (!h || !out) return 1;
    const avae_ctx::Route& r = h->route;
    const int32_t v[7] = {r.tab_src, r.tab_tgt, r.compact, r.compact_d, r.Bx, r.rs, r.top1};
    std::copy(v, v + 7, out);
    for (int k = 0; k < 6; ++k)
        for (int f = 0; f < 5; ++f) out[7 + 5 * k + f] = r.tab_src < 0 ? -1 : r.gru[k][f];
    return 0;
}
// test hook: the row expectations the LAST call left behind (build_compact: what the host expects the compact layout's device-side counts to be
// -- the fill of an earlier call scaled to the call's rows; they shape the launches of the GEMMs over those counts, gemm_plan's dyn_expect).
// out = the real source positions, the decoder's real positions, the unmasked decoder tokens; 0 where the call took no layout or nothing had
// arrived.  Reads host memory only: no launch, no synchronisation.
int avae_debug_row_expect(avae_handle h, int32_t out[3])
{
    if (!h || !out) return 1;
    for (int i = 0; i < 3; ++i) out[i] = h->expect_ptr[i] ? h->expect_val[i] : 0;
    return 0;
}
// test hook: the per-token cross-entropy (model.py:180 loss_gen_samp) of the LAST avae_forward_backward / avae_train_step -- the
// TRAIN forward, word dropout and the latent draw live -- copied to out (device memory, max_n floats); *n_out = its token count.
// (The workspace layout is a pure function of the call geometry, so the array is found again without keeping a pointer.)
int avae_debug_train_ce(avae_handle h, float* out, int32_t max_n, int32_t* n_out)
{
    if (!h || !out || !n_out) return 1;
    if (h->B < 1) return fail(h, "avae_debug_train_ce: no training forward has run on this handle");
    Ws w;
    AV_TRY(get_ws(h, w, h->B, h->Ss, h->St, true));
    int n = 0;
    AV_CHECK(hipMemcpyAsync(&n, w.ntok, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    AV_CHECK(hipStreamSynchronize(h->stream));
    n = std::min(n, (int)max_n);
    AV_CHECK(hipMemcpyAsync(out, w.loss_samp, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    *n_out = n;
    return 0;
}
// diagnostic: per-launch (class, ms, FLOPs) triples of the stamps recorded since timing was switched on, in launch
// order (does not reset them); returns the number of stamps through *n
int avae_debug_timing(avae_handle h, double* out, int max_n, int* n)
{
    if (!h || !out || !n) return 1;
    AV_CHECK(hipStreamSynchronize(h->stream));
    *n = (int)std::min<size_t>(h->stamps_used, (size_t)max_n);
    std::vector<std::pair<const int*, int>> seen;
    for (int i = 0; i < *n; ++i) {
        float ms = 0.f;
        AV_CHECK(hipEventElapsedTime(&ms, h->stamps[i].a, h->stamps[i].b));
        double f = 1.0;
        AV_TRY(dyn_fraction(h, h->stamps[i], seen, &f));
        const double fl = h->stamps[i].flops * f;
        out[3 * i] = h->stamps[i].cls; out[3 * i + 1] = ms; out[3 * i + 2] = fl;
    }
    return 0;
}
// diagnostic: reads and clears the 32 GRU phase-stamp words (option gru_ablate bit 32)
int avae_debug_stamps(avae_handle h, unsigned long long* out)
{
    if (!h || !out) return 1;
    // both on the handle's stream: the read sees every launch enqueued before it, the clear is ordered before every launch after it
    AV_CHECK(hipMemcpyAsync(out, h->errw + 16, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    AV_CHECK(hipMemsetAsync(h->errw + 16, 0, 32 * sizeof(unsigned long long), h->stream));
    AV_CHECK(hipStreamSynchronize(h->stream));
    return 0;
}
// test hook: the MFMA GEMM on caller buffers (see kernels.h for the operand conventions)
int avae_debug_gemm(avae_handle h, int a_mc, int b_nc, const float* A, const float* Bm, float* Cm, const float* bias,
                    int M, int N, int K, int lda, int ldb, int ldc, float alpha, int accumulate, int split_k)
{
    if (!h) return 1;
    // split_k == -1 selects the thin (32x128 tile) variant, -3 the skinny form, 1000 + s the 64x64-tile variant with s K slices
    GemmCall c{A, lda, a_mc != 0, Bm, ldb, b_nc != 0, Cm, ldc, M, N, K};
    c.alpha = alpha; c.bias = bias; c.accumulate = accumulate;
    return gemm(h, c.form(split_k == -3 ? 3 : (split_k < 0 ? 1 : (split_k >= 1000 ? 2 : 0)), split_k < 0 ? 1 : (split_k >= 1000 ? split_k - 1000 : split_k)));
}
// test hook: C = A B^T (A (M, K), B (N, K) row-major) over the first *rows rows of A only, rows read on the DEVICE (dyn_kind 1)
int avae_debug_gemm_dyn(avae_handle h, const float* A, const float* Bm, float* Cm, int M, int N, int K, const int* rows)
{
    if (!h) return 1;
    return gemm(h, nt(A, K, Bm, K, Cm, N, M, N, K).rows(rows).form(0));
}
// test hook (compute_dtype 1): the fp16 output panel of the phased NT GEMM, C16 (M x N) = fp16(alpha * A B^T) over the first *rows rows (rows == nullptr: all);
// returns 3 where the phased kernel does not take the shape
int avae_debug_gemm_c16(avae_handle h, const float* A, const float* Bm, unsigned short* C16, int M, int N, int K, float alpha, const int* rows)
{
    if (!h) return 1;
    if (h->cfg.compute_dtype != 1 || !gemm_bf16_c16_takes(M, N, K, rows, h->bf16_nt8)) return 3;
    GemmCall c = nt(A, K, Bm, K, nullptr, N, M, N, K).scaled(alpha).rows(rows).form(0);
    c.c16 = C16;
    return gemm(h, c);
}
// test hook: C (M x N) += alpha * A^T B with A (K x M, lda), B (K x N, ldb) fp32 row-major, operands rounded to bf16 row by
// row and read through the transposing-LDS-load GEMM (gemm_tn16 / gemm_bf16_tn); C must hold the value to add onto
int avae_debug_gemm_tn16(avae_handle h, const float* A, const float* Bm, float* Cm, int M, int N, int K, int lda, int ldb, int ldc, float alpha)
{
    if (!h) return 1;
    return gemm_tn16(h, tn_grad(A, lda, Bm, ldb, Cm, ldc, M, N, K).scaled(alpha));
}
// test hook (compute_dtype 1): one product whose operands a producer wrote as bf16, through the functions the step calls.  route 0: gemm_bf16_pre --
// A16 row-major with lda, the A panel itself (a_mc 0: (M, lda)) or transposed once from the 2-byte source (a_mc 1: (K, lda)); B fp32 in layout b_nc.
// route 1: gemm_tn16 -- C += alpha A^T B, A (K, lda) and B (K, ldb) row-major, each as bf16 (A16 / B16) or, where that is null, as fp32 (A / Bm).
// wgrad: the call is a weight gradient (tn_grad: the K split comes from the plan and C holds the value to add onto); route 1 always is.  count /
// dyn_kind / expect as in avae_debug_gemm_forced.  The plan, the slab and the options are the product's; a refusal comes back as in the product.
int avae_debug_gemm16(avae_handle h, int route, int a_mc, int b_nc, int wgrad, const unsigned short* A16, const unsigned short* B16, const float* A,
                      const float* Bm, float* Cm, const float* bias, int M, int N, int K, int lda, int ldb, int ldc, float alpha, int accumulate,
                      const int* count, int dyn_kind, int expect)
{
    if (!h) return 1;
    if (h->cfg.compute_dtype != 1) return fail(h, "avae_debug_gemm16: 16-bit operands exist in compute_dtype 1 only");
    if (route < 0 || route > 1 || dyn_kind < 0 || dyn_kind > 2 || (dyn_kind != 0) != (count != nullptr))
        return fail(h, "avae_debug_gemm16: route in 0..1, dyn_kind in 0..2 with a count exactly where it is not 0");
    if (route == 0 && (!A16 || B16)) return fail(h, "avae_debug_gemm16: gemm_bf16_pre takes A16 and an fp32 B");
    GemmCall c = route == 1 ? tn_grad(A, lda, Bm, ldb, Cm, ldc, M, N, K) : GemmCall{nullptr, lda, a_mc != 0, Bm, ldb, b_nc != 0, Cm, ldc, M, N, K};
    c.alpha = alpha; c.bias = bias; c.accumulate = accumulate; c.A16 = A16; c.B16 = B16;
    if (route == 0) c.wgrad = wgrad != 0;
    if (dyn_kind == 2) c.depth(count); else c.rows(count);
    const int* const was_ptr = h->expect_ptr[0]; const int was_val = h->expect_val[0];
    h->expect_ptr[0] = count; h->expect_val[0] = expect;
    const int r = route == 1 ? gemm_tn16(h, c) : gemm_bf16_pre(h, c);
    h->expect_ptr[0] = was_ptr; h->expect_val[0] = was_val;
    return r;
}
// test hook: what gemm_bf16_nt (tn 0) / gemm_bf16_tn (tn 1) launch for a problem whose panels have the leading dimensions lda / ldb
// (gemm_bf16_form: the function both launch from).  wgrad: the K split is the plan's for a weight gradient of the shape (bf16_launch: gemm_plan) and,
// as in gemm_tn16, the slab of slab_floats floats is offered where nt8 is on and that split is above 1; else split_k and the slab as given.
// out = kernel (GemmBf16Kernel: 0 128x128 NT, 1 256x256 NT, 2 phased NT, 3 256x256 TN, 4 phased TN, -1 nothing), the slices it is launched
// with, slab used, refused, the split the caller's was re-derived to, the split asked of the launcher.  Host arithmetic only: callable without a GPU.
int avae_debug_gemm_bf16_form(int tn, int wgrad, int M, int N, int K, int lda, int ldb, int ldc, int split_k, int dyn_kind, int bias, int nt8,
                              int64_t slab_floats, int32_t out[6])
{
    if (!out || slab_floats < 0 || (wgrad && (M < 1 || N < 1))) return 1;      // (the plan of a weight gradient divides by its tile count)
    alignas(16) static float other[4] = {0.f, 0.f, 0.f, 0.f};      // (the form looks at whether there is a bias and a slab, never at what they hold)
    if (wgrad) {
        const GemmShape s{true, true, M, N, K, ldc, 0, 0, -1, dyn_kind, 0, false, false, false, true, 1, true, true, true};
        split_k = gemm_plan(s).launch[0].split_k;
    }
    GemmArgs g{nullptr, nullptr, nullptr, bias ? other : nullptr, M, N, K, lda, ldb, ldc, 1.f, 0, split_k, dyn_kind ? reinterpret_cast<const int*>(other) : nullptr,
               dyn_kind, 0, 0, nullptr, nullptr, nullptr, nullptr};
    g.nt8 = nt8;
    if (slab_floats > 0 && (!wgrad || (nt8 && split_k > 1))) { g.slab = other; g.slab_floats = (size_t)slab_floats; }
    const GemmBf16Form f = gemm_bf16_form(tn != 0, lda, ldb, g);
    const int32_t v[6] = {f.kernel, f.slices, f.slab, f.err != hipSuccess, f.s2, split_k};
    std::copy(v, v + 6, out);
    return 0;
}
// test hook: softmax_ce (ops.hip) on caller buffers, enqueued on the handle's stream.  logits (n_max x V fp32) and panel (n_max x V,
// 2-byte) as CeArgs::logits / grad16: with write_grad the gradient goes to panel as bf16 when panel is given, else over the logits;
// logits16 reads the logits from panel as fp16.  *form_out = softmax_ce_form (0 register, 1 fp16 panel, 2 streaming, -1 refused).
int avae_debug_softmax_ce(avae_handle h, float* logits, unsigned short* panel, int logits16, const int32_t* gold, const int32_t* cidx,
                          const int32_t* n_dev, int n_max, int V, int write_grad, float inv_n, float* loss_samp, float* errt,
                          int32_t* pred, int* form_out)
{
    if (!h || !form_out) return 1;
    CeArgs c{};
    c.logits = logits; c.gold = gold; c.cidx = cidx; c.n_dev = n_dev; c.n_max = n_max; c.V = V;
    c.write_grad = write_grad; c.inv_n = inv_n;
    c.loss_samp = loss_samp; c.errt_samp = errt; c.pred = pred; c.loss_acc = nullptr;
    c.grad16 = panel; c.logits16 = logits16;
    *form_out = softmax_ce_form(c);
    AV_CHECK(softmax_ce(h->stream, c));
    return 0;
}
// test hook: argmax_rows (ops.hip, the stepwise decode's first-maximum) on caller buffers, enqueued on the handle's stream
int avae_debug_argmax_rows(avae_handle h, const float* logits, int32_t* pred, int n, int V)
{
    if (!h) return 1;
    AV_CHECK(argmax_rows(h->stream, logits, pred, n, V));
    return 0;
}
// test hook: the sizes and views of the token-group scratch, so that no test restates the layout.  out[0] = embed_scatter_scratch_ints,
// out[1] = id_groups_ints, out[2..4] = offsets (in ints) of the id_groups_rank / uid / count views, out[5] = id_groups_supported.
// Host arithmetic only: callable without a GPU.
int avae_debug_op_layout(int64_t n, int64_t V, int64_t out[6])
{
    if (!out || n < 0 || V < 0) return 1;
    int32_t base[1];
    out[0] = (int64_t)embed_scatter_scratch_ints((size_t)n, (size_t)V);
    out[1] = (int64_t)id_groups_ints((size_t)n, (size_t)V);
    out[2] = id_groups_rank(base, (int)n, (int)V) - base;
    out[3] = id_groups_uid(base, (int)n, (int)V) - base;
    out[4] = id_groups_count(base, (int)n, (int)V) - base;
    out[5] = id_groups_supported((int)V) ? 1 : 0;
    return 0;
}
// test hook: ONE launcher of the small kernels (ops.hip) named by `op`, on caller-owned device buffers, on the handle's stream.  p: the
// launcher's pointer arguments in the order of its declaration in kernels.h (struct arguments: the order of the fields), i: its integer
// arguments likewise (a uint64 seed as its bit pattern, a bool as 0 / 1), f: its float arguments.  A launcher's refusal comes back as a
// non-zero return with the hipError_t text in avae_last_error.  Nothing else happens here.
//   row_order: p = (lens, perm, slens) per order, then steps_sum; i = n, Breal, B, S, sum_rows, then (add, T, cpj) per order (n <= 4 read)
//   id_groups_build / rows_group_sum: the scratch is p's last entry
//   gru_first_step_fwd: p = gi, bR, h_out, sv, lens; i = ldo, B, D     gru_first_step_bwd: p = dh, sv, dgi, dgh, lens; i = ldd, B, D
int avae_debug_op(avae_handle h, const char* op, void* const* p, const int64_t* i, const float* f)
{
    if (!h || !op || !p || !i || !f) return 1;
    const std::string o(op);
    hipStream_t st = h->stream;
    auto F = [&](int k) { return static_cast<float*>(p[k]); };
    auto I = [&](int k) { return static_cast<int32_t*>(p[k]); };
    if (o == "prep_ids") {
        PrepArgs a{};
        a.src = I(0); a.tgt = I(1); a.keep_mask = static_cast<const uint8_t*>(p[2]); a.src_tm = I(3); a.lens_src = I(4); a.lens_tgt = I(5);
        a.lead = I(6); a.gold = I(7); a.rank = I(8); a.cidx = I(9); a.ntok = I(10); a.zero2 = F(11); a.chunk_counts = I(12);
        a.B = (int)i[0]; a.Ss = (int)i[1]; a.St = (int)i[2]; a.eos = (int)i[3]; a.bos = (int)i[4]; a.train = (int)i[5]; a.seed = (uint64_t)i[6];
        a.keepwd = f[0];
        AV_CHECK(prep_ids(st, a));
    } else if (o == "embed_gather") AV_CHECK(embed_gather(st, F(0), I(1), F(2), (int)i[0], (int)i[1], (int)i[2]));
    else if (o == "embed_scatter_add2") AV_CHECK(embed_scatter_add2(st, F(0), I(1), F(2), (int)i[0], I(3), F(4), (int)i[1], (int)i[2], (int)i[3], I(5)));
    else if (o == "id_groups_build") AV_CHECK(id_groups_build(st, I(0), (int)i[0], (int)i[1], I(1), i[2] != 0));
    else if (o == "rank_rows") AV_CHECK(rank_rows(st, I(0), I(1), I(2), (int)i[0], (int)i[1]));
    else if (o == "rows_gather_ranked") AV_CHECK(rows_gather_ranked(st, F(0), F(1), I(2), I(3), (int)i[0], (int)i[1], (int)i[2]));
    else if (o == "rows_group_sum") AV_CHECK(rows_group_sum(st, F(0), I(1), F(2), (int)i[0], (int)i[1], (int)i[2], I(3)));
    else if (o == "rows_add_indexed") AV_CHECK(rows_add_indexed(st, F(0), F(1), I(2), I(3), (int)i[0], (int)i[1]));
    else if (o == "rows_gather") AV_CHECK(rows_gather(st, F(0), F(1), I(2), I(3), (int)i[0], (int)i[1], I(4)));
    else if (o == "rows_expand") AV_CHECK(rows_expand(st, F(0), F(1), I(2), (int)i[0], (int)i[1], I(3)));
    else if (o == "zero_rows_dyn") AV_CHECK(zero_rows_dyn(st, F(0), I(1), (int)i[0], (int)i[1]));
    else if (o == "zero_fill") AV_CHECK(zero_fill(st, p[0], (size_t)i[0]));
    else if (o == "row_order") {
        RowOrder ro[4];
        const int n = (int)i[0];
        for (int k = 0; k < std::min(n, 4); ++k) ro[k] = RowOrder{I(3 * k), (int)i[5 + 3 * k], (int)i[6 + 3 * k], (int)i[7 + 3 * k], I(3 * k + 1), I(3 * k + 2)};
        AV_CHECK(row_order(st, ro, n, (int)i[1], (int)i[2], (int)i[3], I(3 * std::min(std::max(n, 0), 4)), (int)i[4]));
    } else if (o == "row_map") AV_CHECK(row_map(st, I(0), (int)i[0], (int)i[1], (int)i[2], I(1), I(2), I(3)));
    else if (o == "pick_last") AV_CHECK(pick_last(st, F(0), F(1), I(2), (int)i[0], (int)i[1], I(3)));
    else if (o == "pick_last16") AV_CHECK(pick_last16(st, F(0), static_cast<const unsigned short*>(p[1]), I(2), (int)i[0], (int)i[1], I(3)));
    else if (o == "pick_last_add") AV_CHECK(pick_last_add(st, F(0), F(1), I(2), (int)i[0], (int)i[1], I(3)));
    else if (o == "pick_last_bwd") AV_CHECK(pick_last_bwd(st, F(0), F(1), I(2), (int)i[0], (int)i[1], (int)i[2]));
    else if (o == "latent_fwd") AV_CHECK(latent_fwd(st, F(0), F(1), F(2), F(3), F(4), F(5), (int)i[0], (int)i[1], (uint64_t)i[2], f[0], F(6)));
    else if (o == "latent_bwd") AV_CHECK(latent_bwd(st, F(0), F(1), F(2), F(3), F(4), F(5), (int)i[0], (int)i[1], f[0], f[1]));
    else if (o == "colsum") AV_CHECK(colsum(st, F(0), (int)i[0], (int)i[1], (int)i[2], F(1), I(2)));
    else if (o == "add3") AV_CHECK(add3(st, F(0), F(1), F(2), F(3), i[0]));
    else if (o == "finalize_losses") AV_CHECK(finalize_losses(st, F(0), F(1), I(2), (int)i[0], F(3), (int)i[1], f[0], f[1], f[2]));
    else if (o == "adam_tf") {
        const AdamArgs a{F(0), F(1), F(2), F(3), i[0], f[0], f[1], f[2], f[3], static_cast<const int*>(p[4])};
        AV_CHECK(adam_tf(st, a));
    } else if (o == "g16_permute") AV_CHECK(g16_permute(st, F(0), F(1), (int)i[0], (int)i[1], i[2] != 0));
    else if (o == "gru_first_step_fwd") AV_CHECK(gru_first_step_fwd(st, F(0), F(1), F(2), (int)i[0], F(3), (int)i[1], (int)i[2], I(4)));
    else if (o == "gru_first_step_bwd") AV_CHECK(gru_first_step_bwd(st, F(0), (int)i[0], F(1), F(2), F(3), (int)i[1], (int)i[2], I(4)));
    else return fail(h, "avae_debug_op: no such launcher: " + o);
    return 0;
}

// The shape half of a GRU launch as both GRU hooks take it: i = njobs, S, B, D, ldg, ldh, Bx, G, rows_per_group, p_begin, p_end, item_pipeline,
// bf16, bwd_rs, xbuf_floats.  G = 0: the groups and rows per group the model gives the shape (gru_geometry).
static void gru_shape(const int64_t* i, GruArgs& a)
{
    a.njobs = (int)i[0]; a.S = (int)i[1]; a.B = (int)i[2]; a.D = (int)i[3]; a.ldg = (int)i[4]; a.ldh = (int)i[5]; a.Bx = (int)i[6];
    a.G = (int)i[7]; a.rows_per_group = (int)i[8]; a.p_begin = (int)i[9]; a.p_end = (int)i[10]; a.item_pipeline = (int)i[11];
    a.bf16 = (int)i[12]; a.bwd_rs = (int)i[13]; a.xbuf_floats = (size_t)std::max<int64_t>(i[14], 0);
    if (a.G == 0 && a.D >= 16 && a.njobs >= 1 && a.B >= 1) gru_geometry(a.D, a.njobs, a.B, &a.G, &a.rows_per_group);
}
static void gru_plan_out(const GruArgs& a, const GruPlan& p, int64_t out[10])
{
    const int64_t v[10] = {(int64_t)p.form, p.T, p.C, p.cpj, p.Bg, p.pipe, a.G, a.rows_per_group, (int64_t)gru_bwd_rs_xbuf_floats(a.njobs, p.Bg), p.ring};
    std::copy(v, v + 10, out);
}
// test hook: gru_plan() for one launch shape (i: gru_shape above; a static aligned dummy stands in for the exchange scratch where xbuf_floats > 0).
// out = form (GruForm: 0 stepwise, 1 persistent, 2 item, 3 team, 4 team_rs), T, C, cpj, Bg, pipe, the G and rows_per_group used, the floats of
// exchange scratch the reduce-scatter backward needs for the shape (gru_bwd_rs_xbuf_floats), the depth of the exchange ring (GruPlan::ring, planned with
// GruArgs::ring = 1; 0: one slot per position).  Host arithmetic only: callable without a GPU.
int avae_debug_gru_plan(const int64_t* i, int fwd, int persistent, int64_t out[10])
{
    if (!i || !out) return 1;
    alignas(16) static float dummy[4] = {0.f, 0.f, 0.f, 0.f};
    GruArgs a{};
    gru_shape(i, a);
    a.xbuf = a.xbuf_floats > 0 ? dummy : nullptr; a.ring = 1;
    gru_plan_out(a, gru_plan(a, fwd != 0, persistent != 0), out);
    return 0;
}
// test hook: ONE gru_forward / gru_backward call on caller-owned device buffers, on the handle's stream -- plan, operand check, residency check and
// exchange preparation as in the product.  i: gru_shape above, then stagger, force_slow, sv16, spec, then (reverse, dgi_by_pos) per job; jobs: 19
// pointers per job, GruJob's pointer fields in their order (gi, gi_rows, R, bR, h0, hs, sv, hp, hs16, hp16, dh_out, dgi, dgh, dgi16, dgh16, dh0,
// carry, dbW, dbR); shared: lens, slens, perm, rowmap, xbuf.  counters, err and stamps are the handle's, ring is the handle's option gru_ring, ablate is 0, and only whole-sequence launches
// (p_begin = 0, p_end = S: all the product launches) are taken.  A launcher's refusal comes back as a non-zero return with the hipError_t text in
// avae_last_error.  Synchronises, then reads (and clears) the device error word: an exchange time-out is a non-zero return too.  plan_out: as
// avae_debug_gru_plan's out, the plan that ran.
int avae_debug_gru(avae_handle h, int fwd, int persistent, const int64_t* i, void* const* jobs, void* const* shared, int64_t plan_out[10])
{
    if (!h || !i || !jobs || !shared || !plan_out) return 1;
    GruArgs a{};
    gru_shape(i, a);
    if (a.njobs < 1 || a.njobs > kMaxGruJobs) return fail(h, "avae_debug_gru: njobs in 1..3");
    if (a.p_begin != 0 || a.p_end != a.S) return fail(h, "avae_debug_gru: whole-sequence launches only (p_begin = 0, p_end = S)");
    a.stagger = (int)i[15]; a.force_slow = (int)i[16]; a.sv16 = (int)i[17]; a.spec = (int)i[18];
    for (int k = 0; k < a.njobs; ++k) {
        void* const* p = jobs + 19 * k;
        auto F = [&](int q) { return static_cast<float*>(p[q]); };
        auto H = [&](int q) { return static_cast<unsigned short*>(p[q]); };
        GruJob& j = a.job[k];
        j.gi = F(0); j.gi_rows = static_cast<const int32_t*>(p[1]); j.R = F(2); j.bR = F(3); j.h0 = F(4); j.hs = F(5); j.sv = F(6); j.hp = F(7);
        j.hs16 = H(8); j.hp16 = H(9); j.dh_out = F(10); j.dgi = F(11); j.dgh = F(12); j.dgi16 = H(13); j.dgh16 = H(14); j.dh0 = F(15);
        j.carry = F(16); j.dbW = F(17); j.dbR = F(18);
        j.reverse = (int)i[19 + 2 * k]; j.dgi_by_pos = (int)i[20 + 2 * k];
    }
    a.lens = static_cast<const int*>(shared[0]); a.slens = static_cast<const int*>(shared[1]); a.perm = static_cast<const int*>(shared[2]);
    a.rowmap = static_cast<const int*>(shared[3]); a.xbuf = static_cast<float*>(shared[4]);
    a.counters = h->counters; a.err = h->errw; a.stamps = reinterpret_cast<unsigned long long*>(h->errw + 16); a.ablate = 0;
    a.ring = h->gru_ring;
    gru_plan_out(a, gru_plan(a, fwd != 0, persistent != 0), plan_out);
    AV_CHECK(hipSetDevice(h->device));
    AV_GRU(fwd ? gru_forward(h->stream, a, persistent != 0) : gru_backward(h->stream, a, persistent != 0));
    return check_gru_err(h);
}

// test hook: sample_rows (ops.hip, the launch-per-token sampler) on caller buffers at step t0, row index = batch row
int avae_debug_sample_rows(avae_handle h, const float* logits, int n, int V, int t0, const avae_sample_config* sc, int32_t* pred, float* logp)
{
    if (!h) return 1;
    SampleParams sp{};
    if (!sample_params(h, sc, V, &sp)) return 1;
    if (n < 1 || V < 1 || t0 < 0 || t0 >= (1 << 20)) return fail(h, "sample rows: bad shape or step");
    AV_CHECK(sample_rows(h->stream, logits, n, V, t0, sp, nullptr, h->cfg.eos, pred, logp));
    return 0;
}

// test hook: sample_rows_p on caller buffers at step t0, row index = batch row; lead (n, optional) as sample_rows_p takes it.  With the
// nucleus off it is avae_debug_sample_rows and nkept is filled with -1
int avae_debug_sample_rows_p(avae_handle h, const float* logits, int n, int V, int t0, const avae_sample_p_config* sc, int32_t* pred, float* logp,
                             int32_t* nkept, const int32_t* lead)
{
    if (!h) return 1;
    SampleParams sp{};
    float top_p = 0.f;
    if (!sample_params_p(h, sc, V, &sp, &top_p)) return 1;
    if (n < 1 || V < 1 || t0 < 0 || t0 >= (1 << 20)) return fail(h, "sample rows: bad shape or step");
    if (top_p > 0.f) AV_CHECK(sample_rows_p(h->stream, logits, n, V, t0, sp, top_p, lead, h->cfg.eos, pred, logp, nkept));
    else {
        AV_CHECK(sample_rows(h->stream, logits, n, V, t0, sp, lead, h->cfg.eos, pred, logp));
        if (nkept) AV_CHECK(hipMemsetAsync(nkept, 0xff, (size_t)n * sizeof(int32_t), h->stream));
    }
    return 0;
}

// test hook: one selection step of the beam search (beam_rows + beam_select, beam.hip) on caller buffers: logits (n * width, V), cum and
// fin (n * width) -> parent, token, cum_out, fin_out (n * width)
int avae_debug_beam_select(avae_handle h, const float* logits, int n, int width, int V, const float* cum, const int32_t* fin,
                           int32_t* parent, int32_t* token, float* cum_out, int32_t* fin_out)
{
    if (!h) return 1;
    if (!logits || !cum || !fin || !parent || !token || !cum_out || !fin_out) return fail(h, "beam select: every array must be given");
    if (n < 1 || n > (1 << 20) || V < 1 || width < 1 || width > 32 || width > V) return fail(h, "beam select: bad shape or width");
    AV_CHECK(hipSetDevice(h->device));
    const size_t rows = (size_t)n * width;
    float *cand_sc, *lat_cum; int32_t *cand_tok, *cand_cnt, *len_out, *live;      // (the lengths and the live count are not returned)
    AV_TRY(place_scratch(h, "beam select", [&](Bump& b) {
        cand_sc = b.take<float>(rows * width); lat_cum = b.take<float>(rows);
        cand_tok = b.take<int32_t>(rows * width); cand_cnt = b.take<int32_t>(rows); len_out = b.take<int32_t>(rows); live = b.take<int32_t>(1);
    }));
    AV_CHECK(beam_rows(h->stream, logits, (int)rows, V, width, cum, fin, h->cfg.eos, cand_sc, cand_tok, cand_cnt));
    BeamStep a{};
    a.n = n; a.Win = width; a.W = width; a.eos = h->cfg.eos;
    a.cand_sc = cand_sc; a.cand_tok = cand_tok; a.cand_cnt = cand_cnt; a.fin_in = fin; a.len_in = nullptr;
    a.lat_parent = parent; a.lat_token = token; a.lat_cum = lat_cum; a.cum_out = cum_out; a.fin_out = fin_out; a.len_out = len_out;
    a.live = live;
    AV_CHECK(hipMemsetAsync(a.live, 0, sizeof(int32_t), h->stream));
    AV_CHECK(beam_select(h->stream, a));
    return 0;
}
// test hook: the launch plan of a latent-row entry.  kind 0 knn_plan(n, N, k, chunk_opt), 1 agg_plan(n, N, dim, chunk_opt), 2 probe_plan(N, P, dim,
// chunk_opt); out = every field: qrows or ptiles, qtiles or Ppad, LD or 0, parts, chunk (agg: 0, qtiles, 0, parts, chunk).  Host arithmetic only:
// callable without a GPU.
int avae_debug_latent_plan(int kind, int64_t n, int64_t N, int k_or_P, int dim, int chunk_opt, int32_t out[5])
{
    if (!out || kind < 0 || kind > 2 || n < 0 || n > 0x7fffffff || N < 0 || N > 0x7fffffff) return 1;
    if (kind == 0) { const KnnPlan p = knn_plan((int)n, (int)N, k_or_P, chunk_opt); const int32_t f[5] = {p.qrows, p.qtiles, 0, p.parts, p.chunk}; std::copy(f, f + 5, out); }
    else if (kind == 1) { const AggPlan p = agg_plan((int)n, (int)N, dim, chunk_opt); const int32_t f[5] = {0, p.qtiles, 0, p.parts, p.chunk}; std::copy(f, f + 5, out); }
    else { const ProbePlan p = probe_plan((int)N, k_or_P, dim, chunk_opt); const int32_t f[5] = {p.ptiles, p.Ppad, p.LD, p.parts, p.chunk}; std::copy(f, f + 5, out); }
    return 0;
}

// test hook: sil_plan(N, dim, L, K, chunk_opt, cus) of avae_silhouette; out = TI, TJ, the number of passes, the LDS limit, the staging
// bytes of the first pass, then per pass its first labeling and its LDS bytes (2 L + 5 values at most).  Host arithmetic only: callable
// without a GPU.
int avae_debug_sil_plan(int32_t N, int32_t dim, int32_t L, const int32_t* K, int32_t chunk_opt, int32_t cus, int32_t* out)
{
    if (!K || !out || N < 2 || N > kSilMaxN || L < 1 || L > kSilMaxL || chunk_opt < 0 || cus < 1) return 1;
    for (int l = 0; l < L; ++l) if (K[l] < 1 || K[l] > kSilMaxK) return 1;
    const SilPlan p = sil_plan(N, dim, L, K, chunk_opt, cus);
    out[0] = p.TI; out[1] = p.TJ; out[2] = p.npass; out[3] = kSilLds; out[4] = (int32_t)sil_staging(p.TI, p.begin[1] - p.begin[0]);
    for (int q = 0; q < p.npass; ++q) { out[5 + 2 * q] = p.begin[q]; out[6 + 2 * q] = p.bytes[q]; }
    return 0;
}

// test hook: mmd_plan(N, dim, G, P, chunk_opt, cus) of avae_mmd; out = TI, the relabelings of a full pass, the number of passes, the LDS
// limit, the row tiles, the most slots of a pass, the LDS bytes of the witness pass, then for the first min(passes, cap) passes the first
// relabeling and the LDS bytes (7 + 2 cap values at most).  Host arithmetic only: callable without a GPU.
int avae_debug_mmd_plan(int32_t N, int32_t dim, int32_t G, int32_t P, int32_t chunk_opt, int32_t cus, int32_t* out, int32_t cap)
{
    if (!out || N < 2 || N > kMmdMaxN || G < 1 || G > kMmdMaxG || P < 0 || (long long)G * (1LL + P) > kMmdMaxQ || chunk_opt < 0 || cus < 1 || cap < 0)
        return 1;
    const MmdPlan p = mmd_plan(N, dim, G, P, chunk_opt, cus);
    const int Q = G * (1 + P);
    out[0] = p.TI; out[1] = p.nq; out[2] = p.npass; out[3] = kMmdLds; out[4] = p.tiles; out[5] = p.cap; out[6] = (int32_t)mmd_lds(p.TI, 2 * G, p.W);
    for (int q = 0; q < p.npass && q < cap; ++q) {
        const int q0 = q * p.nq, nq = std::min(p.nq, Q - q0);
        out[7 + 2 * q] = q0; out[8 + 2 * q] = (int32_t)mmd_pass_lds(p, q0, nq, P);
    }
    return 0;
}

// test hook: db_plan(N, dim, chunk_opt, cus) of avae_dbscan; out = TI, row tiles, column parts, column tiles per part, W, the LDS bytes of
// the pair pass, the default max_rounds, then the workspace bytes of a cosine call without count as two 32-bit halves (low, high).  Host
// arithmetic only: callable without a GPU.
int avae_debug_dbscan_plan(int32_t N, int32_t dim, int32_t chunk_opt, int32_t cus, int32_t* out)
{
    if (!out || N < 1 || N > kDbMaxN || dim < 4 || dim > 1024 || (dim & 3) || chunk_opt < 0 || cus < 1) return 1;
    const DbPlan p = db_plan(N, dim, chunk_opt, cus);
    const int32_t f[7] = {p.TI, p.rtiles, p.parts, p.chunk, p.W, p.lds, p.rounds};
    std::copy(f, f + 7, out);
    const size_t n = (size_t)N, W = (size_t)p.W;
    Bump b{nullptr};
    b.take<DbState>(1); b.take<int>((size_t)p.rounds + 1); b.take<unsigned long long>(n * W); b.take<unsigned long long>(W);
    for (int q = 0; q < 4; ++q) b.take<int>(n);
    b.take<int32_t>(n); b.take<double>(n);
    out[7] = (int32_t)(b.off & 0xffffffffu); out[8] = (int32_t)(b.off >> 32);
    return 0;
}

// test hook: pca_plan(N, dim, pad, chunk_opt, form_opt, cus) of avae_pca_fit; out = dreal, tiles, tile pairs, rows of a chunk, chunks, form,
// rounds of a sweep, the default max_sweeps, the launches of a call with it, the LDS bytes of the solve, the rows of a transform tile, then
// the workspace bytes as two 32-bit halves (low, high).  Host arithmetic only: callable without a GPU.
int avae_debug_pca_plan(int32_t N, int32_t dim, int32_t pad, int32_t chunk_opt, int32_t form_opt, int32_t cus, int32_t* out)
{
    if (!out || N < 2 || N > kPcaMaxN || dim < 4 || dim > 1024 || (dim & 3) || pad < 0 || pad > 3 || pad >= dim || chunk_opt < 0 || form_opt < 0 ||
        form_opt > 2 || cus < 1 || (form_opt == 1 && dim - pad > kPcaResident))
        return 1;
    const PcaPlan p = pca_plan(N, dim, pad, chunk_opt, form_opt, cus);
    const int32_t f[11] = {p.dreal, p.tiles, p.pairs, p.rows, p.chunks, p.form, p.rounds, p.sweeps, p.launches, p.lds, p.trows};
    std::copy(f, f + 11, out);
    const size_t nn = (size_t)p.dreal * p.dreal;
    Bump b{nullptr};
    b.take<PcaState>(1); b.take<double>((size_t)p.chunks * dim); b.take<double>((size_t)p.chunks * p.pairs * kPcaT * kPcaT);
    for (int q = 0; q < (p.form == 2 ? 4 : 3); ++q) b.take<double>(nn);
    out[11] = (int32_t)(b.off & 0xffffffffu); out[12] = (int32_t)(b.off >> 32);
    return 0;
}

}  // extern "C"
