// model.cpp -- host orchestration of the VAE step on one MI355X: the per-step hot path and its C entry points (include/argsim_vae.h;
// the handle: handle.cpp, generation: generate.cpp, scoring and search: scoring.cpp, test hooks: hooks.cpp, shared: ctx.h).
//
// Restates the dataflow of reference src/model.py:75-189 as a fixed sequence of kernel launches
// on one HIP stream: prep -> gather -> 3x(bidirectional GRU) -> latent -> 3x GRU decoder ->
// out affine -> tied logits -> softmax-CE, then the hand-derived backward in reverse order and
// TF-style Adam.  No tracing compiler, no autograd: every buffer lives in one workspace laid out
// by a bump allocator.
#include "ctx.h"

using namespace avae;

namespace avae { namespace host {

// A layer whose input is an embedding row (encoder layer 1: E[src]; decoder layer 1: E[lead]) computes W E[id].  With more
// tokens than vocabulary entries the projection is taken once over the U <= V ids present in the batch (their E rows
// gathered, one GEMM with a device-side row count) and gathered by id; the backward sums the per-token gate gradients by id
// (rows_group_sum) and runs dW = (sum)^T E_present and dE[present] += (sum) W over U rows.  The same products grouped by id:
// exact algebra, a different summation order in the backward.  The compact E rows live in emb_src / emb_tgt (unused
// otherwise in this mode), the per-id gradient of E in demb_src / demb_tgt.
// A batch WITHOUT a team-kernel geometry of its own reaches the team kernels through the compact layout, which
// needs the first layers table-fed: such a batch takes the table path below the vocabulary size as well (never more rows than
// tokens: U <= rows).
static bool phantom_batch(const avae_ctx* h, int B)
{
    return h->compact && h->skip_pad && h->persistent && h->cfg.dim_emb == 512 && gru_team_batch(B) > B;
}
bool use_table(const avae_ctx* h, int rows, int B)
{
    if (!h->table_l1 || !id_groups_supported(h->cfg.dim_tgt)) return false;
    return rows >= h->cfg.dim_tgt || (rows >= 1024 && phantom_batch(h, B));
}

void layout(avae_ctx* h, Bump& b, Ws& w, int B, int Ss, int St, bool train)
{
    const int D = h->cfg.dim_emb, V = h->cfg.dim_tgt, R = h->cfg.dim_rep, L = h->cfg.rnn_layers;
    const size_t T = St + 1, rs = (size_t)Ss * B, rt = T * B;
    w.src_tm = b.take<int32_t>(rs); w.lens_src = b.take<int32_t>(B); w.lens_tgt = b.take<int32_t>(B);
    w.lead = b.take<int32_t>(rt); w.gold = b.take<int32_t>(rt); w.rank = b.take<int32_t>(rt);
    w.cidx = b.take<int32_t>(rt); w.ntok = b.take<int32_t>(4 + kPrepChunks); w.pred = b.take<int32_t>(rt);      // (ntok[4..]: prep_ids' chunk counts)
    w.emb_src = b.take<float>(rs * D); w.emb_tgt = b.take<float>(rt * D);
    // table-fed first layers (use_table), taken only where this geometry runs them: W E over the present ids ((U, 6D) encoder
    // layer 1, then (U, 3D) decoder layer 1), the token groups of the id source, the projection row of every token
    const bool tab_s = use_table(h, (int)rs, B), tab_t = use_table(h, (int)rt, B);
    w.ew = b.take<float>(tab_s ? (size_t)V * 6 * D : (tab_t ? (size_t)V * 3 * D : 0));
    w.grp_src = b.take<int32_t>(tab_s ? id_groups_ints(rs, V) : 0); w.grp_tgt = b.take<int32_t>(tab_t ? id_groups_ints(rt, V) : 0);
    w.tokrow_src = b.take<int32_t>(tab_s ? rs : 0); w.tokrow_tgt = b.take<int32_t>(tab_t ? rt : 0);
    w.e_gi.resize(L); w.e_hs.resize(L);
    for (int d = 0; d < 2; ++d) { w.e_sv[d].resize(L); w.e_hp[d].resize(L); }
    w.d_gi.resize(L); w.d_hd.resize(L); w.d_sv.resize(L); w.d_hp.resize(L);
    w.e_hs16.assign(L, nullptr); w.d_hd16.assign(L, nullptr); w.e_hp16[0].assign(L, nullptr); w.e_hp16[1].assign(L, nullptr); w.d_hp16.assign(L, nullptr);
    w.act_e.assign(L, 0); w.act_d.assign(L, 0); w.acth_e.assign(L, 0); w.acth_d.assign(L, 0);
    if (train && h->cfg.compute_dtype == 1 && h->bf16_act && h->bf16_tn && D % 8 == 0)
        for (int i = 0; i < L; ++i) {
            w.e_hs16[i] = b.take<unsigned short>(rs * 2 * D); w.e_hp16[0][i] = b.take<unsigned short>(rs * D); w.e_hp16[1][i] = b.take<unsigned short>(rs * D);
            if (i < L - 1) w.d_hd16[i] = b.take<unsigned short>(rt * D);
            w.d_hp16[i] = b.take<unsigned short>(rt * D);
        }
    w.x16_e.assign(L, nullptr); w.x16_d.assign(L, nullptr);
    w.x16_valid = train && h->cfg.compute_dtype == 1 && h->bf16_tn && !h->bf16_direct && D % 8 == 0;
    if (w.x16_valid)
        for (int i = 1; i < L; ++i) { w.x16_e[i] = b.take<unsigned short>(rs * 2 * D); w.x16_d[i] = b.take<unsigned short>(rt * D); }
    for (int i = 0; i < L; ++i) {
        w.e_gi[i] = b.take<float>(rs * 6 * D);
        w.e_hs[i] = b.take<float>(rs * 2 * D);
        for (int d = 0; d < 2; ++d) {
            w.e_sv[d][i] = train ? b.take<float>(rs * 4 * D) : nullptr;
            w.e_hp[d][i] = train ? b.take<float>(rs * D) : nullptr;
        }
    }
    for (int i = 0; i < L; ++i) {
        w.d_gi[i] = b.take<float>(rt * 3 * D);
        w.d_hd[i] = b.take<float>(rt * D);
        w.d_sv[i] = train ? b.take<float>(rt * 4 * D) : nullptr;
        w.d_hp[i] = train ? b.take<float>(rt * D) : nullptr;
    }
    {   // every GRU launch exchanges through the same scratch: the largest launch is both encoder directions (forward:
        // D floats per row and step, backward: 3D) or one decoder layer
        const int bx = gru_team_batch(B);
        w.Bx = bx > 0 ? bx : B;
        const size_t rows = std::max<size_t>(2 * Ss, T) * (size_t)w.Bx;
        w.xbuf_floats = rows * D * (train ? 3 : 1);
        if (train && D == 512 && h->bwd_rs) w.xbuf_floats = std::max(w.xbuf_floats, gru_bwd_rs_xbuf_floats(2, w.Bx));      // (the reduce-scatter BPTT's ring, gru_rs.hip)
        w.xbuf = b.take<float>(w.xbuf_floats);
    }
    w.map_src = b.take<int32_t>(rs); w.nact_src = b.take<int32_t>(Ss + 1); w.nsrc = b.take<int32_t>(4); w.compact = false;
    w.map_tgt = b.take<int32_t>(rt); w.nact_tgt = b.take<int32_t>(T + 1); w.ntgt = b.take<int32_t>(4); w.compact_d = false;
    for (int k = 0; k < 3; ++k) { w.ord_perm[k] = b.take<int32_t>(w.Bx); w.ord_slens[k] = b.take<int32_t>(w.Bx); w.ord_ok[k] = false; w.ord_T[k] = w.ord_cpj[k] = 0; }
    w.hpick = b.take<float>((size_t)B * 2 * D);
    w.xlast = b.take<float>((size_t)B * 2 * D); w.gib = b.take<float>((size_t)B * 3 * D); w.svb = b.take<float>((size_t)B * 4 * D);
    w.dgib = b.take<float>(train ? (size_t)B * 3 * D : 0); w.dghb = b.take<float>(train ? (size_t)B * 3 * D : 0); w.dxl = b.take<float>(train ? (size_t)B * 2 * D : 0);
    w.mu = b.take<float>((size_t)B * R); w.lv = b.take<float>((size_t)B * R); w.z = b.take<float>((size_t)B * R);
    w.eps = b.take<float>((size_t)B * R); w.kld = b.take<float>((size_t)B * R);
    w.h0 = b.take<float>((size_t)B * D);
    w.hc = b.take<float>(rt * D); w.ho = b.take<float>(rt * D); w.logits = b.take<float>(rt * V);
    w.loss_samp = b.take<float>(rt); w.errt_samp = b.take<float>(rt);
    if (train) {
        w.dho = b.take<float>(rt * D); w.dhc = b.take<float>(rt * D);
        w.dhd[0] = b.take<float>(rt * D); w.dhd[1] = b.take<float>(rt * D);
        w.dgi_d = b.take<float>(rt * 3 * D); w.dgh_d = b.take<float>(rt * 3 * D);
        w.dh0 = b.take<float>((size_t)L * B * D); w.carry = b.take<float>((size_t)3 * w.Bx * D);
        w.dh0sum = b.take<float>((size_t)B * D);
        w.dz = b.take<float>((size_t)B * R); w.dmu = b.take<float>((size_t)B * R); w.dlv = b.take<float>((size_t)B * R);
        w.dhpick = b.take<float>((size_t)B * 2 * D);
        w.dhs[0] = b.take<float>(rs * 2 * D); w.dhs[1] = b.take<float>(rs * 2 * D);
        w.dgi_e = b.take<float>(rs * 6 * D); w.dgh_e = b.take<float>(rs * 6 * D);
        w.demb_src = b.take<float>(rs * D); w.demb_tgt = b.take<float>(rt * D);
        const bool g16 = h->cfg.compute_dtype == 1;
        w.dgi16_d = b.take<unsigned short>(g16 ? rt * 3 * D : 0); w.dgh16_d = b.take<unsigned short>(g16 ? rt * 3 * D : 0);
        w.dgi16_e = b.take<unsigned short>(g16 ? rs * 6 * D : 0); w.dgh16_e = b.take<unsigned short>(g16 ? rs * 6 * D : 0);
        w.scat = b.take<int32_t>(embed_scatter_scratch_ints(rs + rt, V));
        w.dew = b.take<float>(tab_s ? (size_t)V * 6 * D : (tab_t ? (size_t)V * 3 * D : 0));  // gate gradients of a table-fed layer summed by id
    }
}

// the one arena every call lays its buffers out in: grown (never shrunk) to `need` bytes
int reserve_ws(avae_ctx* h, size_t need)
{
    if (need > h->ws_cap) {
        if (h->ws) {                                          // (work enqueued on the old arena; a first arena has nothing to wait for)
            AV_CHECK(hipStreamSynchronize(h->stream));
            AV_CHECK(hipFree(h->ws));
        }
        h->ws = nullptr; h->ws_cap = 0;
        h->cnt_src = h->cnt_tgt = nullptr;                    // (pointed into the old arena)
        for (auto& sp : h->stamps) sp.dyn = nullptr;
        size_t cap = need + need / 8;
        AV_CHECK(hipMalloc(reinterpret_cast<void**>(&h->ws), cap));
        h->ws_cap = cap;
    }
    return 0;
}

int get_ws(avae_ctx* h, Ws& w, int B, int Ss, int St, bool train)
{
    return place_ws(h, "step", [&](Bump& b) { layout(h, b, w, B, Ss, St, train); });
}

static int grow_bf16(avae_ctx* h, unsigned short** buf, size_t* cap, size_t need)
{
    if (need <= *cap) return 0;
    if (*buf) {
        AV_CHECK(hipStreamSynchronize(h->stream));
        AV_CHECK(hipFree(*buf));
    }
    *buf = nullptr; *cap = 0;
    size_t n = need + need / 8;
    AV_CHECK(hipMalloc(reinterpret_cast<void**>(buf), n * sizeof(unsigned short)));
    *cap = n;
    return 0;
}

// what the host expects a device-side row count to be (the compact layout's counts: an earlier call's fill, build_compact); 0 = unknown
static int dyn_expected(const avae_ctx* h, const int* dyn, int dyn_kind)
{
    if (dyn_kind != 1 || !dyn) return 0;
    for (int i = 0; i < 3; ++i) if (dyn == h->expect_ptr[i]) return h->expect_val[i];
    return 0;
}

static GemmShape gemm_shape(const avae_ctx* h, const GemmCall& c)
{
    return GemmShape{c.a_mc, c.b_nc, c.M, c.N, c.K, c.ldc, c.accumulate, c.split_k, c.thin, c.dyn_kind, dyn_expected(h, c.dyn, c.dyn_kind),
                     c.allow_atomic, c.rows_are_batch, c.pair != nullptr, c.wgrad, h->cfg.compute_dtype, h->skinny != 0, h->dyn_split != 0, h->dyn_thin != 0};
}
// the one launch of a product the bf16-operand paths below shape themselves (gemm_bf16_nt / gemm_bf16_tn re-derive the K split): a
// weight gradient takes its split from the plan, anything else runs as it stands
static GemmLaunch bf16_launch(const avae_ctx* h, const GemmCall& c)
{
    if (!c.wgrad) return GemmLaunch{0, c.M, 0, 1, c.accumulate, kZeroNone, c.dyn_kind ? 1 : 0};
    GemmShape s = gemm_shape(h, c);
    s.compute_dtype = 1;
    return gemm_plan(s).launch[0];
}

// one launch of a plan: rows [l.row0, l.row0 + l.rows) of the call on the GEMM kernels of the handle's compute_dtype
static int gemm_launch(avae_ctx* h, const GemmCall& c, const GemmLaunch& l)
{
    if (c.pair && h->cfg.compute_dtype != 0) {     // the other GEMM kernels take one problem per launch
        GemmCall one = c, two = c;
        one.pair = two.pair = nullptr; two.keep_a16 = nullptr;
        two.A = c.pair->A; two.B = c.pair->B; two.C = c.pair->C; two.bias = c.pair->bias;
        AV_TRY(gemm_launch(h, one, l));
        return gemm_launch(h, two, l);
    }
    const float* A = c.A + (size_t)l.row0 * c.lda; float* C = c.C + (size_t)l.row0 * c.ldc;      // (row0 > 0: k-contiguous A only, gemm_plan)
    const int M = l.rows, N = c.N, K = c.K;
    const int* dyn = l.dyn ? c.dyn : nullptr; const int dyn_kind = l.dyn ? c.dyn_kind : 0;
    const Pair* pair = c.pair;
    GemmArgs g{A, c.B, C, c.bias, M, N, K, c.lda, c.ldb, c.ldc, c.alpha, l.accumulate, l.split_k, dyn, dyn_kind, dyn_expected(h, dyn, dyn_kind), l.thin,
               pair ? pair->A : nullptr, pair ? pair->B : nullptr, pair ? pair->C : nullptr, pair ? pair->bias : nullptr};
    Timed t(h, 0, 2.0 * M * N * K * (pair ? 2 : 1), dyn, dyn_kind == 1 ? M : (dyn_kind == 2 ? K : 0));
    if (h->cfg.compute_dtype == 1 && h->bf16_direct) {
        // bf16 operands rounded on the way into LDS, straight from the fp32 operands in whatever layout: no conversion passes
        AV_CHECK(gemm_bf16_direct(h->stream, c.a_mc, c.b_nc, g));
        return 0;
    }
    if (h->cfg.compute_dtype == 1) {
        // bf16 operands: convert (transposing [k][x] operands) into k-contiguous panels, then one NT kernel
        const int Kp = (K + 7) & ~7;
        unsigned short* a16 = nullptr;
        if (c.keep_a16 && !c.a_mc && Kp == K) a16 = c.keep_a16 + (size_t)l.row0 * K;      // a layer input: its bf16 copy [M][K] stays for the weight-gradient GEMM of the backward
        if (!a16) { AV_TRY(grow_bf16(h, &h->bfA, &h->bfA_cap, (size_t)M * Kp)); a16 = h->bfA; }
        AV_TRY(grow_bf16(h, &h->bfB, &h->bfB_cap, (size_t)N * Kp));
        AV_CHECK(cvt_bf16(h->stream, A, c.lda, c.a_mc, c.a_mc ? K : M, c.a_mc ? M : K, a16, Kp));
        AV_CHECK(cvt_bf16(h->stream, c.B, c.ldb, c.b_nc, c.b_nc ? K : N, c.b_nc ? N : K, h->bfB, Kp));
        g.nt8 = h->bf16_nt8;
        g.c16 = c.c16;
        AV_CHECK(gemm_bf16_nt(h->stream, a16, Kp, h->bfB, Kp, g));
        return 0;
    }
    if (c.c16) return fail(h, "the fp16 output panel exists in compute_dtype 1 only");
    // compute_dtype 2: fp32 operands split into 3 x bf16 on the fly (6 partial products, fp32-accurate); thin
    // row panels (a few rows, little work) stay on the exact-fp32 kernel's 32x128 tiles
    if (h->cfg.compute_dtype == 2 && !l.thin) AV_CHECK(gemm_f32s(h->stream, c.a_mc, c.b_nc, g));
    else AV_CHECK(gemm_f32(h->stream, c.a_mc, c.b_nc, g));
    return 0;
}

// the product as gemm_plan() shapes it: per launch, clear what the plan asks for, then launch
int gemm(avae_ctx* h, const GemmCall& c)
{
    const GemmPlan p = gemm_plan(gemm_shape(h, c));
    for (int i = 0; i < p.n; ++i) {
        const GemmLaunch& l = p.launch[i];
        float* C = c.C + (size_t)l.row0 * c.ldc;
        if (l.zero == kZeroAll) AV_CHECK(zero_fill(h->stream, C, sizeof(float) * (size_t)l.rows * c.N));
        if (l.zero == kZeroDynRows) AV_CHECK(zero_rows_dyn(h->stream, C, c.dyn, l.rows, c.N));
        AV_TRY(gemm_launch(h, c, l));
    }
    return 0;
}

// bf16 mode, A already bf16 and row-major (c.A16: (rows, lda), written by the producer -- the softmax gradient, a layer's h): as the A
// panel itself (a_mc = false: k-contiguous) or transposed once from the 2-byte source (a_mc = true); B converted as usual.
int gemm_bf16_pre(avae_ctx* h, const GemmCall& c)
{
    const GemmLaunch l = bf16_launch(h, c);
    const int M = c.M, N = c.N, K = c.K;
    GemmArgs g{nullptr, c.B, c.C, c.bias, M, N, K, c.lda, c.ldb, c.ldc, c.alpha, l.accumulate, l.split_k, c.dyn, c.dyn_kind, 0, 0, nullptr, nullptr, nullptr, nullptr};
    Timed t(h, 0, 2.0 * M * N * K, c.dyn, c.dyn_kind == 1 ? M : (c.dyn_kind == 2 ? K : 0));
    const int Kp = (K + 7) & ~7;
    const unsigned short* Ap = c.A16; int lda_p = c.lda;
    if (c.a_mc) {
        AV_TRY(grow_bf16(h, &h->bfA, &h->bfA_cap, (size_t)M * Kp));
        AV_CHECK(transpose_bf16(h->stream, c.A16, c.lda, K, M, h->bfA, Kp));
        Ap = h->bfA; lda_p = Kp;
    }
    AV_TRY(grow_bf16(h, &h->bfB, &h->bfB_cap, (size_t)N * Kp));
    AV_CHECK(cvt_bf16(h->stream, c.B, c.ldb, c.b_nc, c.b_nc ? K : N, c.b_nc ? N : K, h->bfB, Kp));
    g.nt8 = h->bf16_nt8;
    AV_CHECK(gemm_bf16_nt(h->stream, Ap, lda_p, h->bfB, Kp, g));
    return 0;
}

// bf16 mode, weight gradient C (M x N) += alpha * A^T B over K rows with BOTH operands row-major [k][x]: bf16 as a producer
// wrote them (c.A16 / c.B16) or fp32 converted row by row (c.A / c.B, no transpose); the GEMM reads them through transposing LDS
// loads (gemm_bf16_tn).  C holds the zero-filled gradient; c.dyn: device-side K.
int gemm_tn16(avae_ctx* h, const GemmCall& c)
{
    const GemmLaunch l = bf16_launch(h, c);
    const int M = c.M, N = c.N, K = c.K;
    GemmArgs g{nullptr, nullptr, c.C, c.bias, M, N, K, c.lda, c.ldb, c.ldc, c.alpha, l.accumulate, l.split_k, c.dyn, c.dyn_kind, 0, 0, nullptr, nullptr, nullptr, nullptr};      // (a bias: gemm_bf16_tn refuses it)
    Timed t(h, 0, 2.0 * M * N * K, c.dyn, c.dyn ? K : 0);
    const unsigned short* A16 = c.A16; const unsigned short* B16 = c.B16;
    int la = c.lda, lb = c.ldb;
    if (!A16) {
        la = (M + 7) & ~7;
        AV_TRY(grow_bf16(h, &h->bfA, &h->bfA_cap, (size_t)K * la));
        AV_CHECK(cvt_bf16(h->stream, c.A, c.lda, false, K, M, h->bfA, la));
        A16 = h->bfA;
    }
    if (!B16) {
        lb = (N + 7) & ~7;
        AV_TRY(grow_bf16(h, &h->bfB, &h->bfB_cap, (size_t)K * lb));
        AV_CHECK(cvt_bf16(h->stream, c.B, c.ldb, false, K, N, h->bfB, lb));
        B16 = h->bfB;
    }
    g.nt8 = h->bf16_nt8;
    if (h->bf16_nt8 && l.split_k > 1) {
        if (!h->slab) {
            const size_t n = (size_t)512 << 16;
            AV_CHECK(hipMalloc(reinterpret_cast<void**>(&h->slab), n * sizeof(float)));
            h->slab_floats = n;
        }
        g.slab = h->slab; g.slab_floats = h->slab_floats;
    }
    AV_CHECK(gemm_bf16_tn(h->stream, A16, la, B16, lb, g));
    return 0;
}
static bool tn16_ok(const avae_ctx* h, int M, int N) { return h->cfg.compute_dtype == 1 && h->bf16_tn && gemm_tn16_shape(M, N); }

void gru_geometry(int D, int njobs, int B, int* G, int* rpg)
{
    int HT = D / 16;
    int gmax = 512 / (njobs * HT); if (gmax < 1) gmax = 1; if (gmax > 16) gmax = 16;
    int g = (B + 15) / 16; if (g > gmax) g = gmax; if (g < 1) g = 1;
    int r = (B + g - 1) / g; r = (r + 15) / 16 * 16;
    g = (B + r - 1) / r;
    *G = g; *rpg = r;
}

struct Sched { float keepwd, anneal, lr; };
static Sched schedule(const avae_ctx* h)
{
    // src/model.py:77-80, float32 like the TF graph
    float rate = h->cfg.accelerate * (float)h->step;
    Sched s;
    s.keepwd = 1.f / (1.f + expf(-rate));
    s.anneal = tanhf(rate);
    s.lr = h->cfg.learn_rate / (sqrtf(rate) + 1.f);
    return s;
}

// The top encoder layer's backward direction is consumed at ONE position only -- the pick at len_b - 1 (model.py:135), the
// first step of the reversed sequence, from h = 0: its other S - 1 steps, their input projection and their whole BPTT are
// dead in the reference's graph (zero gradient; dR of that direction is exactly 0, oracle fixtures gnorm/encode/rnnL/bwd/R).
// The build computes that one step for B rows (gru_first_step_*) and runs the layer's GRU launches with the forward
// direction alone.  Same values as the full form (option enc_top1 = 0), a sixth of the encoder's work not executed.
static bool top_one_step(const avae_ctx* h) { return h->enc_top1 && h->cfg.rnn_layers >= 2; }

// The asynchronous fill hint of build_row_orders: real source positions and padded rows of an EARLIER call (no synchronisation;
// real < 0 or rows <= 0 while nothing has arrived).  Both words in ONE 8-byte load: the copy that lands them is 8 bytes, so a
// pair is never half of one call and half of another.  Shapes launches only, never a value.
// The pinned words are read ONCE per call, before the call enqueues a copy of its own (latch_hint): the layout, the row expectations, the
// BPTT form and the exchange protocol of one call all follow the same earlier call.  (Read where each is decided, the backward of a call
// saw the call's own fill whenever the copy had landed by then and the previous call's otherwise -- a FULL batch behind a long-tailed one
// took the compact layout of the one and the BPTT form of the other, by timing.)
struct FillHint { int32_t real, rows; };
static void latch_hint(avae_ctx* h)
{
    h->hint_seen = h->hint_host ? *reinterpret_cast<const volatile uint64_t*>(h->hint_host) : 0xffffffffull;
}
static FillHint fill_hint(const avae_ctx* h)
{
    const uint64_t pair = h->hint_seen;
    return {(int32_t)(uint32_t)(pair & 0xffffffffull), (int32_t)(uint32_t)(pair >> 32)};
}
// the share of the padded source positions that are real, as the host last saw it (1.0 while nothing has arrived)
static double expected_fill(const avae_ctx* h)
{
    const FillHint f = fill_hint(h);
    return (f.real > 0 && f.rows > 0) ? std::min(1.0, (double)f.real / (double)f.rows) : 1.0;
}
// Which BPTT team kernel a launch takes (option bwd_rs = 2).  The reduce-scatter form stores 64 KB per live row and step where the other
// form stores 6 KB, and wins only where a workgroup's teams run out of rows at different times so that most steps belong to one or two
// lone chains -- a ragged batch with a long tail.  Measured: batch 100 x 512 ragged (fill 0.30) -8 % of the step; RAGGED 256 x 64 (fill
// 0.44) a tie; FULL batches lose at every size (64 x 64 +1.8 %, 128 x 64 +4.7 %, 100 x 512 +2.3 %, 256 x 64 +5 %).  So the fill decides,
// not the row count.
static int rs_pick(const avae_ctx* h)
{
    if (h->bwd_rs != 2) return h->bwd_rs;
    return expected_fill(h) < 0.40 ? 1 : 0;
}
// the same regime in the exchange of every team kernel (option gru_spec = 2): a consumer's first operand load goes out without a probe
// round trip in front of it (GruArgs::spec): RAGGED 256 x 64 (fill 0.44) -1.5 %; forced on, a FULL 100 x 512 batch loses 1 %.
static int spec_pick(const avae_ctx* h)
{
    if (h->gru_spec != 2) return h->gru_spec;
    return expected_fill(h) < 0.60 ? 1 : 0;
}

// -------------------------------------------------------------------------------- forward pieces
// GRU launch arguments common to every call site
// (Bx: the launch geometry's rows where the compact layout is in place, 0 elsewhere; w.Bx for a plan that assumes it)
void gru_common(avae_ctx* h, const Ws& w, GruArgs& a, int njobs, int S, int B, int ldg, int ldh, const int32_t* lens, int Bx)
{
    const int D = h->cfg.dim_emb;
    a.njobs = njobs; a.S = S; a.B = B; a.D = D; a.ldg = ldg; a.ldh = ldh; a.lens = lens;
    a.Bx = Bx;
    gru_geometry(D, njobs, B, &a.G, &a.rows_per_group);
    a.p_begin = 0; a.p_end = S; a.counters = h->counters; a.err = h->errw; a.ablate = h->gru_ablate; a.force_slow = h->gru_force_slow;
    a.bf16 = h->cfg.compute_dtype == 1 && h->gru_bf16; a.stagger = h->gru_stagger; a.item_pipeline = h->gru_item;
    a.xbuf = w.xbuf; a.xbuf_floats = w.xbuf_floats; a.stamps = reinterpret_cast<unsigned long long*>(h->errw + 16); a.bwd_rs = h->bwd_rs != 0;
    a.ring = h->gru_ring;
}
// Row orders of this call (one launch, after prep_ids has the lengths): for every GRU launch shape of the step whose team
// kernels can skip padding, the batch rows sorted by length and dealt over the workgroups.  with_dec: the decoder runs too.
// with_enc = false: a call that runs the decoder alone (score_rows_dev).
int build_row_orders(avae_ctx* h, Ws& w, int B, int Ss, int T, bool with_dec, bool with_enc)
{
    latch_hint(h);
    if (!h->skip_pad || !h->persistent || w.Bx % 16) return 0;
    if (w.Bx != B && !h->compact) return 0;                   // (phantom rows need the compact layout)
    const int D = h->cfg.dim_emb;
    RowOrder ord[3]; int n = 0, which[3];
    auto want = [&](int k, int njobs, int S, int ldg, int ldh, const int32_t* lens, int add) {
        GruArgs a{};
        gru_common(h, w, a, njobs, S, B, ldg, ldh, lens, w.Bx);
        const GruPlan p = gru_plan(a, true, true);
        if (p.form != GruForm::team) return;
        ord[n] = RowOrder{lens, add, p.T, p.cpj, w.ord_perm[k], w.ord_slens[k]};
        which[n++] = k; w.ord_T[k] = p.T; w.ord_cpj[k] = p.cpj;
    };
    if (with_enc) want(0, 2, Ss, 6 * D, 2 * D, w.lens_src, 0);          // (every layer but a one-step top layer carries both directions)
    if (with_enc && top_one_step(h)) want(1, 1, Ss, 6 * D, 2 * D, w.lens_src, 0);
    if (with_dec) want(2, 1, T, 3 * D, D, w.lens_tgt, 1);
    if (!n) return 0;
    const bool hint = which[0] == 0 && h->compact == 2;        // (order 0 sorts the source rows: its step sum = the real source positions)
    if (hint && !h->hint_host) {
        int32_t* hp = nullptr;
        if (hipHostMalloc(reinterpret_cast<void**>(&hp), 64, hipHostMallocDefault) == hipSuccess) { hp[0] = -1; hp[1] = 0; h->hint_host = hp; }
    }
    h->hint_dev = reinterpret_cast<int32_t*>(h->errw + 100);     // (spare words of the error block)
    hipError_t e = row_order(h->stream, ord, n, B, w.Bx, std::max(Ss, T), hint ? h->hint_dev : nullptr, Ss * B);
    if (e == hipErrorInvalidValue) return 0;                 // (a batch beyond the kernel's LDS: no order, every step runs)
    AV_CHECK(e);
    if (hint && h->hint_host) {
        AV_CHECK(hipMemcpyAsync(const_cast<int32_t*>(h->hint_host), h->hint_dev, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    }
    for (int i = 0; i < n; ++i) w.ord_ok[which[i]] = true;
    return 0;
}
// bf16 mode: does a layer's forward AND backward launch both run the bf16 team kernels?  Then what passes between them (saved
// gates, h_prev) and on to the GEMMs (h, gate gradients) can be 16-bit.
static bool both_team_bf16(avae_ctx* h, const GruArgs& a, bool train)
{
    return train && a.bf16 && gru_plan(a, true, h->persistent != 0).full() && gru_plan(a, false, h->persistent != 0).full();
}
static void attach_sv16(avae_ctx* h, GruArgs& a, bool train) { a.sv16 = h->bf16_sv && both_team_bf16(h, a, train); }
static void attach_order(avae_ctx* h, const Ws& w, GruArgs& a, bool fwd, int k)
{
    const GruPlan p = gru_plan(a, fwd, h->persistent != 0);
    if (!w.ord_ok[k] || !p.team() || p.T != w.ord_T[k] || p.cpj != w.ord_cpj[k]) return;
    a.slens = w.ord_slens[k]; a.perm = w.ord_perm[k];
}

// Compact layout of this call, decided for the encoder stack and, with T > 1, for the decoder stack: possible where
// every GRU launch of the stack runs the team kernels (they address the external arrays through GruArgs::rowmap) and its first
// layer is table-fed (its per-token arrays keep the padded order).  Taken when the fill hint says the batch is ragged, and
// always for a batch without a team-kernel geometry of its own, which reaches the team kernels through it (Ws::Bx).
static int build_compact(avae_ctx* h, Ws& w, int B, int Ss, int T, bool train)
{
    w.compact = false; w.compact_d = false;
    h->expect_ptr[0] = h->expect_ptr[1] = h->expect_ptr[2] = nullptr;
    if (!h->compact || !h->persistent || Ss < 2 || !use_table(h, Ss * B, B)) return 0;
    const bool phantom = w.Bx != B;        // a batch without a team geometry of its own: the compact layout is what lets it run the team kernels at all
    if (phantom && !(w.ord_ok[0] && (w.ord_ok[1] || !top_one_step(h)))) return 0;
    if (h->compact == 2 && !phantom) {
        // auto: the layout pays where a good share of the padded positions is padding; on FULL batches the static row counts shape
        // the GEMM launches a little better (16.48 vs 16.71 ms at configs[1]; break-even at a fill of 0.93).  Nothing arrived yet: no layout.
        const FillHint f = fill_hint(h);
        if (f.real < 0 || f.rows <= 0 || (double)f.real >= 0.92 * (double)f.rows) return 0;
    }
    const int D = h->cfg.dim_emb;
    // every launch of the stack on the team kernels (training: the BPTT too)
    auto team = [&](int njobs, int S, int ldg, int ldh, const int32_t* lens) {
        GruArgs q{};
        gru_common(h, w, q, njobs, S, B, ldg, ldh, lens, w.Bx);
        return gru_plan(q, true, true).full() && (!train || gru_plan(q, false, true).full());
    };
    if (!team(2, Ss, 6 * D, 2 * D, w.lens_src) || (top_one_step(h) && !team(1, Ss, 6 * D, 2 * D, w.lens_src))) return 0;
    AV_CHECK(row_map(h->stream, w.lens_src, 0, Ss, B, w.map_src, w.nact_src, w.nsrc));
    w.compact = true;
    {   // the fill the host last saw, scaled to this call's rows: shapes the launches of the GEMMs over the compact rows (0: unknown)
        const FillHint f = fill_hint(h);
        const double fill = (f.real > 0 && f.rows > 0) ? std::min(1.0, (double)f.real / (double)f.rows) : 0.0;
        h->expect_ptr[0] = w.nsrc; h->expect_val[0] = (int)(fill * Ss * B);
        h->expect_ptr[1] = w.ntgt; h->expect_val[1] = (int)(fill * T * B);
        h->expect_ptr[2] = w.ntok; h->expect_val[2] = (int)(fill * T * B);      // (the unmasked decoder tokens: the same share of T x B for prefix masks)
    }
    // the decoder stack the same way (training / evaluation calls: T > 1): a row's steps end one behind its last non-eos target id
    if (T < 2 || !use_table(h, T * B, B) || h->compact == 3) return 0;      // (3: the encoder alone, for measurements)
    if ((phantom && !w.ord_ok[2]) || !team(1, T, 3 * D, D, nullptr)) return 0;
    AV_CHECK(row_map(h->stream, w.lens_tgt, 1, T, B, w.map_tgt, w.nact_tgt, w.ntgt));
    w.compact_d = true;
    return 0;
}
// The decoder half of build_compact for a call that runs the decoder alone (score_rows_dev): the same conditions, with the fill of the
// TARGET rows unknown to the host -- the layout is taken where the batch needs it to reach the team kernels (phantom rows) and left alone
// elsewhere (static row counts).
int build_compact_dec(avae_ctx* h, Ws& w, int B, int T)
{
    w.compact = false; w.compact_d = false;
    h->expect_ptr[0] = h->expect_ptr[1] = h->expect_ptr[2] = nullptr;
    if (!h->compact || h->compact == 3 || !h->persistent || T < 2 || !use_table(h, T * B, B)) return 0;
    if (w.Bx == B || !w.ord_ok[2]) return 0;
    GruArgs q{};
    gru_common(h, w, q, 1, T, B, 3 * h->cfg.dim_emb, h->cfg.dim_emb, nullptr, w.Bx);
    if (!gru_plan(q, true, true).full()) return 0;
    AV_CHECK(row_map(h->stream, w.lens_tgt, 1, T, B, w.map_tgt, w.nact_tgt, w.ntgt));
    w.compact_d = true;
    return 0;
}

static int run_encoder(avae_ctx* h, Ws& w, int B, int Ss, bool save)
{
    const int D = h->cfg.dim_emb, V = h->cfg.dim_tgt, L = h->cfg.rnn_layers;
    const int rs = Ss * B;
    const bool table = use_table(h, rs, B);
    h->cnt_src = table ? id_groups_count(w.grp_src, rs, V) : nullptr;
    // compact layout (build_compact): every array between the GEMMs and the GRU launches holds the real rows only; the GEMMs over
    // them take the device-side row count
    const int32_t* const cdyn = w.compact ? w.nsrc : nullptr;
    const int32_t* const cmap = w.compact ? w.map_src : nullptr;
    if (!table) AV_CHECK(embed_gather(h->stream, h->P + h->oE, w.src_tm, w.emb_src, rs, D, V));
    const float* x = w.emb_src; int In = D;
    for (int i = 0; i < L; ++i) {
        const GruP& p = h->enc[i];
        const bool top1 = i == L - 1 && top_one_step(h);      // forward direction only; the backward direction's one live step follows the loop
        if (i == 0 && table) {
            const int32_t* cnt = id_groups_count(w.grp_src, rs, V);
            AV_CHECK(id_groups_build(h->stream, w.src_tm, rs, V, w.grp_src, save));
            AV_CHECK(rows_gather(h->stream, w.emb_src, h->P + h->oE, id_groups_uid(w.grp_src, rs, V), cnt, std::min(V, rs), D));
            AV_TRY(gemm(h, nt(w.emb_src, D, h->P + p.W, D, w.ew, 6 * D, std::min(V, rs), 6 * D, D).biased(h->P + p.bW).rows(cnt)));
        } else if (i > 0 && w.act_e[i - 1]) {       // the layer below wrote its output as bf16: the A operand as it stands
            AV_TRY(gemm_bf16_pre(h, nt(nullptr, In, h->P + p.W, In, w.e_gi[i], 6 * D, rs, top1 ? 3 * D : 6 * D, In).a16(w.e_hs16[i - 1]).biased(h->P + p.bW).rows(cdyn)));
        } else {
        AV_TRY(gemm(h, nt(x, In, h->P + p.W, In, w.e_gi[i], 6 * D, rs, top1 ? 3 * D : 6 * D, In).biased(h->P + p.bW).rows(cdyn).keep(save ? w.x16_e[i] : nullptr)));
        }
        GruArgs a{};
        gru_common(h, w, a, top1 ? 1 : 2, Ss, B, 6 * D, 2 * D, w.lens_src, w.bx_enc());
        // table-fed layer: the team kernels read gi straight out of the per-id projection through a row index per token;
        // the other kernel forms get a per-token copy
        const bool table0 = i == 0 && table, indirect = table0 && gru_plan(a, true, h->persistent != 0).form == GruForm::team;
        if (indirect) AV_CHECK(rank_rows(h->stream, w.tokrow_src, w.src_tm, id_groups_rank(w.grp_src, rs, V), rs, V));
        else if (table0) AV_CHECK(rows_gather_ranked(h->stream, w.e_gi[0], w.ew, w.src_tm, id_groups_rank(w.grp_src, rs, V), rs, 6 * D, V));
        for (int d = 0; d < a.njobs; ++d) {
            GruJob& j = a.job[d];
            j.gi = (indirect ? w.ew : w.e_gi[i]) + d * 3 * D;
            j.gi_rows = indirect ? w.tokrow_src : nullptr;
            j.R = h->P + p.R + (int64_t)d * 3 * D * D;
            j.bR = h->P + p.bR + d * 3 * D;
            j.h0 = nullptr;
            j.hs = w.e_hs[i] + d * D;
            j.sv = save ? w.e_sv[d][i] : nullptr;
            j.hp = save ? w.e_hp[d][i] : nullptr;
            j.reverse = d;
        }
        attach_sv16(h, a, save);
        if (w.e_hs16[i] && tn16_ok(h, 3 * D, D) && both_team_bf16(h, a, save)) {      // h / h_prev as bf16 (a table-fed layer keeps h_prev fp32: its dR runs the fp32-operand path)
            w.act_e[i] = 1; w.acth_e[i] = 1;
            for (int d = 0; d < a.njobs; ++d) { a.job[d].hs16 = w.e_hs16[i] + d * D; a.job[d].hp16 = w.e_hp16[d][i]; }
        }
        attach_order(h, w, a, true, top1 ? 1 : 0);
        a.rowmap = cmap;
        a.spec = spec_pick(h);
        note_gru(h, top1 ? kRouteTopFwd : kRouteEncFwd, a, true);
        { Timed t(h, 1, 2.0 * a.njobs * Ss * (double)B * D * 3 * D);
          DeviceTurn turn(h);
          AV_GRU(gru_forward(h->stream, a, h->persistent != 0)); }
        if (top1) {
            // the backward direction at position len_b - 1: gi = W_b x[len_b - 1] + bW_b for B rows, then one cell step from h = 0
            const int64_t oWb = p.W + (int64_t)3 * D * In;
            if (w.act_e[i - 1]) AV_CHECK(pick_last16(h->stream, w.xlast, w.e_hs16[i - 1], w.lens_src, B, In, cmap));
            else
            AV_CHECK(pick_last(h->stream, w.xlast, x, w.lens_src, B, In, cmap));
            AV_TRY(gemm(h, nt(w.xlast, In, h->P + oWb, In, w.gib, 3 * D, B, 3 * D, In).biased(h->P + p.bW + 3 * D).batch_rows()));
        }
        x = w.e_hs[i]; In = 2 * D;
    }
    if (w.act_e[L - 1]) AV_CHECK(pick_last16(h->stream, w.hpick, w.e_hs16[L - 1], w.lens_src, B, 2 * D, cmap));
    else
    AV_CHECK(pick_last(h->stream, w.hpick, w.e_hs[L - 1], w.lens_src, B, 2 * D, cmap));
    if (top_one_step(h))      // (the pick copied the never-written backward half of the top layer's rows: overwritten here)
        AV_CHECK(gru_first_step_fwd(h->stream, w.gib, h->P + h->enc[L - 1].bR + 3 * D, w.hpick + D, 2 * D, save ? w.svb : nullptr, B, D, w.lens_src));
    return 0;
}

static int run_latent(avae_ctx* h, Ws& w, int B, bool train, uint64_t seed, const float* eps)
{
    const int D = h->cfg.dim_emb, R = h->cfg.dim_rep;
    {   // mu and lv (model.py:149-150): two affines of the same input, one launch
        const Pair lv{w.hpick, h->P + h->oWlv, w.lv, h->P + h->oBlv};
        AV_TRY(gemm(h, nn(w.hpick, 2 * D, h->P + h->oWmu, R, w.mu, R, B, R, 2 * D).biased(h->P + h->oBmu).with(&lv)));      // (rows = the batch rows: the skinny form for every batch size, gemm_plan)
    }
    AV_CHECK(latent_fwd(h->stream, w.mu, w.lv, eps, w.eps, w.z, w.kld, B * R, train ? 1 : 0, seed, h->cfg.free_bits, nullptr));      // (KL scalar: finalize_losses, fixed order)
    return 0;
}

// decoder GRU stack over T steps from per-layer initial states (state stride: layer * B * D; 0 = shared h0)
// share_rows (T, B) with share_n: the first layer's input projection is taken over the share_n rows of w.emb_tgt only and read through
// share_rows by the team kernels (rows of the batch that carry the same ids: score_rows_dev; the caller has checked the kernel form)
int run_decoder_rnn(avae_ctx* h, Ws& w, int B, int T, const float* state_in, int64_t state_stride, bool save, const int32_t* ids0, bool compact, const int32_t* share_rows, int share_n)
{
    // compact layout (build_compact): the arrays between the GEMMs and the GRU launches hold the real rows only
    const int32_t* const cdyn = compact ? w.ntgt : nullptr;
    const int32_t* const cmap = compact ? w.map_tgt : nullptr;
    const int D = h->cfg.dim_emb, L = h->cfg.rnn_layers;
    const int rt = T * B;
    const float* x = w.emb_tgt;
    h->cnt_tgt = ids0 ? id_groups_count(w.grp_tgt, rt, h->cfg.dim_tgt) : nullptr;
    for (int i = 0; i < L; ++i) {
        const GruP& p = h->dec[i];
        if (i == 0 && ids0) {       // (ids0: the layer input is E[ids0], not yet gathered -- use_table decided by the caller)
            const int V = h->cfg.dim_tgt;
            const int32_t* cnt = id_groups_count(w.grp_tgt, rt, V);
            AV_CHECK(id_groups_build(h->stream, ids0, rt, V, w.grp_tgt, save));
            AV_CHECK(rows_gather(h->stream, w.emb_tgt, h->P + h->oE, id_groups_uid(w.grp_tgt, rt, V), cnt, std::min(V, rt), D));
            AV_TRY(gemm(h, nt(w.emb_tgt, D, h->P + p.W, D, w.ew, 3 * D, std::min(V, rt), 3 * D, D).biased(h->P + p.bW).rows(cnt)));
        } else if (i == 0 && share_rows) {
            AV_TRY(gemm(h, nt(x, D, h->P + p.W, D, w.d_gi[0], 3 * D, share_n, 3 * D, D).biased(h->P + p.bW)));
        } else if (i > 0 && w.act_d[i - 1]) {
            AV_TRY(gemm_bf16_pre(h, nt(nullptr, D, h->P + p.W, D, w.d_gi[i], 3 * D, rt, 3 * D, D).a16(w.d_hd16[i - 1]).biased(h->P + p.bW).rows(cdyn)));
        } else {
        AV_TRY(gemm(h, nt(x, D, h->P + p.W, D, w.d_gi[i], 3 * D, rt, 3 * D, D).biased(h->P + p.bW).rows(cdyn).keep(save ? w.x16_d[i] : nullptr)));
        }
        GruArgs a{};
        gru_common(h, w, a, 1, T, B, 3 * D, D, nullptr, compact ? w.Bx : 0);
        GruJob& j = a.job[0];
        const bool table0 = i == 0 && ids0, indirect = table0 && gru_plan(a, true, h->persistent != 0).form == GruForm::team;
        if (indirect) AV_CHECK(rank_rows(h->stream, w.tokrow_tgt, ids0, id_groups_rank(w.grp_tgt, rt, h->cfg.dim_tgt), rt, h->cfg.dim_tgt));
        else if (table0) AV_CHECK(rows_gather_ranked(h->stream, w.d_gi[0], w.ew, ids0, id_groups_rank(w.grp_tgt, rt, h->cfg.dim_tgt), rt, 3 * D, h->cfg.dim_tgt));
        j.gi = indirect ? w.ew : w.d_gi[i]; j.gi_rows = indirect ? w.tokrow_tgt : nullptr;
        if (i == 0 && share_rows) j.gi_rows = share_rows;
        j.R = h->P + p.R; j.bR = h->P + p.bR;
        j.h0 = state_in + state_stride * i;
        j.hs = w.d_hd[i];
        j.sv = save ? w.d_sv[i] : nullptr;
        j.hp = save ? w.d_hp[i] : nullptr;
        j.reverse = 0;
        attach_sv16(h, a, save);
        if (w.d_hp16[i] && tn16_ok(h, 3 * D, D) && both_team_bf16(h, a, save)) {      // (the top layer keeps its fp32 output: the compaction and the out affine's gradient read it)
            if (i < L - 1) { w.act_d[i] = 1; j.hs16 = w.d_hd16[i]; }
            w.acth_d[i] = 1; j.hp16 = w.d_hp16[i];       // (a table-fed layer too: its dR reads bf16 dgh and this, gemm_tn16)
        }
        if (T > 1) attach_order(h, w, a, true, 2);
        a.rowmap = cmap;
        a.spec = spec_pick(h);
        note_gru(h, kRouteDecFwd, a, true);
        { Timed t(h, 1, 2.0 * T * (double)B * D * 3 * D);
          DeviceTurn turn(h);
          AV_GRU(gru_forward(h->stream, a, h->persistent != 0)); }
        x = w.d_hd[i];
    }
    return 0;
}

static int forward(avae_ctx* h, Ws& w, const int32_t* src, const int32_t* tgt, int B, int Ss, int St, bool train,
            uint64_t seed, const uint8_t* keep_mask, const float* eps, float inv_n)
{
    const int D = h->cfg.dim_emb, V = h->cfg.dim_tgt, R = h->cfg.dim_rep;
    const int T = St + 1, rt = T * B;
    Sched sc = schedule(h);
    PrepArgs p = prep_from_ws(w);
    p.src = src; p.tgt = tgt; p.B = B; p.Ss = Ss; p.St = St; p.eos = h->cfg.eos; p.bos = h->cfg.bos;
    p.train = train ? 1 : 0; p.keepwd = sc.keepwd; p.seed = seed; p.keep_mask = keep_mask;
    AV_CHECK(prep_ids(h->stream, p));
    AV_TRY(build_row_orders(h, w, B, Ss, T, true));
    AV_TRY(build_compact(h, w, B, Ss, T, train));
    const bool tab_t = use_table(h, rt, B);
    if (h->route.live) {
        avae_ctx::Route& r = h->route;
        r.tab_src = use_table(h, Ss * B, B); r.tab_tgt = tab_t; r.compact = w.compact; r.compact_d = w.compact_d; r.Bx = w.Bx; r.top1 = top_one_step(h);
    }
    AV_TRY(run_encoder(h, w, B, Ss, train));
    AV_TRY(run_latent(h, w, B, train, seed, eps));
    AV_TRY(gemm(h, nn(w.z, R, h->P + h->oWex, D, w.h0, D, B, D, R).biased(h->P + h->oBex).batch_rows()));
    if (tab_t) AV_TRY(run_decoder_rnn(h, w, B, T, w.h0, 0, train, w.lead, w.compact_d));
    else {
        AV_CHECK(embed_gather(h->stream, h->P + h->oE, w.lead, w.emb_tgt, rt, D, V));
        AV_TRY(run_decoder_rnn(h, w, B, T, w.h0, 0, train));
    }
    AV_TRY(run_logits_ce(h, w, rt, train, inv_n));
    float beta = h->cfg.kl_beta;
    AV_CHECK(finalize_losses(h->stream, h->losses, w.loss_samp, w.ntok, rt, w.kld, B * R, h->cfg.free_bits, 1.f / ((float)B * R), sc.anneal * beta));
    return 0;
}

// the kept positions of the top decoder layer -> out affine -> tied logits -> per-token softmax cross-entropy (w.loss_samp, w.errt_samp,
// w.pred in the compact order of prep_ids; model.py:161-180)
int run_logits_ce(avae_ctx* h, Ws& w, int rt, bool train, float inv_n)
{
    const int D = h->cfg.dim_emb, V = h->cfg.dim_tgt, L = h->cfg.rnn_layers;
    AV_CHECK(rows_gather(h->stream, w.hc, w.d_hd[L - 1], w.cidx, w.ntok, rt, D, w.compact_d ? w.map_tgt : nullptr));
    AV_TRY(gemm(h, nn(w.hc, D, h->P + h->oKout, D, w.ho, D, rt, D, D).biased(h->P + h->oBout).rows(w.ntok)));
    CeArgs c{};
    c.logits = w.logits; c.gold = w.gold; c.cidx = w.cidx; c.n_dev = w.ntok; c.n_max = rt; c.V = V;
    c.write_grad = train ? 1 : 0; c.inv_n = inv_n;
    if (train && h->cfg.compute_dtype == 1 && (V & 7) == 0) {      // bf16 mode: the gradient is written as the backward GEMMs' bf16 operand
        AV_TRY(grow_bf16(h, &h->bfP, &h->bfP_cap, (size_t)rt * V));
        c.grad16 = h->bfP;
        // ... and where the phased GEMM takes the whole product, the logits themselves go THERE as fp16 (2^-11 relative, finer than the bf16
        // gradient they become): no fp32 logits are written or read -- 4.3 GB of 10.8 GB at configs[2]
        if (h->logits16 && !h->bf16_direct && gemm_bf16_c16_takes(rt, V, D, w.ntok, h->bf16_nt8)) c.logits16 = 1;
    }
    GemmCall lg = nt(w.ho, D, h->P + h->oE, D, w.logits, V, rt, V, D).scaled(1.f / sqrtf((float)D)).rows(w.ntok);
    if (c.logits16) lg.form(0).c16 = h->bfP;      // (the panel: one launch of the phased kernel, as the probe above assumed)
    AV_TRY(gemm(h, lg));
    c.loss_samp = w.loss_samp; c.errt_samp = w.errt_samp; c.pred = w.pred; c.loss_acc = nullptr;      // (the scalar is summed from loss_samp in a fixed order: finalize_losses)
    AV_CHECK(softmax_ce(h->stream, c));
    return 0;
}

// Data-parallel hook protocol (include/argsim_vae.h).  A bucket whose gradients are final is not announced at once
// but right AFTER the next persistent GRU launch has been enqueued (or at the end of backward): a collective the
// callee starts then is ordered behind that launch and overlaps the GEMM phase that follows it.  Just BEFORE every
// persistent GRU launch the hook is called with bucket = AVAE_HOOK_FENCE so that the callee makes the compute stream
// wait for the collectives in flight: a persistent launch needs every CU (its workgroups exchange data inside the
// launch) and must never share the device with a kernel that may wait on a peer GPU.
static void fire_hook(avae_ctx* h, int bucket)
{
    if (h->hook && bucket >= 0 && bucket < (int)h->buckets.size()) h->hook_pending.push_back(bucket);
}
static void hook_fence(avae_ctx* h)
{
    if (h->hook) h->hook(h->hook_user, AVAE_HOOK_FENCE, 0, 0);
}
static void hook_flush(avae_ctx* h)
{
    for (int b : h->hook_pending) h->hook(h->hook_user, b, h->buckets[b].first, h->buckets[b].second);
    h->hook_pending.clear();
}

static int backward(avae_ctx* h, Ws& w, int B, int Ss, int St, float b_global)
{
    const int D = h->cfg.dim_emb, V = h->cfg.dim_tgt, R = h->cfg.dim_rep, L = h->cfg.rnn_layers;
    const int T = St + 1, rt = T * B, rs = Ss * B;
    const float isd = 1.f / sqrtf((float)D);
    Sched sc = schedule(h);
    hipStream_t st = h->stream;
    float* G = h->G; const float* P = h->P;
    h->hook_pending.clear();
    AV_CHECK(zero_fill(st, G, sizeof(float) * h->numel));

    // logits: dho = dlogits E / sqrt(D);  dE = dlogits^T ho / sqrt(D)
    if (h->cfg.compute_dtype == 1 && (V & 7) == 0) {
        // bf16 mode: softmax_ce_kernel left the gradient as bf16 (h->bfP): the first GEMM reads it as its A panel, the
        // second transposes the 2-byte source once -- no fp32 gradient is written or converted (10.7 GB less traffic per
        // step at configs[2]); same values as rounding the fp32 gradient, so the results do not change
        AV_TRY(gemm_bf16_pre(h, nn(nullptr, V, P + h->oE, D, w.dho, D, rt, D, V).a16(h->bfP).scaled(isd).rows(w.ntok)));
        const GemmCall dE = tn_grad(nullptr, V, w.ho, D, G + h->oE, D, V, D, rt).a16(h->bfP).scaled(isd).depth(w.ntok);
        AV_TRY(tn16_ok(h, V, D) ? gemm_tn16(h, dE) : gemm_bf16_pre(h, dE));      // (tn16: no transposed copy of the 2-byte gradient)
    } else {
    AV_TRY(gemm(h, nn(w.logits, V, P + h->oE, D, w.dho, D, rt, D, V).scaled(isd).rows(w.ntok).atomic()));
    // (V x D output over K = N rows: 256 tiles of 128x128 x 3 K slices, float atomics into the zero-filled G; the gather
    //  part is scatter-added at the end)
    AV_TRY(gemm(h, tn_grad(w.logits, V, w.ho, D, G + h->oE, D, V, D, rt).scaled(isd).depth(w.ntok)));
    }
    // out affine
    AV_TRY(gemm(h, tn_grad(w.hc, D, w.dho, D, G + h->oKout, D, D, D, rt).depth(w.ntok)));
    AV_CHECK(colsum(st, w.dho, rt, D, D, G + h->oBout, w.ntok));
    AV_TRY(gemm(h, nt(w.dho, D, P + h->oKout, D, w.dhc, D, rt, D, D).rows(w.ntok).atomic()));
    fire_hook(h, 0);
    const int32_t* const ddyn = w.compact_d ? w.ntgt : nullptr;        // compact decoder layout (build_compact)
    const int32_t* const dmap = w.compact_d ? w.map_tgt : nullptr;
    AV_CHECK(rows_expand(st, w.dhd[0], w.dhc, w.rank, rt, D, dmap));

    // decoder GRU stack, top layer first
    int cur = 0;
    for (int i = L - 1; i >= 0; --i) {
        const GruP& p = h->dec[i];
        GruArgs a{};
        gru_common(h, w, a, 1, T, B, 3 * D, D, nullptr, w.bx_dec());
        GruJob& j = a.job[0];
        j.R = P + p.R; j.sv = w.d_sv[i]; j.hp = w.d_hp[i]; j.reverse = 0;
        j.dh_out = w.dhd[cur]; j.dgi = w.dgi_d; j.dgh = w.dgh_d;
        j.dh0 = w.dh0 + (size_t)i * B * D; j.carry = w.carry;
        j.dbW = G + p.bW; j.dbR = G + p.bR;
        // bf16 mode: the team kernels write the gate gradients as bf16, the operand of the three GEMMs below as it stands
        // (a table-fed layer keeps fp32: its gradients are summed by id first)
        const bool team16 = tn16_ok(h, 3 * D, D) && a.bf16 && gru_plan(a, false, h->persistent != 0).full();
        const bool g16 = team16 && !(i == 0 && use_table(h, rt, B));
        // (a table-fed layer: dgh alone as bf16 -- its dR GEMM reads it and the bf16 h_prev as they stand; dgi stays fp32 for the sum by id)
        const bool gh16 = !g16 && w.dgh16_d && team16 && w.acth_d[i];
        if (g16) { j.dgi16 = w.dgi16_d; j.dgh16 = w.dgh16_d; }
        if (gh16) j.dgh16 = w.dgh16_d;
        if (!g16 && !gh16 && w.acth_d[i]) return fail(h, "internal: the forward kept this layer's h_prev as bf16 only and the backward cannot read it");
        if (w.acth_d[i]) j.hp16 = w.d_hp16[i];
        attach_sv16(h, a, true);
        attach_order(h, w, a, false, 2);
        a.rowmap = dmap;
        if (dmap && i == 0) j.dgi_by_pos = 1;       // (table-fed: its gate gradients are summed by token id)
        a.bwd_rs = rs_pick(h); a.spec = spec_pick(h);
        if (h->route.live) h->route.rs = a.bwd_rs;
        note_gru(h, kRouteDecBwd, a, false);
        hook_fence(h);
        { Timed t(h, 2, 2.0 * T * (double)B * D * 3 * D);
          DeviceTurn turn(h);
          AV_GRU(gru_backward(st, a, h->persistent != 0)); }
        hook_flush(h);
        if (i == 0 && use_table(h, rt, B)) {
            // table-fed layer: gate gradients summed by id, then dW = (sum)^T E and dE += (sum) W over V rows
            const int32_t* cnt = id_groups_count(w.grp_tgt, rt, V); const int U = std::min(V, rt);
            AV_CHECK(rows_group_sum(st, w.dew, w.lead, w.dgi_d, rt, 3 * D, V, w.grp_tgt));
            AV_TRY(gemm(h, tn_grad(w.dew, 3 * D, w.emb_tgt, D, G + p.W, D, 3 * D, D, U).depth(cnt)));
            if (gh16) AV_TRY(gemm_tn16(h, tn_grad(nullptr, 3 * D, nullptr, D, G + p.R, D, 3 * D, D, rt).a16(w.dgh16_d).b16(w.d_hp16[i]).depth(ddyn)));
            else
            AV_TRY(gemm(h, tn_grad(w.dgh_d, 3 * D, w.d_hp[i], D, G + p.R, D, 3 * D, D, rt).depth(ddyn)));
            AV_TRY(gemm(h, nn(w.dew, 3 * D, P + p.W, D, w.demb_tgt, D, U, D, 3 * D).rows(cnt).atomic()));
            AV_CHECK(rows_add_indexed(st, G + h->oE, w.demb_tgt, id_groups_uid(w.grp_tgt, rt, V), cnt, U, D));
        } else if (g16) {
            const float* x = i == 0 ? w.emb_tgt : w.d_hd[i - 1];
            AV_TRY(gemm_tn16(h, tn_grad(nullptr, 3 * D, x, D, G + p.W, D, 3 * D, D, rt).a16(w.dgi16_d).b16((i > 0 && w.act_d[i - 1]) ? w.d_hd16[i - 1] : w.x16_kept_d(i)).depth(ddyn)));
            AV_TRY(gemm_tn16(h, tn_grad(nullptr, 3 * D, w.d_hp[i], D, G + p.R, D, 3 * D, D, rt).a16(w.dgh16_d).b16(w.acth_d[i] ? w.d_hp16[i] : nullptr).depth(ddyn)));
            float* dx = i == 0 ? w.demb_tgt : w.dhd[cur ^ 1];
            AV_TRY(gemm_bf16_pre(h, nn(nullptr, 3 * D, P + p.W, D, dx, D, rt, D, 3 * D).a16(w.dgi16_d).rows(ddyn)));
        } else {
        const float* x = i == 0 ? w.emb_tgt : w.d_hd[i - 1];
        {   // dW = dgi^T x and dR = dgh^T h_prev: same shape over the same rows, one launch
            const Pair dR{w.dgh_d, w.d_hp[i], G + p.R, nullptr};
            AV_TRY(gemm(h, tn_grad(w.dgi_d, 3 * D, x, D, G + p.W, D, 3 * D, D, rt).depth(ddyn).with(&dR)));
        }
        float* dx = i == 0 ? w.demb_tgt : w.dhd[cur ^ 1];
        AV_TRY(gemm(h, nn(w.dgi_d, 3 * D, P + p.W, D, dx, D, rt, D, 3 * D).rows(ddyn).atomic()));
        }
        cur ^= 1;
        fire_hook(h, 1 + (L - 1 - i));
    }

    // latent
    AV_CHECK(add3(st, w.dh0sum, w.dh0, L > 1 ? w.dh0 + (size_t)B * D : nullptr, L > 2 ? w.dh0 + (size_t)2 * B * D : nullptr, (int64_t)B * D));
    for (int i = 3; i < L; ++i) AV_CHECK(add3(st, w.dh0sum, w.dh0sum, w.dh0 + (size_t)i * B * D, nullptr, (int64_t)B * D));
    AV_TRY(gemm(h, tn_grad(w.z, R, w.dh0sum, D, G + h->oWex, D, R, D, B)));
    AV_CHECK(colsum(st, w.dh0sum, B, D, D, G + h->oBex, nullptr));
    AV_TRY(gemm(h, nt(w.dh0sum, D, P + h->oWex, D, w.dz, R, B, R, D)));
    float bg = b_global > 0.f ? b_global : (float)B;
    AV_CHECK(latent_bwd(st, w.dz, w.mu, w.lv, w.eps, w.dmu, w.dlv, B, R, sc.anneal * h->cfg.kl_beta / (bg * R), h->cfg.free_bits));
    {
        const Pair dlv{w.hpick, w.dlv, G + h->oWlv, nullptr};
        AV_TRY(gemm(h, tn_grad(w.hpick, 2 * D, w.dmu, R, G + h->oWmu, R, 2 * D, R, B).with(&dlv)));
    }
    AV_CHECK(colsum(st, w.dmu, B, R, R, G + h->oBmu, nullptr));
    AV_CHECK(colsum(st, w.dlv, B, R, R, G + h->oBlv, nullptr));
    AV_TRY(gemm(h, nt(w.dmu, R, P + h->oWmu, R, w.dhpick, 2 * D, B, 2 * D, R)));
    AV_TRY(gemm(h, nt(w.dlv, R, P + h->oWlv, R, w.dhpick, 2 * D, B, 2 * D, R).plus()));
    fire_hook(h, 1 + L);
    const int32_t* const cdyn = w.compact ? w.nsrc : nullptr;        // compact encoder layout (build_compact)
    const int32_t* const cmap = w.compact ? w.map_src : nullptr;
    if (w.compact) {
        AV_CHECK(zero_rows_dyn(st, w.dhs[0], w.nsrc, rs, 2 * D));
        AV_CHECK(pick_last_add(st, w.dhs[0], w.dhpick, w.lens_src, B, 2 * D, cmap));
    } else
    AV_CHECK(pick_last_bwd(st, w.dhs[0], w.dhpick, w.lens_src, Ss, B, 2 * D));

    // encoder stack
    cur = 0;
    for (int i = L - 1; i >= 0; --i) {
        const GruP& p = h->enc[i];
        const int In = i == 0 ? D : 2 * D;
        const bool top1 = i == L - 1 && top_one_step(h);
        const int64_t oWb = p.W + (int64_t)3 * D * In;
        if (top1) {
            // backward direction of the top layer: BPTT of its one live step (dH = the pick's gradient, nothing carried),
            // bias gradients = column sums over the B rows; dR of this direction stays exactly zero (h_prev = 0)
            AV_CHECK(gru_first_step_bwd(st, w.dhpick + D, 2 * D, w.svb, w.dgib, w.dghb, B, D, w.lens_src));
            AV_CHECK(colsum(st, w.dgib, B, 3 * D, 3 * D, G + p.bW + 3 * D, nullptr));
            AV_CHECK(colsum(st, w.dghb, B, 3 * D, 3 * D, G + p.bR + 3 * D, nullptr));
        }
        GruArgs a{};
        gru_common(h, w, a, top1 ? 1 : 2, Ss, B, 6 * D, 2 * D, w.lens_src, w.bx_enc());
        for (int d = 0; d < a.njobs; ++d) {
            GruJob& j = a.job[d];
            j.R = P + p.R + (int64_t)d * 3 * D * D; j.sv = w.e_sv[d][i]; j.hp = w.e_hp[d][i]; j.reverse = d;
            j.dh_out = w.dhs[cur] + d * D; j.dgi = w.dgi_e + d * 3 * D; j.dgh = w.dgh_e + d * 3 * D;
            j.dh0 = nullptr; j.carry = w.carry + (size_t)d * w.Bx * D;
            j.dbW = G + p.bW + d * 3 * D; j.dbR = G + p.bR + d * 3 * D;
        }
        const bool team16 = tn16_ok(h, 3 * D, D) && a.bf16 && gru_plan(a, false, h->persistent != 0).full();
        const bool g16 = team16 && !(i == 0 && use_table(h, rs, B));
        const bool gh16 = !g16 && w.dgh16_e && team16 && w.acth_e[i];      // (table-fed layer: see the decoder)
        if (g16) for (int d = 0; d < a.njobs; ++d) { a.job[d].dgi16 = w.dgi16_e + d * 3 * D; a.job[d].dgh16 = w.dgh16_e + d * 3 * D; }
        if (gh16) for (int d = 0; d < a.njobs; ++d) a.job[d].dgh16 = w.dgh16_e + d * 3 * D;
        if (!g16 && !gh16 && w.acth_e[i]) return fail(h, "internal: the forward kept this layer's h_prev as bf16 only and the backward cannot read it");
        if (w.acth_e[i]) for (int d = 0; d < a.njobs; ++d) a.job[d].hp16 = w.e_hp16[d][i];
        attach_sv16(h, a, true);
        attach_order(h, w, a, false, top1 ? 1 : 0);
        a.rowmap = cmap;
        if (cmap && i == 0) for (int d = 0; d < a.njobs; ++d) a.job[d].dgi_by_pos = 1;      // (table-fed: its gate gradients are summed by token id)
        a.bwd_rs = rs_pick(h); a.spec = spec_pick(h);
        note_gru(h, top1 ? kRouteTopBwd : kRouteEncBwd, a, false);
        hook_fence(h);
        { Timed t(h, 2, 2.0 * a.njobs * (Ss - 1) * (double)B * D * 3 * D);
          DeviceTurn turn(h);
          AV_GRU(gru_backward(st, a, h->persistent != 0)); }
        hook_flush(h);
        const bool table = i == 0 && use_table(h, rs, B);
        const float* x = i == 0 ? w.emb_src : w.e_hs[i - 1];
        float* dx = i == 0 ? w.demb_src : w.dhs[cur ^ 1];
        if (g16) {
            // bf16 mode, gate gradients written as bf16 by the BPTT kernels: every GEMM of the layer reads them as they stand
            const int Gc = a.njobs * 3 * D;                          // gate columns of the directions that ran
            if (i == 0) {     // first layer (per-token form): input gradient, scatter, embedding bucket -- the fixed order of announcements
                AV_TRY(gemm_bf16_pre(h, nn(nullptr, 6 * D, P + p.W, In, dx, In, rs, In, Gc).a16(w.dgi16_e)));
                AV_CHECK(embed_scatter_add2(st, G + h->oE, w.src_tm, w.demb_src, rs, w.lead, w.demb_tgt, use_table(h, rt, B) ? 0 : rt, D, V, w.scat));
                fire_hook(h, 2 + 2 * L);
                hook_flush(h);
            }
            AV_TRY(gemm_tn16(h, tn_grad(nullptr, 6 * D, x, In, G + p.W, In, Gc, In, rs).a16(w.dgi16_e).b16((i > 0 && w.act_e[i - 1]) ? w.e_hs16[i - 1] : w.x16_kept_e(i)).depth(cdyn)));
            if (top1) AV_TRY(gemm(h, tn_grad(w.dgib, 3 * D, w.xlast, In, G + oWb, In, 3 * D, In, B)));
            for (int d = 0; d < a.njobs; ++d)
                AV_TRY(gemm_tn16(h, tn_grad(nullptr, 6 * D, w.e_hp[d][i], D, G + p.R + (int64_t)d * 3 * D * D, D, 3 * D, D, rs).a16(w.dgh16_e + d * 3 * D).b16(w.acth_e[i] ? w.e_hp16[d][i] : nullptr).depth(cdyn)));
            if (i > 0) AV_TRY(gemm_bf16_pre(h, nn(nullptr, 6 * D, P + p.W, In, dx, In, rs, In, Gc).a16(w.dgi16_e).rows(cdyn)));
            if (top1) {
                AV_TRY(gemm(h, nn(w.dgib, 3 * D, P + oWb, In, w.dxl, In, B, In, 3 * D).atomic()));
                AV_CHECK(pick_last_add(st, dx, w.dxl, w.lens_src, B, In, cmap));
            }
            cur ^= 1;
            fire_hook(h, 2 + L + (L - 1 - i));
            continue;
        }
        if (i == 0) {
            // First encoder layer: its input gradient completes the embedding gradient.  That bucket is ALWAYS announced here,
            // before this layer's two weight-gradient GEMMs (its all-reduce runs beside them), and this layer's own bucket
            // ends backward -- in the table-fed form and in the per-token form alike.  The order of announcements must not
            // depend on the batch shape: data-parallel ranks pad their shards to their own longest row, so one rank can be
            // on either side of use_table() while its peer is on the other, and the collectives are paired by call order.
            if (table) {
                // table-fed layer (use_table): gate gradients summed by id, dE[present] += (sum) W over U rows
                const int32_t* cnt = id_groups_count(w.grp_src, rs, V); const int U = std::min(V, rs);
                AV_CHECK(rows_group_sum(st, w.dew, w.src_tm, w.dgi_e, rs, 6 * D, V, w.grp_src));
                AV_TRY(gemm(h, nn(w.dew, 6 * D, P + p.W, D, w.demb_src, D, U, D, 6 * D).rows(cnt).atomic()));
                AV_CHECK(rows_add_indexed(st, G + h->oE, w.demb_src, id_groups_uid(w.grp_src, rs, V), cnt, U, D));
            } else
            AV_TRY(gemm(h, nn(w.dgi_e, 6 * D, P + p.W, In, dx, In, rs, In, 6 * D).atomic()));
            // gather gradients of the per-token forms on top of the logits term (a table-fed side has added its rows already)
            AV_CHECK(embed_scatter_add2(st, G + h->oE, w.src_tm, w.demb_src, table ? 0 : rs, w.lead, w.demb_tgt, use_table(h, rt, B) ? 0 : rt, D, V, w.scat));
            fire_hook(h, 2 + 2 * L);
            hook_flush(h);
            if (table) {
                const int32_t* cnt = id_groups_count(w.grp_src, rs, V); const int U = std::min(V, rs);
                AV_TRY(gemm(h, tn_grad(w.dew, 6 * D, w.emb_src, D, G + p.W, D, 6 * D, D, U).depth(cnt)));
            } else
            AV_TRY(gemm(h, tn_grad(w.dgi_e, 6 * D, x, In, G + p.W, In, 6 * D, In, rs)));
        } else if (top1) {
            AV_TRY(gemm(h, tn_grad(w.dgi_e, 6 * D, x, In, G + p.W, In, 3 * D, In, rs).depth(cdyn)));       // forward direction's W
            AV_TRY(gemm(h, tn_grad(w.dgib, 3 * D, w.xlast, In, G + oWb, In, 3 * D, In, B)));              // backward direction's: B rows
        } else
        AV_TRY(gemm(h, tn_grad(w.dgi_e, 6 * D, x, In, G + p.W, In, 6 * D, In, rs).depth(cdyn)));
        if (gh16) {
            for (int d = 0; d < a.njobs; ++d)
                AV_TRY(gemm_tn16(h, tn_grad(nullptr, 6 * D, nullptr, D, G + p.R + (int64_t)d * 3 * D * D, D, 3 * D, D, rs).a16(w.dgh16_e + d * 3 * D).b16(w.e_hp16[d][i]).depth(cdyn)));
        } else if (top1) AV_TRY(gemm(h, tn_grad(w.dgh_e, 6 * D, w.e_hp[0][i], D, G + p.R, D, 3 * D, D, rs).depth(cdyn)));
        else {   // dR of the two directions: same shape, one launch
            const Pair bwd{w.dgh_e + 3 * D, w.e_hp[1][i], G + p.R + (int64_t)3 * D * D, nullptr};
            AV_TRY(gemm(h, tn_grad(w.dgh_e, 6 * D, w.e_hp[0][i], D, G + p.R, D, 3 * D, D, rs).depth(cdyn).with(&bwd)));
        }
        if (i > 0)
        AV_TRY(gemm(h, nn(w.dgi_e, 6 * D, P + p.W, In, dx, In, rs, In, top1 ? 3 * D : 6 * D).rows(cdyn).atomic()));
        if (top1) {       // the backward direction's input gradient lands on the rows at len_b - 1
            AV_TRY(gemm(h, nn(w.dgib, 3 * D, P + oWb, In, w.dxl, In, B, In, 3 * D).atomic()));      // (B rows: the skinny form, 43 -> 16 us)
            AV_CHECK(pick_last_add(st, dx, w.dxl, w.lens_src, B, In, cmap));
        }
        cur ^= 1;
        fire_hook(h, 2 + L + (L - 1 - i));
    }
    hook_flush(h);
    return 0;
}

// encoder + latent affines over src (b, t): w.mu, w.lv
int encode_ws(avae_ctx* h, Ws& w, const int32_t* src, int b, int t)
{
    PrepArgs p = prep_from_ws(w);
    p.src = src; p.tgt = src; p.B = b; p.Ss = t; p.St = 1; p.eos = h->cfg.eos; p.bos = h->cfg.bos;
    // tgt is unused by the encoder; feed the first column of src as a 1-wide dummy target
    AV_CHECK(prep_ids(h->stream, p));
    AV_TRY(build_row_orders(h, w, b, t, 2, false));
    AV_TRY(build_compact(h, w, b, t, 0, false));
    AV_TRY(run_encoder(h, w, b, t, false));
    AV_TRY(run_latent(h, w, b, false, 0, nullptr));
    return 0;
}

}}  // namespace avae::host

using namespace avae::host;

extern "C" {

int avae_get_schedule(avae_handle h, float out[3])
{
    if (!h || !out) return 1;
    Sched s = schedule(h); out[0] = s.keepwd; out[1] = s.anneal; out[2] = s.lr;
    return 0;
}

int avae_forward_backward(avae_handle h, const int32_t* src, const int32_t* tgt, int32_t B, int32_t Ss, int32_t St,
                          uint64_t seed, const uint8_t* keep_mask, const float* eps, float n_tok_global, float b_global)
{
    if (!h) return 1;
    AV_TRY(check_bound(h));
    if (B < 1 || Ss < 1 || St < 1) return fail(h, "empty batch");
    AV_CHECK(hipSetDevice(h->device));
    Ws w;
    AV_TRY(get_ws(h, w, B, Ss, St, true));
    h->B = B; h->Ss = Ss; h->St = St;
    h->route = avae_ctx::Route{};
    for (auto& g : h->route.gru) g[0] = -1;
    struct Noting { avae_ctx* h; ~Noting() { h->route.live = false; } } noting{h};      // (the route is noted while THIS call enqueues, whichever way it returns)
    h->route.live = true;
    AV_TRY(forward(h, w, src, tgt, B, Ss, St, true, seed, keep_mask, eps, n_tok_global > 0.f ? 1.f / n_tok_global : 0.f));
    AV_TRY(backward(h, w, B, Ss, St, b_global));
    if (h->persistent && !h->first_step_checked) {
        // the first step of a handle is checked at once (one synchronisation, once): a device shared with another process
        // fails HERE with the message above instead of training on past time-outs until the losses are next fetched
        h->first_step_checked = true;
        AV_TRY(check_gru_err(h));
    }
    return 0;
}

int avae_adam_step(avae_handle h)
{
    if (!h) return 1;
    AV_TRY(check_bound(h));
    Sched sc = schedule(h);
    const double b1 = 0.9, b2 = 0.999;
    double t = (double)h->step + 1.0;
    AdamArgs a{h->P, h->G, h->M, h->Vv, h->numel, (float)(sc.lr * std::sqrt(1.0 - std::pow(b2, t)) / (1.0 - std::pow(b1, t))), 0.9f, 0.999f, 1e-8f, h->errw};
    AV_CHECK(adam_tf(h->stream, a));
    h->step += 1;
    return 0;
}

int avae_train_step(avae_handle h, const int32_t* src, const int32_t* tgt, int32_t B, int32_t Ss, int32_t St,
                    uint64_t seed, const uint8_t* keep_mask, const float* eps)
{
    AV_TRY(avae_forward_backward(h, src, tgt, B, Ss, St, seed, keep_mask, eps, 0.f, 0.f));
    return avae_adam_step(h);
}

int avae_get_losses(avae_handle h, float out[3])
{
    if (!h || !out) return 1;
    AV_CHECK(hipMemcpyAsync(out, h->losses, 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    AV_TRY(check_gru_err(h));
    return 0;
}

int avae_eval(avae_handle h, const int32_t* src, const int32_t* tgt, int32_t B, int32_t Ss, int32_t St,
              float* errt_samp, float* loss_gen_samp, float* loss_kld_samp, int32_t* n_out)
{
    if (!h) return 1;
    AV_TRY(check_bound(h));
    if (B < 1 || Ss < 1 || St < 1) return fail(h, "empty batch");
    AV_CHECK(hipSetDevice(h->device));
    Ws w;
    AV_TRY(get_ws(h, w, B, Ss, St, false));
    AV_TRY(forward(h, w, src, tgt, B, Ss, St, false, 0, nullptr, nullptr, 0.f));
    const size_t rt = (size_t)(St + 1) * B;
    if (errt_samp) AV_CHECK(hipMemcpyAsync(errt_samp, w.errt_samp, rt * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (loss_gen_samp) AV_CHECK(hipMemcpyAsync(loss_gen_samp, w.loss_samp, rt * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (loss_kld_samp) AV_CHECK(hipMemcpyAsync(loss_kld_samp, w.kld, (size_t)B * h->cfg.dim_rep * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    int n = 0;
    AV_CHECK(hipMemcpyAsync(&n, w.ntok, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    AV_TRY(check_gru_err(h));
    if (n_out) *n_out = n;
    return 0;
}

int avae_encode(avae_handle h, const int32_t* src, int32_t b, int32_t t, float* z_out, float* lv_out)
{
    if (!h) return 1;
    AV_TRY(check_bound(h));
    if (b < 1 || t < 1) return fail(h, "empty batch");
    AV_CHECK(hipSetDevice(h->device));
    Ws w;
    AV_TRY(get_ws(h, w, b, t, 1, false));
    AV_TRY(encode_ws(h, w, src, b, t));
    const size_t n = (size_t)b * h->cfg.dim_rep * sizeof(float);
    if (z_out) AV_CHECK(hipMemcpyAsync(z_out, w.mu, n, hipMemcpyDeviceToDevice, h->stream));
    if (lv_out) AV_CHECK(hipMemcpyAsync(lv_out, w.lv, n, hipMemcpyDeviceToDevice, h->stream));
    return check_gru_err(h);       // synchronises: a z computed past a timed-out wait must not be handed out silently
}

}  // extern "C"
