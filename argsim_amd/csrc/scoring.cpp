// scoring.cpp -- scoring and search over latent rows: the importance-weighted likelihood (avae_score, avae_score_z; score.hip) and
// nearest neighbours (avae_knn; knn.hip), the aggregate-posterior diagnostics (avae_agg_logq, avae_latent_moments; agg.hip) and the
// kernel two-sample test (avae_mmd, avae_mmd_relabel; mmd.hip).
#include "ctx.h"

using namespace avae;
using namespace avae::host;

namespace {

// -------------------------------------------------------------------------------- importance-weighted likelihood
// (contract: include/argsim_vae.h, avae_score / avae_score_z; kernels: score.hip)
constexpr int kScoreErrWord = 110;      // spare word of the error block: an eps that is not finite (score_draw)

// Decoder batch size of the score path.  The k draws of B rows are k * B decoder rows; they run in batches of at most N rows, N the
// largest count whose logits panel (N x (S_tgt + 1) x V floats) stays within what avae_eval sizes for the same batch (B rows) or 2^27
// floats (the panel of the headline batch, 256 x 65 x 8192, is 1.02 x that), whichever is larger, and at most 256 rows, the headline
// batch the GRU team kernels are tuned at.  A batch is rc rows under kc draws each (their first-layer projection is shared, run_decoder_rnn):
// all k draws of N / k rows, or N draws of one row where k > N.
struct ScorePlan { int N, rc, kc; };
ScorePlan score_plan(const avae_ctx* h, int B, int k, int St)
{
    const size_t per_row = (size_t)(St + 1) * h->cfg.dim_tgt;
    const size_t budget = std::max((size_t)B * per_row, (size_t)1 << 27);
    size_t n = std::min<size_t>({(size_t)k * B, (size_t)256, budget / per_row});
    ScorePlan p; p.N = (int)std::max<size_t>(n, 1);
    if (k <= p.N) { p.kc = k; p.rc = std::min(B, p.N / k); }
    else { p.kc = p.N; p.rc = 1; }
    return p;
}
// buffers of a score call that outlive its decoder batches: behind the largest layout of the call, in the same arena
struct ScoreWs { float *z, *lat, *logpx; int32_t *ntok, *tgt_rep, *ids0, *tokrow; };
void score_layout(Bump& b, ScoreWs& s, int B, int k, int R, int N, int St)
{
    const size_t kb = (size_t)k * B, T = St + 1;
    s.z = b.take<float>(kb * R); s.lat = b.take<float>(kb); s.logpx = b.take<float>(kb); s.ntok = b.take<int32_t>(B);
    s.tgt_rep = b.take<int32_t>((size_t)N * St); s.ids0 = b.take<int32_t>((size_t)N * T); s.tokrow = b.take<int32_t>((size_t)N * T);
}
// one arena for the encoder pass over (B, Ss) (Ss = 0: none), every decoder batch of the plan and the buffers above
int score_ws(avae_ctx* h, const ScorePlan& sp, int B, int k, int Ss, int St, ScoreWs& s)
{
    Ws w; size_t top = 0; std::vector<int> seen;
    if (Ss > 0) { Bump b{nullptr}; layout(h, b, w, B, Ss, 1, false); top = b.off; }
    for (int r0 = 0; r0 < B; r0 += sp.rc)
        for (int k0 = 0; k0 < k; k0 += sp.kc) {
            const int n = std::min(sp.rc, B - r0) * std::min(sp.kc, k - k0);
            if (std::find(seen.begin(), seen.end(), n) != seen.end()) continue;
            seen.push_back(n);
            Bump b{nullptr}; layout(h, b, w, n, 1, St, false); top = std::max(top, b.off);
        }
    return place_ws(h, "score", [&](Bump& b) { score_layout(b, s, B, k, h->cfg.dim_rep, sp.N, St); }, top);
}

// Teacher-forced log p(tgt row | z row) for the k draws of B rows, s.z in decoder-batch order (kernels.h ScoreDraw): s.logpx (k, B),
// s.ntok (B).  Per decoder batch: the ids of its rows replicated over its draws on the device, prep (lead = [bos] + tgt, no word dropout,
// mask, compaction), initial state from z, the decoder stack with ONE first-layer projection for the draws of a row (the per-id table
// where the batch is table-fed, else the projection of the block's own rows read through a row index), logits, per-token CE, row sums.
int score_rows_dev(avae_ctx* h, const ScorePlan& sp, const ScoreWs& s, const int32_t* tgt, int B, int k, int St)
{
    const int D = h->cfg.dim_emb, V = h->cfg.dim_tgt, R = h->cfg.dim_rep;
    const int T = St + 1;
    h->score_plan[0] = sp.N; h->score_plan[1] = sp.rc; h->score_plan[2] = sp.kc; h->score_plan[3] = 0;
    for (int r0 = 0; r0 < B; r0 += sp.rc)
        for (int k0 = 0; k0 < k; k0 += sp.kc) {
            const int rc = std::min(sp.rc, B - r0), kc = std::min(sp.kc, k - k0), n = rc * kc, rt = T * n;
            const float* z = s.z + ((size_t)r0 * k + (size_t)k0 * rc) * R;
            Ws w;
            Bump real{h->ws};
            layout(h, real, w, n, 1, St, false);
            const int32_t* ids = tgt + (size_t)r0 * St;
            if (kc > 1) { AV_CHECK(tile_ids(h->stream, s.tgt_rep, ids, n, rc, St)); ids = s.tgt_rep; }
            PrepArgs p = prep_from_ws(w);
            p.src = ids; p.tgt = ids; p.B = n; p.Ss = 1; p.St = St; p.eos = h->cfg.eos; p.bos = h->cfg.bos;      // (no source here: its first column stands in)
            AV_CHECK(prep_ids(h->stream, p));
            AV_TRY(build_row_orders(h, w, n, 1, T, true, false));
            AV_TRY(build_compact_dec(h, w, n, T));
            AV_TRY(gemm(h, nn(z, R, h->P + h->oWex, D, w.h0, D, n, D, R).biased(h->P + h->oBex).batch_rows()));
            if (use_table(h, rt, n)) AV_TRY(run_decoder_rnn(h, w, n, T, w.h0, 0, false, w.lead, w.compact_d));
            else {
                GruArgs q{};
                gru_common(h, w, q, 1, T, n, 3 * D, D, nullptr, 0);
                if (kc > 1 && gru_plan(q, true, h->persistent != 0).form == GruForm::team) {
                    AV_CHECK(lead_rows(h->stream, w.lead, T, n, rc, s.ids0, s.tokrow));
                    AV_CHECK(embed_gather(h->stream, h->P + h->oE, s.ids0, w.emb_tgt, T * rc, D, V));
                    AV_TRY(run_decoder_rnn(h, w, n, T, w.h0, 0, false, nullptr, false, s.tokrow, T * rc));
                    ++h->score_plan[3];
                } else {
                    AV_CHECK(embed_gather(h->stream, h->P + h->oE, w.lead, w.emb_tgt, rt, D, V));
                    AV_TRY(run_decoder_rnn(h, w, n, T, w.h0, 0, false));
                }
            }
            AV_TRY(run_logits_ce(h, w, rt, false, 0.f));
            const ScoreRows sr{w.loss_samp, w.rank, T, n, rc, k0, r0, B, s.logpx, s.ntok};
            AV_CHECK(score_rows(h->stream, sr));
        }
    return 0;
}

// the GRU time-out word and the eps word in one synchronisation
int check_score_err(avae_ctx* h)
{
    int e = 0;
    AV_CHECK(hipMemcpyAsync(&e, h->errw + kScoreErrWord, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    const int gru = check_gru_err(h);
    if (e) (void)hipMemsetAsync(h->errw + kScoreErrWord, 0, sizeof(int), h->stream);      // (whatever the GRU check said: the flag must not outlive its call)
    if (gru) return gru;
    if (e) return fail(h, "score: eps holds a value that is not finite");
    return 0;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- nearest neighbours (contract: include/argsim_vae.h, avae_knn; kernels: knn.hip)
int avae_knn(avae_handle h, const float* q, int32_t n, const float* bank, int32_t N, int32_t dim, const avae_knn_config* kc,
             int64_t* out_idx, float* out_score)
{
    if (!h) return 1;
    if (!kc) return fail(h, "knn config is null");
    if (!q || !out_idx || !out_score) return fail(h, "knn: q, out_idx and out_score must be given");
    if (n < 1 || N < 0) return fail(h, "knn: n must be >= 1 and N >= 0");
    if (N > 0 && !bank) return fail(h, "knn: bank must be given");
    if (N > 0x7fffffff - 256) return fail(h, "knn: at most 2^31 - 256 bank rows per call (stream a larger bank with carry)");
    if (kc->k < 1 || kc->k > 32) return fail(h, "knn: k must be in [1, 32]");
    if (kc->metric < 0 || kc->metric > 2) return fail(h, "knn: metric must be 0 (dot), 1 (cosine) or 2 (squared Euclidean)");
    if (kc->idx_base < 0 || kc->self_base < -1) return fail(h, "knn: idx_base must be >= 0 and self_base >= -1");
    if (kc->carry != 0 && kc->carry != 1) return fail(h, "knn: carry must be 0 or 1");
    if (kc->reserved != 0) return fail(h, "knn: the reserved field must be 0");
    AV_TRY(check_rows(h, "knn", dim, "q and bank", {q, bank}));
    AV_CHECK(hipSetDevice(h->device));
    const KnnPlan p = knn_plan(n, N, kc->k, h->knn_chunk);
    if ((long long)p.qtiles * std::max(p.parts, 1) > 0x7fffffffLL) return fail(h, "knn: too many (query tile, bank part) workgroups for one launch");
    KnnWs w{};
    AV_TRY(place_ws(h, "knn", [&](Bump& b) {
        w.qn = b.take<float>((size_t)n); w.bn = b.take<float>((size_t)N);
        w.lists = b.take<unsigned long long>((size_t)n * p.parts * kc->k);
    }));
    KnnArgs a{};
    a.q = q; a.bank = bank; a.n = n; a.N = N; a.dim = dim; a.k = kc->k; a.metric = kc->metric;
    a.idx_base = kc->idx_base; a.self_base = kc->self_base; a.carry = kc->carry; a.out_idx = out_idx; a.out_score = out_score;
    AV_CHECK(knn_search(h->stream, a, p, w));
    return 0;
}

// ---------------------------------------------------------------- aggregate-posterior diagnostics (contract: include/argsim_vae.h, avae_agg_logq /
// avae_latent_moments; kernels: agg.hip)
int avae_agg_logq(avae_handle h, const float* z, int32_t n, const float* mu, const float* lv, int32_t N, int32_t dim, const avae_agg_config* ac,
                  float* logq, float* logqx)
{
    if (!h) return 1;
    if (!ac) return fail(h, "agg config is null");
    if (!z || !mu || !lv || !logq) return fail(h, "agg: z, mu, lv and logq must be given");
    if (n < 1 || N < 1) return fail(h, "agg: n and N must be >= 1");
    if (N > 0x7fffffff - 256) return fail(h, "agg: at most 2^31 - 256 bank rows per call");
    AV_TRY(check_rows(h, "agg", dim, "z, mu and lv", {z, mu, lv}));
    if (ac->self_base < -1) return fail(h, "agg: self_base must be >= -1");
    if (ac->self_base >= 0 && ac->self_base + (int64_t)n > (int64_t)N) return fail(h, "agg: self_base + n exceeds N (query i's own bank row is self_base + i)");
    if (logqx && ac->self_base < 0) return fail(h, "agg: logqx needs self_base >= 0");
    if (ac->reserved[0] != 0 || ac->reserved[1] != 0) return fail(h, "agg: the reserved fields must be 0");
    AV_CHECK(hipSetDevice(h->device));
    const AggPlan p = agg_plan(n, N, dim, h->agg_chunk);
    if ((long long)p.qtiles * p.parts > 0x7fffffffLL) return fail(h, "agg: too many (query tile, bank part) workgroups for one launch");
    float2* parts_ms = nullptr;
    AV_TRY(place_ws(h, "agg", [&](Bump& b) { parts_ms = b.take<float2>((size_t)p.parts * n); }));
    AggArgs a{};
    a.z = z; a.mu = mu; a.lv = lv; a.n = n; a.N = N; a.dim = dim; a.self_base = ac->self_base; a.logq = logq; a.logqx = logqx;
    AV_CHECK(agg_logq(h->stream, a, p, parts_ms));
    return 0;
}

int avae_latent_moments(avae_handle h, const float* mu, const float* lv, int32_t N, int32_t dim, float* out)
{
    if (!h) return 1;
    if (!mu || !lv || !out) return fail(h, "moments: mu, lv and out must be given");
    if (N < 1) return fail(h, "moments: N must be >= 1");
    if (N > 0x7fffffff - 256) return fail(h, "moments: at most 2^31 - 256 rows per call");
    AV_TRY(check_rows(h, "moments", dim, "mu and lv", {mu, lv}));
    AV_CHECK(hipSetDevice(h->device));
    double *mean = nullptr, *part = nullptr;
    AV_TRY(place_ws(h, "moments", [&](Bump& b) { mean = b.take<double>((size_t)dim); part = b.take<double>((size_t)moments_blocks(N) * 3 * dim); }));
    AV_CHECK(latent_moments(h->stream, mu, lv, N, dim, out, mean, part));
    return 0;
}

// ---------------------------------------------------------------- kernel two-sample test (contract: include/argsim_vae.h, avae_mmd /
// avae_mmd_relabel; kernels: mmd.hip)
int avae_mmd(avae_handle h, const float* x, int32_t N, int32_t dim, const avae_mmd_config* mc, const uint64_t* valid, const uint64_t* inA,
             double* stat, double* pvalue, int32_t* counts, double* sums, double* ull, double* witness, int32_t* stat_out)
{
    if (!h) return 1;
    if (!mc) return fail(h, "mmd config is null");
    if (!x) return fail(h, "mmd: x is null");
    if (!valid || !inA) return fail(h, "mmd: valid and inA must be given");
    if (!stat || !pvalue || !counts || !stat_out) return fail(h, "mmd: stat, pvalue, counts and stat_out must be given");
    if (N < 2 || N > kMmdMaxN) return fail(h, "mmd: N must be in [2, 2^17]");
    if (dim < 4 || dim > 1024 || (dim & 3)) return fail(h, "mmd: dim must be a multiple of 4 in [4, 1024]");
    if (mc->G < 1 || mc->G > kMmdMaxG) return fail(h, "mmd: G must be in [1, 64]");
    if (mc->P < 0 || (long long)mc->G * (1LL + mc->P) > kMmdMaxQ) return fail(h, "mmd: P must be >= 0 with G (1 + P) <= 16384");
    if (mc->kernel < 0 || mc->kernel > 1) return fail(h, "mmd: kernel must be 0 (rbf) or 1 (energy)");
    if (mc->metric < 0 || mc->metric > 1) return fail(h, "mmd: metric must be 0 (euclidean) or 1 (cosine)");
    if (mc->kernel == 0) {
        if (mc->nbw < 1 || mc->nbw > kMmdMaxBw) return fail(h, "mmd: nbw must be in [1, 8]");
        for (int b = 0; b < mc->nbw; ++b)
            if (!(mc->gamma[b] > 0.0) || !std::isfinite(mc->gamma[b])) return fail(h, "mmd: gamma[" + std::to_string(b) + "] must be finite and > 0");
    }
    if ((uintptr_t)x & 15) return fail(h, "mmd: x must be 16-byte aligned");
    if (mc->reserved != 0) return fail(h, "mmd: the reserved field must be 0");
    AV_CHECK(hipSetDevice(h->device));
    int cus = 0, lds = 0;
    AV_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
    AV_CHECK(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, h->device));
    if (lds < kMmdLds) return fail(h, "mmd: the device gives a workgroup less than the 160 KiB of LDS the pair pass is planned for");
    const int G = mc->G, P = mc->P;
    const MmdPlan plan = mmd_plan(N, dim, G, P, h->mmd_chunk, cus);
    // Workspace, every buffer on a 256-byte boundary: m and n (G, 2) int, the word of the first bad relabeling, with the
    // cosine the row norms (N), the row tiles' partial sums of a pass (tiles, 2, cap), U_AA and U_BB (G, 1 + P, 2) unless the caller gives
    // sums, U_LL (G) unless the caller gives ull
    MmdArgs a{};
    a.x = x; a.valid = reinterpret_cast<const unsigned long long*>(valid); a.inA = reinterpret_cast<const unsigned long long*>(inA);
    a.N = N; a.dim = dim; a.W = plan.W; a.G = G; a.P = P; a.kernel = mc->kernel; a.nbw = mc->kernel == 0 ? mc->nbw : 0; a.cap = plan.cap;
    for (int b = 0; b < a.nbw; ++b) a.gamma[b] = mc->gamma[b];
    a.witness = witness;
    int* dcounts = nullptr; unsigned* bad = nullptr; double* rnorm = nullptr;
    AV_TRY(place_ws(h, "mmd", [&](Bump& b) {
        dcounts = b.take<int>(2 * (size_t)G);
        bad = b.take<unsigned>(1);
        rnorm = b.opt<double>(mc->metric == 1, (size_t)N);
        a.part = b.take<double>((size_t)plan.tiles * 2 * plan.cap);
        a.sums = sums ? sums : b.take<double>(2 * (size_t)G * (1 + P));
        a.ull = ull ? ull : b.take<double>((size_t)G);
    }));
    a.rnorm = rnorm; a.counts = dcounts;
    AV_CHECK(mmd_prepare(h->stream, a, dcounts));
    // m, n >= 2 is the one check that needs the masks: G pairs of counts come to the host before anything is written
    std::vector<int> hc(2 * (size_t)G);
    AV_CHECK(hipMemcpyAsync(hc.data(), dcounts, hc.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    AV_CHECK(hipStreamSynchronize(h->stream));
    for (int g = 0; g < G; ++g)
        if (hc[2 * g] < 2 || hc[2 * g + 1] < 2)
            return fail(h, "mmd: comparison " + std::to_string(g) + " has " + std::to_string(hc[2 * g]) + " rows in A and " + std::to_string(hc[2 * g + 1]) +
                               " in B; both samples need at least 2");
    AV_CHECK(hipMemcpyAsync(counts, dcounts, hc.size() * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
    AV_CHECK(hipMemsetAsync(bad, 0xff, sizeof(unsigned), h->stream));
    AV_CHECK(mmd_pairs(h->stream, a, plan));
    if (witness) AV_CHECK(mmd_witness(h->stream, a, plan));
    AV_CHECK(mmd_stats(h->stream, a, stat, pvalue, bad, stat_out));
    return 0;
}

int avae_mmd_relabel(avae_handle h, int32_t N, int32_t G, int32_t P, const uint64_t* valid, uint64_t* inA, uint64_t seed)
{
    if (!h) return 1;
    if (!valid || !inA) return fail(h, "mmd relabel: valid and inA must be given");
    if (N < 2 || N > kMmdMaxN) return fail(h, "mmd relabel: N must be in [2, 2^17]");
    if (G < 1 || G > kMmdMaxG) return fail(h, "mmd relabel: G must be in [1, 64]");
    if (P < 0 || (long long)G * (1LL + P) > kMmdMaxQ) return fail(h, "mmd relabel: P must be >= 0 with G (1 + P) <= 16384");
    AV_CHECK(hipSetDevice(h->device));
    AV_CHECK(mmd_relabel(h->stream, reinterpret_cast<const unsigned long long*>(valid), reinterpret_cast<unsigned long long*>(inA), N, G, P, seed));
    return 0;
}

int avae_score_z(avae_handle h, const float* z, const int32_t* tgt, int32_t b, int32_t St, float* logpx, int32_t* ntok)
{
    if (!h) return 1;
    AV_TRY(check_bound(h));
    if (b < 1 || St < 1) return fail(h, "score: empty batch");
    if (!z || !tgt || !logpx) return fail(h, "score: z, tgt and logpx must be given");
    AV_CHECK(hipSetDevice(h->device));
    const int R = h->cfg.dim_rep;
    const ScorePlan sp = score_plan(h, b, 1, St);
    ScoreWs s;
    AV_TRY(score_ws(h, sp, b, 1, 0, St, s));
    AV_CHECK(hipMemcpyAsync(s.z, z, (size_t)b * R * sizeof(float), hipMemcpyDeviceToDevice, h->stream));      // (k = 1: the batch order is the row order)
    AV_TRY(score_rows_dev(h, sp, s, tgt, b, 1, St));
    AV_CHECK(hipMemcpyAsync(logpx, s.logpx, (size_t)b * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (ntok) AV_CHECK(hipMemcpyAsync(ntok, s.ntok, (size_t)b * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
    return check_gru_err(h);
}

int avae_score(avae_handle h, const int32_t* src, const int32_t* tgt, int32_t B, int32_t Ss, int32_t St, const avae_score_config* sc,
               const float* eps, float* eps_out, float* logpx, float* logw, float* bound, int32_t* ntok)
{
    if (!h) return 1;
    AV_TRY(check_bound(h));
    if (!sc) return fail(h, "score config is null");
    if (sc->k < 1) return fail(h, "score: k must be >= 1");
    if (B < 1 || Ss < 1 || St < 1) return fail(h, "score: empty batch");
    if (!bound) return fail(h, "score: bound must be given");
    if (!src || !tgt) return fail(h, "score: src and tgt must be given");
    const int R = h->cfg.dim_rep, k = sc->k;
    if (k > (1 << 20) || R > (1 << 20)) return fail(h, "score: the draw index holds 2^20 draws and 2^20 latent dimensions");
    if ((size_t)k * B > ((size_t)1 << 30) / R) return fail(h, "score: k x B x dim_rep exceeds 2^30 elements");
    AV_CHECK(hipSetDevice(h->device));
    const ScorePlan sp = score_plan(h, B, k, St);
    ScoreWs s;
    AV_TRY(score_ws(h, sp, B, k, Ss, St, s));
    {   // the encoder once, then every draw
        Ws w;
        Bump real{h->ws};
        layout(h, real, w, B, Ss, 1, false);
        AV_TRY(encode_ws(h, w, src, B, Ss));
        const ScoreDraw d{w.mu, w.lv, eps, eps_out, s.z, s.lat, h->errw + kScoreErrWord, k, B, R, sp.rc, sc->seed};
        AV_CHECK(score_draw(h->stream, d));
    }
    AV_TRY(score_rows_dev(h, sp, s, tgt, B, k, St));
    AV_CHECK(score_bound(h->stream, s.logpx, s.lat, k, B, logw, bound));
    if (logpx) AV_CHECK(hipMemcpyAsync(logpx, s.logpx, (size_t)k * B * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (ntok) AV_CHECK(hipMemcpyAsync(ntok, s.ntok, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
    return check_score_err(h);
}

}  // extern "C"
