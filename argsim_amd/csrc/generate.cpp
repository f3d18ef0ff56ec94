// generate.cpp -- generation from a latent row: one decoder step, the greedy and sampled loops (stepwise and in one persistent
// launch, decode.hip), the nucleus, beam search (beam.hip).  Every user of h->scratch lays its buffers out over a Bump (place_scratch).
#include "ctx.h"

using namespace avae;
using namespace avae::host;

namespace {

// ---- the users of h->scratch: each a struct of pointers and one layout over a Bump, run by place_scratch for the size and the pointers
// the launch-per-token loop: ping-pong states (L, b, D), time-major ids (steps + 1, b), logp / nkept (steps, b) where sampled / nucleus
struct StepwiseBufs { float* state[2]; int32_t* ids_tm; float* logp_tm; int32_t* nkept_tm; };
void stepwise_layout(Bump& b, StepwiseBufs& s, size_t sn, int rows, int steps, bool sampled, bool nucleus)
{
    s.state[0] = b.take<float>(sn); s.state[1] = b.take<float>(sn);
    s.ids_tm = b.take<int32_t>((size_t)(steps + 1) * rows);
    s.logp_tm = b.opt<float>(sampled, (size_t)steps * rows);
    s.nkept_tm = b.opt<int32_t>(nucleus, (size_t)steps * rows);
}
// the one-launch loop: every scratch buffer of DecodeArgs (kernels.h); G = workgroups.  No kernel indexes from one buffer into another.
void decode_layout(Bump& bp, DecodeArgs& a, int G, int b, int steps, int D, int V, int L, bool sampled, bool topk, bool logp, bool nkept)
{
    const size_t sn = (size_t)L * b * D, gb = (size_t)G * b;
    a.state[0] = bp.take<float>(sn); a.state[1] = bp.take<float>(sn);
    a.o = bp.take<float>((size_t)b * D); a.part_val = bp.take<float>(gb);
    a.part_x = bp.opt<float>(sampled, gb); a.part_m = bp.opt<float>(sampled, gb); a.part_s = bp.opt<float>(sampled, gb);
    a.logits = bp.opt<float>(topk, (size_t)b * V);
    a.logp_tm = bp.opt<float>(logp, (size_t)steps * b);
    a.part_idx = bp.take<int32_t>(gb); a.ids_tm = bp.take<int32_t>((size_t)(steps + 1) * b);
    a.kept = bp.take<int32_t>(1); a.bar = bp.take<unsigned>(1);
    a.nkept_tm = bp.opt<int32_t>(nkept, (size_t)steps * b);
}
// the beam search over groups of at most rmax = gmax * W decoder rows: ping-pong state / cum / fin / len, the group lattice (steps, rmax),
// the step's candidates (rmax, W), len^alpha, the live counts per step, the first token's bos ids
struct BeamBufs {
    float *state[2], *cum[2], *lat_cum, *cand_sc, *lenpow;
    int32_t *fin[2], *len[2], *lat_parent, *lat_token, *cand_tok, *cand_cnt, *live, *bos;
};
void beam_layout(Bump& b, BeamBufs& q, size_t sn, int rmax, int W, int steps, int gmax)
{
    const size_t lat = (size_t)steps * rmax, cand = (size_t)rmax * W;
    for (int i = 0; i < 2; ++i) q.state[i] = b.take<float>(sn);
    for (int i = 0; i < 2; ++i) q.cum[i] = b.take<float>(rmax);
    q.lat_cum = b.take<float>(lat); q.cand_sc = b.take<float>(cand); q.lenpow = b.take<float>((size_t)steps + 1);
    for (int i = 0; i < 2; ++i) q.fin[i] = b.take<int32_t>(rmax);
    for (int i = 0; i < 2; ++i) q.len[i] = b.take<int32_t>(rmax);
    q.lat_parent = b.take<int32_t>(lat); q.lat_token = b.take<int32_t>(lat);
    q.cand_tok = b.take<int32_t>(cand); q.cand_cnt = b.take<int32_t>(rmax);
    q.live = b.take<int32_t>(steps); q.bos = b.take<int32_t>(gmax);
}

// (n, b) time-major on the host -> (b, steps) row-major, `fill` beyond the n steps
template <class T> std::vector<T> rows_major(const T* tm, int n, int b, int steps, T fill)
{
    std::vector<T> out((size_t)b * steps, fill);
    for (int s = 0; s < n; ++s) for (int i = 0; i < b; ++i) out[(size_t)i * steps + s] = tm[(size_t)s * b + i];
    return out;
}

}  // namespace

extern "C" {

int avae_decode_init(avae_handle h, const float* z, int32_t b, float* state_out)
{
    if (!h) return 1;
    AV_TRY(check_bound(h));
    AV_CHECK(hipSetDevice(h->device));
    const int D = h->cfg.dim_emb, R = h->cfg.dim_rep, L = h->cfg.rnn_layers;
    AV_TRY(gemm(h, nn(z, R, h->P + h->oWex, D, state_out, D, b, D, R).biased(h->P + h->oBex).batch_rows()));
    for (int i = 1; i < L; ++i)
        AV_CHECK(hipMemcpyAsync(state_out + (size_t)i * b * D, state_out, (size_t)b * D * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

// one decoder step up to the tied logits (b, V) in w.logits
static int decode_logits_ws(avae_handle h, Ws& w, const int32_t* lead, const float* state_in, int b, float* state_out)
{
    const int D = h->cfg.dim_emb, V = h->cfg.dim_tgt, L = h->cfg.rnn_layers;
    AV_CHECK(embed_gather(h->stream, h->P + h->oE, lead, w.emb_tgt, b, D, V));
    AV_TRY(run_decoder_rnn(h, w, b, 1, state_in, (int64_t)b * D, false));
    for (int i = 0; i < L && state_out; ++i)      // (null: the caller takes the new state out of w.d_hd itself -- the beam search gathers it by parent)
        AV_CHECK(hipMemcpyAsync(state_out + (size_t)i * b * D, w.d_hd[i], (size_t)b * D * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    AV_TRY(gemm(h, nn(w.d_hd[L - 1], D, h->P + h->oKout, D, w.ho, D, b, D, D).biased(h->P + h->oBout)));
    AV_TRY(gemm(h, nt(w.ho, D, h->P + h->oE, D, w.logits, V, b, V, D).scaled(1.f / sqrtf((float)D))));
    return 0;
}
static int decode_step_ws(avae_handle h, Ws& w, const int32_t* lead, const float* state_in, int b, int32_t* pred_out, float* state_out)
{
    AV_TRY(decode_logits_ws(h, w, lead, state_in, b, state_out));
    AV_CHECK(argmax_rows(h->stream, w.logits, pred_out, b, h->cfg.dim_tgt));
    return 0;
}

int avae_decode_step(avae_handle h, const int32_t* lead, const float* state_in, int32_t b, int32_t* pred_out, float* state_out)
{
    if (!h) return 1;
    AV_TRY(check_bound(h));
    AV_CHECK(hipSetDevice(h->device));
    Ws w;
    AV_TRY(get_ws(h, w, b, 1, 1, false));
    AV_TRY(decode_step_ws(h, w, lead, state_in, b, pred_out, state_out));
    return check_gru_err(h);
}

// one launch sequence per token with a host check every 16 tokens: the fallback where the persistent kernel's geometry
// does not fit (decode.hip) and the reference form for tests (option "persistent" = 0).  sp: null = the greedy loop of
// model.py:204-219; else sampled decoding (sample_rows per token: a row that has emitted eos stays eos, logp_out optional); top_p > 0:
// with the nucleus (sample_rows_p; nkept_out optional)
static int decode_stepwise(avae_handle h, const float* z, int32_t b, int32_t steps, const SampleParams* sp, int32_t* out_ids, float* logp_out, int32_t* n_steps,
                           float top_p = 0.f, int32_t* nkept_out = nullptr)
{
    const int D = h->cfg.dim_emb, L = h->cfg.rnn_layers;
    Ws w;
    AV_TRY(get_ws(h, w, b, 1, 1, false));
    StepwiseBufs sb;
    AV_TRY(place_scratch(h, "stepwise decoding: the states and ids", [&](Bump& bp) { stepwise_layout(bp, sb, (size_t)L * b * D, b, steps, sp != nullptr, top_p > 0.f); }));
    AV_TRY(avae_decode_init(h, z, b, sb.state[0]));
    std::vector<int32_t> host((size_t)(steps + 1) * b);
    for (int i = 0; i < b; ++i) host[i] = h->cfg.bos;
    // (host lives to the end of the function, and the first pass of the loop below -- steps >= 1 -- synchronises behind this copy)
    AV_CHECK(hipMemcpyAsync(sb.ids_tm, host.data(), b * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    int done = 0, kept = steps, cur = 0;
    const int chunk = 16;
    while (done < steps) {
        int n = std::min(chunk, steps - done);
        for (int s = 0; s < n; ++s) {
            const int t = done + s;
            if (!sp) AV_TRY(decode_step_ws(h, w, sb.ids_tm + (size_t)t * b, sb.state[cur], b, sb.ids_tm + (size_t)(t + 1) * b, sb.state[cur ^ 1]));
            else {
                AV_TRY(decode_logits_ws(h, w, sb.ids_tm + (size_t)t * b, sb.state[cur], b, sb.state[cur ^ 1]));
                if (top_p > 0.f)
                    AV_CHECK(sample_rows_p(h->stream, w.logits, b, h->cfg.dim_tgt, t, *sp, top_p, sb.ids_tm + (size_t)t * b, h->cfg.eos, sb.ids_tm + (size_t)(t + 1) * b,
                                           sb.logp_tm + (size_t)t * b, sb.nkept_tm + (size_t)t * b));
                else
                    AV_CHECK(sample_rows(h->stream, w.logits, b, h->cfg.dim_tgt, t, *sp, sb.ids_tm + (size_t)t * b, h->cfg.eos, sb.ids_tm + (size_t)(t + 1) * b, sb.logp_tm + (size_t)t * b));
            }
            cur ^= 1;
        }
        AV_CHECK(hipMemcpyAsync(host.data() + (size_t)(done + 1) * b, sb.ids_tm + (size_t)(done + 1) * b, (size_t)n * b * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        AV_CHECK(hipStreamSynchronize(h->stream));
        bool stop = false;
        for (int s = 0; s < n && !stop; ++s) {
            bool all = true;
            for (int i = 0; i < b; ++i) all &= host[(size_t)(done + s + 1) * b + i] == h->cfg.eos;
            if (all) { kept = done + s; stop = true; }      // model.py:217: break before appending
        }
        done += n;
        if (stop) break;
    }
    if (kept > done) kept = done;
    // transpose (kept, b) time-major -> (b, steps) row-major on the host (tiny), eos-fill the rest
    // outv, lpv and nkv are function-local and copied from asynchronously: the synchronise in front of `*n_steps = kept` completes all three
    // copies before they go out of scope
    const std::vector<int32_t> outv = rows_major(host.data() + b, kept, b, steps, (int32_t)h->cfg.eos);
    AV_CHECK(hipMemcpyAsync(out_ids, outv.data(), outv.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    std::vector<float> lpv;
    std::vector<int32_t> nkv;
    const bool want_lp = sp && logp_out, want_nk = sb.nkept_tm && nkept_out;
    if (want_lp || want_nk) {    // the same transpose; position `kept` holds the closing eos of the longest rows, 0 beyond (a finished row's
        const int nl = std::min(kept + 1, steps);      // logp 0 and nkept 0 are already there); both arrays come back under one synchronise
        std::vector<float> lp(want_lp ? (size_t)nl * b : 0);
        std::vector<int32_t> nk(want_nk ? (size_t)nl * b : 0);
        if (want_lp) AV_CHECK(hipMemcpyAsync(lp.data(), sb.logp_tm, lp.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        if (want_nk) AV_CHECK(hipMemcpyAsync(nk.data(), sb.nkept_tm, nk.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        AV_CHECK(hipStreamSynchronize(h->stream));
        if (want_lp) {
            lpv = rows_major(lp.data(), nl, b, steps, 0.f);
            AV_CHECK(hipMemcpyAsync(logp_out, lpv.data(), lpv.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
        }
        if (want_nk) {
            nkv = rows_major(nk.data(), nl, b, steps, (int32_t)0);
            AV_CHECK(hipMemcpyAsync(nkept_out, nkv.data(), nkv.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        }
    }
    AV_CHECK(hipStreamSynchronize(h->stream));
    if (n_steps) *n_steps = kept;
    return check_gru_err(h);
}

}  // extern "C"

// Which loop a decoding call of b rows runs (decode_loop below goes by this and by nothing else; avae_debug_decode_plan reports it):
// 0 the one persistent launch of *plan, 1 one launch sequence per token by option "persistent" 0 or by batch, 2 the same because
// decode_plan refuses the geometry; -1: no HIP device to ask.  G or lds_max 0: the current device's (asked only where the answer
// depends on them).  top_k as SampleParams holds it, nucleus: top_p > 0.
// Measured at D = 512, V = 8192, steps = 512 (scripts/decode_bench.py, profiles/r03_decode_bench.txt): the persistent launch
// takes 42 / 74 / 145 us per token at b = 1 / 16 / 64, the launch-per-token loop 116-130 us at any b <= 128 (its
// GEMMs are far from full): one launch up to 32 rows, the per-token loop above
int avae::host::decode_route(bool persistent, int b, bool sampled, int top_k, bool nucleus, int D, int V, int L, int G, int lds_max, DecodePlan* plan)
{
    *plan = DecodePlan{0, decode_mode(sampled, V, top_k, nucleus), 0, 0, 0, 0, G, lds_max};
    if (!persistent || b > 32) return 1;
    if (G < 1 || lds_max < 1) {
        int dg = 0, dl = 0;
        if (decode_device(&dg, &dl) != hipSuccess || dg < 1) return -1;
        if (G < 1) G = dg;
        if (lds_max < 1) lds_max = dl;
    }
    *plan = decode_plan(plan->mode, D, V, L, G, lds_max);
    return plan->ok ? 0 : 2;
}

extern "C" {

// the greedy (sp null) or sampled loop: one persistent launch where it serves, else the launch-per-token loop.  top_p > 0: the
// nucleus is on (0 < top_p < 1, sp->noise), nkept_out optional
static int decode_loop(avae_handle h, const float* z, int32_t b, int32_t steps, const SampleParams* sp, int32_t* out_ids, float* logp_out, int32_t* n_steps,
                       float top_p = 0.f, int32_t* nkept_out = nullptr)
{
    if (!h) return 1;
    AV_TRY(check_bound(h));
    if (b < 1 || steps < 1) return fail(h, "empty batch");
    AV_CHECK(hipSetDevice(h->device));
    const int D = h->cfg.dim_emb, V = h->cfg.dim_tgt, L = h->cfg.rnn_layers;
    DecodePlan plan;
    const int route = decode_route(h->persistent != 0, b, sp != nullptr, sp ? sp->top_k : 0, top_p > 0.f, D, V, L, 0, 0, &plan);
    if (route < 0) return fail(h, "no HIP device");
    if (route != 0) return decode_stepwise(h, z, b, steps, sp, out_ids, logp_out, n_steps, top_p, nkept_out);      // same results, more launches
    // the whole loop in ONE persistent launch (decode.hip); state, partial maxima and the id log live in the scratch buffer
    const int G = plan.G;
    const bool topk = sp && (sp->top_k > 0 || top_p > 0.f);          // the owner of a row reads its logits from the scratch
    const bool want_nk = top_p > 0.f && nkept_out;
    DecodeArgs a{};
    AV_TRY(place_scratch(h, "decoding in one launch: the states, partial results and ids",
                         [&](Bump& bp) { decode_layout(bp, a, G, b, steps, D, V, L, sp != nullptr, topk, sp && logp_out, want_nk); }));
    a.E = h->P + h->oE;
    for (int l = 0; l < L; ++l) { a.W[l] = h->P + h->dec[l].W; a.R[l] = h->P + h->dec[l].R; a.bW[l] = h->P + h->dec[l].bW; a.bR[l] = h->P + h->dec[l].bR; }
    a.Kout = h->P + h->oKout; a.bout = h->P + h->oBout;
    if (sp) { a.sp = *sp; a.logp_out = logp_out; }
    a.top_p = top_p;
    if (want_nk) a.nkept_out = nkept_out;
    a.out_ids = out_ids; a.err = h->errw;
    a.b = b; a.steps = steps; a.D = D; a.V = V; a.L = L; a.eos = h->cfg.eos; a.isd = 1.f / sqrtf((float)D);
    AV_TRY(avae_decode_init(h, z, b, a.state[0]));
    std::vector<int32_t> bos((size_t)b, h->cfg.bos);        // (lives to the end of the function; check_gru_err below synchronises behind the copy)
    AV_CHECK(hipMemcpyAsync(a.ids_tm, bos.data(), b * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    AV_CHECK(hipMemsetAsync(a.kept, 0, sizeof(int32_t), h->stream));
    AV_CHECK(hipMemsetAsync(a.bar, 0, sizeof(unsigned), h->stream));
    int grid = 0;
    hipError_t e = sp ? decode_sample(h->stream, a, &grid) : decode_greedy(h->stream, a, &grid);
    if (e == hipErrorCooperativeLaunchTooLarge) return fail(h, "persistent decode kernel: one workgroup per CU does not fit this device");
    AV_CHECK(e);
    int kept = 0;
    AV_CHECK(hipMemcpyAsync(&kept, a.kept, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    AV_TRY(check_gru_err(h));                               // synchronises
    if (n_steps) *n_steps = kept;
    return 0;
}

int avae_decode_greedy(avae_handle h, const float* z, int32_t b, int32_t steps, int32_t* out_ids, int32_t* n_steps)
{
    return decode_loop(h, z, b, steps, nullptr, out_ids, nullptr, n_steps);
}

}  // extern "C"

// avae_sample_config -> what the kernels take; false with the message set
bool avae::host::sample_params(avae_ctx* h, const avae_sample_config* sc, int V, SampleParams* sp)
{
    if (!sc) { fail(h, "sample config is null"); return false; }
    if (!(sc->temperature >= 0.f) || std::isinf(sc->temperature)) { fail(h, "sample: temperature must be a finite number >= 0"); return false; }
    if (sc->top_k < 0) { fail(h, "sample: top_k must be >= 0"); return false; }
    if (V > (1 << 20)) { fail(h, "sample: the noise index holds 2^20 vocabulary ids"); return false; }
    const bool greedy = sc->temperature == 0.f;
    sp->inv_t = greedy ? 1.f : 1.f / sc->temperature;
    sp->top_k = greedy || sc->top_k >= V ? 0 : sc->top_k;         // temperature 0: logp is over all of V
    sp->noise = !greedy && sc->top_k != 1;
    sp->seed = sc->seed;
    return true;
}

extern "C" {

int avae_decode_sample(avae_handle h, const float* z, int32_t b, int32_t steps, const avae_sample_config* sc,
                       int32_t* out_ids, float* logp_out, int32_t* n_steps)
{
    if (!h) return 1;
    SampleParams sp{};
    if (!sample_params(h, sc, h->cfg.dim_tgt, &sp)) return 1;
    if (steps > (1 << 20)) return fail(h, "sample: the noise index holds 2^20 steps");
    return decode_loop(h, z, b, steps, &sp, out_ids, logp_out, n_steps);
}

}  // extern "C"

// avae_sample_p_config -> the kernels' parameters and *top_p: the nucleus share, 0 where the nucleus is off (top_p 0 or >= 1,
// temperature 0, top_k 1: the call is avae_decode_sample's); false with the message set
bool avae::host::sample_params_p(avae_ctx* h, const avae_sample_p_config* sc, int V, SampleParams* sp, float* top_p)
{
    if (!sc) { fail(h, "sample config is null"); return false; }
    const avae_sample_config base{sc->temperature, sc->top_k, sc->seed};
    if (!sample_params(h, &base, V, sp)) return false;
    if (!(sc->top_p >= 0.f)) { fail(h, "sample: top_p must be a number >= 0"); return false; }
    if (sc->reserved != 0) { fail(h, "sample: the reserved field must be 0"); return false; }
    *top_p = sp->noise && sc->top_p > 0.f && sc->top_p < 1.f ? sc->top_p : 0.f;
    return true;
}

extern "C" {

int avae_decode_sample_p(avae_handle h, const float* z, int32_t b, int32_t steps, const avae_sample_p_config* sc,
                         int32_t* out_ids, float* logp_out, int32_t* nkept_out, int32_t* n_steps)
{
    if (!h) return 1;
    SampleParams sp{};
    float top_p = 0.f;
    if (!sample_params_p(h, sc, h->cfg.dim_tgt, &sp, &top_p)) return 1;
    if (steps > (1 << 20)) return fail(h, "sample: the noise index holds 2^20 steps");
    AV_TRY(decode_loop(h, z, b, steps, &sp, out_ids, logp_out, n_steps, top_p, nkept_out));
    if (top_p == 0.f && nkept_out) {            // nucleus off: avae_decode_sample's own path above; there is no nucleus to size
        AV_CHECK(hipMemsetAsync(nkept_out, 0xff, (size_t)b * steps * sizeof(int32_t), h->stream));
        AV_CHECK(hipStreamSynchronize(h->stream));
    }
    return 0;
}

// ---------------------------------------------------------------- beam search (contract: include/argsim_vae.h, avae_decode_beam; kernels: beam.hip)
int avae_decode_beam(avae_handle h, const float* z, int32_t b, int32_t steps, const avae_beam_config* bc, int32_t* out_ids, float* score,
                     float* cum, int32_t* len, int32_t* lat_parent, int32_t* lat_token, float* lat_cum, int32_t* n_steps)
{
    if (!h) return 1;
    AV_TRY(check_bound(h));
    if (!bc) return fail(h, "beam config is null");
    if (!z || !out_ids) return fail(h, "beam: z and out_ids must be given");
    if (b < 1 || steps < 1) return fail(h, "beam: empty batch");
    const int D = h->cfg.dim_emb, V = h->cfg.dim_tgt, L = h->cfg.rnn_layers, R = h->cfg.dim_rep, eos = h->cfg.eos, W = bc->width;
    if (W < 1 || W > 32) return fail(h, "beam: width must be in [1, 32]");
    if (W > V) return fail(h, "beam: width exceeds dim_tgt");
    if (!(bc->length_alpha >= 0.f) || std::isinf(bc->length_alpha)) return fail(h, "beam: length_alpha must be a finite number >= 0");
    if (steps > (1 << 20)) return fail(h, "beam: at most 2^20 steps");
    AV_CHECK(hipSetDevice(h->device));
    // sentences go through the search in groups of at most floor(1024 / width): at most 1024 decoder rows per step and a bounded workspace
    const int gs = 1024 / W, gmax = std::min<int>(b, gs), rmax = gmax * W;
    { Ws probe; AV_TRY(get_ws(h, probe, rmax, 1, 1, false)); }      // the workspace grows HERE if it has to, never inside the loop
    // scratch, sized once per call.  (The group lattice is 12 bytes x steps x rows: 6 MB at steps 512 x 1024 rows, 12 GB at the 2^20 steps
    // the contract admits -- a size the device cannot serve is refused with a message that names it)
    BeamBufs q;
    AV_TRY(place_scratch(h, "beam: the search lattice (12 bytes x steps x min(b x width, 1024 rows)) and state",
                         [&](Bump& bp) { beam_layout(bp, q, (size_t)L * rmax * D, rmax, W, steps, gmax); }));
    const bool norm = bc->length_alpha != 0.f;
    std::vector<float> lp;
    if (norm) {      // len^alpha in double on the host, rounded to fp32; the kernel divides in fp32
        lp.resize((size_t)steps + 1);
        for (int i = 0; i <= steps; ++i) lp[i] = (float)std::pow((double)std::max(i, 1), (double)bc->length_alpha);
        AV_CHECK(hipMemcpyAsync(q.lenpow, lp.data(), lp.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    }
    std::vector<int32_t> bos((size_t)gmax, h->cfg.bos);
    AV_CHECK(hipMemcpyAsync(q.bos, bos.data(), bos.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    AV_CHECK(hipStreamSynchronize(h->stream));      // the two host vectors are read: an early return below leaves no copy pending on them
    int n_max = 0;
    const int chunk = 16;
    for (int r0 = 0; r0 < b; r0 += gs) {
        const int n = std::min(gs, b - r0), rows = n * W;
        Ws w0, w1;                 // the decoder's buffers for the n rows of the first token and the n * W rows of every later one
        AV_TRY(get_ws(h, w0, n, 1, 1, false));
        AV_TRY(get_ws(h, w1, rows, 1, 1, false));
        AV_CHECK(hipMemsetAsync(q.live, 0, (size_t)steps * sizeof(int32_t), h->stream));
        AV_TRY(avae_decode_init(h, z + (size_t)r0 * R, n, q.state[0]));
        int done = 0, n_run = 0, cur = 0;
        while (done < steps && !n_run) {
            const int m = std::min(chunk, steps - done);
            for (int s = 0; s < m; ++s) {
                const int t = done + s, Win = t ? W : 1, rin = n * Win;
                Ws& w = t ? w1 : w0;
                const int32_t* lead = t ? q.lat_token + (size_t)(t - 1) * rows : q.bos;
                AV_TRY(decode_logits_ws(h, w, lead, q.state[cur], rin, nullptr));
                AV_CHECK(beam_rows(h->stream, w.logits, rin, V, W, t ? q.cum[cur] : nullptr, t ? q.fin[cur] : nullptr, eos, q.cand_sc, q.cand_tok, q.cand_cnt));
                BeamStep a{};
                a.n = n; a.Win = Win; a.W = W; a.eos = eos;
                a.cand_sc = q.cand_sc; a.cand_tok = q.cand_tok; a.cand_cnt = q.cand_cnt;
                a.fin_in = t ? q.fin[cur] : nullptr; a.len_in = t ? q.len[cur] : nullptr;
                a.lat_parent = q.lat_parent + (size_t)t * rows; a.lat_token = q.lat_token + (size_t)t * rows; a.lat_cum = q.lat_cum + (size_t)t * rows;
                a.cum_out = q.cum[cur ^ 1]; a.fin_out = q.fin[cur ^ 1]; a.len_out = q.len[cur ^ 1];
                a.live = q.live + t;
                AV_CHECK(beam_select(h->stream, a));
                AV_CHECK(beam_gather(h->stream, w.d_hd.data(), L, n, Win, W, D, a.lat_parent, q.state[cur ^ 1]));
                cur ^= 1;
            }
            int32_t alive[chunk];
            AV_CHECK(hipMemcpyAsync(alive, q.live + done, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
            AV_CHECK(hipStreamSynchronize(h->stream));
            for (int s = 0; s < m && !n_run; ++s) if (alive[s] == 0) n_run = done + s + 1;
            done += m;
        }
        if (!n_run) n_run = done;
        // (the steps a chunk ran beyond n_run moved nothing: every slot was finished, the beam stays in its order)
        BeamEnd e{};
        e.n = n; e.W = W; e.n_run = n_run; e.steps = steps; e.eos = eos;
        e.lat_parent = q.lat_parent; e.lat_token = q.lat_token; e.lat_cum = q.lat_cum;
        e.cum = q.cum[cur]; e.len = q.len[cur]; e.lenpow = norm ? q.lenpow : nullptr;
        const size_t o = (size_t)r0 * W;
        e.out_ids = out_ids + o * steps;
        e.score_out = score ? score + o : nullptr; e.cum_out = cum ? cum + o : nullptr; e.len_out = len ? len + o : nullptr;
        e.o_parent = lat_parent ? lat_parent + o : nullptr; e.o_token = lat_token ? lat_token + o : nullptr; e.o_cum = lat_cum ? lat_cum + o : nullptr;
        e.out_step = (size_t)b * W;
        AV_CHECK(beam_backtrack(h->stream, e));
        n_max = std::max(n_max, n_run);
    }
    AV_TRY(check_gru_err(h));       // synchronises
    if (n_steps) *n_steps = n_max;
    return 0;
}

}  // extern "C"
