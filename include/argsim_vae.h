/* argsim_vae.h -- C ABI of libargsim_vae.so, the MI355X (gfx950) implementation of the
 * argsim/argsim sequence-VAE hot path.
 *
 * The reference has no FFI: its de-facto boundary is the Record returned by vAe()
 * (reference src/model.py:73,191) and the feed->fetch pairs its callers use.  Every entry
 * point below names the reference call site it replaces (paths relative to the reference
 * repository root).  INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - opaque handle; one handle = one GPU = one host thread.
 *   - every tensor pointer is a DEVICE pointer owned by the caller (e.g. a PyTorch-ROCm
 *     tensor's data_ptr()); the library never frees caller memory.  It owns only its
 *     workspace.  Parameters, gradients and Adam slots live in four caller-allocated flat
 *     float32 buffers bound with avae_bind_state().  (One exception: group_off and k of avae_ward /
 *     avae_ward_cut are host arrays, as their section says.)
 *   - int return: 0 = ok, non-zero = error, text via avae_last_error().  No C++ exception
 *     crosses the ABI.
 *   - all work is enqueued on the stream given to avae_set_stream() (default: the null
 *     stream) and is asynchronous unless the entry returns host scalars.
 *   - ids are row-major (B, S) int32, eos-padded, exactly as util_np.vpack makes them
 *     (src/util_np.py:5-13).  z is row-major (b, dim_rep) float32 as np.save'd by
 *     src/eval_embed_reason.py:41.
 */
#ifndef ARGSIM_VAE_H
#define ARGSIM_VAE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct avae_ctx* avae_handle;

/* model section of src/config.json:10-21 + vAe() keyword defaults (src/model.py:48-66) */
typedef struct avae_config {
    int32_t dim_tgt;      /* vocab size V                      */
    int32_t dim_emb;      /* model dim D (16,32,64,128,256,512) */
    int32_t dim_rep;      /* latent dim R (multiple of 4)      */
    int32_t rnn_layers;   /* L                                 */
    float   accelerate;   /* schedule speed, model.py:77       */
    float   learn_rate;   /* model.py:80                       */
    int32_t bos, eos;     /* model.py:65-66                    */
    int32_t max_batch;    /* workspace sizing hints; grown on  */
    int32_t max_len;      /*   demand if exceeded              */
    /* extensions (not in the reference; identity at beta=1, free_bits=0) */
    float   kl_beta;      /* multiplies rate_anneal            */
    float   free_bits;    /* per-dimension KL floor (nats)     */
    int32_t compute_dtype;/* 0 = exact fp32 (reference);       */
                          /* 1 = bf16 operands in every contraction (GEMMs, GRU recurrence), fp32 accumulate/state/weights (BASELINE configs[2]) */
                          /* 2 = fp32 GEMMs on the bf16 matrix cores: each operand element split into 3 bf16 */
                          /*     in registers, 6 partial products, fp32 accumulate (fp32-accurate)          */
} avae_config;

/* kind selector for avae_get_tensor / avae_set_tensor */
enum { AVAE_PARAM = 0, AVAE_GRAD = 1, AVAE_ADAM_M = 2, AVAE_ADAM_V = 3 };

/* ---- lifetime -------------------------------------------------------------------------- */
/* replaces graph construction vAe(mode, **C)  (src/train.py:74,85; src/eval_embed_reason.py:24) */
int  avae_create(const avae_config* cfg, int device, avae_handle* out);
void avae_destroy(avae_handle h);
const char* avae_last_error(avae_handle h);           /* h may be NULL: last create error */
int  avae_set_stream(avae_handle h, void* hip_stream);

/* vae.mu.shape[1] etc. (src/explore_infer.py:33) */
int  avae_get_dims(avae_handle h, int32_t* V, int32_t* D, int32_t* R, int32_t* L);

/* ---- state (tf.train.Saver over global variables: src/train.py:92-96,121) --------------- */
int64_t avae_state_numel(avae_handle h);              /* floats in each flat buffer          */
int  avae_bind_state(avae_handle h, float* params, float* grads, float* adam_m, float* adam_v);
int  avae_param_count(avae_handle h);
const char* avae_param_name(avae_handle h, int i);
/* natural (checkpoint) shape of a named variable; internal storage may be permuted */
int  avae_param_info(avae_handle h, const char* name, int64_t* offset, int32_t* ndim, int64_t shape[4]);
/* copy a named variable between its natural layout (device buffer `buf`) and the flat state */
int  avae_get_tensor(avae_handle h, const char* name, int kind, float* buf);
int  avae_set_tensor(avae_handle h, const char* name, int kind, const float* buf);
/* global_step (src/model.py:76, src/train.py:119) */
int  avae_get_step(avae_handle h, int64_t* step);
int  avae_set_step(avae_handle h, int64_t step);
/* rate_keepwd, rate_anneal, rate_update at the current step (src/model.py:78-80) */
int  avae_get_schedule(avae_handle h, float out[3]);

/* ---- training: sess.run(model_train.train_step)  (src/train.py:118, src/model.py:189) --- */
/* src, tgt     (B,S_src),(B,S_tgt) int32 device
 * seed         counter-RNG key for word-dropout and the reparameterisation draw
 * keep_mask    optional (S_tgt,B) uint8 device, time-major: overrides random_uniform<keepwd
 * eps          optional (B,R) float device: overrides random_normal
 * n_tok_global tokens N of the GLOBAL batch (data-parallel exactness, mean over N in
 *              model.py:181); <= 0 means "this call's own N"
 * b_global     rows of the global batch; <= 0 means B                                  */
int  avae_forward_backward(avae_handle h, const int32_t* src, const int32_t* tgt,
                           int32_t B, int32_t S_src, int32_t S_tgt, uint64_t seed,
                           const uint8_t* keep_mask, const float* eps,
                           float n_tok_global, float b_global);
/* TF-style Adam (epsilon outside the bias-corrected sqrt) + global_step += 1 */
int  avae_adam_step(avae_handle h);
/* = avae_forward_backward + avae_adam_step */
int  avae_train_step(avae_handle h, const int32_t* src, const int32_t* tgt,
                     int32_t B, int32_t S_src, int32_t S_tgt, uint64_t seed,
                     const uint8_t* keep_mask, const float* eps);
/* loss_gen, loss_kld, loss of the last forward (synchronises the stream) */
int  avae_get_losses(avae_handle h, float out[3]);
/* data-parallel hook, called on the host while backward is being ENQUEUED.
 *   bucket >= 0: grads[offset, offset+count) is final (no later kernel of this step writes it).  The call is made
 *                right after the next persistent GRU launch has been enqueued (or at the end of backward), so a
 *                collective the callee orders behind the compute stream's current tail (event + side stream) runs
 *                beside the GEMM phase that follows that launch.
 *   bucket == AVAE_HOOK_FENCE (offset = count = 0): a persistent GRU launch comes next; the callee must make the
 *                compute stream wait for every collective it has in flight (the launch needs all CUs resident and
 *                must not share the device with a kernel that may wait on a peer GPU).                          */
enum { AVAE_HOOK_FENCE = -1 };
typedef void (*avae_grad_hook)(void* user, int bucket, int64_t offset, int64_t count);
int  avae_set_grad_hook(avae_handle h, avae_grad_hook hook, void* user);
/* The buckets the hook speaks of: contiguous ranges of the flat gradient buffer, indexed in buffer order
 *   0 decode/out | 1..L decode/rnn/lL..l1 | L+1 latent | L+2..2L+1 encode/rnnL..rnn1 | 2L+2 embed/embedding
 * (src/model.py:108-168 variable scopes).  ANNOUNCEMENT order within a step is fixed and does not depend on
 * the batch shape -- ranks whose shards differ in width pair their collectives by call order:
 *   0, 1, .., 2L (encode/rnn2), 2L+2 (embedding), 2L+1 (encode/rnn1)
 * i.e. buffer order except that the embedding bucket, complete once the first encoder layer's input gradient is
 * scattered, goes out before that layer's weight-gradient GEMMs and overlaps them.                               */
int  avae_bucket_count(avae_handle h);
int  avae_bucket_info(avae_handle h, int i, int64_t* offset, int64_t* count);

/* ---- validation: (errt_samp, loss_gen_samp, loss_kld_samp)  (src/train.py:109-110) ------ */
/* mode 'valid': no word dropout, z = mu.  outputs: errt_samp,loss_gen_samp (>= B*(S_tgt+1))
 * float device; loss_kld_samp (B,R) float device; *n_out = N (host; synchronises)         */
int  avae_eval(avae_handle h, const int32_t* src, const int32_t* tgt,
               int32_t B, int32_t S_src, int32_t S_tgt,
               float* errt_samp, float* loss_gen_samp, float* loss_kld_samp, int32_t* n_out);

/* ---- inference ------------------------------------------------------------------------- */
/* model.z.eval({model.src: data})  (src/model.py:194-201; src/eval_embed_reason.py:38,50):
 * z = mu (b,R); lv_out optional                                                          */
int  avae_encode(avae_handle h, const int32_t* src, int32_t b, int32_t t, float* z_out, float* lv_out);
/* vae.state_in.eval({vae.z: z})  (src/model.py:213): (L,b,D)                              */
int  avae_decode_init(avae_handle h, const float* z, int32_t b, float* state_out);
/* sess.run((vae.pred, vae.state_ex), {vae.lead: x, vae.state_in: s})  (src/model.py:216)  */
int  avae_decode_step(avae_handle h, const int32_t* lead, const float* state_in, int32_t b,
                      int32_t* pred_out, float* state_out);
/* the whole greedy loop of decode() (src/model.py:204-219) without a host round trip per
 * token: out_ids (b, steps) int32 device, *n_steps = tokens kept per row (host)           */
int  avae_decode_greedy(avae_handle h, const float* z, int32_t b, int32_t steps,
                        int32_t* out_ids, int32_t* n_steps);


/* ---- sampled decoding ------------------------------------------------------------------ */
/* Draw sentences from the decoder: temperature and top-k, on the device, reproducible from a seed.
 * For batch row r, step t (0-based) and vocabulary id v, with l[v] the tied logits of src/model.py:166:
 *   noise   u = ((x >> 41) + 0.5) 2^-23,  x = mix64(mix64(seed ^ (3 * 0xD6E8FEB86659FD93)) + idx),
 *           idx = ((r 2^20) + t) 2^20 + v  (stream 3 of the library's counter generator; mix64 is splitmix64's
 *           finaliser);  g = -log(-log u) in fp32 (logf).  u is exact in fp32 and strictly inside (0, 1).  idx holds
 *           neither b nor steps: a row's draws do not depend on the rows after it or on the step cap.
 *           dim_tgt > 2^20 or steps > 2^20 is refused.
 *   top-k   0 < top_k < V keeps {v : l[v] >= the top_k-th largest l}, ties at the threshold all kept;
 *           top_k = 0 or >= V keeps everything.
 *   token   the first maximum over the kept set of l[v] / temperature + g[v] (Gumbel-max: a draw from
 *           softmax(l / temperature) over the kept set).  temperature == 0 or top_k == 1: no noise, the first
 *           maximum of l.  A negative or non-finite temperature or a negative top_k is an error.
 *   logp    the log-softmax of l / temperature over the kept set at the token; at temperature 0 the log-softmax
 *           of l over all of V.
 *   rows    a row that has emitted eos is finished: every later token is eos with logp 0.  (The greedy loop keeps
 *           feeding such rows, as the reference does.)  The loop ends after the first step at which every row is
 *           finished, or at `steps`.
 * out_ids (b, steps) int32 device, eos-padded; logp_out optional (b, steps) float device: [r, j] belongs to
 * out_ids[r, j] up to and including the row's first eos (column *n_steps is the closing eos of the longest rows when
 * *n_steps < steps), 0 after it; *n_steps (host) = length of the longest row without its eos, as avae_decode_greedy.
 * One persistent launch up to 32 rows (top_k > 0: dim_tgt <= 8192), else one launch sequence per token.             */
typedef struct avae_sample_config { float temperature; int32_t top_k; uint64_t seed; } avae_sample_config;
int  avae_decode_sample(avae_handle h, const float* z, int32_t b, int32_t steps, const avae_sample_config* sc,
                        int32_t* out_ids, float* logp_out, int32_t* n_steps);

/* ---- nucleus (top-p) sampling ------------------------------------------------------------ */
/* avae_decode_sample with a nucleus, alone or after top-k.  noise (stream 3), the top-k rule, the Gumbel-max token, the
 * finished-row rule, the end of the loop, out_ids, logp_out and *n_steps are exactly avae_decode_sample's.  New, for batch
 * row r at step t, with l[v] the tied logits:
 *   K0      the set top-k keeps, or all of V when top-k is off; a NaN logit is absent.
 *   weights x[v] = l[v] * (1 / temperature) in fp32, as the sampler forms it; m = max x over K0;
 *           w[v] = (uint64) floor(expf(x[v] - m) 2^40), and x[v] == m gives exactly 2^40 without an exponential (the
 *           convention of the sampler's log-sum-exp: a +inf logit weighs 2^40 and everything beside it 0; a row of -inf only
 *           weighs 2^40 each).  A token more than about 27.7 below the maximum weighs 0.
 *   mass    W = sum of w over K0, an integer: the same in any order of summation (no float atomics anywhere);
 *           need = (uint64) ceil((double) top_p * (double) W), clamped to [1, W].
 *   nucleus tau = the largest logit value among K0 with (sum of w[v] over l[v] >= tau) >= need; kept = {v in K0 : l[v] >= tau}.
 *           Ties at tau are all kept, as top-k keeps them; the first maximum is always kept.
 *   token   the first maximum of x + g over the kept set; logp = the log-softmax of x over the kept set at the token.
 *   nkept   nkept_out, optional (b, steps) int32 device: the size of the kept set at every emitted position, the closing eos
 *           included; 0 where the row had already finished and beyond column *n_steps.
 *   off     top_p == 0, top_p >= 1, temperature == 0 or top_k == 1: the call IS avae_decode_sample with the first three fields
 *           (the very same kernels: out_ids and logp_out are bit-equal); nkept_out, if given, is filled with -1.
 * Errors: a null sc, a negative or NaN top_p, reserved != 0, and everything avae_decode_sample refuses.
 * One persistent launch up to 32 rows with dim_tgt <= 8192, else one launch sequence per token (dim_tgt > 8192 is no error).
 * expf is the device's: the two paths and the float64 reference of tests/nucleus_ref.py agree on the kept set wherever the
 * boundary is further from top_p than the measured tolerance.                                           */
typedef struct avae_sample_p_config { float temperature; int32_t top_k; uint64_t seed; float top_p; int32_t reserved; } avae_sample_p_config;
int  avae_decode_sample_p(avae_handle h, const float* z, int32_t b, int32_t steps, const avae_sample_p_config* sc,
                          int32_t* out_ids, float* logp_out, int32_t* nkept_out, int32_t* n_steps);
/* test hook: the per-token nucleus kernel alone on caller logits (n, V) device at step t0, row index = batch row: pred (n) int32,
 * logp (n) float and nkept (n) int32 device, the last two optional; lead (n) int32 device, optional: the ids fed at this step, a row
 * fed eos at t0 > 0 is finished (token eos, logp 0, nkept 0)                                                              */
int  avae_debug_sample_rows_p(avae_handle h, const float* logits, int n, int V, int t0, const avae_sample_p_config* sc,
                              int32_t* pred, float* logp, int32_t* nkept, const int32_t* lead);

/* ---- beam-search decoding --------------------------------------------------------------- */
/* The third decoder beside avae_decode_greedy and avae_decode_sample: the `width` best continuations per sentence, on the device,
 * on the launch-per-token path (the b x width hypotheses are the decoder's batch rows).  For sentence r, step t (0-based) and the
 * hypothesis in slot w, with l[w, v] the tied logits of src/model.py:166:
 *   logp    logp[w, v] = l[w, v] - logsumexp_v l[w, .] in fp32, the maximum subtracted first: (l - max) - log(sum exp(l - max)).
 *           Reductions run in a fixed order (a thread's own terms in index order, a wave by shuffles, a workgroup through LDS);
 *           no float atomics: the same arguments give the same bits.
 *   start   one hypothesis per sentence, [bos] with cum = 0 and the state of avae_decode_init; the other width - 1 slots do not
 *           exist at step 0 (the first step selects among the V candidates of that one row).
 *   cands   a live hypothesis w offers the V candidates (w, v) with cum[w] + logp[w, v]; a finished one (its last token is eos)
 *           offers exactly one, itself: token eos, cum unchanged (the sampler's rule: a finished row emits eos with logp 0).
 *   select  the `width` candidates largest under the total order (score descending, parent slot ascending, token ascending)
 *           become slots 0 .. width - 1 in that order; a NaN sorts below -inf, as in the sampler's radix keys.  width == 1 takes
 *           the first maximum of l itself, as temperature == 0 does in the sampler: ids are bit-equal to avae_decode_greedy up to
 *           the row's first eos, and eos after it.
 *   end     the loop ends after the first step at which every slot of every sentence is finished, or at `steps`; *n_steps is the
 *           number of steps run.  The lattice beyond it is (parent = slot, token = eos, cum unchanged).
 *   output  per sentence the final beam is re-ranked by score = cum / len^length_alpha (len^length_alpha evaluated in double on the
 *           host and rounded to fp32, the division in fp32; length_alpha == 0: score = cum), ties to the lower slot, and
 *           backtracked on the device into out_ids.  len counts the closing eos of a finished hypothesis; otherwise it is *n_steps.
 *   groups  sentences are independent and go through the search in groups of at most floor(1024 / width): at most 1024 decoder
 *           rows per step.  A finished group stops; *n_steps is the maximum over the groups.
 * Errors (text through avae_last_error): a null bc, z or out_ids; b < 1, steps < 1, width < 1, width > 32, width > dim_tgt; a
 * length_alpha that is negative or not finite; steps > 2^20; a lattice the device has no memory for (the call keeps 12 bytes x steps x
 * min(b x width, 1024) of it in its scratch: 6 MB at steps 512, refused with the size named where the allocation fails).  */
typedef struct avae_beam_config { int32_t width; float length_alpha; } avae_beam_config;
int  avae_decode_beam(avae_handle h, const float* z, int32_t b, int32_t steps, const avae_beam_config* bc,
                      int32_t* out_ids,    /* (b, width, steps) int32 device, eos-padded, best first         */
                      float*   score,      /* (b, width) optional: final score (above)                       */
                      float*   cum,        /* (b, width) optional: raw sum of token log-probabilities        */
                      int32_t* len,        /* (b, width) optional: tokens incl. the closing eos if it has one */
                      int32_t* lat_parent, /* (steps, b, width) optional: the search lattice, time-major     */
                      int32_t* lat_token,  /* (steps, b, width) optional                                     */
                      float*   lat_cum,    /* (steps, b, width) optional                                     */
                      int32_t* n_steps);   /* host: steps the search ran                                     */

/* ---- importance-weighted sentence likelihood --------------------------------------------- */
/* A K-sample importance-weighted bound on log p(tgt row) with the proposal q(z | src row), and its decoder half alone:
 * the teacher-forced log p(tgt row | z row) of sentences the caller supplies (the inverse of avae_decode_sample).
 * For batch row r, draw k (0-based) and latent dimension j:
 *   mu, lv  the valid-mode encoder of src, as avae_encode returns them.
 *   eps     eps[k, r, j] of the caller's array if given, else normal01(seed, 4, idx), idx = ((r 2^20) + k) 2^20 + j: stream 4
 *           of the library's counter generator (1 word dropout, 2 epsilon, 3 Gumbel), Box-Muller in fp32 on
 *           u1 = uniform01(2 idx), u2 = uniform01(2 idx + 1): sqrt(-2 log u1) cos(2 pi u2), uniform01(i) = ((x >> 40) + 0.5) 2^-24,
 *           x = mix64(mix64(seed ^ (4 * 0xD6E8FEB86659FD93)) + i).  idx holds neither B nor K: a row's draws do not depend on
 *           the rows around it, and the first K' draws of a K-sample call are the draws of a K'-sample call.
 *           k > 2^20 or dim_rep > 2^20 is refused.
 *   z       z[k, r] = mu[r] + exp(0.5 lv[r]) eps[k, r] in fp32, as the training forward draws it.
 *   logpx   logpx[k, r] = - sum of the per-token cross-entropy over the positions of row r that the decoder mask keeps
 *           (src/model.py:90-91: position 0 and every position whose preceding target id is not eos), the decoder fed
 *           lead = [bos] + tgt WITHOUT word dropout from the initial state of z[k, r]: log p(tgt row | z[k, r]).
 *   ntok    ntok[r] = how many positions that is (>= 1).
 *   logw    logw[k, r] = logpx[k, r] - 1/2 sum_j (z_j^2 - eps_j^2 - lv_j) = log p(x | z) + log p(z) - log q(z | x); the log 2 pi
 *           terms cancel and are never computed.
 *   bound   bound[r] = logsumexp_k logw[k, r] - log K, the maximum over k subtracted before the exponentials (at dim_emb 512
 *           logw is around -600 and its own exponential is 0 in fp32).  mean_k logw is the K-sample ELBO estimate; the
 *           caller can form it from logw.
 * Errors (text through avae_last_error): k < 1, B < 1, S_src < 1, S_tgt < 1, a null sc, a null bound, a null src or tgt, an eps that
 * is not finite (the caller's array is checked on the device while it is read), k > 2^20, dim_rep > 2^20, k B dim_rep > 2^30
 * elements.  avae_score_z refuses b < 1, S_tgt < 1 and a null z, tgt or logpx; it does NOT check z: a z that is not finite gives a
 * logpx that is not finite.
 * Every array is device memory.  The encoder runs once; the K x B (k, r) pairs go through the decoder as rows, in batches
 * of at most 256 rows whose logits fit the workspace, the draws of a row sharing one first-layer input
 * projection.  No float atomics anywhere on the path: the same arguments give the same bits.  Both entries are enqueued on
 * the handle's stream and end with the GRU time-out check, which synchronises it, as avae_encode does.                   */
typedef struct avae_score_config { int32_t k; uint64_t seed; } avae_score_config;
int  avae_score(avae_handle h, const int32_t* src, const int32_t* tgt, int32_t B, int32_t S_src, int32_t S_tgt,
                const avae_score_config* sc,
                const float* eps,      /* optional (k,B,R) device: overrides the generator              */
                float* eps_out,        /* optional (k,B,R) device: the draws used                       */
                float* logpx,          /* optional (k,B)                                                */
                float* logw,           /* optional (k,B)                                                */
                float* bound,          /* (B)                                                           */
                int32_t* ntok);        /* optional (B) device: positions scored per row                 */
/* teacher-forced log p(tgt row | z row): the decoder half alone, z (b, dim_rep) supplied by the caller */
int  avae_score_z(avae_handle h, const float* z, const int32_t* tgt, int32_t b, int32_t S_tgt,
                  float* logpx /* (b) */, int32_t* ntok /* optional (b) */);

/* ---- nearest neighbours among latent rows ------------------------------------------------ */
/* The encoder-side counterpart of the decoders above: for each of n query rows the k best of N bank rows under a similarity,
 * on the device, without the (n, N) score panel ever reaching memory.  q (n, dim) and bank (N, dim) are row-major float32
 * device arrays, 16-byte aligned (e.g. z of avae_encode); dim is a multiple of 4 in [4, 1024] and independent of the handle's
 * dim_rep; n >= 1, 0 <= N <= 2^31 - 256.  The work is enqueued on the handle's stream; nothing is synchronised.
 *   score   of a pair depends on the two rows and the metric ALONE -- not on n, N, k, the rows' positions, the tile a pair falls
 *           in or the launch shape:
 *           dot (0)    d = sum_j q_j b_j in fp32 on v_mfma_f32_32x32x2_f32, in this fixed order: j in blocks of 32, ascending
 *                      (the last block zero filled); inside a block 16 steps s = 0 .. 15, step s adding the two products
 *                      j = 8 (s >> 2) + (s & 3) and j + 4 to the running sum in one matrix instruction.
 *           cosine (1) d / (|q| |b|): the fp32 product of the norms, then an IEEE division.  |x| = the fp32 square root of the
 *                      sum of squares of that row alone, in a fixed order (lane l of a wave: elements 4 l .. 4 l + 3, then
 *                      256 + 4 l .., fused multiply-adds in index order; the 64 lanes by an xor butterfly 32, 16, .., 1).
 *                      A row of norm zero on either side scores 0.
 *           Euclid (2) - max(0, (|q|^2 - 2 d) + |b|^2) in exactly that order of operations: the negated squared distance, so
 *                      that larger is always better.  This form carries the cancellation error of the expansion, a few ulp of
 *                      |q|^2 + |b|^2: an identical pair scores about -1e-7 for rows of norm 1, not exactly 0.  (A NaN is no
 *                      number to clamp: it stays a NaN.)
 *   order   score descending, then global index ascending.  Scores compare through the sampler's order_key: +0 and -0 are equal
 *           and a NaN sorts below -inf (among NaNs the lower index first).  out_score holds the canonical value of the key: a -0
 *           is returned as +0, any NaN as the quiet NaN 0x7fc00000.
 *   index   bank row c of THIS call has global index idx_base + c (idx_base >= 0).
 *   self    self_base >= 0: query i never returns global index self_base + i (queries that are rows of the bank); -1: off.
 *   missing slots beyond the number of admissible rows hold index -1 and score -inf.
 *   carry   carry = 1: out_idx / out_score hold the list of earlier calls (sorted as above, -1 entries empty); it is merged as one
 *           more sorted list.  One call over bank rows [0, N) and carried calls over [0, N1), [N1, N) .. with idx_base = N1 ..
 *           give the same bits of indices and scores: this is how a bank larger than device memory is streamed.
 *   bits    no float atomics, fixed-order reductions: the same arguments give the same bits.
 * Errors (text through avae_last_error): a null kc, q, out_idx or out_score; a null bank with N > 0; n < 1, N < 0 or N > 2^31 - 256;
 * k outside [1, 32]; an unknown metric; dim not a multiple of 4 in [4, 1024]; idx_base < 0, self_base < -1; carry not 0 or 1;
 * reserved != 0; q or bank not 16-byte aligned.
 * Option knn_chunk (avae_set_option; a test aid): caps the bank rows one workgroup walks, so that small tests run many parts and
 * the merge; 0 lets the planner decide.  A cap that would give more parts than the merge ranks at once is raised.           */
typedef struct avae_knn_config {
    int32_t k;          /* 1..32 */
    int32_t metric;     /* 0 dot, 1 cosine, 2 squared Euclidean */
    int64_t idx_base;   /* global index of bank row 0 of THIS call */
    int64_t self_base;  /* -1: off; else query i never returns global index self_base + i */
    int32_t carry;      /* 1: out_idx/out_score hold a list from earlier calls; merge into it */
    int32_t reserved;
} avae_knn_config;
int  avae_knn(avae_handle h, const float* q, int32_t n, const float* bank, int32_t N, int32_t dim,
              const avae_knn_config* kc, int64_t* out_idx /* (n,k) */, float* out_score /* (n,k) */);

/* ---- aggregate-posterior diagnostics ------------------------------------------------------ */
/* Whether the latent code carries information: the density of samples under the AGGREGATE posterior q(z) = 1/N sum_j q(z | x_j)
 * of N encoded sentences, from which the caller forms the mutual information I(x; z) = E[log q(z | x) - log q(z)] and the marginal
 * KL(q(z) || p(z)) = E[log q(z) - log p(z)], and the per-dimension moments behind the active-unit count.  The (n, N) panel of pair
 * terms never reaches memory.  z (n, dim), mu and lv (N, dim) are row-major float32 device arrays, 16-byte aligned (e.g. mu and
 * lv of avae_encode); dim is a multiple of 4 in [4, 1024] and independent of the handle's dim_rep; n >= 1, 1 <= N <= 2^31 - 256.
 * Both entries are enqueued on the handle's stream; nothing is synchronised.
 *   pair    t(i, j) = -1/2 sum_d [(z_id - mu_jd)^2 a_jd + lv_jd], a_jd = expf(-lv_jd), in fp32 in its DIRECT form: the difference
 *           is formed before the square, then one fused multiply-add of the square with a_jd; even and odd dims run in two
 *           chains that are added at the end, then c_j = sum_d lv_jd (its own fixed-order fp32 sum) is added and the sum is
 *           halved.  The expansion into z^2 a - 2 z mu a + mu^2 a is NOT used: it cancels in the own pair, where z - mu is
 *           sigma eps while the three products are of size mu^2 / sigma^2.  A pair's value depends on the two
 *           rows alone, not on n, N, the tile or the launch shape.
 *   logq    logq[i] = logsumexp_j t(i, j) - log N - (dim / 2) log 2 pi, the maximum subtracted before the exponentials: an online
 *           (max, sum) pair per query over 64-row bank tiles, the parts of the bank merged in part order.
 *   logqx   self_base >= 0: logqx[i] = t(i, self_base + i) - (dim / 2) log 2 pi = log q(z_i | x_{self_base + i}), the very value
 *           that entered the sum (queries that are samples from rows self_base .. self_base + n - 1 of the bank).
 *   edges   a bank row whose t is -inf (lv = +inf, say) weighs 0; a query whose every term is -inf gets -inf, not NaN.  A NaN in a
 *           bank row reaches every query, a NaN in a query row that row alone (logq, and logqx where the own pair holds it).
 *           Inputs are not checked.  Rows beyond N and n are never read or stored.
 *   bits    no float atomics, fixed-order reductions, a launch shape that is a function of (n, N, dim) and option agg_chunk
 *           alone: the same arguments and options give the same bits.  Another agg_chunk sums in another order.
 * avae_latent_moments: out (4, dim), per dimension j over the N rows
 *           row 0  mean of mu_j
 *           row 1  unbiased variance of mu_j (divisor N - 1; exactly 0 for N = 1), two passes: the mean, then centred squares
 *           row 2  mean of exp(lv_j)
 *           row 3  mean of KL_j = 1/2 (mu_j^2 + exp(lv_j) - lv_j - 1)
 *           summed in double on the device in a fixed order, rounded to fp32 at the end.
 * Errors (text through avae_last_error): a null ac, z, mu, lv, logq or out; n < 1, N < 1 or N > 2^31 - 256; dim not a multiple of
 * 4 in [4, 1024]; z, mu or lv not 16-byte aligned; self_base < -1; self_base + n > N; a logqx with self_base = -1; reserved != 0.
 * Option agg_chunk (avae_set_option; a test aid): caps the bank rows of a part, so that small tests run several parts and the
 * merge; 0 lets the planner decide.  A cap that would give more than 1024 parts is raised.                                  */
typedef struct avae_agg_config {
    int64_t self_base;  /* -1: off; else query i's own bank row is self_base + i */
    int32_t reserved[2];
} avae_agg_config;
int  avae_agg_logq(avae_handle h, const float* z, int32_t n, const float* mu, const float* lv, int32_t N, int32_t dim,
                   const avae_agg_config* ac, float* logq /* (n) */, float* logqx /* (n), optional; needs self_base >= 0 */);
int  avae_latent_moments(avae_handle h, const float* mu, const float* lv, int32_t N, int32_t dim, float* out /* (4, dim) */);

/* ---- linear probes of latent rows ---------------------------------------------------------- */
/* Whether a code is linearly useful: P independent L2-regularised logistic regressions over ONE matrix of latent rows, fitted in
 * lockstep on the device -- a cross-validation over topics x folds x classes is one call.  x (N, dim), s (P, N), w (P, dim + 1),
 * stats (P, 4) and out (n, P) are row-major float32 device arrays; x and w are 16-byte aligned; dim is a multiple of 4 in
 * [4, 1024] and independent of the handle's dim_rep; 1 <= N <= 2^31 - 256, 1 <= P <= 2^20.
 *   objective  problem p minimises f_p(w) = 1/2 |w|^2 + sum_i |s_pi| softplus(-sgn(s_pi) w . x~_i), x~_i = (x_i, 1): the SIGN of
 *              s_pi is the label of row i in problem p, its MAGNITUDE the row's cost, and a cost of 0 leaves the row out of the
 *              problem (a held-out fold, another topic's row): it contributes exactly nothing.  The last component of w is the
 *              bias; it is penalised like the rest (liblinear with intercept_scaling = 1).  f_p is strongly convex with modulus 1:
 *              one optimum w*, and any w carries the certificate |w - w*| <= |grad f_p(w)|.  softplus and the sigmoid are
 *              evaluated from exp(-|margin|): nothing overflows whatever the margin.
 *   method     truncated Newton from w = 0.  The Newton system H v = v + X~^T (D o (X~ v)), D_i = |s_i| sigma(m_i) sigma(-m_i), is
 *              solved by conjugate gradients from 0 until |r| <= 0.1 |g| or max_cg iterations; the step p is taken with the first
 *              alpha in 1, 1/2, .. 2^-20 for which f(w + alpha p) <= f(w) + 1e-4 alpha g . p.  Both sides of that test come from
 *              the kept panels X~ w and X~ p (x is not read again) and are summed in double.  Every loop is bounded.
 *   stop       a problem stops at the first Newton iteration where |grad f_p(w)| <= tol |grad f_p(0)| and is frozen from then on,
 *              whatever its companions still do.  A problem whose costs are all 0 returns w = 0 exactly after 0 iterations.
 *   stats      stats[p] = f_p(w), |grad f_p(w)| as the device evaluated it at the returned w, the Newton iterations taken, and a
 *              status: 0 converged, 1 max_newton reached, 2 the line search was exhausted or a value that is not finite was met.
 *              Inputs are NOT checked for finiteness: such a value ends the affected problem with status 2, never a hang.
 *   bits       w[p] and stats[p] depend on x, on row p of s, on the config and on option probe_chunk alone -- not on P, on p or on
 *              the other problems of the call.  No float atomics, fixed-order reductions: the same arguments give the same bits.
 *   launches   per Newton iteration 11 + 2 max_cg, whatever the problems need (those of a tile of 32 problems that has finished a
 *              phase return at once), and ONE stream synchronisation, after the gradient, to learn whether every problem is
 *              frozen; what a problem does next is decided on the device, so the result does not depend on when the host looks.
 *   workspace  4 (4 N Pp + 5 Pp (dim + 4) + parts (dim + 5) Pp) + 56 parts Pp + 128 Pp bytes, Pp = P rounded up to 32, parts <= 256
 *              (DESIGN.md 4.3h), reserved once per call.
 * avae_probe_decision: out[i, p] = w_p . x~_i in fp32 (dot product order of avae_knn, then the bias).  Enqueued only; nothing is
 * synchronised.
 * Errors (text through avae_last_error): a null pc, x, s, w or out; N, n or P < 1; N or n > 2^31 - 256; P > 2^20; max_newton < 1, max_cg < 1;
 * a tol that is negative or NaN; reserved != 0; dim not a multiple of 4 in [4, 1024]; x or w not 16-byte aligned; a workspace the
 * device cannot give (the text names its size).
 * Option probe_chunk (avae_set_option; a test aid): caps the rows of a part, so that small tests run several parts and the merge;
 * 0 lets the planner decide.  A cap that would give more than 256 parts is raised.  Another probe_chunk sums in another order. */
typedef struct avae_probe_config { int32_t max_newton; int32_t max_cg; float tol; int32_t reserved; } avae_probe_config;
int  avae_probe_fit(avae_handle h, const float* x /* (N, dim) */, int32_t N, int32_t dim,
                    const float* s /* (P, N) signed costs */, int32_t P, const avae_probe_config* pc,
                    float* w /* (P, dim + 1) out */, float* stats /* (P, 4) optional */);
int  avae_probe_decision(avae_handle h, const float* x /* (n, dim) */, int32_t n, int32_t dim,
                         const float* w /* (P, dim + 1) */, int32_t P, float* out /* (n, P) */);

/* ---- L1 probes: sparse logistic fits and the selection of useful dimensions ------------------ */
/* The dimension selection of the reference (src/eval_clustering.py:46-60: LogisticRegression(penalty='l1', C=0.1,
 * solver='liblinear'), then the columns whose coefficients are not all zero): P independent L1-regularised logistic regressions over
 * ONE matrix of latent rows, fitted in lockstep on the device.  Arrays, alignment and the ranges of N, P and dim as for
 * avae_probe_fit; avae_probe_decision evaluates the fitted w.
 *   objective  problem p minimises F_p(w) = |w|_1 + sum_i |s_pi| softplus(-sgn(s_pi) w . x~_i), x~_i = (x_i, 1).  The bias is the
 *              last component and IS inside the 1-norm (liblinear with intercept_scaling = 1).  The costs mean what they mean in
 *              avae_probe_fit: the sign is the label, the magnitude C times the weight, and 0 leaves the row out.
 *   optimality with g = X~^T r the gradient of the smooth part, the minimum-norm subgradient of F_p is v(w), v_j = g_j + sgn(w_j)
 *              where w_j != 0 and v_j = sgn(g_j) max(|g_j| - 1, 0) where w_j = 0; w is optimal iff v(w) = 0.  F_p is not smooth and
 *              not strongly convex: there is NO certificate |w - w*| <= |grad f| here; |v(w)|_1 is what a caller can check.
 *   method     proximal Newton from w = 0 (the structure of liblinear's newGLMNET).  Per iteration the inner problem
 *              min_d g.d + 1/2 d.Hd + |w + d|_1, H = X~^T D X~, is solved by FISTA with adaptive restart: the candidate
 *              d+ = soft(w + y - (g + Hy) / L, 1 / L) - w, ONE Hessian product per inner iteration (H y follows by linearity); L
 *              starts at the largest diagonal entry of H (from the second iteration on at half of what the last inner solve ended
 *              with, relative to that entry) and doubles whenever (d+ - y).H(d+ - y) > L |d+ - y|^2, which spends that product and
 *              resets the momentum; the inner solve ends at |v_q(d)|_1 <= 0.1 |v(w)|_1, v_q the minimum-norm subgradient of the inner
 *              problem, or after max_inner products.  The step is taken with the first alpha in 1, 1/2, .. 2^-20 for which
 *              F(w + alpha d) <= F(w) + 0.01 alpha (g.d + |w + d|_1 - |w|_1) (liblinear's sufficient decrease); the smooth sums come
 *              from the kept panels in double, the 1-norms are summed in double.  Every loop is bounded.
 *   stop       a problem stops, and is frozen, at the first iteration where |v(w)|_1 <= tol |v(0)|_1.  This is liblinear's own
 *              measure (Gnorm1) WITHOUT its min(#pos, #neg) / l scaling of tol.  A problem with v(0) = 0 -- every |g_j(0)| <= 1:
 *              tiny costs, all costs 0 -- converges at iteration 0 with w exactly 0.
 *   zeros      a returned zero is an exact +0.0f, produced by the soft-threshold: the selection reads w != 0, no threshold.
 *   stats      stats[p] = F_p(w), |v(w)|_1 as the device evaluated it at the returned w, the outer iterations taken, and a status:
 *              0 converged, 1 max_newton reached, 2 the line search was exhausted or a value that is not finite was met.
 *              Inputs are NOT checked for finiteness: such a value ends the affected problem with status 2, never a hang.  A row
 *              of x that holds such a value ends, before the first pass, the problems whose cost on it is not 0, and only those:
 *              the fit runs on a copy of x with that row zeroed, so the others keep their bits.
 *   bits       w[p] and stats[p] depend on x, on row p of s, on the config and on option probe_chunk alone -- not on P, on p or on
 *              the other problems of the call.  No float atomics, fixed-order reductions: the same arguments give the same bits.
 *   launches   per iteration 13 + 2 max_inner, whatever the problems need, and ONE stream synchronisation, after the gradient.
 *   workspace  that of avae_probe_fit + 12 Pp (dim + 4) + 4 N dim bytes (three more vectors per problem and the copy of x), reserved
 *              once per call.
 * Errors (text through avae_last_error): a null pc, x, s or w; N or P < 1; N > 2^31 - 256; P > 2^20; max_newton < 1, max_inner < 1;
 * a tol that is negative or NaN; reserved != 0; dim not a multiple of 4 in [4, 1024]; x or w not 16-byte aligned; a workspace the
 * device cannot give (the text names its size).  Option probe_chunk applies as in avae_probe_fit. */
typedef struct avae_probe_l1_config { int32_t max_newton; int32_t max_inner; float tol; int32_t reserved; } avae_probe_l1_config;
int  avae_probe_fit_l1(avae_handle h, const float* x /* (N, dim) */, int32_t N, int32_t dim,
                       const float* s /* (P, N) signed costs */, int32_t P, const avae_probe_l1_config* pc,
                       float* w /* (P, dim + 1) out */, float* stats /* (P, 4) optional */);

/* ---- hierarchical clustering of latent rows -------------------------------------------------- */
/* The clustering evaluation of the reference (src/eval_clustering.py:82-103, src/eval_clustering_explorative.py:138-176:
 * AgglomerativeClustering, Ward linkage, per selection of rows) as ONE call over G independent groups of rows.  x (N, dim) is a
 * row-major float32 device array, 16-byte aligned, dim a multiple of 4 in [4, 1024] and independent of the handle's dim_rep.
 * group_off (G + 1) and k (G) are HOST arrays -- the one exception to "every tensor pointer is a device pointer": the host sizes the
 * workspace and the launches from them.  Group g is rows group_off[g] .. group_off[g + 1] of x, n_g >= 1 of them (n_g <= 2^15,
 * 1 <= G <= 2^16); its n_g - 1 merges are rows group_off[g] - g .. of pair (N - G, 2), delta (N - G) and size (N - G, optional).
 *   identity   a cluster lives in the SLOT of its smallest member row (group-local index).  Merge t joins the slots a < b into slot
 *              a: pair[t] = (a, b), size[t] the member count afterwards.
 *   value      Delta(A, B) = |A||B| / (|A| + |B|) |c_A - c_B|^2, the increase of the within-cluster sum of squares (scipy's Ward
 *              height is sqrt(2 Delta)).  Evaluated in double: per-cluster sums of member rows kept in double, c = sum / count, the
 *              difference first and then its square (never |a|^2 - 2 a.b + |b|^2, which cancels exactly where Ward decides its first
 *              merges), accumulated in a fixed order, times the size factor in double and rounded ONCE to fp32.  That fp32 value is
 *              what is stored, compared and returned in delta.  It depends on the two clusters alone -- not on n_g, G, the group's
 *              position or the kernel form -- and is symmetric by construction.
 *   order      every step merges the alive pair with the smallest stored value; ties go to the lowest a, then the lowest b.  Values
 *              compare through an order key in which a NaN is the largest value, so some alive pair always wins.
 *   not finite inputs are NOT checked.  A row that is not finite gives an unspecified but complete tree: exactly n_g - 1 merges, every
 *              slot b merged away exactly once, every loop bounded by n_g, never a hang.
 *   bits       no float atomics, fixed-order reductions: the same arguments give the same bits, and a group's result does not depend
 *              on its companions, on its position or on the kernel form.
 *   forms      one workgroup per group runs all merges of the call in ONE launch (largest group <= 128 rows), or two launches
 *              per merge over (groups, row tiles) with max n_g - 1 rounds enqueued without a synchronisation.  No kernel waits on
 *              another workgroup.  Option ward_form (avae_set_option; a test aid): 0 the planner, 1 one-workgroup, 2 launch-per-merge.
 *   workspace  per group 4 n_g^2 + 8 n_g dim + 12 n_g bytes (+ 256-byte rounding) and 56 G bytes, reserved once per call
 *              (DESIGN.md 4.3i).
 * N = G (every group a single row) is legal: no merge, the outputs are not touched.
 * avae_ward_cut: label[i] = the slot (smallest member row, group-local) of row i's cluster after its group's first n_g - k[g]
 * merges: p[b_t] = a_t, followed downwards from every leaf (slots only decrease: at most n_g steps).  Enqueued only; nothing is
 * synchronised.
 * Errors (text through avae_last_error): a null wc, x, group_off, pair or delta; G < 1 or G > 2^16; a group_off that does not ascend
 * from 0 or has an empty group; n_g > 2^15; dim not a multiple of 4 in [4, 1024]; x not 16-byte aligned; reserved != 0; a workspace
 * the device cannot give (the text names its size); for the cut a null pair, group_off, k or label, or k[g] outside [1, n_g].      */
typedef struct avae_ward_config { int32_t reserved[2]; } avae_ward_config;
int  avae_ward(avae_handle h, const float* x /* (N, dim) device */, int32_t dim,
               const int32_t* group_off /* HOST (G + 1) */, int32_t G, const avae_ward_config* wc,
               int32_t* pair /* (N - G, 2) */, float* delta /* (N - G) */, int32_t* size /* (N - G), optional */);
int  avae_ward_cut(avae_handle h, const int32_t* pair /* device, as returned */, const int32_t* group_off /* HOST */, int32_t G,
                   const int32_t* k /* HOST (G) */, int32_t* label /* (N) */);

/* ---- affinity propagation of latent rows ------------------------------------------------------ */
/* The explorative clustering of the reference (src/eval_clustering_explorative.py:83-103: AffinityPropagation on Euclidean and on
 * cosine similarities) as ONE call over one set of rows: similarities, preference, the message passing with its stopping rule and the
 * labels, enqueued on the handle's stream with no synchronisation inside.  x (N, dim) is a row-major float32 device array,
 * 1 <= N <= 2^14; for metric 0 and 1 dim is a multiple of 4 in [4, 1024], x 16-byte aligned, independent of the handle's dim_rep;
 * for metric 2 x IS the (N, N) similarity matrix and dim == N, whatever N.
 *   similarity S_ik is evaluated in double, accumulated in a fixed order and rounded ONCE to fp32.  Metric 0: -|x_i - x_k|^2, the
 *              difference first and then its square.  Metric 1: -(1 - x_i.x_k / (|x_i||x_k|)); a zero row gives NaN.  Symmetric by
 *              construction, S_ii = 0 before the preference.
 *   preference use_preference 0: numpy's median of all N^2 entries of that fp32 matrix, the diagonal included -- the middle value,
 *              or for even N^2 the fp32 sum of the two middle values, halved -- found by a radix select over order keys with integer
 *              histograms.  use_preference 1: `preference`.  The diagonal is then set to it.
 *   noise      noise 1: S_ik += (2^-23 S_ik + 100 FLT_MIN) normal01(seed, 5, i N + k) in fp32, the diagonal included: sklearn's
 *              perturbation on the library's counter generator, stream 5.  A draw depends on (seed, i, k, N) alone.
 *   s_out      optional: S exactly as the iterations use it.
 *   iteration  sklearn's loop with lambda = damping, all arithmetic in fp32 but the column sums:
 *                R_ik <- lambda R_ik + (1 - lambda) (S_ik - max_{k' != k} (A_ik' + S_ik'))
 *                A_ik <- lambda A_ik + (1 - lambda) min(0, R_kk + sum_{i' not in {i, k}} max(0, R_i'k))      i != k
 *                A_kk <- lambda A_kk + (1 - lambda) sum_{i' != k} max(0, R_i'k)
 *              The first maximum of A + S takes the lowest column on ties.  The column sums are taken in double in a fixed order
 *              (ascending rows within a block of rows, then ascending blocks) and rounded once; E_k = (A_kk + R_kk > 0) in fp32.
 *   stop       run_k counts the latest consecutive iterations, the current one included, in which E_k kept its value.  After
 *              iteration it (0-based) the call stops if it >= convergence_iter, min_k run_k >= convergence_iter and K = sum E_k > 0
 *              (sklearn's rolling window); otherwise after max_iter iterations.  The stop is decided on the device: all max_iter
 *              rounds of three launches are enqueued, and a launch that finds the stop decided returns at once.
 *   labels     whenever K > 0, converged or not: (1) c_i = argmax over the exemplars k of S_ik, the lowest k on ties, an exemplar
 *              takes itself; (2) every cluster's exemplar is replaced by its member j with the largest sum of S_ij over the
 *              cluster's rows i, S_jj included -- the sum in double in ascending i, rounded once to fp32, compared by order key,
 *              the lowest j on ties; (3) step 1 again with the new exemplars.  label[i] is the ROW of i's exemplar; every label is
 *              -1 if K = 0.  stat = (iterations run, converged 0 / 1, K, 0).  N = 1: label 0, stat (0, 1, 1, 0), nothing else runs.
 *   a, r       optional, both or neither: the (N, N) messages.  The call works in them and leaves the final messages there; with
 *              warm 1 it starts from their contents, else from zero.
 *   not finite inputs are NOT checked.  A value that is not finite gives an unspecified but complete result: every label is -1 or the
 *              row of an exemplar (-1 also where no exemplar's similarity to the row is a number above -inf); never a hang.
 *   bits       no float atomics, fixed-order reductions: the same arguments give the same bits.  No kernel waits on another
 *              workgroup; every loop is bounded by N, dim or max_iter.
 *   workspace  4 N^2 bytes for each of S, A and R that the caller does not give (s_out, a, r), 8 N ceil(N / rb) bytes of column
 *              partials (rb = 4 rows up to N = 4096, then ceil(N / 1024)), 32 N bytes of vectors and the state, reserved once per call.
 * Errors (text through avae_last_error): a null ac, x, label or stat; N outside [1, 2^14]; a metric outside 0 .. 2; metric 2 with
 * dim != N; for the other metrics dim not a multiple of 4 in [4, 1024] or x not 16-byte aligned; max_iter outside [1, 10000];
 * convergence_iter outside [1, max_iter]; damping outside [0.5, 1); only one of a and r; warm without a and r; reserved != 0; a
 * workspace the device cannot give (the text names its size).                                                                      */
typedef struct avae_affinity_config {
    int32_t metric;            /* 0: -|xi - xk|^2   1: -(1 - cos(xi, xk))   2: x IS the (N, N) similarity, dim == N */
    int32_t max_iter;          /* [1, 10000]; sklearn's default 200 */
    int32_t convergence_iter;  /* [1, max_iter]; 15 */
    int32_t use_preference;    /* 0: the median of the similarities; 1: `preference` */
    int32_t noise;             /* 1: the degeneracy-breaking perturbation from `seed`; 0: none */
    int32_t warm;              /* 1: start from the contents of a / r; 0: from zero */
    float   damping;           /* [0.5, 1) */
    float   preference;
    uint64_t seed;
    int32_t reserved[2];
} avae_affinity_config;
int  avae_affinity(avae_handle h, const float* x /* (N, dim) device */, int32_t N, int32_t dim,
                   const avae_affinity_config* ac,
                   int32_t* label /* (N) */, int32_t* stat /* (4) */,
                   float* s_out /* (N, N), optional */, float* a /* (N, N) */, float* r /* (N, N), both or neither */);

/* ---- exact t-SNE of latent rows ---------------------------------------------------------------- */
/* The embedding plot of the reference (src/eval_clustering_explorative.py:45-66: TSNE(n_components=2, perplexity=40, n_iter=20000)
 * over the post embeddings) as ONE call: distances, the perplexity bisection, the joint matrix and sklearn's exact gradient descent
 * with its two phases and its stopping rule, enqueued on the handle's stream with no synchronisation inside.  Two components only.
 * x (N, dim) is a row-major float32 device array, 16-byte aligned, dim a multiple of 4 in [4, 1024] and independent of the handle's
 * dim_rep; 2 <= N <= 2^14; perplexity in (0, N).  With p_in, an (N, N) double joint matrix exactly as the iterations use it, x may
 * be null and the distance and bisection stages do not run (one P, several seeds).  Every other array is a device array too.
 *   distances  D_ij is evaluated in double, the difference first and then its square, in a fixed order, and rounded ONCE to fp32:
 *              exactly the negative of avae_affinity's metric 0 (the same kernel).
 *   condit.    per row i sklearn's _binary_search_perplexity in double over the fp32 D_ij, j != i: beta = 1, lo = -inf, hi = +inf, at
 *              most 100 steps of: p_j = exp(-D_ij beta); s = sum p_j in a fixed order, the fp32 value nearest 1e-8 if that is 0;
 *              p_j /= s; h = log s + beta sum D_ij p_j; stop when |h - log perplexity| <= the fp32 value nearest 1e-5; if h is too
 *              large lo = beta and beta = 2 beta while hi is infinite, else (beta + hi) / 2; if too small hi = beta and beta = beta / 2
 *              while lo is infinite, else (beta + lo) / 2.  beta_out (N) double, optional: the beta the row's p were evaluated at.
 *   joint      i != j: P_ij = max((c_ij + c_ji) / max(Sigma, eps), eps), eps = 2^-52, Sigma the sum of all c_ij + c_ji (per row in a
 *              fixed order, then over ascending rows); P_ii = 0.  P is double and symmetric bit for bit.  p_out (N, N) double,
 *              optional (with p_in: a copy of it).
 *   init       init 0: y (N, 2) fp32, in and out, holds the start.  init 1: y_ic = 1e-4f normal01(seed, 6, 2 i + c) in fp32 on the
 *              library's counter generator, stream 6.  A warm call reads y whatever init says.
 *   rate       learning_rate > 0 is used; otherwise max(N / early_exaggeration / 4, 50), in double on the host, rounded to fp32.
 *   loop       iterations i = it0 .. max_iter - 1 in two phases, as sklearn's _tsne runs them.  Phase 1 covers i < X =
 *              min(exaggeration_iter, max_iter): P' = early_exaggeration P (the product in double), momentum 0.5, window W = X.  Phase
 *              2 starts at the iteration after phase 1's last -- exaggeration_iter - 1, or the iteration at which a check ended phase 1
 *              -- and runs to max_iter - 1; it may be empty: P' = P, momentum 0.8, W = n_iter_without_progress.  At a phase's start
 *              update = 0, gains = 1, best_error = DBL_MAX, best_iter = the phase's first i.  (A call that ends before
 *              exaggeration_iter - 1 leaves phase 1 open: ug and prog hold its state.  A call whose last iteration ended phase 1
 *              returns the fresh state of phase 2 there.)
 *   iteration  from the fp32 y in double: d_ij = y_i - y_j, q_ij = 1 / (1 + |d_ij|^2) by IEEE division, Z = sum_{i != j} q_ij;
 *              g_i = fp32(4 (sum_j P'_ij q_ij d_ij - (sum_j q_ij^2 d_ij) / Z)), the sums in double in a fixed order (a lane's columns
 *              ascending, the wave butterfly, the column parts ascending; Z over all partials in one fixed order), one rounding at the end.  This is
 *              sklearn's gradient WITHOUT its floor on Q: it differs only where q_ij / Z < eps, by less than eps q_ij |d_ij| per
 *              pair.  Z and both sums come out of ONE pass over P.  Then in fp32, every operation rounded, nothing fused:
 *                gains = (update g < 0) ? gains + 0.2f : gains 0.8f;  gains = max(gains, 0.01f);  g' = g gains
 *                update = fl(fl(m update) - fl(lr g'));  y = fl(y + update)
 *   error      computed when check = ((i + 1) % n_iter_check == 0) holds or i is the last planned iteration of its phase (X - 1, or
 *              max_iter - 1): sum_{i != j} P'_ij log(max(P'_ij, eps) / max(q_ij / Z, eps)) in double in a fixed order, at the y the
 *              iteration started from: sklearn's quantity.
 *   checks     when check holds, gn = sqrt(sum g'^2) in double, then sklearn's rule: if error < best_error record it and i; else if
 *              i - best_iter > W the phase ends; then, if it has not ended, gn <= min_grad_norm ends it.  A phase-1 end of either
 *              kind starts phase 2 at i + 1; a phase-2 end stops the call.
 *   stop       decided on the device: all iterations are enqueued (two launches each, three where the error may be computed) and a
 *              launch that finds the stop decided returns at once.  No kernel waits on another workgroup; every loop is bounded by
 *              N, dim, 100 or max_iter.
 *   outputs    y; kl (2) double: [0] the last error computed (sklearn's kl_divergence_), [1] the error at phase 1's last iteration
 *              (NaN where the call ran none of either); with an empty phase 2, [0] = [1].  stat (4) int32: the last iteration index run
 *              (it0 - 1 if none), how phase 2 ended (0 ran out, 1 no progress, 2 gradient norm), phase 1's last iteration (-1 if the
 *              call ran none), 0.  trace (2, max_iter) double, optional: the error and gn of every iteration that computed them, NaN
 *              elsewhere (a warm call leaves the entries before it0 alone).  grad (N, 2) fp32, optional: the last iteration's g
 *              before the gains.  ug (2, N, 2) fp32: update, then gains; prog (4) double: best_error, best_iter, phase, 0.  ug and
 *              prog come both or neither; with warm 1 the call continues from it0 using y, ug and prog as found, and a warm
 *              continuation is bit-identical to the uninterrupted call: after a call over [it0, m) with max_iter = m and a warm one
 *              over [m, max_iter), y, ug and prog hold the bits that one call over [it0, max_iter) leaves.  (The call that ends at m
 *              computes one more error, at its own last iteration; that changes kl and trace there, and no state.)
 *   range      max_iter in [0, 32768]; with it0 = max_iter the call returns the init and P only.
 *   not finite inputs are NOT checked.  The result is then unspecified but complete; never a hang.
 *   bits       no float atomics, fixed-order reductions: the same arguments and option give the same bits.
 *   workspace  8 N^2 bytes for P unless p_out or p_in is given; with x 4 N^2 bytes for D and 16 N bytes of vectors; 48 N parts bytes of
 *              row partials (five doubles of the pair walk and one of the error walk per row and column part; parts is at most
 *              max(1, floor(1024 / ceil(N / rb)), ceil(N / 4096)), rb = 4 rows up to N = 4096, then 16); 16 N bytes of state
 *              unless ug is given; + 256-byte rounding, reserved once per call.  The conditionals are symmetrised
 *              in place, one thread owning the pair (i, j), (j, i).
 * Errors (text through avae_last_error; checked on the host, before any launch): a null tc, y, kl or stat; neither x nor p_in; N
 * outside [2, 2^14]; with x: dim not a multiple of 4 in [4, 1024], x not 16-byte aligned, perplexity outside (0, N); y or ug not
 * 8-byte aligned; max_iter outside [0, 32768]; it0 outside [0, max_iter]; exaggeration_iter < 0; n_iter_check < 1;
 * n_iter_without_progress < 0; early_exaggeration < 1; a NaN learning_rate; init outside 0 .. 1; only one of ug and prog; warm
 * without them; reserved != 0; a workspace the device cannot give (the text names its size).
 * Option tsne_chunk (avae_set_option; a test aid): caps the columns of a part, so that small tests run several parts that are no
 * tile multiples; 0 lets the planner decide.  A cap above 4096 or one that would give more than 256 parts is adjusted.  Another
 * tsne_chunk sums in another order.                                                                                              */
typedef struct avae_tsne_config {
    double  perplexity;               /* (0, N); sklearn's default 30, the reference's 40 */
    double  early_exaggeration;       /* >= 1; 12 */
    double  min_grad_norm;            /* 1e-7 */
    float   learning_rate;            /* > 0: used as it is; otherwise max(N / early_exaggeration / 4, 50) */
    int32_t max_iter;                 /* [0, 32768]; 1000 */
    int32_t it0;                      /* first iteration index, [0, max_iter] */
    int32_t exaggeration_iter;        /* 250 */
    int32_t n_iter_check;             /* >= 1; 50 */
    int32_t n_iter_without_progress;  /* 300 */
    int32_t init;                     /* 0: y holds the start; 1: random from `seed` */
    int32_t warm;                     /* 1: continue from it0 with y, ug and prog as found */
    uint64_t seed;
    int32_t reserved[2];
} avae_tsne_config;
int  avae_tsne(avae_handle h, const float* x /* (N, dim) device, or null with p_in */, int32_t N, int32_t dim,
               const avae_tsne_config* tc, const double* p_in /* (N, N), optional */,
               float* y /* (N, 2) */, double* kl /* (2) */, int32_t* stat /* (4) */,
               double* p_out /* (N, N), optional */, double* beta_out /* (N), optional */, double* trace /* (2, max_iter), optional */,
               float* grad /* (N, 2), optional */, float* ug /* (2, N, 2) */, double* prog /* (4), both or neither */);

/* ---- k-means of latent rows ----------------------------------------------------------------------------------------------------
 * scikit-learn's KMeans(algorithm='lloyd') of N rows into k clusters, n_init restarts side by side, in ONE call: everything is enqueued
 * on the handle's stream without a synchronisation; each restart decides its stop on the device and a launch that finds the stop
 * decided returns at once.  Every pointer is device memory.  All arithmetic that a decision or an output depends on is double; the rows
 * are fp32.  (The float64 restatement of this contract is tests/kmeans_ref.py.)
 *   tolerance  tol_abs = tol x the mean over the dim columns of the population variance of the rows.
 *   iteration  from centres c: (1) label_i = argmin_c sum_j (x_ij - c_cj)^2, the FIRST minimum; (2) counts and sums of the member rows;
 *              (3) the empty clusters in ascending order: the e-th takes the row with the e-th largest distance to its own centre (ties:
 *              the smaller row), which leaves its old cluster's sum and count -- a relocation; (4) new centres = sums / counts;
 *              (5) shift = sum |c_new - c|^2; (6) stop "converged" (0) if the labels equal the previous iteration's; (7) else stop
 *              "tol" (1) if shift <= tol_abs; (8) else go on, to max_iter (2).  After a stop that was not "converged" the labels are
 *              assigned once more against the final centres.  inertia = sum_i |x_i - c_label_i|^2 over the final labels and centres.
 *              Iterations count from 1.  The best restart is the first one with the smallest inertia.
 *   cosine     metric 1 is the same algorithm on the rows divided by their norms (a zero row stays zero); every new centre is divided
 *              by its norm (a zero centre stays zero): spherical k-means, inertia = sum 2 (1 - cos).
 *   seeding    init 0 is sklearn's greedy k-means++ with this library's generator: u = uniform01(seed, stream 7, ((r 2^20) + c) 2^20 + t)
 *              for restart r, centre c, trial t.  Centre 0 is row floor(u N).  Every further centre draws T = 2 + floor(ln k) candidates:
 *              a candidate is the first row whose inclusive cumulative sum of the current closest squared distances, in ascending row
 *              order, reaches u x the total, clipped to N - 1; chosen is the candidate with the smallest new potential
 *              sum_i min(closest_i, d(i, candidate)), the first of equals.  Restart r does not depend on n_init.  init 1 reads the start
 *              of every restart from centers_in (for the cosine they are taken as given).
 *   outputs    label (N) and centers (k, dim; the double values rounded once) of the best restart; stat (4) = best restart, its
 *              iterations, how it stopped, its relocations; inertia (n_init).  Optional: label_all (n_init, N), centers_all (n_init, k,
 *              dim) double, stat_all (n_init, 4) = iterations, stop, relocations, 0.
 *   range      1 <= N <= 2^22; 1 <= k <= min(N, 4096); dim a multiple of 4 in [4, 1024]; x and centers_in 16-byte aligned.
 *   not finite inputs are NOT checked.  The result is then unspecified but complete; never a hang.  A row without a nearest centre
 *              takes cluster 0.
 *   bits       no float atomics; every sum has an order fixed by the shape: the same arguments and option give the
 *              same bits in every output.
 *   cost       an iteration is seven launches whether or not a restart has stopped; relocation sweeps the rows once per empty cluster
 *              in one workgroup per restart.
 *   workspace  per restart 28 N bytes of labels, distances, sorted rows and part minima (+ 12 N per further centre part, at most 16
 *              parts, only where there are few row tiles), 8 k dim of centres, 8 (slices + k) dim of member-sum partials (slices =
 *              ceil(N / 256), from 2^16 rows ceil(N / 1024)), 8 blocks k of histograms (blocks <= 256); with init 0 another
 *              8 N (1 + T) + 8 T dim; + 256-byte rounding, reserved once per call.
 * Errors (text through avae_last_error; checked on the host, before any launch): a null kc, x, label, centers, stat or inertia; N or dim
 * out of range; x or centers_in not 16-byte aligned; k outside [1, min(N, 4096)]; n_init outside [1, 64]; max_iter outside [1, 10000];
 * metric or init outside 0 .. 1; init 1 without centers_in; tol negative or NaN; reserved != 0; a workspace the device cannot give (the
 * text names its size).
 * Option kmeans_chunk (avae_set_option; a test aid): caps the centres of a part and the rows of a tile, a slice and a sort block, so that
 * small tests run several parts and their merges; 0 lets the planner decide.  Another kmeans_chunk sums in another order.            */
typedef struct avae_kmeans_config {
    int32_t k;          /* clusters, 1 <= k <= min(N, 4096) */
    int32_t n_init;     /* restarts run side by side in the one call, 1 .. 64 */
    int32_t max_iter;   /* Lloyd iterations per restart, 1 .. 10000 (sklearn: 300) */
    int32_t metric;     /* 0 euclidean; 1 cosine = spherical k-means */
    int32_t init;       /* 0: greedy k-means++ from `seed`; 1: the centres in `centers_in` */
    int32_t reserved;   /* 0 */
    double  tol;        /* >= 0, relative as sklearn's (1e-4): scaled by the mean column variance */
    uint64_t seed;
} avae_kmeans_config;
int  avae_kmeans(avae_handle h, const float* x /* (N, dim) device */, int32_t N, int32_t dim, const avae_kmeans_config* kc,
                 const float* centers_in /* (n_init, k, dim) device, init = 1 only */,
                 int32_t* label /* (N) */, float* centers /* (k, dim) */, int32_t* stat /* (4) */, double* inertia /* (n_init) */,
                 int32_t* label_all /* optional (n_init, N) */, double* centers_all /* optional (n_init, k, dim) */,
                 int32_t* stat_all /* optional (n_init, 4) */);

/* ---- Gaussian mixture of latent rows -----------------------------------------------------------------------------------------------
 * scikit-learn 1.7.2's GaussianMixture(covariance_type = 'diag' | 'spherical') of N rows with k components, n_init restarts side by side,
 * in ONE call: everything is enqueued on the handle's stream without a synchronisation; each restart decides its stop on the device and a
 * launch that finds the stop decided returns at once.  Every pointer is device memory.  The rows are fp32; everything else is double.
 * (The float64 restatement of this contract is tests/gmm_ref.py.)
 *   E-step     p_cj = 1 / cov_cj.  q_ic = sum_j (x_ij - mu_cj)^2 p_cj: the difference is formed before the square, j runs in ascending
 *              order as one chain q <- fma(d d, p, q); a term depends on the row and the component only, never on tile, part or plan.
 *              t_ic = ((log w_c - 1/2 sum_j log cov_cj) - (dim / 2) log 2 pi) - 1/2 q_ic.  lse_i = m_i + log sum_c exp(t_ic - m_i) with
 *              m_i the maximum over c, kept as a running (max, sum) pair: a thread takes its components in ascending order, the 16
 *              threads of a row are merged by a butterfly, the component parts in ascending order.  r_ic = exp(t_ic - lse_i).  The
 *              iteration's lower bound is (1 / N) sum_i lse_i (blocks of 256 rows, ascending).
 *   M-step     n_c = sum_i r_ic + 10 x 2^-52; mu_c = sum_i r_ic x_i / n_c; cov_cj = sum_i r_ic x_ij^2 / n_c - mu_cj^2 + reg_covar
 *              (sklearn's one-pass form, kept so that results are comparable: it cancels where a variance is small against mu^2).  The
 *              sums run over the rows of a slice in ascending order, then over the slices in ascending order.  Spherical: every column of
 *              cov_c is the mean over j of these values, summed in ascending j; the outputs keep the (k, dim) shape with equal columns.
 *              w_c = n_c / N, then divided by sum_c w_c (ascending c).
 *   start      init 0: row i of restart r has responsibility 1 for label_in[r, i] if that lies in [0, k) and none otherwise (for the
 *              start only); one M-step follows.  init 1: the parameters are taken as given (the weights are not normalised).
 *   loop       lower_prev = -inf; iteration it runs E, then M; change = lower - lower_prev; stop "converged" (0) if |change| < tol, else
 *              go on to max_iter (stop 1).  Stop "degenerate" (2) if after an M-step -- the start included, and the given variances of
 *              init 1 -- a variance is <= 0 or not finite, or if the bound is not finite: that restart has lower = -inf and is never the
 *              best unless all are degenerate, in which case the best is restart 0 and stat[2] = 2.  lower[r] is the last iteration's
 *              bound, evaluated before the last M-step (sklearn's lower_bound_); -inf with max_iter = 0.  trace[r, it] holds each
 *              iteration's bound; entries past the stop are -inf.
 *   result     the best restart is the first one with the largest lower among those not degenerate.  A final E-step under its final
 *              parameters gives logp (= lse_i), resp and label = the first maximum of t_ic (a row without a number takes component 0).
 *              avae_gmm_score is that final E-step for any rows and parameters: on the fitted rows, the fit's own bits.
 *   outputs    weights (k), means and covars (k, dim), label (N) of the best restart; stat (4) = best restart, its iterations, its stop,
 *              0; lower (n_init).  Optional: logp (N), resp (N, k), weights_all (n_init, k), means_all and covars_all (n_init, k, dim),
 *              stat_all (n_init, 4) = iterations, stop, 0, 0; trace (n_init, max_iter).
 *   range      2 <= N <= 2^22 (score: 1 <= n); 1 <= k <= min(N, 1024); dim a multiple of 4 in [4, 1024]; x 16-byte aligned.
 *   not finite inputs are NOT checked.  The result is then unspecified but complete; never a hang.
 *   bits       no float atomics; every sum has an order fixed by the plan, and the plan is a function of N, k, dim, n_init and the
 *              option alone: the same arguments and option give the same bits.
 *   cost       an iteration is five launches whether or not a restart has stopped.  The M-step forms t_ic again instead of storing
 *              the (N, k) panel.
 *   workspace  per restart 36 N bytes of lse and part records (+ 28 N per further component part, at most 16, only where there are few
 *              row tiles), 24 k dim of means, variances and precisions, 8 slices k (2 dim + 1) of M-step partials (slices <= 64; with
 *              the option <= 256); + 256-byte rounding, reserved once per call.
 * Errors (text through avae_last_error; checked on the host, before any launch; the outputs are left untouched): a null gc, x, weights,
 * means, covars, label, stat or lower; N, dim, k, n_init or max_iter out of range; x not 16-byte aligned; init or covariance outside
 * 0 .. 1; init 0 without label_in; init 1 without w_in, mu_in and cov_in; only some of weights_all, means_all, covars_all; tol or
 * reg_covar negative or NaN; reserved != 0; a workspace the device cannot give (the text names its size).
 * Option gmm_chunk (avae_set_option; a test aid): caps the components of a part and the rows of a tile and of a slice, so that small
 * tests run several of each and their merges; 0 lets the planner decide.  Another value may change last bits of sums; never a t_ic.
 * Option gmm_pad (0 .. 3; rows whose real column count is no multiple of 4): the last gmm_pad columns of x are padding.  Whatever they
 * hold, their variance is 1 (given variances there are not read), they have no share in the spherical mean, and the constant of t_ic
 * counts dim - gmm_pad columns.  With zeros in them (and zero means with init 1) they add exactly nothing to any q_ic: the other columns'
 * results are those of the unpadded rows.                                                                                             */
typedef struct avae_gmm_config {
    int32_t k;          /* components, 1 <= k <= min(N, 1024) */
    int32_t n_init;     /* restarts side by side in the one call, 1 .. 16 */
    int32_t max_iter;   /* EM iterations per restart, 0 .. 10000 (sklearn: 100); 0 = the start's parameters and the final E-step only */
    int32_t covariance; /* 0 diag, 1 spherical */
    int32_t init;       /* 0: label_in (n_init, N) -> one-hot responsibilities -> one M-step; 1: the parameters in w_in, mu_in, cov_in */
    int32_t reserved;   /* 0 */
    double  tol;        /* >= 0: stop when |change of the lower bound| < tol (sklearn: 1e-3) */
    double  reg_covar;  /* >= 0, added to every variance (sklearn: 1e-6) */
} avae_gmm_config;
int  avae_gmm_fit(avae_handle h, const float* x /* (N, dim) device */, int32_t N, int32_t dim, const avae_gmm_config* gc,
                  const int32_t* label_in /* (n_init, N), init 0 */,
                  const double* w_in /* (n_init, k) */, const double* mu_in, const double* cov_in /* (n_init, k, dim) each, init 1 */,
                  double* weights /* (k) */, double* means /* (k, dim) */, double* covars /* (k, dim) */,
                  int32_t* label /* (N) */, int32_t* stat /* (4) */, double* lower /* (n_init) */,
                  double* logp /* optional (N) */, double* resp /* optional (N, k) */,
                  double* weights_all, double* means_all, double* covars_all /* optional, all three or none: (n_init, ..) */,
                  int32_t* stat_all /* optional (n_init, 4) */, double* trace /* optional (n_init, max_iter) */);
int  avae_gmm_score(avae_handle h, const float* x /* (n, dim) device */, int32_t n, int32_t dim, int32_t k,
                    const double* weights, const double* means, const double* covars,
                    double* logp /* (n) */, int32_t* label /* optional (n) */, double* resp /* optional (n, k) */);

/* ---- cluster-quality scores of latent rows ----------------------------------------------------------------------------------------
 * scikit-learn's silhouette_samples / silhouette_score, calinski_harabasz_score (CH) and davies_bouldin_score (DB) of N rows for L
 * labelings of the SAME rows in ONE call: every pair distance is formed once per pass and binned for all labelings of the pass; no
 * (N, N) panel is kept.  Everything is enqueued on the handle's stream without a synchronisation.  Every pointer is device memory
 * except K, which the host reads.  All arithmetic is double; the rows are fp32.  Kmax = max_l K[l].  (The float64 restatement of this
 * contract is tests/sil_ref.py.)
 *   rows       X = double(x); for metric 1 X_i = x_i / sqrt(sum_j x_ij^2), a division in double; a zero row stays zero.
 *   distance   d(i, k): metric 0 sqrt(sum_j (X_ij - X_kj)^2); metric 2 the same sum without the root; metric 1
 *              min(max(1 - sum_j X_ij X_kj, 0), 2).  Differences, not the Gram trick: duplicate rows give exactly 0 under metrics 0
 *              and 2.  A pair's sum runs over j in ascending order.
 *   labeling   row i of labeling l is labelled c = label[l, i] if 0 <= c < K[l]; otherwise it is unlabelled in l: it belongs to no
 *              cluster, its values enter none of l's sums (a NaN row unlabelled in l leaves l's outputs finite), its sil and ab are 0,
 *              its nearest is -1 and it is left out of score.  (One labeling per topic with the other topics' rows at -1 gives
 *              per-topic scores in the same call.)
 *   silhouette n_c = members of cluster c; S_i(c) = sum of d(i, k) over the k labelled c, k != i, in ascending k.
 *              a_i = S_i(c_i) / (n_{c_i} - 1), 0 for a singleton; b_i = min over c != c_i with n_c > 0 of S_i(c) / n_c, 0 if there is
 *              none; nearest_i = the first c attaining it, -1 if there is none.  s_i = 0 if n_{c_i} = 1, if no other cluster is
 *              non-empty or if max(a_i, b_i) = 0; otherwise (b_i - a_i) / max(a_i, b_i): sklearn's values, its 0 for singletons and
 *              its nan_to_num included.  score[l] = the mean of s_i over the labelled rows (thread t of 256 the rows t, t + 256 ..,
 *              then the wave butterfly and the four waves ascending), 0 if there are none.  cluster_mean[l, c] = the mean of s_i over
 *              the members of c in ascending i, 0 where c is empty; count[l, c] = n_c; both are 0 at c >= K[l].
 *   CH, DB     on the rows X above (metric 2: those of metric 0).  k' = non-empty clusters, n' = labelled rows, m_c the member means
 *              (sums in ascending i), m = the mean of the labelled rows (the clusters' sums in ascending c, / n').  trW = sum_i |X_i -
 *              m_{c_i}|^2, trB = sum_c n_c |m_c - m|^2.  CH = (trB / (k' - 1)) / (trW / (n' - k')); NaN if k' < 2 or n' = k';
 *              otherwise 1.0 if trW = 0 (sklearn).  S_c = the mean Euclidean distance of the members to m_c, M_cc' = |m_c - m_c'|,
 *              R_cc' = (S_c + S_c') / M_cc', 0 where M = 0; DB = the mean over the non-empty c of max_{c' != c} R_cc'; NaN if k' < 2.
 *              index (L, 2) = CH, DB.
 *   outputs    score (L).  Optional: sil (L, N) = s; ab (L, N, 2) = a, b; nearest (L, N); count (L, Kmax); cluster_mean (L, Kmax);
 *              index (L, 2).
 *   range      2 <= N <= 2^18; dim a multiple of 4 in [4, 1024]; x 16-byte aligned; 1 <= K[l] <= 4096; 1 <= L <= 64.
 *   not finite values in labelled rows are NOT checked.  The result is then unspecified but complete; never a hang, never a write outside
 *              the outputs.  A label never indexes outside the bins.
 *   bits       no float atomics.  sil, ab and nearest are a function of the arguments alone: they do not depend on how the planner
 *              tiles the rows or groups the labelings (option sil_chunk).  Every other output has an order fixed by the shape.
 *   plan       a workgroup owns TI in {4, 8, 16, 32, 64} rows and walks all N columns in ascending tiles of 64; the bins of a pass
 *              (TI x sum K x 8 bytes) and the staging lie in the workgroup's LDS (160 KiB).  The planner takes the largest TI that
 *              needs no more passes over the labelings than TI = 4 does, then halves it while there are fewer row tiles than CUs; a
 *              pass forms the distances once for its labelings.  K = 4096 alone is one pass at TI = 4.
 *   workspace  4 (2 L + 1 + sum K) bytes of counts, 8 N of norms for the cosine, 8 L N unless sil is given; with index another
 *              8 (sum K)(dim + 2) + 8 L (2 N + dim + 4); + 256-byte rounding, reserved once per call.  Nothing is
 *              proportional to N^2 or N K.
 * Errors (text through avae_last_error; checked on the host, before any launch; each with its own text): a null sc, x, label, K or
 * score; N, dim, L, a K[l] or metric out of range; x not 16-byte aligned; a reserved field != 0; a device whose workgroups get less
 * than 160 KiB of LDS; a workspace the device cannot give (the text names its size).
 * Option sil_chunk (avae_set_option; a test aid): a value > 0 caps TI (the largest allowed value within it, at least 4; the CU
 * preference is then off), the columns of a tile and the bin columns of a pass (a labeling alone is always taken), so that small tests
 * run ragged tiles and several passes; 0 lets the planner decide.  sil, ab and nearest are the same bits for every value.            */
typedef struct avae_silhouette_config {
    int32_t metric;    /* 0 euclidean, 1 cosine, 2 squared euclidean */
    int32_t L;         /* labelings, 1 .. 64 */
    int32_t reserved;  /* 0 */
    int32_t reserved2; /* 0 */
} avae_silhouette_config;
int  avae_silhouette(avae_handle h, const float* x /* (N, dim) device */, int32_t N, int32_t dim, const avae_silhouette_config* sc,
                     const int32_t* label /* (L, N) device */, const int32_t* K /* (L) HOST */,
                     double* score /* (L) */, double* sil /* optional (L, N) */, double* ab /* optional (L, N, 2) */,
                     int32_t* nearest /* optional (L, N) */, int32_t* count /* optional (L, Kmax) */,
                     double* cluster_mean /* optional (L, Kmax) */, double* index /* optional (L, 2): CH, DB */);

/* ---- density clustering of latent rows ----------------------------------------------------------------------------------------------
 * DBSCAN of N rows in ONE call: no cluster count, clusters of any shape, and the rows that belong to no cluster (-1, which
 * avae_silhouette takes as "left out").  The labels are an exact, order-free function of the rows: scikit-learn's
 * DBSCAN(algorithm='brute') gives the same ones.  Everything is enqueued on the handle's stream without a synchronisation or a host
 * read; every stop is decided on the device.  Every pointer is device memory.  (The float64 restatement is tests/dbscan_ref.py.)
 *   pair value p(i, j) = sum_e (v_i[e] - v_j[e])^2 in double, e ascending for every tile shape; v = double(x), for metric 1 divided by
 *              the row's double norm sqrt(sum_e x_e^2) (a zero row stays zero).  p is symmetric by construction.  Metric 1: a pair
 *              with a zero row and i != j has p = 2 (distance 1, sklearn's value); p(i, i) = 0.
 *   within eps metric 0: p <= eps * eps (the product formed once, in double); metric 1: p <= 2 eps, that is 1 - cos <= eps.  Inclusive.
 *   core       row i is core when count[i] >= min_samples; count[i] = the rows within eps of i, itself included.
 *   clusters   core rows within eps of each other are in the same cluster (the transitive closure over core rows only); clusters are
 *              numbered 0, 1, .. in ascending order of their lowest core row.  A non-core row with a core row within eps takes the
 *              lowest cluster number among those core rows (a border row; it never joins two clusters); every other non-core row is
 *              noise: -1.
 *   outputs    label (N); count (N), optional; stat (8) = clusters, core rows, border rows, noise rows, rounds used, verify flag, 0, 0.
 *   rounds     the components are found in rounds of hook and pointer jump over a bit matrix of the pairs within eps; max_rounds
 *              rounds are enqueued (0: the planner's default, 2 (ceil(log2 N) + 1)), and those behind the fixed point return at once.
 *              A last pass walks every core-core pair: verify flag 0 = each joins equal labels; 1 = not converged within max_rounds,
 *              label then holds a partition that is too fine.  Call again with a larger max_rounds.
 *   range      1 <= N <= 2^17; dim a multiple of 4 in [4, 1024]; x 16-byte aligned; min_samples >= 1; eps > 0 and finite;
 *              0 <= max_rounds <= 4096.
 *   not finite values in the rows are NOT checked: a pair whose p is NaN is not within eps.  Never a hang, never a write outside the outputs.
 *   bits       no float atomics.  label, count and stat are a function of the arguments alone: they do not depend on how the planner
 *              tiles the pairs (option dbscan_chunk) nor on the interleaving of the hooks (integer minima).
 *   workspace  8 N ceil(N / 64) bytes of bit matrix (2 GiB at N = 2^17: why N stops there), 16 N of parents and numbers, 8 ceil(N / 64),
 *              4 (max_rounds + 1) + 16, 4 N unless count is given, 8 N of norms for the cosine; + 256-byte rounding, reserved once
 *              per call.
 * Errors (text through avae_last_error; checked on the host, before any launch; each with its own text): a null dc, x, label or stat;
 * N, dim, metric, min_samples, max_rounds or eps out of range; x not 16-byte aligned; reserved != 0; a workspace the device cannot give
 * (the text names its size).
 * Option dbscan_chunk (avae_set_option; a test aid): the low 8 bits of a value > 0 cap the rows TI of a tile (the largest of 4 .. 64
 * within them; 0: the planner's), the bits above give the column tiles of a part (0: the planner's).  Same bits for every value.    */
typedef struct avae_dbscan_config {
    int32_t metric;       /* 0 euclidean, 1 cosine */
    int32_t min_samples;  /* >= 1 */
    int32_t max_rounds;   /* 0: the planner's default */
    int32_t reserved;     /* 0 */
    double  eps;          /* > 0, finite */
} avae_dbscan_config;
int  avae_dbscan(avae_handle h, const float* x /* (N, dim) device */, int32_t N, int32_t dim, const avae_dbscan_config* dc,
                 int32_t* label /* (N) */, int32_t* count /* optional (N) */, int32_t* stat /* (8) */);

/* ---- principal components of latent rows ---------------------------------------------------------------------------------------------
 * PCA of N rows in ONE call: the mean, the covariance and its eigen-decomposition in double, everything enqueued on the handle's stream
 * without a synchronisation or a host read; every stop is decided on the device.  Every pointer is device memory.  (The float64
 * restatement is tests/pca_ref.py.)  dreal = dim - pad: the last pad columns of the rows are padding and are ignored.
 *   mean       the column means in double (the fp32 rows are exact as doubles).
 *   covariance C = sum_i (x_i - mean)(x_i - mean)^T / (N - 1) in double from the centred rows: two passes over the rows.
 *   solve      two-sided cyclic Jacobi on the dreal x dreal matrix, the pairs in round-robin order: with m = dreal rounded up to even,
 *              in round r = 0 .. m - 2 column m - 1 meets column r and every other column j meets (2 r - j) mod (m - 1); a partner
 *              >= dreal is the bye.  A pair p < q is rotated iff |a_pq| > thr = 2^-52 ||C||_F / dreal (absolute), with
 *              theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(1 + theta^2)), sign(0) = +1, c = 1 / sqrt(1 + t^2),
 *              s = t c; afterwards a_pq = 0 exactly, a_pp -= t a_pq, a_qq += t a_pq.  All rotations of a round are read off the
 *              matrix as it stands at the start of the round and applied together: A <- J^T A J, V <- V J.  The solve stops behind the
 *              first sweep without a rotation (converged) or behind max_sweeps sweeps (0: the planner's default, 58).
 *   order      eigenvalues descending, ties the smaller position on the diagonal first; var = the eigenvalues clipped below at 0.
 *   comp       row c = eigenvector c, its entry of largest magnitude (the first of equals) positive; row stride dim.
 *   stat (8)   sweeps run, converged 0 / 1, rotations (low 31 bits), rank = the number of var > thr, 0, 0, 0, 0.
 *   written    the leading dreal entries of mean and var and the leading dreal x dreal block of comp; the rest is left untouched.
 *   range      2 <= N <= 2^22; dim a multiple of 4 in [4, 1024]; 0 <= pad <= 3, pad < dim; x 16-byte aligned; 0 <= max_sweeps <= 256.
 *   not finite values in the rows are NOT checked: a pair whose a_pq is NaN is not rotated.  Never a hang, never a write outside the outputs.
 *   bits       no float atomics; partial sums are merged in ascending chunk order; the outputs are a function of the arguments and of
 *              option pca_chunk alone, the same for both forms of the solve (option pca_form) and for every call.
 *   workspace  8 (chunks dim + chunks pairs 4096 + 2 dreal^2) bytes, 4 dreal^2 for the launched solve, + 256-byte rounding; the partial
 *              tiles are capped at 256 MiB.
 * avae_pca_transform: y[i][c] = scale_c sum_j (x_ij - mean_j) comp[c][j], c < k, the sum over ALL dim columns in ascending order in
 * double, rounded once to fp32 (scale null: 1): a value depends on the row and the model alone.  It has no pad: the padding columns of
 * mean and comp must hold zeros (the Python layer allocates them so).  1 <= n <= 2^22, 1 <= k <= dim.
 * Errors (text through avae_last_error; checked on the host, before any launch; each with its own text): a null pc, x, mean, var, comp,
 * stat or y; N, n, dim, pad, max_sweeps or k out of range; x not 16-byte aligned; a reserved field != 0; pca_form 1 with dreal > 128;
 * a workspace the device cannot give.
 * Options (avae_set_option; test aids): pca_chunk > 0 caps the rows of a covariance chunk and of a transform tile; pca_form 0 the
 * planner's solve (resident where dreal <= 128), 1 resident, 2 launched.                                                              */
typedef struct avae_pca_config {
    int32_t pad;          /* the last 0..3 columns of the rows are padding */
    int32_t max_sweeps;   /* 0: the planner's default; else 1..256 */
    int32_t reserved;     /* 0 */
    int32_t reserved2;    /* 0 */
} avae_pca_config;
int  avae_pca_fit(avae_handle h, const float* x /* (N, dim) device */, int32_t N, int32_t dim, const avae_pca_config* pc,
                  double* mean /* (dim) */, double* var /* (dim) descending */, double* comp /* (dim, dim) row c = component c */,
                  int32_t* stat /* (8) */);
int  avae_pca_transform(avae_handle h, const float* x /* (n, dim) device */, int32_t n, int32_t dim, const double* mean /* (dim) */,
                        const double* comp /* (k, dim) */, const double* scale /* (k) or null */, int32_t k, float* y /* (n, k) */);

/* ---- kernel two-sample test of latent rows -------------------------------------------------------------------------------------------
 * Do two sets of rows come from the same distribution?  The unbiased kernel two-sample statistic MMD^2_u with a permutation null, for
 * G comparisons of 1 + P relabelings each over the SAME N rows in ONE call: every kernel value is formed once per pass and added for
 * all relabelings of the pass; nothing of size (N, N) or (N, G (1 + P)) reaches memory.  With kernel 1 the statistic is the energy
 * distance.  Every pointer is device memory; gamma is part of the config, which the host reads.  All arithmetic is double; the rows
 * are fp32.  (The float64 restatement of this contract is tests/mmd_ref.py.)
 *   rows       X = double(x); for metric 1 X_i = x_i / sqrt(sum_e x_ie^2), a division in double; a zero row stays zero.
 *   distance   d2(i, j) = sum_e (X_ie - X_je)^2, e ascending for every tile shape.  Duplicate rows give exactly 0.
 *   kernel     k(i, j): kernel 0 (rbf) sum_b exp(-(gamma[b] d2)) over b = 0 .. nbw - 1 ascending; kernel 1 (energy) -sqrt(d2).
 *   masks      W = ceil(N / 64) 64-bit words per bit row; bit i % 64 of word i / 64 is row i.  valid (G, W): the rows that take part
 *              in comparison g.  inA (G, 1 + P, W): A = valid & inA, B = valid & ~inA.  Relabeling 0 is the observed split; the
 *              others are the null (avae_mmd_relabel writes them).  Bits beyond N and inA bits outside valid are ignored.  A row
 *              that is valid in no comparison is never read as a number: it may hold NaN.
 *   statistic  per (g, p), over the unordered pairs i < j: U_AA = sum of k over the pairs with both rows in A, U_BB likewise for B;
 *              per comparison U_LL = the same over the valid rows; U_AB = U_LL - U_AA - U_BB.  With m = |A|, n = |B| of relabeling 0
 *              stat = 2 U_AA / (m (m - 1)) + 2 U_BB / (n (n - 1)) - 2 U_AB / (m n), evaluated left to right.
 *   order      a row's sum runs over its columns j > i in ascending j (only the columns on the row's own side); the 64 rows of a
 *              mask word are summed by the balanced binary tree over adjacent rows; the words in ascending order.
 *   outputs    stat (G, 1 + P); pvalue (G) = (1 + #{p >= 1: stat[g][p] >= stat[g][0]}) / (1 + P), 1 when P = 0; counts (G, 2) = m, n.
 *              Optional (may be null): sums (G, 1 + P, 2) = U_AA, U_BB; ull (G) = U_LL; witness (G, N) for relabeling 0, w_i = the
 *              mean of k(i, j) over the j in A, j != i, minus the mean over the j in B, j != i (columns ascending), 0 for a row
 *              that is not valid in g.  stat_out (1): 0, or 1 + g (1 + P) + p of the first relabeling whose |A| is not m (its stat
 *              is then computed with m and n all the same; nothing is read past a mask).
 *   range      2 <= N <= 2^17; dim a multiple of 4 in [4, 1024]; x 16-byte aligned; 1 <= G <= 64; 0 <= P; G (1 + P) <= 16384;
 *              1 <= nbw <= 8 and every gamma finite and > 0 (kernel 0); m >= 2 and n >= 2 in every comparison.
 *   bits       no float atomics.  Every output is a function of the arguments alone: the same bits however the planner tiles the
 *              rows or groups the relabelings (option mmd_chunk) and on every CU count.
 *   plan       a workgroup owns TI in {8, 16, 32, 64} rows and walks the column tiles of 64 from its own word on; the accumulators
 *              of a pass (TI x (relabelings + comparisons of the pass) x 8 bytes) and the staging lie in the workgroup's LDS
 *              (160 KiB); a pass forms the kernel values once for its relabelings.  A column tile is skipped when no comparison of
 *              the pass has valid rows in both the row tile and the column tile: per-topic comparisons of rows sorted by topic
 *              cost what their own rows cost.
 *   sync       m and n are checked on the host: the call waits once, for G pairs of counts, before the pair passes are enqueued.
 *              Everything else is enqueued on the handle's stream without a synchronisation.
 *   workspace  8 N of norms for the cosine, 8 G of counts, 16 (row tiles) (slots of a pass) of partial sums, 16 G (1 + P) unless sums
 *              is given, 8 G unless ull is given; + 256-byte rounding, reserved once per call.
 * avae_mmd_relabel writes the relabelings 1 .. P of every comparison from valid, relabeling 0 and a seed; the caller never builds the
 * masks on the host.  With mix64 the mixer of the library's generator, base = mix64(seed ^ (8 * 0xD6E8FEB86659FD93)) (stream 8),
 * c = mix64(base + ((g << 32) | p)) and key(i) = mix64(c + i), A of (g, p) is the m valid rows with the smallest (key, i) pairs, m =
 * |A| of relabeling 0.  The masks are an exact function of (valid, m, seed, g, p).  One launch, no synchronisation.
 * Errors (text through avae_last_error; checked on the host, before any output is written; each with its own text): a null mc, x,
 * valid, inA, stat, pvalue, counts or stat_out; N, dim, G, P, G (1 + P), nbw, kernel, metric or a gamma out of range; x not 16-byte
 * aligned; reserved != 0; a comparison with fewer than 2 rows in A or in B; a device whose workgroups get less than 160 KiB of LDS;
 * a workspace the device cannot give.
 * Option mmd_chunk (avae_set_option; a test aid): a value > 0 caps TI (the largest of 8 .. 64 within it, at least 8; the CU
 * preference is then off) and the relabelings of a pass, so that small tests run ragged tiles and several passes; 0 lets the planner
 * decide.  Same bits for every value.                                                                                                */
typedef struct avae_mmd_config {
    int32_t kernel;    /* 0 rbf, 1 energy */
    int32_t metric;    /* 0 euclidean, 1 cosine */
    int32_t G;         /* comparisons, 1 .. 64 */
    int32_t P;         /* relabelings behind the observed one, >= 0 */
    int32_t nbw;       /* bandwidths of the rbf kernel, 1 .. 8 (ignored for kernel 1) */
    int32_t reserved;  /* 0 */
    double  gamma[8];  /* the first nbw are read */
} avae_mmd_config;
int  avae_mmd(avae_handle h, const float* x /* (N, dim) device */, int32_t N, int32_t dim, const avae_mmd_config* mc,
              const uint64_t* valid /* (G, W) */, const uint64_t* inA /* (G, 1 + P, W) */,
              double* stat /* (G, 1 + P) */, double* pvalue /* (G) */, int32_t* counts /* (G, 2) */,
              double* sums /* optional (G, 1 + P, 2) */, double* ull /* optional (G) */, double* witness /* optional (G, N) */,
              int32_t* stat_out /* (1) */);
int  avae_mmd_relabel(avae_handle h, int32_t N, int32_t G, int32_t P, const uint64_t* valid /* (G, W) */,
                      uint64_t* inA /* (G, 1 + P, W): relabeling 0 is read, 1 .. P are written */, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* ARGSIM_VAE_H */
