// handle.cpp -- the handle's life and what hangs on it: create / destroy, options, the stream, the parameter table, tensor get / set,
// gradient buckets, timing collection, the shared scratch buffer and the GRU time-out check.
#include "ctx.h"

using namespace avae;
using namespace avae::host;

static std::string g_create_err;

namespace avae { namespace host {

// h->scratch is ONE buffer shared by get / set_tensor staging, the greedy and sampled loops, the beam search and its debug hook: every
// user lays it out afresh per call and all work is ordered on the handle's stream, so no call sees another's data.
int grow_scratch(avae_ctx* h, size_t need, const char* what)
{
    if (h->scratch_n >= (int64_t)need) return 0;
    if (h->scratch) {                                         // (work enqueued on the old buffer; a first buffer has nothing to wait for)
        AV_CHECK(hipStreamSynchronize(h->stream));
        AV_CHECK(hipFree(h->scratch));
    }
    h->scratch = nullptr; h->scratch_n = 0;
    if (hipMalloc(reinterpret_cast<void**>(&h->scratch), need) != hipSuccess) {
        (void)hipGetLastError();
        h->scratch = nullptr;
        char b_[256]; snprintf(b_, sizeof b_, "%s: %.0f MB of scratch could not be allocated on the device", what, (double)need / 1048576.0);
        return fail(h, b_);
    }
    h->scratch_n = (int64_t)need;
    return 0;
}

// -------------------------------------------------------------------------------- parameter table
static void add_param(avae_ctx* h, const std::string& name, std::initializer_list<int64_t> shape, int g16, int bucket, int64_t* off_out)
{
    ParamEntry e; e.name = name; e.offset = h->numel; e.ndim = (int)shape.size(); e.g16 = g16; e.bucket = bucket;
    int64_t n = 1; int k = 0;
    for (int i = 0; i < 4; ++i) e.shape[i] = 1;
    for (auto s : shape) { e.shape[k++] = s; n *= s; }
    if (off_out) *off_out = e.offset;
    h->numel += (n + 3) / 4 * 4;
    h->params.push_back(e);
}

static void build_params(avae_ctx* h)
{
    const int64_t D = h->cfg.dim_emb, V = h->cfg.dim_tgt, R = h->cfg.dim_rep; const int L = h->cfg.rnn_layers;
    h->enc.resize(L); h->dec.resize(L);
    auto close_bucket = [&](int64_t start) { h->buckets.push_back({start, h->numel - start}); };
    int bucket = 0; int64_t start = 0;
    add_param(h, "decode/out/kernel", {D, D}, 0, bucket, &h->oKout);
    add_param(h, "decode/out/bias", {D}, 0, bucket, &h->oBout);
    close_bucket(start);
    for (int i = L - 1; i >= 0; --i) {
        ++bucket; start = h->numel;
        std::string p = "decode/rnn/l" + std::to_string(i + 1) + "/";
        add_param(h, p + "W", {3 * D, D}, 1, bucket, &h->dec[i].W);
        add_param(h, p + "R", {3 * D, D}, 1, bucket, &h->dec[i].R);
        add_param(h, p + "bW", {3 * D}, 1, bucket, &h->dec[i].bW);
        add_param(h, p + "bR", {3 * D}, 1, bucket, &h->dec[i].bR);
        close_bucket(start);
    }
    ++bucket; start = h->numel;
    add_param(h, "latent/ex/kernel", {R, D}, 0, bucket, &h->oWex);
    add_param(h, "latent/ex/bias", {D}, 0, bucket, &h->oBex);
    add_param(h, "latent/mu/kernel", {2 * D, R}, 0, bucket, &h->oWmu);
    add_param(h, "latent/mu/bias", {R}, 0, bucket, &h->oBmu);
    add_param(h, "latent/lv/kernel", {2 * D, R}, 0, bucket, &h->oWlv);
    add_param(h, "latent/lv/bias", {R}, 0, bucket, &h->oBlv);
    close_bucket(start);
    for (int i = L - 1; i >= 0; --i) {
        ++bucket; start = h->numel;
        const int64_t In = i == 0 ? D : 2 * D;
        std::string p = "encode/rnn" + std::to_string(i + 1) + "/";
        int64_t o;
        add_param(h, p + "fwd/W", {3 * D, In}, 1, bucket, &h->enc[i].W);
        add_param(h, p + "bwd/W", {3 * D, In}, 1, bucket, &o);
        add_param(h, p + "fwd/R", {3 * D, D}, 1, bucket, &h->enc[i].R);
        add_param(h, p + "bwd/R", {3 * D, D}, 1, bucket, &o);
        add_param(h, p + "fwd/bW", {3 * D}, 1, bucket, &h->enc[i].bW);
        add_param(h, p + "bwd/bW", {3 * D}, 1, bucket, &o);
        add_param(h, p + "fwd/bR", {3 * D}, 1, bucket, &h->enc[i].bR);
        add_param(h, p + "bwd/bR", {3 * D}, 1, bucket, &o);
        close_bucket(start);
    }
    ++bucket; start = h->numel;
    add_param(h, "embed/embedding", {V, D}, 0, bucket, &h->oE);
    close_bucket(start);
}

static const ParamEntry* find_param(avae_ctx* h, const char* name)
{
    for (auto& e : h->params) if (e.name == name) return &e;
    return nullptr;
}

static float* state_buf(avae_ctx* h, int kind)
{
    switch (kind) { case AVAE_PARAM: return h->P; case AVAE_GRAD: return h->G; case AVAE_ADAM_M: return h->M; case AVAE_ADAM_V: return h->Vv; }
    return nullptr;
}

int check_gru_err(avae_ctx* h)
{
    int e = 0;
    AV_CHECK(hipMemcpyAsync(&e, h->errw, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    AV_CHECK(hipStreamSynchronize(h->stream));
    if (e) {
        (void)hipMemsetAsync(h->errw, 0, sizeof(int), h->stream);
        return fail(h, "GRU persistent kernel: an exchange wait timed out -- its workgroups were not all resident at once.  A persistent "
                       "launch needs every CU of the device (one handle = one GPU = one process, include/argsim_vae.h): another process or "
                       "stream computing on this GPU holds CUs the launch is waiting for.  Give the handle the device to itself, or "
                       "run with avae_set_option(\"persistent\", 0) (one launch per time step)");
    }
    return 0;
}
// the row / depth count a dyn-count GEMM ran with, as a fraction of the static bound its stamp was priced at.  Only the
// last step's count is still on the device (the bench repeats one batch, so it is every stamped step's count); each
// distinct count word is read once per collection.
int dyn_fraction(avae_ctx* h, const avae_ctx::Stamp& s, std::vector<std::pair<const int*, int>>& seen, double* f)
{
    *f = 1.0;
    if (!s.dyn || s.dyn_max <= 0) return 0;
    int c = -1;
    for (auto& e : seen) if (e.first == s.dyn) c = e.second;
    if (c < 0) {
        AV_CHECK(hipMemcpyAsync(&c, s.dyn, sizeof(int), hipMemcpyDeviceToHost, h->stream));      // behind the step that wrote the count
        AV_CHECK(hipStreamSynchronize(h->stream));
        if (c < 0) c = 0;
        seen.push_back({s.dyn, c});
    }
    *f = (double)std::min(c, s.dyn_max) / (double)s.dyn_max;
    return 0;
}

}}  // namespace avae::host

extern "C" {

int avae_create(const avae_config* cfg, int device, avae_handle* out)
{
    if (!cfg || !out) { g_create_err = "null argument"; return 1; }
    *out = nullptr;
    if (!gru_dim_supported(cfg->dim_emb)) { g_create_err = "dim_emb must be one of 16, 32, 64, 128, 256, 512 (the GRU kernels are instantiated for these widths only; the reference leaves dim_emb free, config.json uses 512)"; return 1; }
    if (cfg->compute_dtype < 0 || cfg->compute_dtype > 2) { g_create_err = "compute_dtype must be 0 (fp32 MFMA), 1 (bf16 GEMM operands) or 2 (fp32 via split bf16 MFMA)"; return 1; }
    if (cfg->dim_rep % 4 || cfg->dim_tgt % 4 || cfg->rnn_layers < 1 || cfg->rnn_layers > 8) { g_create_err = "dim_rep and dim_tgt must be multiples of 4 (16-byte rows); 1 <= rnn_layers <= 8"; return 1; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_create_err = "no HIP device available: the gfx950 kernels cannot run (no CPU fallback)"; return 1; }
    if (device < 0 || device >= ndev) { g_create_err = "bad device index"; return 1; }
    avae_ctx* h = new avae_ctx();
    h->cfg = *cfg; h->device = device;
    if (h->cfg.kl_beta == 0.f) h->cfg.kl_beta = 1.f;
    build_params(h);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->losses), 64 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->errw), 128 * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->counters), 2048 * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(h->losses, 0, 64 * sizeof(float));
    if (e == hipSuccess) e = hipMemset(h->errw, 0, 128 * sizeof(int));
    if (e == hipSuccess) e = hipMemset(h->counters, 0, 2048 * sizeof(unsigned));
    if (e != hipSuccess) { g_create_err = std::string("hip init failed: ") + hipGetErrorString(e); delete h; return 1; }
    h->acc = h->losses + 8;
    *out = h;
    return 0;
}

void avae_destroy(avae_handle h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream); else (void)hipDeviceSynchronize();
    if (h->ws) (void)hipFree(h->ws);
    if (h->losses) (void)hipFree(h->losses);
    if (h->errw) (void)hipFree(h->errw);
    if (h->hint_host) (void)hipHostFree(const_cast<int32_t*>(h->hint_host));
    if (h->counters) (void)hipFree(h->counters);
    if (h->stage_host) (void)hipHostFree(h->stage_host);
    if (h->stage_ev) (void)hipEventDestroy(h->stage_ev);
    if (h->scratch) (void)hipFree(h->scratch);
    if (h->bfA) (void)hipFree(h->bfA);
    if (h->slab) (void)hipFree(h->slab);
    if (h->bfP) (void)hipFree(h->bfP);
    if (h->bfB) (void)hipFree(h->bfB);
    if (h->lock_fd >= 0) (void)close(h->lock_fd);
    delete h;
}

const char* avae_last_error(avae_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int avae_set_stream(avae_handle h, void* s) { if (!h) return 1; h->stream = reinterpret_cast<hipStream_t>(s); return 0; }

int avae_get_dims(avae_handle h, int32_t* V, int32_t* D, int32_t* R, int32_t* L)
{
    if (!h) return 1;
    if (V) *V = h->cfg.dim_tgt; if (D) *D = h->cfg.dim_emb; if (R) *R = h->cfg.dim_rep; if (L) *L = h->cfg.rnn_layers;
    return 0;
}

int64_t avae_state_numel(avae_handle h) { return h ? h->numel : 0; }

int avae_bind_state(avae_handle h, float* p, float* g, float* m, float* v)
{
    if (!h) return 1;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return fail(h, "state buffers must be 16-byte aligned");
    h->P = p; h->G = g; h->M = m; h->Vv = v;
    return 0;
}

int avae_param_count(avae_handle h) { return h ? (int)h->params.size() : 0; }
const char* avae_param_name(avae_handle h, int i) { return (h && i >= 0 && i < (int)h->params.size()) ? h->params[i].name.c_str() : nullptr; }

int avae_param_info(avae_handle h, const char* name, int64_t* offset, int32_t* ndim, int64_t shape[4])
{
    if (!h) return 1;
    const ParamEntry* e = find_param(h, name);
    if (!e) return fail(h, std::string("unknown variable: ") + (name ? name : "(null)"));
    if (offset) *offset = e->offset; if (ndim) *ndim = e->ndim;
    if (shape) for (int i = 0; i < 4; ++i) shape[i] = e->shape[i];
    return 0;
}

static int xfer_tensor(avae_handle h, const char* name, int kind, float* buf, bool get)
{
    if (!h) return 1;
    AV_TRY(check_bound(h));
    const ParamEntry* e = find_param(h, name);
    if (!e) return fail(h, std::string("unknown variable: ") + (name ? name : "(null)"));
    float* base = state_buf(h, kind);
    if (!base) return fail(h, "bad tensor kind");
    float* flat = base + e->offset;
    int64_t n = e->shape[0] * e->shape[1] * e->shape[2] * e->shape[3];
    if (!e->g16) {
        AV_CHECK(hipMemcpyAsync(get ? buf : flat, get ? flat : buf, n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    } else {
        int D = h->cfg.dim_emb, cols = (int)(e->ndim == 2 ? e->shape[1] : 1);
        if (get) AV_CHECK(g16_permute(h->stream, buf, flat, D, cols, false));
        else     AV_CHECK(g16_permute(h->stream, flat, buf, D, cols, true));
    }
    return 0;
}
int avae_get_tensor(avae_handle h, const char* name, int kind, float* buf) { return xfer_tensor(h, name, kind, buf, true); }
int avae_set_tensor(avae_handle h, const char* name, int kind, const float* buf) { return xfer_tensor(h, name, kind, const_cast<float*>(buf), false); }

int avae_get_step(avae_handle h, int64_t* s) { if (!h || !s) return 1; *s = h->step; return 0; }
int avae_set_step(avae_handle h, int64_t s) { if (!h) return 1; h->step = s; return 0; }

int avae_set_grad_hook(avae_handle h, avae_grad_hook hook, void* user) { if (!h) return 1; h->hook = hook; h->hook_user = user; return 0; }

// undocumented knob used by tests/bench: 1 = persistent GRU kernels (default), 0 = one launch per time step
int avae_set_option(avae_handle h, const char* key, int value)
{
    if (!h || !key) return 1;
    if (!strcmp(key, "persistent")) { h->persistent = value; return 0; }
    if (!strcmp(key, "gru_item")) { h->gru_item = value; return 0; }
    if (!strcmp(key, "gru_stagger")) { h->gru_stagger = value; return 0; }
    if (!strcmp(key, "gru_force_slow")) { h->gru_force_slow = value; return 0; }
    if (!strcmp(key, "gru_bf16")) { h->gru_bf16 = value != 0; return 0; }
    if (!strcmp(key, "bwd_rs")) { h->bwd_rs = value; return 0; }
    if (!strcmp(key, "dyn_split")) { h->dyn_split = value != 0; return 0; }
    if (!strcmp(key, "shared_device")) { h->shared_device = value != 0; return 0; }
    if (!strcmp(key, "gru_spec")) { h->gru_spec = value; return 0; }
    if (!strcmp(key, "gru_ring")) { h->gru_ring = value != 0; return 0; }
    if (!strcmp(key, "bf16_nt8")) { h->bf16_nt8 = value != 0; return 0; }
    if (!strcmp(key, "logits16")) { h->logits16 = value != 0; return 0; }
    if (!strcmp(key, "bf16_direct")) { h->bf16_direct = value != 0; return 0; }
    if (!strcmp(key, "bf16_tn")) { h->bf16_tn = value != 0; return 0; }
    if (!strcmp(key, "bf16_sv")) { h->bf16_sv = value != 0; return 0; }
    if (!strcmp(key, "bf16_act")) { h->bf16_act = value != 0; return 0; }
    if (!strcmp(key, "table_l1")) { h->table_l1 = value != 0; return 0; }
    if (!strcmp(key, "enc_top1")) { h->enc_top1 = value != 0; return 0; }
    if (!strcmp(key, "dyn_thin")) { h->dyn_thin = value != 0; return 0; }
    if (!strcmp(key, "skip_pad")) { h->skip_pad = value != 0; return 0; }
    if (!strcmp(key, "compact")) { h->compact = value; return 0; }
    if (!strcmp(key, "skinny")) { h->skinny = value; return 0; }
    if (!strcmp(key, "knn_chunk")) { if (value < 0) return fail(h, "knn_chunk must be >= 0"); h->knn_chunk = value; return 0; }
    if (!strcmp(key, "agg_chunk")) { if (value < 0) return fail(h, "agg_chunk must be >= 0"); h->agg_chunk = value; return 0; }
    if (!strcmp(key, "ward_form")) { if (value < 0 || value > 2) return fail(h, "ward_form must be 0 (planner), 1 (one-workgroup) or 2 (launch-per-merge)"); h->ward_form = value; return 0; }
    if (!strcmp(key, "probe_chunk")) { if (value < 0) return fail(h, "probe_chunk must be >= 0"); h->probe_chunk = value; return 0; }
    if (!strcmp(key, "sil_chunk")) { if (value < 0) return fail(h, "sil_chunk must be >= 0"); h->sil_chunk = value; return 0; }
    if (!strcmp(key, "dbscan_chunk")) { if (value < 0) return fail(h, "dbscan_chunk must be >= 0"); h->dbscan_chunk = value; return 0; }
    if (!strcmp(key, "pca_chunk")) { if (value < 0) return fail(h, "pca_chunk must be >= 0"); h->pca_chunk = value; return 0; }
    if (!strcmp(key, "mmd_chunk")) { if (value < 0) return fail(h, "mmd_chunk must be >= 0"); h->mmd_chunk = value; return 0; }
    if (!strcmp(key, "pca_form")) { if (value < 0 || value > 2) return fail(h, "pca_form must be 0 (planner), 1 (resident) or 2 (launched)"); h->pca_form = value; return 0; }
    if (!strcmp(key, "kmeans_chunk")) { if (value < 0) return fail(h, "kmeans_chunk must be >= 0"); h->kmeans_chunk = value; return 0; }
    if (!strcmp(key, "gmm_chunk")) { if (value < 0) return fail(h, "gmm_chunk must be >= 0"); h->gmm_chunk = value; return 0; }
    if (!strcmp(key, "gmm_pad")) { if (value < 0 || value > 3) return fail(h, "gmm_pad must be in [0, 3]"); h->gmm_pad = value; return 0; }
    if (!strcmp(key, "tsne_chunk")) { if (value < 0) return fail(h, "tsne_chunk must be >= 0"); h->tsne_chunk = value; return 0; }
    if (!strcmp(key, "gru_ablate")) {
        // timing experiments that change results exist only in the diagnostic build (make DIAG=1)
        if (value && !gru_diag_build()) return fail(h, "gru_ablate needs the diagnostic build of libargsim_vae.so (make -C argsim_amd/csrc DIAG=1)");
        h->gru_ablate = value; return 0;
    }
    if (!strcmp(key, "timing")) { h->timing = value; h->timing_on = value; h->stamps_used = 0; return 0; }
    if (!strcmp(key, "timing_pause")) { h->timing = value ? 0 : h->timing_on; return 0; }
    return fail(h, "unknown option");
}
// synchronises, sums the HIP-event durations recorded since timing was switched on / last collected:
// out[3*c + 0..2] = total ms, launches, EXECUTED FLOPs of kernel class c (0 GEMM, 1 GRU fwd, 2 GRU bwd): a GEMM whose
// row count or depth is a device-side count (the table-fed layers' present ids, the kept tokens) exits at that count,
// so its 2MNK is scaled by count / static bound
int avae_timing_collect(avae_handle h, double* out)
{
    if (!h || !out) return 1;
    AV_CHECK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < 9; ++i) out[i] = 0.0;
    std::vector<std::pair<const int*, int>> seen;
    for (size_t i = 0; i < h->stamps_used; ++i) {
        float ms = 0.f;
        AV_CHECK(hipEventElapsedTime(&ms, h->stamps[i].a, h->stamps[i].b));
        double f = 1.0;
        AV_TRY(dyn_fraction(h, h->stamps[i], seen, &f));
        int c = h->stamps[i].cls;
        out[3 * c] += ms; out[3 * c + 1] += 1.0; out[3 * c + 2] += h->stamps[i].flops * f;
    }
    h->stamps_used = 0;
    return 0;
}
int avae_bucket_count(avae_handle h) { return h ? (int)h->buckets.size() : 0; }
int avae_bucket_info(avae_handle h, int i, int64_t* offset, int64_t* count)
{
    if (!h || i < 0 || i >= (int)h->buckets.size()) return 1;
    *offset = h->buckets[i].first; *count = h->buckets[i].second; return 0;
}

}  // extern "C"
