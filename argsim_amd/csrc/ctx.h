// ctx.h -- what the host files share (model.cpp, handle.cpp, generate.cpp, scoring.cpp, hooks.cpp): the handle, the error macros, the
// workspace and its bump allocator, the GEMM call builder and the helpers that more than one file calls.  Internal: not part of the
// C ABI (include/argsim_vae.h); what is declared here has hidden visibility, so nothing in avae::host is exported from the shared object.
#pragma once
#include "../../include/argsim_vae.h"
#include "kernels.h"

#include <fcntl.h>
#include <sys/file.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)
namespace avae { namespace host {

struct ParamEntry {
    std::string name;
    int64_t offset;
    int ndim;
    int64_t shape[4];
    int g16;          // rows are stored gate-interleaved (GRU W/R/bW/bR)
    int bucket;
};

struct GruP { int64_t W, R, bW, bR; };     // offsets into the flat state

}}  // namespace avae::host
#pragma GCC visibility pop

struct avae_ctx {
    avae_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    std::vector<avae::host::ParamEntry> params;
    int64_t numel = 0;
    std::vector<std::pair<int64_t, int64_t>> buckets;    // (offset, count) in completion order
    float *P = nullptr, *G = nullptr, *M = nullptr, *Vv = nullptr;
    int64_t step = 0;
    avae_grad_hook hook = nullptr; void* hook_user = nullptr;
    std::vector<int> hook_pending;     // buckets complete but not yet announced (see hook_flush)
    int persistent = 1;
    bool first_step_checked = false;
    int gru_ablate = 0, gru_force_slow = 0, gru_stagger = 0, gru_item = 2;
    int skinny = 1;       // a few rows (latent block, one-step top layer; backward: remainder rows, small products): one 32x32 tile per workgroup,
                          // K split over its waves (gemm_f32.hip); 0: the tiled forms
    int score_plan[4] = {0, 0, 0, 0};      // last avae_score / avae_score_z: decoder batch size N, rows rc and draws kc per batch, batches whose draws shared one first-layer projection through a row index
    const int* expect_ptr[3] = {nullptr, nullptr, nullptr}; int expect_val[3] = {0, 0, 0};      // (dyn_expected)
    int compact = 2;      // encoder activations stored over the REAL rows only (row_map / GruArgs::rowmap): padded rows of a ragged batch cost nothing in the
                          // encoder's GEMMs.  0 off, 1 on, 2 auto: on where the share of real positions the previous calls reported is below 0.85 (fill_hint)
    int skip_pad = 1;     // team GRU kernels skip the steps behind a row block's longest row (rows sorted by length, ops.hip row_order); 0: every step of every row
    int shared_device = 0; int lock_fd = -1;      // option shared_device: persistent launches are taken one at a time ACROSS processes (DeviceTurn)
    int dyn_split = 1;    // ragged batches: narrow backward GEMMs over few expected rows split K instead of leaving the chip at one workgroup per CU (gemm())
    int dyn_thin = 1;     // device-row-count GEMMs with a narrow output run 64x64 tiles (gemm())
    int enc_top1 = 1;     // the top encoder layer's backward direction runs its ONE live step only (gru_reg.hip "one step from a zero state"); 0: all S steps like the reference's graph
    int table_l1 = 1;     // layers fed by embedding rows project the TABLE once and gather / scatter by id where a batch has more tokens than the vocabulary (use_table)
    int bf16_act = 1;     // compute_dtype 1: h / h_prev row-major copies written as bf16 by the forward team kernels (the GEMM operands as they stand)
    int bf16_sv = 1;      // compute_dtype 1: saved gates as bf16 where a layer's forward and backward both run the team kernels
    int bf16_tn = 1;      // compute_dtype 1: the BPTT team kernels write the gate gradients as bf16 and the weight-gradient GEMMs read row-major bf16 operands through transposing LDS loads (gemm_bf16_tn): no transposed copies
    int logits16 = 1;     // compute_dtype 1, training forward: the logits leave the phased GEMM as an fp16 panel that softmax_ce turns into the bf16 gradient in place (no fp32 logits)
    int bf16_nt8 = 1;     // compute_dtype 1: NT GEMMs on the phased LDS-DMA kernel (gemm_bf16_p8.hip) where the shape allows (0: the register-staged 256x256 kernel)
    int bf16_direct = 0;  // (measured at configs[2]: 50.2 ms with it, 43.3 ms with the conversion passes + 256x256 NT kernel: off)
    //  compute_dtype 1: GEMMs read their fp32 operands directly and round to bf16 while staging (0: conversion passes + NT kernel)
    int gru_spec = 2;     // team kernels load a consumer's operand at once, without a probe round trip in front of it: 0 never, 1 always, 2 where few rows are alive per
                          // step (spec_pick: RAGGED 256 x 64 10.41 -> 10.23 ms; always-on costs a FULL 100 x 512 batch 1 %, 71.5 -> 72.3 ms, and a FULL 256 x 64 nothing)
    int gru_ring = 1;     // fp32 team kernels with one row block per workgroup exchange through a 4-slot ring the producers re-arm themselves (GruPlan::ring): the launcher
                          // fills min(S, 4) slots per job instead of S; 0: one slot per position (in-process A/B runs)
    int bwd_rs = 2;       // fp32 BPTT team kernels in the reduce-scatter form (gru_rs.hip: own gate columns x resident R slice, partial dH summed through the
                          // exchange): 0 never, 1 wherever the geometry allows, 2 auto -- where few rows are alive per step (rs_pick)
    int knn_chunk = 0;    // avae_knn test aid: caps the bank rows one workgroup walks (small tests run many parts and the merge); 0: knn_plan decides
    int agg_chunk = 0;    // avae_agg_logq test aid: caps the bank rows of a part (small tests run several parts and the merge); 0: agg_plan decides
    int ward_form = 0;    // avae_ward test aid: 0 the planner picks the kernel form from the largest group, 1 one-workgroup, 2 launch-per-merge (same bits)
    int probe_chunk = 0;  // avae_probe_fit / avae_probe_decision test aid: caps the rows of a part (small tests run several parts and the merge); 0: probe_plan decides
    int tsne_chunk = 0;   // avae_tsne test aid: caps the columns of a part of the pair walks (small tests run several parts); 0: tsne_plan decides
    int kmeans_chunk = 0; // avae_kmeans test aid: caps the centres of a part and the rows of a tile, a slice and a sort block (small tests run several parts); 0: km_plan decides
    int gmm_chunk = 0;    // avae_gmm_fit / avae_gmm_score test aid: caps the components of a part and the rows of a tile and of a slice (small tests run several of each); 0: gm_plan decides
    int gmm_pad = 0;      // avae_gmm_fit / avae_gmm_score: the last 0 .. 3 columns of the rows are padding to the multiple of 4 (variance 1, no share in the constants)
    int sil_chunk = 0;  // avae_silhouette test aid: caps the rows and columns of a tile and the bin columns of a pass (small tests run ragged tiles and several passes); 0: sil_plan decides
    int dbscan_chunk = 0;  // avae_dbscan test aid: the low 8 bits cap the rows of a tile, the bits above give the column tiles of a part (small tests run several tile shapes and parts); 0: db_plan decides
    int pca_chunk = 0;     // avae_pca_fit / avae_pca_transform test aid: caps the rows of a covariance chunk and of a transform tile (small tests run several chunks); 0: pca_plan decides
    int mmd_chunk = 0;     // avae_mmd test aid: caps the rows of a tile and the relabelings of a pass (small tests run ragged tiles and several passes); 0: mmd_plan decides
    int pca_form = 0;      // avae_pca_fit: 0 the planner's solve, 1 the resident one (one workgroup, dreal <= 128), 2 the launched one (a launch per round); same bits
    int gru_bf16 = 1;     // compute_dtype 1 only: the recurrent product of the team kernels takes bf16 operands too (0: fp32 recurrence)
    // offsets
    int64_t oE = 0, oKout = 0, oBout = 0, oWmu = 0, oBmu = 0, oWlv = 0, oBlv = 0, oWex = 0, oBex = 0;
    std::vector<avae::host::GruP> enc;     // per layer: W = [fwd;bwd] (6D,In), R = [fwd;bwd], bW (6D), bR (6D)
    std::vector<avae::host::GruP> dec;
    // small persistent device state
    float* losses = nullptr;   // [3]
    float* acc = nullptr;      // [2] sum loss_gen_samp, sum kld
    int* errw = nullptr;       // GRU spin time-out word
    unsigned* counters = nullptr;
    float* scratch = nullptr;  // staging for get/set tensor
    int64_t scratch_n = 0;
    // workspace
    char* ws = nullptr; size_t ws_cap = 0;
    // last forward geometry
    int B = 0, Ss = 0, St = 0;
    // optional per-kernel-class timing with HIP events on the launch stream (bench.py roofline leg)
    int timing = 0, timing_on = 0;
    // bf16-operand GEMM mode (compute_dtype = 1): converted operand panels
    unsigned short *bfA = nullptr, *bfB = nullptr; size_t bfA_cap = 0, bfB_cap = 0;
    float* slab = nullptr; size_t slab_floats = 0;     // bf16 mode: the K slices' partial tiles of the weight-gradient GEMMs (gemm_bf16_p8.hip; 512 tiles of 256 x 256)
    unsigned short* bfP = nullptr; size_t bfP_cap = 0;     // bf16 mode: (softmax - onehot)/N as written by softmax_ce_kernel, (N,V) bf16
    // (dyn / dyn_max: a GEMM whose M or K is a device-side count -- its FLOPs are scaled by count / static bound at collection)
    struct Stamp { hipEvent_t a, b; int cls; double flops; const int* dyn; int dyn_max; };
    std::vector<Stamp> stamps; size_t stamps_used = 0;
    // fill hint: the real source positions of an earlier call, copied to pinned host memory without a synchronisation (whatever has
    // arrived is read; it only ever decides the LAYOUT, never a value) and the padded positions of the call that issued the copy
    int32_t* hint_dev = nullptr; volatile int32_t* hint_host = nullptr;
    // what had arrived where the current call began (latch_hint, build_row_orders): every decision of ONE call reads this pair, so a call's own
    // copy landing while the call is still being enqueued cannot give its forward one hint and its backward another
    uint64_t hint_seen = 0xffffffffull;
    // pinned staging of the small host tables a call uploads and does not wait for (stage_h2d): it outlives the call, stage_ev says when the
    // last upload from it has been read
    void* stage_host = nullptr; size_t stage_cap = 0; hipEvent_t stage_ev = nullptr;
    const int32_t *cnt_src = nullptr, *cnt_tgt = nullptr;     // present-id counts of the last forward (table-fed layers), device
    // The route of the last avae_forward_backward (avae_debug_step_route), noted by the step where it decides (note_gru, model.cpp): the first
    // layers table-fed (use_table), Ws::compact / compact_d / Bx, the BPTT form rs_pick gave, whether the top encoder layer ran its one-job
    // launch + the one-step kernels (top_one_step), and per kind of GRU launch (RouteGru) the plan it ran as form, T, C, pipe, ring (form -1:
    // no such launch).  live: a step is being enqueued -- the other callers of the same pieces (encode, eval, score) note nothing.
    struct Route { bool live = false; int tab_src = -1, tab_tgt = -1, compact = -1, compact_d = -1, Bx = -1, rs = -1, top1 = -1; int gru[6][5] = {}; } route;
};

#pragma GCC visibility push(hidden)
namespace avae { namespace host {

#define AV_CHECK(expr)                                                                              \
    do { hipError_t e_ = (expr); if (e_ != hipSuccess) {                                            \
        char b_[512]; snprintf(b_, sizeof b_, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
        h->err = b_; return 1; } } while (0)
#define AV_TRY(expr) do { int r_ = (expr); if (r_) return r_; } while (0)

inline int fail(avae_ctx* h, const std::string& m) { h->err = m; return 1; }
// Upload a small host table on the handle's stream from a call that returns WITHOUT synchronising: the caller's array (a function-local
// vector) may die at return, while a stream that is still busy reads the source only when it gets there.  The bytes go through pinned
// memory the handle owns; the event says when the previous upload has been read, so the wait is over at once unless the stream is
// still in front of that copy.
inline int stage_h2d(avae_ctx* h, void* dst, const void* src, size_t bytes)
{
    if (!bytes) return 0;
    if (!h->stage_ev) AV_CHECK(hipEventCreateWithFlags(&h->stage_ev, hipEventDisableTiming));
    else AV_CHECK(hipEventSynchronize(h->stage_ev));
    if (bytes > h->stage_cap) {
        if (h->stage_host) AV_CHECK(hipHostFree(h->stage_host));
        h->stage_host = nullptr; h->stage_cap = 0;
        const size_t cap = (bytes + 4095) & ~(size_t)4095;
        AV_CHECK(hipHostMalloc(&h->stage_host, cap, hipHostMallocDefault));
        h->stage_cap = cap;
    }
    memcpy(h->stage_host, src, bytes);
    AV_CHECK(hipMemcpyAsync(dst, h->stage_host, bytes, hipMemcpyHostToDevice, h->stream));
    AV_CHECK(hipEventRecord(h->stage_ev, h->stream));
    return 0;
}
// the rule every latent-row entry has for its row operands: dim a multiple of 4 in [4, 1024], the pointers in `ptrs` (which `names`
// names in the message) 16-byte aligned
inline int check_rows(avae_ctx* h, const char* what, int dim, const char* names, std::initializer_list<const void*> ptrs)
{
    if (dim < 4 || dim > 1024 || (dim & 3)) return fail(h, std::string(what) + ": dim must be a multiple of 4 in [4, 1024]");
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= (uintptr_t)p;
    if (bits & 15) return fail(h, std::string(what) + ": " + names + " must be 16-byte aligned");
    return 0;
}

// persistent GRU launches: the residency check of the GRU launchers (gru_dev.h) answers hipErrorCooperativeLaunchTooLarge
#define AV_GRU(expr)                                                                                                \
    do { hipError_t e_ = (expr);                                                                                    \
         if (e_ == hipErrorCooperativeLaunchTooLarge)                                                               \
             return fail(h, "persistent GRU kernel: its workgroups cannot all be resident on this device at once (occupancy query x CU count < grid); " \
                            "run with avae_set_option(\"persistent\", 0)");                                         \
         if (e_ != hipSuccess) { char b_[512]; snprintf(b_, sizeof b_, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
             h->err = b_; return 1; } } while (0)

// A persistent GRU launch needs every CU, so two PROCESSES computing on one device (several data-parallel ranks rehearsed on one
// GPU, a second job) can each get part of the chip and both run into the 2 s exchange time-out.  Option shared_device = 1: every
// persistent launch is taken in turn across processes -- an exclusive flock on a per-device lock file from before the launch
// is enqueued until it has COMPLETED (one stream synchronisation per launch: slower, never wrong).  Non-persistent kernels of another
// process only delay a persistent launch; they cannot strand it.
struct DeviceTurn {
    avae_ctx* h; bool held = false;
    explicit DeviceTurn(avae_ctx* h_) : h(h_) {
        if (!h->shared_device || !h->persistent) return;
        if (h->lock_fd < 0) {
            char path[64]; snprintf(path, sizeof path, "/tmp/argsim_vae_dev%d.lock", h->device);
            h->lock_fd = open(path, O_CREAT | O_RDWR, 0666);
        }
        if (h->lock_fd >= 0 && flock(h->lock_fd, LOCK_EX) == 0) held = true;
    }
    ~DeviceTurn() { if (held) { (void)hipStreamSynchronize(h->stream); (void)flock(h->lock_fd, LOCK_UN); } }
};

// kernel classes for the timing hook: 0 = MFMA GEMM, 1 = GRU forward, 2 = GRU backward
struct Timed {
    avae_ctx* h; avae_ctx::Stamp* s = nullptr;
    Timed(avae_ctx* h_, int cls, double flops, const int* dyn = nullptr, int dyn_max = 0) : h(h_) {
        if (!h->timing) return;
        if (h->stamps_used == h->stamps.size()) {
            avae_ctx::Stamp n{};
            if (hipEventCreate(&n.a) != hipSuccess || hipEventCreate(&n.b) != hipSuccess) return;
            h->stamps.push_back(n);
        }
        s = &h->stamps[h->stamps_used++];
        s->cls = cls; s->flops = flops; s->dyn = dyn; s->dyn_max = dyn_max;
        (void)hipEventRecord(s->a, h->stream);
    }
    ~Timed() { if (s) (void)hipEventRecord(s->b, h->stream); }
};

// -------------------------------------------------------------------------------- workspace
struct Ws {
    // ints
    int32_t *src_tm, *lens_src, *lens_tgt, *lead, *gold, *rank, *cidx, *ntok, *pred;
    // forward
    float *emb_src, *emb_tgt, *ew, *dew;
    std::vector<float*> e_gi, e_hs, e_sv[2], e_hp[2];
    std::vector<float*> d_gi, d_hd, d_sv, d_hp;
    float *hpick, *mu, *lv, *z, *eps, *kld, *h0;
    float *xlast, *gib, *svb, *dgib, *dghb, *dxl;     // one-step top backward direction (top_one_step): (B,2D) (B,3D) (B,D,4) (B,3D) (B,3D) (B,2D)
    float *hc, *ho, *logits;
    float *loss_samp, *errt_samp;
    // backward
    float *dho, *dhc, *dhd[2], *dgi_d, *dgh_d, *dh0, *carry, *dh0sum, *dz, *dmu, *dlv, *dhpick;
    float *dhs[2], *dgi_e, *dgh_e, *demb_src, *demb_tgt;
    std::vector<unsigned short*> e_hs16, d_hd16, e_hp16[2], d_hp16;      // bf16 mode: h / h_prev as the forward team kernels write them (bf16_act)
    std::vector<char> act_e, act_d, acth_e, acth_d;                       // per layer: hs16 / hp16 in use this call
    std::vector<unsigned short*> x16_e, x16_d;                 // bf16 mode: the layer inputs as the forward GEMMs converted them (row-major: the backward's TN operand)
    const unsigned short* x16_kept_e(int i) const { return x16_valid ? x16_e[i] : nullptr; }
    const unsigned short* x16_kept_d(int i) const { return x16_valid ? x16_d[i] : nullptr; }
    bool x16_valid = false;
    unsigned short *dgi16_d, *dgh16_d, *dgi16_e, *dgh16_e;      // bf16 mode: the gate gradients as the BPTT team kernels write them (bf16_tn)
    int32_t* scat;                        // embed_scatter_add2's token lists
    int32_t *grp_src, *grp_tgt;           // id_groups_build scratch of the two id sources (use_table)
    int32_t *tokrow_src, *tokrow_tgt;
    float* xbuf; size_t xbuf_floats;      // exchange scratch of the GRU team kernels (GruArgs::xbuf)
    // row orders of the padding-skipping team kernels (build_row_orders): 0 = encoder, both directions; 1 = encoder, one job
    // (top layer); 2 = decoder.  ord_ok: built for this call with geometry (ord_T, ord_cpj)
    int32_t *ord_perm[3], *ord_slens[3]; int ord_T[3], ord_cpj[3]; bool ord_ok[3];
    // compact encoder layout (build_compact): map_src[(t, b)] = row among the real source positions or -1, nsrc = how many
    int32_t *map_src, *nact_src, *nsrc; bool compact;
    // the decoder's: map_tgt[(t, b)] over the positions t <= (last non-eos target position of row b) + 1, ntgt = how many
    int32_t *map_tgt, *nact_tgt, *ntgt; bool compact_d;
    // rows of the GRU team kernels' launch geometry (gru_team_batch): = B where B itself has one, else the next row count that has;
    // the slots beyond B hold phantom rows (GruArgs::Bx), which exist through the row order + the compact layout only
    int Bx;
    int bx_enc() const { return compact ? Bx : 0; }
    int bx_dec() const { return compact_d ? Bx : 0; }
};

struct Bump {
    char* base; size_t off = 0;
    template <class T> T* take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
    // a buffer a kernel takes only with `on`: null without (the kernels read the pointer as the flag)
    template <class T> T* opt(bool on, size_t n) { return on ? take<T>(n) : nullptr; }
};

// second problem of a pair (same shape, layout, scalars): see GemmArgs in kernels.h
struct Pair { const float* A; const float* B; float* C; const float* bias; };

// One GEMM product as a value: C = alpha * op(A) op(B) (+bias) (+C), layouts as in GemmArgs (kernels.h).  Built by nt() / nn() / tn_grad()
// and the setters below; gemm() takes its launches from gemm_plan() (gemm_plan.cpp), which sees the shape, the flags here and the options.
struct GemmCall {
    const float* A; int lda; bool a_mc;
    const float* B; int ldb; bool b_nc;
    float* C; int ldc;
    int M, N, K;
    float alpha = 1.f; const float* bias = nullptr; int accumulate = 0;
    const int* dyn = nullptr; int dyn_kind = 0;      // device-side count: 1 the rows (M), 2 the depth (K)
    const Pair* pair = nullptr;
    bool wgrad = false;                 // weight gradient: C holds the zero-filled gradient (tn_grad)
    bool allow_atomic = false;          // backward: the plan may split K with float atomics into the cleared output
    bool rows_are_batch = false;        // forward: the rows are the batch rows -- the skinny form whatever the batch size (gemm_plan)
    int thin = -1, split_k = 0;         // a caller's own tile form (GemmArgs::thin) / K split; -1 / 0: the plan's
    // bf16 mode only
    const unsigned short* A16 = nullptr; const unsigned short* B16 = nullptr;      // the operand as a producer wrote it in bf16, row-major with the same leading dimension (gemm_bf16_pre, gemm_tn16)
    unsigned short* keep_a16 = nullptr; // the k-contiguous A operand is converted HERE and left for the backward's weight-gradient GEMM
    unsigned short* c16 = nullptr;      // GemmArgs::c16: the result as an fp16 panel instead of C

    GemmCall& scaled(float a) { alpha = a; return *this; }
    GemmCall& biased(const float* b) { bias = b; return *this; }
    GemmCall& plus() { accumulate = 1; return *this; }
    GemmCall& rows(const int* d) { dyn = d; dyn_kind = d ? 1 : 0; return *this; }
    GemmCall& depth(const int* d) { dyn = d; dyn_kind = d ? 2 : 0; return *this; }
    GemmCall& with(const Pair* p) { pair = p; return *this; }
    GemmCall& atomic() { allow_atomic = true; return *this; }
    GemmCall& batch_rows() { rows_are_batch = true; return *this; }
    GemmCall& form(int thin_, int split_k_ = 1) { thin = thin_; split_k = split_k_; return *this; }
    GemmCall& a16(const unsigned short* p) { A16 = p; return *this; }
    GemmCall& b16(const unsigned short* p) { B16 = p; return *this; }
    GemmCall& keep(unsigned short* p) { keep_a16 = p; return *this; }
};
// C (M x N) = A B^T: A (M, K) and B (N, K), both k-contiguous
inline GemmCall nt(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K) { return GemmCall{A, lda, false, B, ldb, false, C, ldc, M, N, K}; }
// C (M x N) = A B: A (M, K), B (K, N)
inline GemmCall nn(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K) { return GemmCall{A, lda, false, B, ldb, true, C, ldc, M, N, K}; }
// dW (M x N) += A^T B over K rows: A (K, M), B (K, N); the gradients are zero-filled beforehand
inline GemmCall tn_grad(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K)
{
    GemmCall c{A, lda, true, B, ldb, true, C, ldc, M, N, K};
    c.wgrad = true;
    return c;
}

// ---- model.cpp: the step's workspace, GEMM calls and forward pieces that other files run too
bool use_table(const avae_ctx* h, int rows, int B);
void layout(avae_ctx* h, Bump& b, Ws& w, int B, int Ss, int St, bool train);
int reserve_ws(avae_ctx* h, size_t need);
// reserve_ws for a call that sizes its workspace once: a refusal names the call and the byte count
inline int reserve_named(avae_ctx* h, size_t need, const char* what)
{
    if (reserve_ws(h, need)) {
        (void)hipGetLastError();                                   // (the refused allocation is reported here, not by a later launch check)
        char b[256]; snprintf(b, sizeof b, "%s: the device cannot give the workspace of %zu bytes this call needs", what, need);
        h->err = b;
        return 1;
    }
    return 0;
}
int get_ws(avae_ctx* h, Ws& w, int B, int Ss, int St, bool train);
int gemm(avae_ctx* h, const GemmCall& c);
int gemm_bf16_pre(avae_ctx* h, const GemmCall& c);
int gemm_tn16(avae_ctx* h, const GemmCall& c);
// batch groups per job and rows per group (a multiple of 16) of a GRU launch over B rows: at most 512 workgroups, at most 16 groups
void gru_geometry(int D, int njobs, int B, int* G, int* rpg);
void gru_common(avae_ctx* h, const Ws& w, GruArgs& a, int njobs, int S, int B, int ldg, int ldh, const int32_t* lens, int Bx);
int build_row_orders(avae_ctx* h, Ws& w, int B, int Ss, int T, bool with_dec, bool with_enc = true);
int build_compact_dec(avae_ctx* h, Ws& w, int B, int T);
int run_decoder_rnn(avae_ctx* h, Ws& w, int B, int T, const float* state_in, int64_t state_stride, bool save, const int32_t* ids0 = nullptr, bool compact = false,
                    const int32_t* share_rows = nullptr, int share_n = 0);
int run_logits_ce(avae_ctx* h, Ws& w, int rt, bool train, float inv_n);
int encode_ws(avae_ctx* h, Ws& w, const int32_t* src, int b, int t);
// the pointer half of prep_ids' arguments: the id arrays of a workspace (the caller sets the ids, the geometry and the dropout fields)
inline PrepArgs prep_from_ws(const Ws& w)
{
    PrepArgs p{};
    p.src_tm = w.src_tm; p.lens_src = w.lens_src; p.lens_tgt = w.lens_tgt; p.lead = w.lead; p.gold = w.gold;
    p.rank = w.rank; p.cidx = w.cidx; p.ntok = w.ntok; p.chunk_counts = w.ntok + 4;
    return p;
}

// the kinds of GRU launch a step makes (avae_ctx::Route::gru): the encoder's two-direction launches, the top encoder layer's one-job
// launches (top_one_step), the decoder's
enum RouteGru { kRouteEncFwd, kRouteEncBwd, kRouteTopFwd, kRouteTopBwd, kRouteDecFwd, kRouteDecBwd };
// notes the plan of the launch the step is about to make: gru_plan on the very arguments gru_forward / gru_backward get
inline void note_gru(avae_ctx* h, int kind, const GruArgs& a, bool fwd)
{
    if (!h->route.live) return;
    const GruPlan p = gru_plan(a, fwd, h->persistent != 0);
    const int v[5] = {(int)p.form, p.T, p.C, p.pipe ? 1 : 0, p.ring};
    std::copy(v, v + 5, h->route.gru[kind]);
}

// ---- handle.cpp
int grow_scratch(avae_ctx* h, size_t need, const char* what);
int check_gru_err(avae_ctx* h);
int dyn_fraction(avae_ctx* h, const avae_ctx::Stamp& s, std::vector<std::pair<const int*, int>>& seen, double* f);
inline int check_bound(avae_ctx* h)
{
    if (!h->P || !h->G || !h->M || !h->Vv) return fail(h, "state buffers not bound (avae_bind_state)");
    return 0;
}
// One user's buffers in h->scratch: `lay` takes them from a Bump, once without a base for the size and, the buffer grown to it, once for
// the pointers -- the size and the pointers cannot disagree.  Never inside a token loop: growing synchronises and reallocates.
template <class F> int place_scratch(avae_ctx* h, const char* what, F lay)
{
    Bump probe{nullptr};
    lay(probe);
    AV_TRY(grow_scratch(h, probe.off, what));
    Bump real{reinterpret_cast<char*>(h->scratch)};
    lay(real);
    return 0;
}
// The same for a call's buffers in the workspace h->ws, sized once per call: nothing is allocated between the launches.  A refusal
// names the call and the byte count (reserve_named).  `from`: the buffers start behind that many bytes, which the caller lays out itself.
template <class F> int place_ws(avae_ctx* h, const char* what, F lay, size_t from = 0)
{
    Bump probe{nullptr, from};
    lay(probe);
    AV_TRY(reserve_named(h, probe.off + 4096, what));
    Bump real{h->ws, from};
    lay(real);
    return 0;
}

// ---- generate.cpp: which loop a decoding call runs (0 one launch, 1 per token by option or batch, 2 per token: geometry refused)
int decode_route(bool persistent, int b, bool sampled, int top_k, bool nucleus, int D, int V, int L, int G, int lds_max, DecodePlan* plan);
// ---- generate.cpp: avae_sample_config / avae_sample_p_config -> what the kernels take
bool sample_params(avae_ctx* h, const avae_sample_config* sc, int V, SampleParams* sp);
bool sample_params_p(avae_ctx* h, const avae_sample_p_config* sc, int V, SampleParams* sp, float* top_p);

}}  // namespace avae::host
#pragma GCC visibility pop
