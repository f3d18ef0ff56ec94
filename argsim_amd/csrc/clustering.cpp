// clustering.cpp -- clustering of latent rows: the plan, the workspace and the launch sequences of avae_ward and avae_ward_cut
// (kernels: ward.hip), of avae_affinity (kernels: affinity.hip), of avae_tsne (kernels: tsne.hip, the distances affinity.hip's) and of
// avae_kmeans (kernels: kmeans.hip), of avae_gmm_fit and avae_gmm_score (kernels: gmm.hip), of avae_silhouette (kernels: silhouette.hip)
// of avae_dbscan (kernels: dbscan.hip), and of avae_pca_fit and avae_pca_transform (kernels: pca.hip).
// Contract: include/argsim_vae.h.
#include "ctx.h"

using namespace avae;
using namespace avae::host;

namespace {

// Workspace of a call, every buffer on a 256-byte boundary: G descriptors, then per group of n rows
//   4 n^2 bytes     the square of stored pair values (its upper triangle is used)
//   8 n dim bytes   the double sums of member rows
//   12 n + 16 bytes counts, nearest-neighbour cache words, the last merge
void ward_layout(Bump& b, std::vector<WardGroup>& gs, WardGroup** dev, const int32_t* off, int G, int dim)
{
    *dev = b.take<WardGroup>((size_t)G);
    for (int g = 0; g < G; ++g) {
        WardGroup& w = gs[g];
        const size_t n = (size_t)(off[g + 1] - off[g]);
        w.off = off[g]; w.n = (int)n; w.mrg = off[g] - g; w.pad = 0;
        w.D = b.take<float>(n * n);
        w.S = b.take<double>(n * dim);
        w.nn = b.take<unsigned long long>(n);
        w.cnt = b.take<int>(n);
        w.st = b.take<int>(4);
    }
}

// group_off as the header states it; *nmax <- the largest group
int check_groups(avae_ctx* h, const char* what, const int32_t* off, int G, int* nmax)
{
    const std::string w(what);
    if (G < 1 || G > (1 << 16)) return fail(h, w + ": G must be in [1, 2^16]");
    if (off[0] != 0) return fail(h, w + ": group_off[0] must be 0");
    *nmax = 0;
    for (int g = 0; g < G; ++g) {
        if (off[g + 1] <= off[g]) return fail(h, w + ": group_off must ascend, with at least one row per group");
        if (off[g + 1] - off[g] > (1 << 15)) return fail(h, w + ": at most 2^15 rows per group");
        *nmax = std::max(*nmax, off[g + 1] - off[g]);
    }
    return 0;
}

}  // namespace

extern "C" {

int avae_ward(avae_handle h, const float* x, int32_t dim, const int32_t* group_off, int32_t G, const avae_ward_config* wc,
              int32_t* pair, float* delta, int32_t* size)
{
    if (!h) return 1;
    if (!wc) return fail(h, "ward config is null");
    if (!x || !group_off || !pair || !delta) return fail(h, "ward: x, group_off, pair and delta must be given");
    int nmax = 0;
    AV_TRY(check_groups(h, "ward", group_off, G, &nmax));
    AV_TRY(check_rows(h, "ward", dim, "x", {x}));
    if (wc->reserved[0] != 0 || wc->reserved[1] != 0) return fail(h, "ward: the reserved fields must be 0");
    if (nmax < 2) return 0;                                     // every group a single row: no merge, nothing written
    AV_CHECK(hipSetDevice(h->device));
    std::vector<WardGroup> gs((size_t)G);
    WardGroup* dev = nullptr;
    AV_TRY(place_ws(h, "ward", [&](Bump& b) { ward_layout(b, gs, &dev, group_off, G, dim); }));
    AV_TRY(stage_h2d(h, dev, gs.data(), gs.size() * sizeof(WardGroup)));                // (gs dies at return, nothing below synchronises)
    AV_CHECK(ward_init(h->stream, dev, G, nmax, x, dim));
    const int form = h->ward_form ? h->ward_form : (nmax <= kWardOneWgMax ? 1 : 2);
    if (form == 1) {
        AV_CHECK(ward_tree(h->stream, dev, G, nmax, dim, pair, delta, size));
    } else {
        // the same two launches for every merge; a group with fewer merges returns at once.  Never a synchronisation: what a round
        // merges is decided on the device
        for (int t = 0; t < nmax - 1; ++t) AV_CHECK(ward_round(h->stream, dev, G, nmax, dim, t, pair, delta, size));
    }
    return 0;
}

int avae_ward_cut(avae_handle h, const int32_t* pair, const int32_t* group_off, int32_t G, const int32_t* k, int32_t* label)
{
    if (!h) return 1;
    if (!pair || !group_off || !k || !label) return fail(h, "ward cut: pair, group_off, k and label must be given");
    int nmax = 0;
    AV_TRY(check_groups(h, "ward cut", group_off, G, &nmax));
    std::vector<WardCutGroup> gs((size_t)G);
    for (int g = 0; g < G; ++g) {
        const int n = group_off[g + 1] - group_off[g];
        if (k[g] < 1 || k[g] > n) return fail(h, "ward cut: k[g] must be in [1, n_g]");
        gs[g] = WardCutGroup{group_off[g], n, group_off[g] - g, n - k[g]};
    }
    AV_CHECK(hipSetDevice(h->device));
    WardCutGroup* dev = nullptr; int32_t* parent = nullptr;
    AV_TRY(place_ws(h, "ward cut", [&](Bump& b) { dev = b.take<WardCutGroup>((size_t)G); parent = b.take<int32_t>((size_t)group_off[G]); }));
    AV_TRY(stage_h2d(h, dev, gs.data(), gs.size() * sizeof(WardCutGroup)));             // (gs dies at return, nothing below synchronises)
    AV_CHECK(ward_cut(h->stream, dev, G, nmax, pair, parent, label));
    return 0;
}

int avae_affinity(avae_handle h, const float* x, int32_t N, int32_t dim, const avae_affinity_config* ac, int32_t* label, int32_t* stat,
                  float* s_out, float* a, float* r)
{
    if (!h) return 1;
    if (!ac) return fail(h, "affinity config is null");
    if (!x || !label || !stat) return fail(h, "affinity: x, label and stat must be given");
    if (N < 1 || N > kApMaxN) return fail(h, "affinity: N must be in [1, 2^14]");
    if (ac->metric < 0 || ac->metric > 2) return fail(h, "affinity: metric must be 0 (euclidean), 1 (cosine) or 2 (precomputed)");
    if (ac->metric == 2) {
        if (dim != N) return fail(h, "affinity: a precomputed similarity is (N, N): dim must equal N");
    } else AV_TRY(check_rows(h, "affinity", dim, "x", {x}));
    if (ac->max_iter < 1 || ac->max_iter > 10000) return fail(h, "affinity: max_iter must be in [1, 10000]");
    if (ac->convergence_iter < 1 || ac->convergence_iter > ac->max_iter) return fail(h, "affinity: convergence_iter must be in [1, max_iter]");
    if (!(ac->damping >= 0.5f && ac->damping < 1.f)) return fail(h, "affinity: damping must be in [0.5, 1)");
    if ((a == nullptr) != (r == nullptr)) return fail(h, "affinity: a and r are given together or not at all");
    if (ac->warm && !a) return fail(h, "affinity: a warm start reads a and r, which are not given");
    if (ac->reserved[0] != 0 || ac->reserved[1] != 0) return fail(h, "affinity: the reserved fields must be 0");
    AV_CHECK(hipSetDevice(h->device));
    if (N == 1) { AV_CHECK(ap_single(h->stream, label, stat)); return 0; }
    // Workspace, every buffer on a 256-byte boundary: S, A and R of 4 N^2 bytes each where the caller does not give
    // the buffer itself, the column partials (row blocks x N doubles), five vectors of N and the state
    const size_t n = (size_t)N, nblk = (n + ap_row_block(N) - 1) / ap_row_block(N);
    ApBuffers b{};
    AV_TRY(place_ws(h, "affinity", [&](Bump& bp) {
        b.st = bp.take<ApState>(1);
        b.S = s_out ? s_out : bp.take<float>(n * n);
        b.A = a ? a : bp.take<float>(n * n);
        b.R = r ? r : bp.take<float>(n * n);
        b.part = bp.take<double>(nblk * n);
        b.cv = bp.take<double>(n);
        b.best = bp.take<unsigned long long>(n);
        b.E = bp.take<int>(n); b.run = bp.take<int>(n); b.E2 = bp.take<int>(n);
        b.c = bp.take<int32_t>(n);
    }));
    AV_CHECK(hipMemsetAsync(b.st, 0, sizeof(ApState), h->stream));
    AV_CHECK(hipMemsetAsync(b.E, 0, n * sizeof(int), h->stream));
    if (!ac->warm) {
        AV_CHECK(hipMemsetAsync(b.A, 0, n * n * sizeof(float), h->stream));
        AV_CHECK(hipMemsetAsync(b.R, 0, n * n * sizeof(float), h->stream));
    }
    if (ac->metric == 2) {
        if (b.S != x) AV_CHECK(hipMemcpyAsync(b.S, x, n * n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    } else {
        AV_CHECK(ap_similarity(h->stream, x, N, dim, ac->metric, b.S));
    }
    AV_CHECK(ap_prepare(h->stream, b.S, N, ac->use_preference, ac->preference, ac->noise, ac->seed, b.st));
    // every round is enqueued; a launch that finds the stop decided returns at once.  Never a synchronisation
    for (int it = 0; it < ac->max_iter; ++it) AV_CHECK(ap_iteration(h->stream, b, N, ac->damping, it, ac->convergence_iter));
    AV_CHECK(ap_labels(h->stream, b, N, label, stat));
    return 0;
}

int avae_tsne(avae_handle h, const float* x, int32_t N, int32_t dim, const avae_tsne_config* tc, const double* p_in, float* y, double* kl,
              int32_t* stat, double* p_out, double* beta_out, double* trace, float* grad, float* ug, double* prog)
{
    if (!h) return 1;
    if (!tc) return fail(h, "tsne config is null");
    if (!y || !kl || !stat) return fail(h, "tsne: y, kl and stat must be given");
    if (!x && !p_in) return fail(h, "tsne: x or p_in must be given");
    if (N < 2 || N > kTsneMaxN) return fail(h, "tsne: N must be in [2, 2^14]");
    if (!p_in) {
        AV_TRY(check_rows(h, "tsne", dim, "x", {x}));
        if (!(tc->perplexity > 0.0 && tc->perplexity < (double)N)) return fail(h, "tsne: perplexity must be in (0, N)");
    }
    if (((uintptr_t)y | (uintptr_t)ug) & 7) return fail(h, "tsne: y and ug must be 8-byte aligned");
    if (tc->max_iter < 0 || tc->max_iter > 32768) return fail(h, "tsne: max_iter must be in [0, 32768]");
    if (tc->it0 < 0 || tc->it0 > tc->max_iter) return fail(h, "tsne: it0 must be in [0, max_iter]");
    if (tc->exaggeration_iter < 0) return fail(h, "tsne: exaggeration_iter must be >= 0");
    if (tc->n_iter_check < 1) return fail(h, "tsne: n_iter_check must be >= 1");
    if (tc->n_iter_without_progress < 0) return fail(h, "tsne: n_iter_without_progress must be >= 0");
    if (!(tc->early_exaggeration >= 1.0)) return fail(h, "tsne: early_exaggeration must be >= 1");
    if (tc->learning_rate != tc->learning_rate) return fail(h, "tsne: learning_rate is NaN");
    if (tc->init < 0 || tc->init > 1) return fail(h, "tsne: init must be 0 (y holds the start) or 1 (random)");
    if ((ug == nullptr) != (prog == nullptr)) return fail(h, "tsne: ug and prog are given together or not at all");
    if (tc->warm && !ug) return fail(h, "tsne: a warm continuation reads ug and prog, which are not given");
    if (tc->reserved[0] != 0 || tc->reserved[1] != 0) return fail(h, "tsne: the reserved fields must be 0");
    AV_CHECK(hipSetDevice(h->device));
    // Workspace, every buffer on a 256-byte boundary: P of 8 N^2 bytes unless the caller gives p_in or p_out, with x the
    // distances of 4 N^2 bytes, beta and the row sums, the partials of the walks (48 N parts bytes), update and gains unless ug is
    // given, and the state
    const size_t n = (size_t)N;
    const TsnePlan plan = tsne_plan(N, h->tsne_chunk);
    if (plan.chunk > kTsneMaxChunk || plan.parts < 1) return fail(h, "tsne: no plan for this N");
    TsneArgs a{};
    double *P = nullptr, *beta = nullptr, *rowsum = nullptr; float* D = nullptr;
    AV_TRY(place_ws(h, "tsne", [&](Bump& b) {
        a.st = b.take<TsneState>(1);
        P = p_out ? p_out : (p_in ? nullptr : b.take<double>(n * n));
        if (!p_in) { D = b.take<float>(n * n); rowsum = b.take<double>(n); beta = beta_out ? beta_out : b.take<double>(n); }
        a.part = b.take<double>(n * plan.parts * 5);
        a.errp = b.take<double>(n * plan.parts);
        a.upd = ug ? ug : b.take<float>(2 * n);
        a.gains = ug ? ug + 2 * n : b.take<float>(2 * n);
    }));
    if (p_in) {
        if (P && P != p_in) AV_CHECK(hipMemcpyAsync(P, p_in, n * n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        a.P = P ? P : p_in;
    } else {
        AV_CHECK(ap_similarity(h->stream, x, N, dim, 0, D));
        AV_CHECK(tsne_conditionals(h->stream, D, N, tc->perplexity, P, beta));
        AV_CHECK(tsne_joint(h->stream, P, N, rowsum));
        a.P = P;
    }
    a.y = y; a.grad = grad; a.trace = trace;
    a.N = N; a.rs = plan.rs; a.parts = plan.parts; a.chunk = plan.chunk;
    a.max_iter = tc->max_iter; a.exag_iter = tc->exaggeration_iter; a.X = std::min(tc->exaggeration_iter, tc->max_iter);
    a.nic = tc->n_iter_check; a.nwp = tc->n_iter_without_progress;
    a.lr = tc->learning_rate > 0.f ? tc->learning_rate : (float)std::max((double)N / tc->early_exaggeration / 4.0, 50.0);
    a.ee = tc->early_exaggeration; a.min_gn = tc->min_grad_norm;
    AV_CHECK(tsne_init(h->stream, a, tc->it0, tc->warm, tc->init, tc->seed, prog));
    // every iteration is enqueued; a launch that finds the stop decided returns at once.  Never a synchronisation
    for (int it = tc->it0; it < tc->max_iter; ++it) AV_CHECK(tsne_iteration(h->stream, a, it));
    AV_CHECK(tsne_finish(h->stream, a, kl, stat, prog));
    return 0;
}

int avae_kmeans(avae_handle h, const float* x, int32_t N, int32_t dim, const avae_kmeans_config* kc, const float* centers_in, int32_t* label,
                float* centers, int32_t* stat, double* inertia, int32_t* label_all, double* centers_all, int32_t* stat_all)
{
    if (!h) return 1;
    if (!kc) return fail(h, "kmeans config is null");
    if (!x || !label || !centers || !stat || !inertia) return fail(h, "kmeans: x, label, centers, stat and inertia must be given");
    if (N < 1 || N > kKmMaxN) return fail(h, "kmeans: N must be in [1, 2^22]");
    AV_TRY(check_rows(h, "kmeans", dim, "x and centers_in", {x, centers_in}));
    if (kc->k < 1 || kc->k > std::min(N, kKmMaxK)) return fail(h, "kmeans: k must be in [1, min(N, 4096)]");
    if (kc->n_init < 1 || kc->n_init > kKmMaxInit) return fail(h, "kmeans: n_init must be in [1, 64]");
    if (kc->max_iter < 1 || kc->max_iter > 10000) return fail(h, "kmeans: max_iter must be in [1, 10000]");
    if (kc->metric < 0 || kc->metric > 1) return fail(h, "kmeans: metric must be 0 (euclidean) or 1 (cosine)");
    if (kc->init < 0 || kc->init > 1) return fail(h, "kmeans: init must be 0 (k-means++) or 1 (centers_in)");
    if (kc->init == 1 && !centers_in) return fail(h, "kmeans: init 1 reads centers_in, which is not given");
    if (!(kc->tol >= 0.0)) return fail(h, "kmeans: tol must be >= 0");
    if (kc->reserved != 0) return fail(h, "kmeans: the reserved field must be 0");
    AV_CHECK(hipSetDevice(h->device));
    // Workspace, every buffer on a 256-byte boundary, R = n_init: the state (R), the centres (R, k, dim) double, the parts'
    // minima (R, parts, N) double + int, labels and sorted rows (R, N) int each, distances (R, N) double, histograms and offsets
    // (R, blocks, k) int each, first positions (R, k + 1), member-sum partials (R, slices + k, dim) double, relocations (R, k, 3),
    // shift (R, k) and inertia (R, tiles) partials, the variance's (256 + 1, dim), with the cosine the row norms (N); with init 0 the
    // closest distances (R, N), candidate distances (R, T, N), candidate rows (R, T, dim) and (R, T), scan-tile sums (R, scans) and
    // potential partials (R, T, scans)
    const size_t n = (size_t)N, R = (size_t)kc->n_init, k = (size_t)kc->k, d = (size_t)dim;
    KmArgs a{};
    a.x = x; a.N = N; a.dim = dim; a.k = kc->k; a.R = kc->n_init; a.max_iter = kc->max_iter; a.seed = kc->seed;
    a.T = std::min(kKmMaxTrials, 2 + (int)std::floor(std::log((double)kc->k)));
    a.p = km_plan(N, kc->k, kc->n_init, h->kmeans_chunk);
    const KmPlan& p = a.p;
    double* rnorm = nullptr;
    AV_TRY(place_ws(h, "kmeans", [&](Bump& b) {
        a.st = b.take<KmState>(R);
        a.best = b.take<int>(1);
        a.C = b.take<double>(R * k * d);
        a.pd = b.take<double>(R * p.parts * n); a.pi = b.take<int>(R * p.parts * n);
        a.lab = b.take<int>(R * n); a.order = b.take<int>(R * n); a.dist = b.take<double>(R * n);
        a.hist = b.take<int>(R * p.blks * k); a.off = b.take<int>(R * p.blks * k);
        a.start = b.take<int>(R * (k + 1));
        a.psum = b.take<double>(R * ((size_t)p.slices + k) * d);
        a.rel = b.take<int>(R * k * 3);
        a.shiftp = b.take<double>(R * k); a.ipart = b.take<double>(R * p.tiles);
        a.vpart = b.take<double>((size_t)kKmMaxBlocks * d); a.mean = b.take<double>(d);
        rnorm = b.opt<double>(kc->metric == 1, n);
        if (kc->init == 0) {
            a.closest = b.take<double>(R * n); a.D = b.take<double>(R * a.T * n); a.candC = b.take<double>(R * a.T * d);
            a.cand = b.take<int>(R * a.T); a.tsum = b.take<double>(R * p.scans); a.ppart = b.take<double>(R * a.T * p.scans);
        }
    }));
    a.rnorm = rnorm;
    AV_CHECK(hipMemsetAsync(a.st, 0, R * sizeof(KmState), h->stream));
    AV_CHECK(hipMemsetAsync(a.lab, 0xff, R * n * sizeof(int), h->stream));
    AV_CHECK(hipMemsetAsync(a.hist, 0, R * p.blks * k * sizeof(int), h->stream));
    AV_CHECK(km_prepare(h->stream, a, kc->tol));
    if (kc->init == 1) AV_CHECK(km_load(h->stream, a, centers_in));
    else AV_CHECK(km_seed(h->stream, a));
    // every iteration is enqueued; a launch that finds the restart's stop decided returns at once.  Never a synchronisation
    for (int it = 0; it < kc->max_iter; ++it) AV_CHECK(km_iteration(h->stream, a, it));
    AV_CHECK(km_finish(h->stream, a, label, centers, stat, inertia, label_all, centers_all, stat_all));
    return 0;
}

// the buffers of a mixture call, every one on a 256-byte boundary, R restarts: the state (R), weights, n_c, half log determinants,
// t_ic constants and bad flags (R, k) each, means, variances and precisions (R, k, dim) each, the parts' (max, sum, first maximum, its
// component) (R, parts, N) 28 bytes a row, lse (R, N), the bound's partials (R, ceil(N / 256)), the M-step's partials (R, slices, k, 2 dim + 1)
static void gmm_layout(Bump& b, GmArgs& a)
{
    const size_t n = (size_t)a.N, R = (size_t)a.R, k = (size_t)a.k, d = (size_t)a.dim;
    a.st = b.take<GmState>(R); a.best = b.take<int>(1);
    a.W = b.take<double>(R * k); a.NC = b.take<double>(R * k); a.HLD = b.take<double>(R * k); a.LC = b.take<double>(R * k); a.bad = b.take<int>(R * k);
    a.MU = b.take<double>(R * k * d); a.COV = b.take<double>(R * k * d); a.PREC = b.take<double>(R * k * d);
    a.pm = b.take<double>(R * a.p.parts * n); a.ps = b.take<double>(R * a.p.parts * n); a.pt = b.take<double>(R * a.p.parts * n);
    a.pi = b.take<int>(R * a.p.parts * n);
    a.lse = b.take<double>(R * n); a.bpart = b.take<double>(R * a.p.blks);
    a.mpart = b.take<double>(R * a.p.slices * k * (2 * d + 1));
}

int avae_gmm_fit(avae_handle h, const float* x, int32_t N, int32_t dim, const avae_gmm_config* gc, const int32_t* label_in, const double* w_in,
                 const double* mu_in, const double* cov_in, double* weights, double* means, double* covars, int32_t* label, int32_t* stat,
                 double* lower, double* logp, double* resp, double* weights_all, double* means_all, double* covars_all, int32_t* stat_all,
                 double* trace)
{
    if (!h) return 1;
    if (!gc) return fail(h, "gmm config is null");
    if (!x || !weights || !means || !covars || !label || !stat || !lower)
        return fail(h, "gmm: x, weights, means, covars, label, stat and lower must be given");
    if (N < 2 || N > kGmMaxN) return fail(h, "gmm: N must be in [2, 2^22]");
    AV_TRY(check_rows(h, "gmm", dim, "x", {x}));
    if (gc->k < 1 || gc->k > std::min(N, kGmMaxK)) return fail(h, "gmm: k must be in [1, min(N, 1024)]");
    if (gc->n_init < 1 || gc->n_init > kGmMaxInit) return fail(h, "gmm: n_init must be in [1, 16]");
    if (gc->max_iter < 0 || gc->max_iter > 10000) return fail(h, "gmm: max_iter must be in [0, 10000]");
    if (gc->covariance < 0 || gc->covariance > 1) return fail(h, "gmm: covariance must be 0 (diag) or 1 (spherical)");
    if (gc->init < 0 || gc->init > 1) return fail(h, "gmm: init must be 0 (label_in) or 1 (w_in, mu_in, cov_in)");
    if (gc->init == 0 && !label_in) return fail(h, "gmm: init 0 reads label_in, which is not given");
    if (gc->init == 1 && (!w_in || !mu_in || !cov_in)) return fail(h, "gmm: init 1 reads w_in, mu_in and cov_in, which are not all given");
    if ((weights_all != nullptr) != (means_all != nullptr) || (weights_all != nullptr) != (covars_all != nullptr))
        return fail(h, "gmm: weights_all, means_all and covars_all are given together or not at all");
    if (!(gc->tol >= 0.0)) return fail(h, "gmm: tol must be >= 0");
    if (!(gc->reg_covar >= 0.0)) return fail(h, "gmm: reg_covar must be >= 0");
    if (gc->reserved != 0) return fail(h, "gmm: the reserved field must be 0");
    AV_CHECK(hipSetDevice(h->device));
    GmArgs a{};
    a.x = x; a.N = N; a.dim = dim; a.k = gc->k; a.R = gc->n_init; a.max_iter = gc->max_iter; a.spherical = gc->covariance;
    a.tol = gc->tol; a.reg = gc->reg_covar; a.trace = trace; a.dreal = dim - h->gmm_pad;
    a.p = gm_plan(N, gc->k, gc->n_init, h->gmm_chunk);
    AV_TRY(place_ws(h, "gmm", [&](Bump& b) { gmm_layout(b, a); }));
    AV_CHECK(hipMemsetAsync(a.st, 0, (size_t)a.R * sizeof(GmState), h->stream));
    if (gc->init == 1) AV_CHECK(gm_load(h->stream, a, w_in, mu_in, cov_in, 1));
    else AV_CHECK(gm_start_labels(h->stream, a, label_in));
    // every iteration is enqueued; a launch that finds the restart's stop decided returns at once.  Never a synchronisation
    for (int it = 0; it < gc->max_iter; ++it) AV_CHECK(gm_iteration(h->stream, a, it));
    AV_CHECK(gm_pick(h->stream, a, stat, lower, stat_all));
    AV_CHECK(gm_final(h->stream, a, logp, label, resp));
    AV_CHECK(gm_copy(h->stream, a, weights, means, covars, weights_all, means_all, covars_all));
    return 0;
}

int avae_gmm_score(avae_handle h, const float* x, int32_t n, int32_t dim, int32_t k, const double* weights, const double* means,
                   const double* covars, double* logp, int32_t* label, double* resp)
{
    if (!h) return 1;
    if (!x || !weights || !means || !covars || !logp) return fail(h, "gmm score: x, weights, means, covars and logp must be given");
    if (n < 1 || n > kGmMaxN) return fail(h, "gmm score: n must be in [1, 2^22]");
    AV_TRY(check_rows(h, "gmm score", dim, "x", {x}));
    if (k < 1 || k > kGmMaxK) return fail(h, "gmm score: k must be in [1, 1024]");
    AV_CHECK(hipSetDevice(h->device));
    GmArgs a{};
    a.x = x; a.N = n; a.dim = dim; a.k = k; a.R = 1; a.dreal = dim - h->gmm_pad;
    a.p = gm_plan(n, k, 1, h->gmm_chunk);
    AV_TRY(place_ws(h, "gmm score", [&](Bump& b) { gmm_layout(b, a); }));
    AV_CHECK(hipMemsetAsync(a.st, 0, sizeof(GmState), h->stream));
    AV_CHECK(hipMemsetAsync(a.best, 0, sizeof(int), h->stream));
    AV_CHECK(gm_load(h->stream, a, weights, means, covars, 0));
    AV_CHECK(gm_final(h->stream, a, logp, label, resp));
    return 0;
}

int avae_silhouette(avae_handle h, const float* x, int32_t N, int32_t dim, const avae_silhouette_config* sc, const int32_t* label, const int32_t* K,
                    double* score, double* sil, double* ab, int32_t* nearest, int32_t* count, double* cluster_mean, double* index)
{
    if (!h) return 1;
    if (!sc) return fail(h, "silhouette config is null");
    if (!x) return fail(h, "silhouette: x is null");
    if (!label) return fail(h, "silhouette: label is null");
    if (!K) return fail(h, "silhouette: K is null");
    if (!score) return fail(h, "silhouette: score is null");
    if (N < 2 || N > kSilMaxN) return fail(h, "silhouette: N must be in [2, 2^18]");
    if (dim < 4 || dim > 1024 || (dim & 3)) return fail(h, "silhouette: dim must be a multiple of 4 in [4, 1024]");
    if (sc->L < 1 || sc->L > kSilMaxL) return fail(h, "silhouette: L must be in [1, 64]");
    for (int l = 0; l < sc->L; ++l)
        if (K[l] < 1 || K[l] > kSilMaxK) return fail(h, "silhouette: K[" + std::to_string(l) + "] must be in [1, 4096]");
    if (sc->metric < 0 || sc->metric > 2) return fail(h, "silhouette: metric must be 0 (euclidean), 1 (cosine) or 2 (squared euclidean)");
    if ((uintptr_t)x & 15) return fail(h, "silhouette: x must be 16-byte aligned");
    if (sc->reserved != 0 || sc->reserved2 != 0) return fail(h, "silhouette: the reserved fields must be 0");
    AV_CHECK(hipSetDevice(h->device));
    int cus = 0, lds = 0;
    AV_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
    AV_CHECK(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, h->device));
    if (lds < kSilLds) return fail(h, "silhouette: the device gives a workgroup less than the 160 KiB of LDS the pair pass is planned for");
    // Workspace, every buffer on a 256-byte boundary: K and its prefix sums (2 L + 1) int, the member counts (sum K) int, with
    // the cosine the row norms (N), the silhouette values (L, N) unless the caller gives sil; with index the member sums (sum K, dim), the
    // labelled rows' mean (L, dim), a row's squared distance to its cluster's mean and the root (L, N) each, S_c and the largest R (sum K)
    // each, (L, 4) traces and counts
    const size_t n = (size_t)N, L = (size_t)sc->L, d = (size_t)dim;
    std::vector<int> meta(2 * L + 1);
    int kmax = 0;
    meta[L] = 0;
    for (size_t l = 0; l < L; ++l) { meta[l] = K[l]; meta[L + l + 1] = meta[L + l] + K[l]; kmax = std::max(kmax, (int)K[l]); }
    const size_t sumk = (size_t)meta[2 * L];
    SilArgs a{};
    a.x = x; a.label = label; a.N = N; a.dim = dim; a.L = sc->L; a.metric = sc->metric; a.Kmax = kmax; a.ab = ab; a.nearest = nearest;
    int* dmeta = nullptr; double* rnorm = nullptr;
    AV_TRY(place_ws(h, "silhouette", [&](Bump& b) {
        dmeta = b.take<int>(2 * L + 1);
        a.cnt = b.take<int>(sumk);
        rnorm = b.opt<double>(sc->metric == 1, n);
        a.s = sil ? sil : b.take<double>(L * n);
        if (index) {
            a.msum = b.take<double>(sumk * d); a.gmean = b.take<double>(L * d);
            a.e = b.take<double>(L * n); a.r = b.take<double>(L * n);
            a.Sc = b.take<double>(sumk); a.dbp = b.take<double>(sumk); a.tr = b.take<double>(4 * L);
        }
    }));
    a.meta = dmeta; a.rnorm = rnorm;
    const SilPlan plan = sil_plan(N, dim, sc->L, K, h->sil_chunk, cus);
    AV_TRY(stage_h2d(h, dmeta, meta.data(), meta.size() * sizeof(int)));                // (meta dies at return, nothing below synchronises)
    AV_CHECK(hipMemsetAsync(a.cnt, 0, sumk * sizeof(int), h->stream));
    AV_CHECK(sil_prepare(h->stream, a));
    AV_CHECK(sil_pairs(h->stream, a, plan));
    AV_CHECK(sil_scores(h->stream, a, score, count, cluster_mean));
    if (index) AV_CHECK(sil_indices(h->stream, a, index));
    return 0;
}

int avae_dbscan(avae_handle h, const float* x, int32_t N, int32_t dim, const avae_dbscan_config* dc, int32_t* label, int32_t* count, int32_t* stat)
{
    if (!h) return 1;
    if (!dc) return fail(h, "dbscan config is null");
    if (!x) return fail(h, "dbscan: x is null");
    if (!label) return fail(h, "dbscan: label is null");
    if (!stat) return fail(h, "dbscan: stat is null");
    if (N < 1 || N > kDbMaxN) return fail(h, "dbscan: N must be in [1, 2^17]");
    if (dim < 4 || dim > 1024 || (dim & 3)) return fail(h, "dbscan: dim must be a multiple of 4 in [4, 1024]");
    if (dc->metric < 0 || dc->metric > 1) return fail(h, "dbscan: metric must be 0 (euclidean) or 1 (cosine)");
    if (dc->min_samples < 1) return fail(h, "dbscan: min_samples must be >= 1");
    if (dc->max_rounds < 0 || dc->max_rounds > kDbMaxRounds) return fail(h, "dbscan: max_rounds must be in [0, 4096]");
    if (!(dc->eps > 0.0) || !std::isfinite(dc->eps)) return fail(h, "dbscan: eps must be > 0 and finite");
    if ((uintptr_t)x & 15) return fail(h, "dbscan: x must be 16-byte aligned");
    if (dc->reserved != 0) return fail(h, "dbscan: the reserved field must be 0");
    AV_CHECK(hipSetDevice(h->device));
    int cus = 0;
    AV_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
    const DbPlan plan = db_plan(N, dim, h->dbscan_chunk, cus);
    const int rounds = dc->max_rounds > 0 ? dc->max_rounds : plan.rounds;
    // Workspace, every buffer on a 256-byte boundary: the state, the rounds' flags (rounds + 1) int, the bit matrix
    // (N, W) of 8-byte words, W = ceil(N / 64), the core mask (W), three parent arrays and the roots' numbers (N) int each, the counts
    // (N) int unless the caller gives count, with the cosine the row norms (N)
    const size_t n = (size_t)N, W = (size_t)plan.W;
    DbArgs a{};
    a.x = x; a.N = N; a.dim = dim; a.W = plan.W; a.min_samples = dc->min_samples; a.label = label;
    a.thr = dc->metric == 1 ? 2.0 * dc->eps : dc->eps * dc->eps;
    double* rnorm = nullptr;
    AV_TRY(place_ws(h, "dbscan", [&](Bump& b) {
        a.st = b.take<DbState>(1);
        a.flag = b.take<int>((size_t)rounds + 1);
        a.adj = b.take<unsigned long long>(n * W);
        a.cmask = b.take<unsigned long long>(W);
        for (int q = 0; q < 3; ++q) a.par[q] = b.take<int>(n);
        a.num = b.take<int>(n);
        a.count = count ? count : b.take<int32_t>(n);
        rnorm = b.opt<double>(dc->metric == 1, n);
    }));
    a.rnorm = rnorm;
    AV_CHECK(hipMemsetAsync(a.st, 0, sizeof(DbState), h->stream));
    AV_CHECK(hipMemsetAsync(a.flag, 0, ((size_t)rounds + 1) * sizeof(int), h->stream));
    AV_CHECK(hipMemsetAsync(a.count, 0, n * sizeof(int32_t), h->stream));
    AV_CHECK(db_prepare(h->stream, a));
    AV_CHECK(db_pairs(h->stream, a, plan));
    AV_CHECK(db_core(h->stream, a));
    // every round is enqueued; a launch that finds the fixed point reached returns at once.  Never a synchronisation
    for (int t = 0; t < rounds; ++t) AV_CHECK(db_round(h->stream, a, t));
    AV_CHECK(db_finish(h->stream, a, stat));
    return 0;
}

int avae_pca_fit(avae_handle h, const float* x, int32_t N, int32_t dim, const avae_pca_config* pc, double* mean, double* var, double* comp,
                 int32_t* stat)
{
    if (!h) return 1;
    if (!pc) return fail(h, "pca config is null");
    if (!x) return fail(h, "pca: x is null");
    if (!mean) return fail(h, "pca: mean is null");
    if (!var) return fail(h, "pca: var is null");
    if (!comp) return fail(h, "pca: comp is null");
    if (!stat) return fail(h, "pca: stat is null");
    if (N < 2 || N > kPcaMaxN) return fail(h, "pca: N must be in [2, 2^22]");
    if (dim < 4 || dim > 1024 || (dim & 3)) return fail(h, "pca: dim must be a multiple of 4 in [4, 1024]");
    if (pc->pad < 0 || pc->pad > 3 || pc->pad >= dim) return fail(h, "pca: pad must be in [0, 3] and below dim");
    if (pc->max_sweeps < 0 || pc->max_sweeps > kPcaMaxSweeps) return fail(h, "pca: max_sweeps must be in [0, 256]");
    if ((uintptr_t)x & 15) return fail(h, "pca: x must be 16-byte aligned");
    if (pc->reserved != 0 || pc->reserved2 != 0) return fail(h, "pca: the reserved fields must be 0");
    if (h->pca_form == 1 && dim - pc->pad > kPcaResident) return fail(h, "pca: pca_form 1 (the resident solve) needs dim - pad <= 128");
    AV_CHECK(hipSetDevice(h->device));
    int cus = 0;
    AV_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
    const PcaPlan plan = pca_plan(N, dim, pc->pad, h->pca_chunk, h->pca_form, cus);
    const int sweeps = pc->max_sweeps > 0 ? pc->max_sweeps : plan.sweeps;
    // Workspace, every buffer on a 256-byte boundary: the state, the chunks' column sums (chunks, dim), their partial
    // tiles (chunks, pairs, 64, 64), the matrix and the rotations (dreal, dreal) each -- twice each for the launched solve
    PcaArgs a{};
    a.x = x; a.N = N; a.dim = dim; a.dreal = plan.dreal; a.mean = mean;
    const size_t nn = (size_t)plan.dreal * plan.dreal;
    AV_TRY(place_ws(h, "pca", [&](Bump& b) {
        a.st = b.take<PcaState>(1);
        a.msum = b.take<double>((size_t)plan.chunks * dim);
        a.part = b.take<double>((size_t)plan.chunks * plan.pairs * kPcaT * kPcaT);
        a.A[0] = b.take<double>(nn); a.A[1] = b.take<double>(nn);      // [1]: the launched solve's other buffer, the resident one's staging
        a.Vt[0] = b.take<double>(nn); a.Vt[1] = b.opt<double>(plan.form == 2, nn);
    }));
    AV_CHECK(hipMemsetAsync(a.st, 0, sizeof(PcaState), h->stream));
    AV_CHECK(pca_cov(h->stream, a, plan));
    AV_CHECK(pca_solve(h->stream, a, plan, sweeps));
    AV_CHECK(pca_finish(h->stream, a, plan, var, comp, stat));
    return 0;
}

int avae_pca_transform(avae_handle h, const float* x, int32_t n, int32_t dim, const double* mean, const double* comp, const double* scale,
                       int32_t k, float* y)
{
    if (!h) return 1;
    if (!x) return fail(h, "pca transform: x is null");
    if (!mean) return fail(h, "pca transform: mean is null");
    if (!comp) return fail(h, "pca transform: comp is null");
    if (!y) return fail(h, "pca transform: y is null");
    if (n < 1 || n > kPcaMaxN) return fail(h, "pca transform: n must be in [1, 2^22]");
    if (dim < 4 || dim > 1024 || (dim & 3)) return fail(h, "pca transform: dim must be a multiple of 4 in [4, 1024]");
    if (k < 1 || k > dim) return fail(h, "pca transform: k must be in [1, dim]");
    if ((uintptr_t)x & 15) return fail(h, "pca transform: x must be 16-byte aligned");
    AV_CHECK(hipSetDevice(h->device));
    const PcaPlan plan = pca_plan(n, dim, 0, h->pca_chunk, 2, 1);
    AV_CHECK(pca_transform(h->stream, x, n, dim, mean, comp, scale, k, y, plan.trows));
    return 0;
}

}  // extern "C"
