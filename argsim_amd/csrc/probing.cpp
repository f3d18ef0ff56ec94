// probing.cpp -- linear probes of latent rows: the lockstep Newton loop that avae_probe_fit (truncated Newton) and avae_probe_fit_l1
// (proximal Newton) share, and avae_probe_decision (contract: include/argsim_vae.h; kernels: probe.hip).
#include "ctx.h"

using namespace avae;
using namespace avae::host;

namespace {

// Workspace of a fit, every buffer on a 256-byte boundary:
//   4 N Ppad floats            costs, decisions, curvature, step panel
//   5 Ppad LD floats           iterate, gradient, CG direction, CG residual, Newton step   (LD = dim + 4, Ppad = P rounded up to 32)
//   parts (LD + 1) Ppad floats the parts' partials of a pass and their loss sums
//   7 parts Ppad doubles       the parts' trial loss sums
//   Ppad (8 ints + 8 floats + 8 doubles) of per-problem state
void probe_layout(Bump& b, ProbeWs& w, const ProbePlan& p, int N, int dim)
{
    const size_t panel = (size_t)N * p.Ppad, vec = (size_t)p.Ppad * p.LD;
    w.sT = b.take<float>(panel); w.z = b.take<float>(panel); w.D = b.take<float>(panel); w.u = b.take<float>(panel);
    w.W = b.take<float>(5 * vec);
    if (w.W) { w.G = w.W + vec; w.Dv = w.G + vec; w.Rv = w.Dv + vec; w.Pv = w.Rv + vec; }
    w.gp = b.take<float>((size_t)p.parts * vec); w.lp = b.take<float>((size_t)p.parts * p.Ppad);
    w.tp = b.take<double>((size_t)p.parts * kProbeAlphas * p.Ppad);
    w.is = b.take<int>((size_t)p.Ppad * 8); w.fs = b.take<float>((size_t)p.Ppad * 8); w.ds = b.take<double>((size_t)p.Ppad * 8);
    w.N = N; w.dim = dim; w.LD = p.LD; w.Ppad = p.Ppad; w.parts = p.parts; w.chunk = p.chunk;
}

// Workspace of an L1 fit: that of the L2 fit, then
//   3 Ppad LD floats           the FISTA point y, H d of the accepted d, H y
//   N dim floats               x with the rows that are not finite zeroed
void probe_l1_layout(Bump& b, ProbeWs& w, const ProbePlan& p, int N, int dim)
{
    probe_layout(b, w, p, N, dim);
    const size_t vec = (size_t)p.Ppad * p.LD;
    w.Yv = b.take<float>(3 * vec);
    if (w.Yv) { w.Hd = w.Yv + vec; w.Hy = w.Hd + vec; }
    w.xs = b.take<float>((size_t)N * dim);
}

// the trial rounds of the Armijo search: step length 0 (the loss at w from the same panels) and 1, 1/2, .. 2^-20
void probe_rounds(ProbeAlphas (&r)[4])
{
    int e = 0;
    for (int i = 0; i < 4; ++i) {
        r[i] = ProbeAlphas{};
        r[i].n = i == 0 ? 2 : i == 3 ? 6 : kProbeAlphas;          // 0, 1 | 1/2 .. 2^-7 | 2^-8 .. 2^-14 | 2^-15 .. 2^-20: the full step is nearly always taken
        r[i].last = i == 3;
        for (int j = 0; j < r[i].n; ++j) {
            if (i == 0 && j == 0) { r[i].a[j] = 0.f; continue; }
            r[i].a[j] = std::ldexp(1.f, -e); ++e;
        }
    }
}

// what the three entries ask of their shape: n rows of x (n, dim) against P problems w (P, dim + 1)
int check_probe_shape(avae_ctx* h, const char* what, int n, int P, int dim, const float* x, const float* w)
{
    const std::string p(what);
    if (n < 1 || P < 1) return fail(h, p + ": N and P must be >= 1");
    if (P > (1 << 20)) return fail(h, p + ": at most 2^20 problems per call");
    if (n > 0x7fffffff - 255) return fail(h, p + ": at most 2^31 - 256 rows per call");
    return check_rows(h, what, dim, "x and w", {x, w});
}

// One fit as the two entries state it: l1 -- the proximal Newton method; inner -- max_cg or max_inner.
struct ProbeFit { const char* what; bool l1; int max_newton, inner; float tol; int reserved; };

// Per Newton iteration GRAD + vec, the synchronisation, max `inner` x (HV + vec), PANEL, 4 x (trial + vec).  The L1 fit has the
// workspace of the L2 fit, 3 more vectors per problem and the copy xs of x (probe_l1_layout) which its passes read in place of x,
// its own per-problem kernel, and the curvature sums + vec behind the synchronisation.
int probe_fit(avae_ctx* h, const ProbeFit& f, const float* x, int N, int dim, const float* s, int P, float* w, float* stats)
{
    const std::string name(f.what);
    if (!x || !s || !w) return fail(h, name + ": x, s and w must be given");
    AV_TRY(check_probe_shape(h, f.what, N, P, dim, x, w));
    if (f.max_newton < 1 || f.inner < 1) return fail(h, name + (f.l1 ? ": max_newton and max_inner must be >= 1" : ": max_newton and max_cg must be >= 1"));
    if (!(f.tol >= 0.f)) return fail(h, name + ": tol must be >= 0 (and not NaN)");
    if (f.reserved != 0) return fail(h, name + ": the reserved field must be 0");
    AV_CHECK(hipSetDevice(h->device));
    const ProbePlan p = probe_plan(N, P, dim, h->probe_chunk);
    if ((long long)p.parts * p.ptiles > 0x7fffffffLL) return fail(h, name + ": too many (row part, problem tile) workgroups for one launch");
    ProbeWs b{};
    AV_TRY(place_ws(h, f.what, [&](Bump& bp) { f.l1 ? probe_l1_layout(bp, b, p, N, dim) : probe_layout(bp, b, p, N, dim); }));
    ProbeAlphas rounds[4];
    probe_rounds(rounds);
    const ProbeAlphas none{};
    auto vec = [&](int phase, int k, const ProbeAlphas& al) {
        return f.l1 ? probe_l1_vec(h->stream, b, P, phase, k, f.max_newton, f.inner, f.tol, al) : probe_vec(h->stream, b, P, phase, k, f.max_newton, f.inner, f.tol, al);
    };
    std::vector<int> state((size_t)p.Ppad * 8);
    if (f.l1) { AV_CHECK(probe_l1_prepare(h->stream, b, x, s, P)); x = b.xs; }
    else AV_CHECK(probe_prepare(h->stream, b, s, P));
    for (int it = 0; it <= f.max_newton; ++it) {
        AV_CHECK(probe_pass(h->stream, b, x, 0));
        AV_CHECK(vec(0, it, none));
        // the one synchronisation of a Newton iteration: is any problem still running?  (What every problem does next is decided on
        // the device; an answer read later would stop the loop later and change nothing.)
        AV_CHECK(hipMemcpyAsync(state.data(), b.is, state.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        AV_CHECK(hipStreamSynchronize(h->stream));
        bool alive = false;
        for (int q = 0; q < P; ++q) alive = alive || state[(size_t)q * 8 + 2] == 0;
        if (!alive) break;
        if (f.l1) {
            AV_CHECK(probe_l1_curv(h->stream, b));
            AV_CHECK(vec(3, it, none));
        }
        for (int k = 0; k < f.inner; ++k) {
            AV_CHECK(probe_pass(h->stream, b, x, 1));
            AV_CHECK(vec(1, k, none));
        }
        AV_CHECK(probe_pass(h->stream, b, x, 2));
        for (int r = 0; r < 4; ++r) {
            AV_CHECK(probe_trial(h->stream, b, rounds[r]));
            AV_CHECK(vec(2, r, rounds[r]));
        }
    }
    AV_CHECK(probe_finish(h->stream, b, P, w, stats));
    return 0;
}

}  // namespace

extern "C" {

int avae_probe_fit(avae_handle h, const float* x, int32_t N, int32_t dim, const float* s, int32_t P, const avae_probe_config* pc, float* w, float* stats)
{
    if (!h) return 1;
    if (!pc) return fail(h, "probe config is null");
    return probe_fit(h, ProbeFit{"probe", false, pc->max_newton, pc->max_cg, pc->tol, pc->reserved}, x, N, dim, s, P, w, stats);
}

int avae_probe_fit_l1(avae_handle h, const float* x, int32_t N, int32_t dim, const float* s, int32_t P, const avae_probe_l1_config* pc, float* w, float* stats)
{
    if (!h) return 1;
    if (!pc) return fail(h, "probe l1 config is null");
    return probe_fit(h, ProbeFit{"probe l1", true, pc->max_newton, pc->max_inner, pc->tol, pc->reserved}, x, N, dim, s, P, w, stats);
}

int avae_probe_decision(avae_handle h, const float* x, int32_t n, int32_t dim, const float* w, int32_t P, float* out)
{
    if (!h) return 1;
    if (!x || !w || !out) return fail(h, "probe decision: x, w and out must be given");
    AV_TRY(check_probe_shape(h, "probe decision", n, P, dim, x, w));
    AV_CHECK(hipSetDevice(h->device));
    const ProbePlan p = probe_plan(n, P, dim, h->probe_chunk);
    if ((long long)p.parts * p.ptiles > 0x7fffffffLL ) return fail(h, "probe decision: too many (row part, problem tile) workgroups for one launch");
    float* W = nullptr;
    AV_TRY(place_ws(h, "probe decision", [&](Bump& b) { W = b.take<float>((size_t)p.Ppad * p.LD); }));
    AV_CHECK(probe_decision(h->stream, p, x, n, dim, w, P, W, out));
    return 0;
}

}  // extern "C"
