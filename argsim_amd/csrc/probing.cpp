// probing.cpp -- linear probes of latent rows: the lockstep truncated-Newton loop of avae_probe_fit, the lockstep proximal-Newton loop
// of avae_probe_fit_l1, and avae_probe_decision (contract: include/argsim_vae.h; kernels: probe.hip).
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

}  // namespace

extern "C" {

int avae_probe_fit(avae_handle h, const float* x, int32_t N, int32_t dim, const float* s, int32_t P, const avae_probe_config* pc, float* w, float* stats)
{
    if (!h) return 1;
    if (!pc) return fail(h, "probe config is null");
    if (!x || !s || !w) return fail(h, "probe: x, s and w must be given");
    if (N < 1 || P < 1) return fail(h, "probe: N and P must be >= 1");
    if (P > (1 << 20)) return fail(h, "probe: at most 2^20 problems per call");
    if (N > 0x7fffffff - 255) return fail(h, "probe: at most 2^31 - 256 rows per call");
    if (pc->max_newton < 1 || pc->max_cg < 1) return fail(h, "probe: max_newton and max_cg must be >= 1");
    if (!(pc->tol >= 0.f)) return fail(h, "probe: tol must be >= 0 (and not NaN)");
    if (pc->reserved != 0) return fail(h, "probe: the reserved field must be 0");
    if (dim < 4 || dim > 1024 || (dim & 3)) return fail(h, "probe: dim must be a multiple of 4 in [4, 1024]");
    if (((uintptr_t)x | (uintptr_t)w) & 15) return fail(h, "probe: x and w must be 16-byte aligned");
    AV_CHECK(hipSetDevice(h->device));
    const ProbePlan p = probe_plan(N, P, dim, h->probe_chunk);
    if ((long long)p.parts * p.ptiles > 0x7fffffffLL ) return fail(h, "probe: too many (row part, problem tile) workgroups for one launch");
    ProbeWs b{};
    Bump probe{nullptr};
    probe_layout(probe, b, p, N, dim);
    AV_TRY(reserve_named(h, probe.off + 4096, "probe"));        // sized once per call; nothing is allocated between the launches
    Bump real{h->ws};
    probe_layout(real, b, p, N, dim);
    ProbeAlphas rounds[4];
    probe_rounds(rounds);
    const ProbeAlphas none{};
    std::vector<int> state((size_t)p.Ppad * 8);
    AV_CHECK(probe_prepare(h->stream, b, s, P));
    for (int it = 0; it <= pc->max_newton; ++it) {
        AV_CHECK(probe_pass(h->stream, b, x, 0));
        AV_CHECK(probe_vec(h->stream, b, P, 0, it, pc->max_newton, pc->max_cg, pc->tol, none));
        // the one synchronisation of a Newton iteration: is any problem still running?  (What every problem does next is decided on
        // the device; an answer read later would stop the loop later and change nothing.)
        AV_CHECK(hipMemcpyAsync(state.data(), b.is, state.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        AV_CHECK(hipStreamSynchronize(h->stream));
        bool alive = false;
        for (int q = 0; q < P; ++q) alive = alive || state[(size_t)q * 8 + 2] == 0;
        if (!alive) break;
        for (int k = 0; k < pc->max_cg; ++k) {
            AV_CHECK(probe_pass(h->stream, b, x, 1));
            AV_CHECK(probe_vec(h->stream, b, P, 1, k, pc->max_newton, pc->max_cg, pc->tol, none));
        }
        AV_CHECK(probe_pass(h->stream, b, x, 2));
        for (int r = 0; r < 4; ++r) {
            AV_CHECK(probe_trial(h->stream, b, rounds[r]));
            AV_CHECK(probe_vec(h->stream, b, P, 2, r, pc->max_newton, pc->max_cg, pc->tol, rounds[r]));
        }
    }
    AV_CHECK(probe_finish(h->stream, b, P, w, stats));
    return 0;
}

// The L1 fit: the workspace of the L2 fit, 3 more vectors per problem and the copy of x (probe_l1_layout), and per proximal Newton
// iteration GRAD + vec, the synchronisation, the curvature sums + vec, max_inner x (HV + vec), PANEL, 4 x (trial + vec).
int avae_probe_fit_l1(avae_handle h, const float* x, int32_t N, int32_t dim, const float* s, int32_t P, const avae_probe_l1_config* pc, float* w, float* stats)
{
    if (!h) return 1;
    if (!pc) return fail(h, "probe l1 config is null");
    if (!x || !s || !w) return fail(h, "probe l1: x, s and w must be given");
    if (N < 1 || P < 1) return fail(h, "probe l1: N and P must be >= 1");
    if (P > (1 << 20)) return fail(h, "probe l1: at most 2^20 problems per call");
    if (N > 0x7fffffff - 255) return fail(h, "probe l1: at most 2^31 - 256 rows per call");
    if (pc->max_newton < 1 || pc->max_inner < 1) return fail(h, "probe l1: max_newton and max_inner must be >= 1");
    if (!(pc->tol >= 0.f)) return fail(h, "probe l1: tol must be >= 0 (and not NaN)");
    if (pc->reserved != 0) return fail(h, "probe l1: the reserved field must be 0");
    if (dim < 4 || dim > 1024 || (dim & 3)) return fail(h, "probe l1: dim must be a multiple of 4 in [4, 1024]");
    if (((uintptr_t)x | (uintptr_t)w) & 15) return fail(h, "probe l1: x and w must be 16-byte aligned");
    AV_CHECK(hipSetDevice(h->device));
    const ProbePlan p = probe_plan(N, P, dim, h->probe_chunk);
    if ((long long)p.parts * p.ptiles > 0x7fffffffLL ) return fail(h, "probe l1: too many (row part, problem tile) workgroups for one launch");
    ProbeWs b{};
    Bump probe{nullptr};
    probe_l1_layout(probe, b, p, N, dim);
    AV_TRY(reserve_named(h, probe.off + 4096, "probe l1"));     // sized once per call; nothing is allocated between the launches
    Bump real{h->ws};
    probe_l1_layout(real, b, p, N, dim);
    ProbeAlphas rounds[4];
    probe_rounds(rounds);
    const ProbeAlphas none{};
    std::vector<int> state((size_t)p.Ppad * 8);
    AV_CHECK(probe_l1_prepare(h->stream, b, x, s, P));
    for (int it = 0; it <= pc->max_newton; ++it) {
        AV_CHECK(probe_pass(h->stream, b, b.xs, 0));
        AV_CHECK(probe_l1_vec(h->stream, b, P, 0, it, pc->max_newton, pc->max_inner, pc->tol, none));
        // the one synchronisation of an iteration, as in avae_probe_fit
        AV_CHECK(hipMemcpyAsync(state.data(), b.is, state.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        AV_CHECK(hipStreamSynchronize(h->stream));
        bool alive = false;
        for (int q = 0; q < P; ++q) alive = alive || state[(size_t)q * 8 + 2] == 0;
        if (!alive) break;
        AV_CHECK(probe_l1_curv(h->stream, b));
        AV_CHECK(probe_l1_vec(h->stream, b, P, 3, it, pc->max_newton, pc->max_inner, pc->tol, none));
        for (int k = 0; k < pc->max_inner; ++k) {
            AV_CHECK(probe_pass(h->stream, b, b.xs, 1));
            AV_CHECK(probe_l1_vec(h->stream, b, P, 1, k, pc->max_newton, pc->max_inner, pc->tol, none));
        }
        AV_CHECK(probe_pass(h->stream, b, b.xs, 2));
        for (int r = 0; r < 4; ++r) {
            AV_CHECK(probe_trial(h->stream, b, rounds[r]));
            AV_CHECK(probe_l1_vec(h->stream, b, P, 2, r, pc->max_newton, pc->max_inner, pc->tol, rounds[r]));
        }
    }
    AV_CHECK(probe_finish(h->stream, b, P, w, stats));
    return 0;
}

int avae_probe_decision(avae_handle h, const float* x, int32_t n, int32_t dim, const float* w, int32_t P, float* out)
{
    if (!h) return 1;
    if (!x || !w || !out) return fail(h, "probe decision: x, w and out must be given");
    if (n < 1 || P < 1) return fail(h, "probe decision: n and P must be >= 1");
    if (P > (1 << 20)) return fail(h, "probe decision: at most 2^20 problems per call");
    if (n > 0x7fffffff - 255) return fail(h, "probe decision: at most 2^31 - 256 rows per call");
    if (dim < 4 || dim > 1024 || (dim & 3)) return fail(h, "probe decision: dim must be a multiple of 4 in [4, 1024]");
    if (((uintptr_t)x | (uintptr_t)w) & 15) return fail(h, "probe decision: x and w must be 16-byte aligned");
    AV_CHECK(hipSetDevice(h->device));
    const ProbePlan p = probe_plan(n, P, dim, h->probe_chunk);
    if ((long long)p.parts * p.ptiles > 0x7fffffffLL ) return fail(h, "probe decision: too many (row part, problem tile) workgroups for one launch");
    AV_TRY(reserve_named(h, (size_t)p.Ppad * p.LD * sizeof(float) + 4096, "probe decision"));
    AV_CHECK(probe_decision(h->stream, p, x, n, dim, w, P, reinterpret_cast<float*>(h->ws), out));
    return 0;
}

}  // extern "C"
