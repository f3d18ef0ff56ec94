// probe.hip -- linear probes of latent rows: P independent L2-regularised logistic regressions over one matrix X (N, dim), solved
// in lockstep by a truncated Newton method (contract: include/argsim_vae.h, avae_probe_fit / avae_probe_decision).
//
//   probe_pass   grid = (row parts) x (problem tiles of 32).  A workgroup walks its part in tiles of 128 rows.  Per tile:
//                  A  the 128 x 32 panel tile X V^T with the NT K-tile step of mfma_tile.h (k-contiguous operands, 32-deep K tiles through
//                     LDS, v_mfma_f32_32x32x2_f32, the next K tile's loads in flight), one 32 x 32 MFMA tile per wave; the bias
//                     column of x~ = (x, 1) is never materialised: the bias component of the vector is added in the epilogue;
//                  E  the epilogue in registers: GRAD stores the decision z and the curvature D = |s| sigma(m) sigma(-m) and forms
//                     the residual -|s| sgn(s) sigma(-m) and the loss; HV forms D o u; both leave their 128 x 32 tile in LDS;
//                  B  X_tile^T (dim x 128) times that tile, wave w owning dims [w dim4, (w + 1) dim4): the row pair (2 i, 2 i + 1) is
//                     one MFMA step.  The 128 x dim row tile does not fit in LDS at dim 1024 (512 KB), so B RE-READS the tile's rows
//                     from memory straight into the MFMA operand registers (for one row 32 lanes read consecutive floats): X comes
//                     from HBM once per pass, the second read is served by L2 / the Infinity Cache while the tile is hot.  This is
//                     done at every dim, not only where the tile would not fit.
//                The (dim + 1) x 32 partial of the part goes to the workspace; the bias row is the column sum of the tile in E.
//                PANEL mode is A + the bias alone: the panel X~ V^T (the Newton step's u, and avae_probe_decision).
//   probe_vec    one workgroup per problem: merges the parts' partials in part order, does the CG and Newton vector updates (dot
//                products over dim + 1 in double, a fixed tree), the Armijo bookkeeping and the freeze flags.
//   probe_trial  elementwise over the kept panels z = X~ w and u = X~ p: the loss sums at up to 7 step lengths, in double (the
//                Armijo test compares losses that differ in the 9th digit near the optimum), per part; X is not read.
// A problem is one column of every MFMA tile and one column of every panel: its arithmetic does not see the other columns, and the
// row parts are a function of (N, probe_chunk) alone, so its bits do not depend on P, on its position or on its companions.  A
// launch whose 32 problems are all idle returns at once; an idle problem in a busy tile is computed and ignored.  No float atomics.
// The L1 fit (avae_probe_fit_l1: proximal Newton, the inner problem by FISTA) runs the same passes and trial kernel with its own
// per-problem kernel probe_l1_vec, the curvature column sums probe_l1_curv and the row check probe_l1_rows, at the end of this file's kernels.
#include "kernels.h"
#include "mfma_tile.h"
#include "row_parts.h"

#include <algorithm>
#include <type_traits>

namespace avae {

namespace {

constexpr int kTR = 128;           // rows per tile
constexpr int kTP = kProbeTile;    // problems per tile
constexpr int kNA = kProbeAlphas;  // step lengths per probe_trial launch

// per-problem state words (ProbeWs::is, ::fs, ::ds)
enum { I_ITER = 0, I_STATUS = 1, I_FROZEN = 2, I_CG = 3, I_LS = 4, I_ALIVE = 5 };
enum { F_F = 0, F_GNORM = 1, F_G0 = 2 };
enum { D_RR = 0, D_GTP = 1, D_WTP = 2, D_PP = 3, D_PHI0 = 4 };

struct ProbePassArgs {
    const float* x;          // (N, dim)
    const float* v;          // (Ppad, LD): the vector of every problem, its bias component at [dim]
    const float* sT;         // (N, Ppad) signed costs
    float* z; float* D;      // (N, Ppad) panels: GRAD writes both, HV reads D
    float* out; int ldo, pout;      // PANEL: out[row * ldo + p] for p < pout
    float* gp;               // (parts, LD, Ppad) partials of X~^T (tile)
    float* lp;               // (parts, Ppad) loss partials (GRAD)
    const int* flags; int flag;     // per-problem state words; the launch returns where no problem of the tile has is[flag] != 0
    int N, dim, LD, Ppad, parts, chunk;
};

// MODE 0 GRAD, 1 HV, 2 PANEL.  DT: 32-dim MFMA tiles per wave in step B (4 x 32 x DT >= dim).
template <int MODE, int DT>
__global__ __launch_bounds__(256) void probe_pass_kernel(ProbePassArgs a)
{
    constexpr int VW = DT >= 4 ? 4 : DT;          // floats a lane loads per row in step B
    __shared__ __attribute__((aligned(16))) float s_tile[(kTR + kTP) * kTileLDK];
    __shared__ float s_R[kTR * kTP];
    __shared__ float s_red[2][8][kTP];
    float* As = s_tile;
    float* Bs = s_tile + kTR * kTileLDK;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l31 = lane & 31;
    const int part = blockIdx.x % a.parts, pt = blockIdx.x / a.parts;
    const int p0 = pt * kTP, prob = p0 + l31;
    const int dim = a.dim, Ppad = a.Ppad;
    if (a.flags) {
        const int busy = tid < kTP ? a.flags[(size_t)(p0 + tid) * 8 + a.flag] : 0;
        if (!__syncthreads_or(busy)) return;
    }
    long long c_begin; int c_end;
    part_range(part, a.chunk, a.N, c_begin, c_end);
    const float vb = a.v[(size_t)prob * a.LD + dim];

    f32x16 g[MODE == 2 ? 1 : DT];
    if (MODE != 2) {
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) g[t][r] = 0.f;
    }
    float bsum = 0.f, lsum = 0.f;

    for (int row0 = (int)c_begin; row0 < c_end; row0 += kTR) {
        // ---- A: acc = X[row0 + 32 wave ..][:] . V[p0 ..][:]^T
        f32x16 acc[1][1];
        zero_acc(acc);
        float4 ra[kTR / 32], rb[kTP / 32];
        load_tile<false, kTR>(ra, a.x, dim, row0, c_end, 0, dim, tid);
        load_tile<false, kTP>(rb, a.v, a.LD, p0, Ppad, 0, dim, tid);
        for (int k0 = 0; k0 < dim; k0 += kTileBK) {
            store_tile<false, kTR>(As, ra, tid);
            store_tile<false, kTP>(Bs, rb, tid);
            if (k0 + kTileBK < dim) {         // the next K tile's loads go out before the barrier that publishes this one
                load_tile<false, kTR>(ra, a.x, dim, row0, c_end, k0 + kTileBK, dim, tid);
                load_tile<false, kTP>(rb, a.v, a.LD, p0, Ppad, k0 + kTileBK, dim, tid);
            }
            __syncthreads();
            mfma_ktile<false, false, 1, 1, kTR, kTP>(acc, As, Bs, wave, 0, h, l31);      // (no s_setprio here: not measured in this kernel)
            __syncthreads();
        }

        // ---- E: the wave's 32 x 32 tile (C/D map: mfma32_row; col = problem)
        float pv[16];             // the tile's costs (GRAD) or curvature (HV): unconditional loads, all in flight at once
        if (MODE != 2) {
            const float* panel = MODE == 0 ? a.sT : a.D;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row0 + 32 * wave + mfma32_row(r, h);
                const float v = panel[(size_t)min(row, c_end - 1) * Ppad + prob];
                pv[r] = row < c_end ? v : 0.f;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = 32 * wave + mfma32_row(r, h), row = row0 + rl;
            const bool valid = row < c_end;
            const size_t at = (size_t)row * Ppad + prob;
            const float zz = acc[0][0][r] + vb;
            if (MODE == 2) {
                if (valid && prob < a.pout) a.out[(size_t)row * a.ldo + prob] = zz;
            } else {
                float R = 0.f;
                if (MODE == 0) {
                    const float s = pv[r];
                    float Dv = 0.f;
                    if (s != 0.f) {                       // (a NaN cost is != 0: it ends the problem through the sums)
                        const float c = fabsf(s), y = s > 0.f ? 1.f : -1.f;
                        const float m = y * zz;
                        const float e = expf(-fabsf(m));                  // in (0, 1]: nothing overflows whatever |m|
                        const float big = 1.f / (1.f + e), small = e / (1.f + e);
                        const float sig_neg = m >= 0.f ? small : big;    // sigma(-m)
                        lsum += c * (fmaxf(-m, 0.f) + log1pf(e));
                        Dv = c * big * small;
                        R = -c * y * sig_neg;
                    }
                    if (valid) { a.z[at] = zz; a.D[at] = Dv; }
                } else {
                    const float Dv = pv[r];
                    R = Dv != 0.f ? Dv * zz : 0.f;
                }
                s_R[rl * kTP + l31] = R;
                bsum += R;
            }
        }
        if (MODE == 2) continue;
        __syncthreads();

        // ---- B: g[d][p] += sum over the tile's rows of X[row][d] R[row][p]; one MFMA step takes rows 2 i (lanes 0..31) and 2 i + 1
        // (lanes 32..63); MFMA tile t = blk VW + e of this wave holds dims d0 + blk 32 VW + VW j + e, j = 0..31 (a lane loads VW
        // consecutive floats of its row)
        const int d0 = wave * 32 * DT;
        const int steps = min(kTR, c_end - row0 + 1) >> 1;
        constexpr int U = DT >= 8 ? 4 : 8;        // row pairs whose loads are in flight at once (every load is unconditional: a
                                                  // lane outside the matrix reads x[0] and drops it)
        for (int i0 = 0; i0 < steps; i0 += U) {
            float xv[U][DT], bval[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = 2 * (i0 + u) + h, row = row0 + k;      // (k <= 127: U divides 64)
                bval[u] = s_R[k * kTP + l31];
#pragma unroll
                for (int blk = 0; blk < DT / VW; ++blk) {
                    const int d = d0 + blk * 32 * VW + VW * l31;
                    const bool ok = row < c_end && d < dim;
                    const float* src = ok ? a.x + (size_t)row * dim + d : a.x;
                    float t[4] = {0.f, 0.f, 0.f, 0.f};
                    if (VW == 4) { const float4 v = *reinterpret_cast<const float4*>(src); t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w; }
                    else if (VW == 2) { const float2 v = *reinterpret_cast<const float2*>(src); t[0] = v.x; t[1] = v.y; }
                    else t[0] = *src;
#pragma unroll
                    for (int e = 0; e < VW; ++e) xv[u][blk * VW + e] = ok ? t[e] : 0.f;
                }
            }
            __builtin_amdgcn_sched_barrier(0);      // (keeps the scheduler from sinking every load to its first use)
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int t = 0; t < DT; ++t) g[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[u][t], bval[u], g[t], 0, 0, 0);
        }
        __syncthreads();          // (s_R is rewritten by the next tile's epilogue)
    }
    if (MODE == 2) return;

    // ---- the part's partial: rows d < dim from the accumulators, row dim (the bias) and the loss from the lanes' sums, added in
    // a fixed order (wave 0..3, half 0..1)
    float* gp = a.gp + (size_t)part * a.LD * Ppad;
    const int d0 = wave * 32 * DT;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        const int blk = t / VW, e = t % VW;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = mfma32_row(r, h);
            const int d = d0 + blk * 32 * VW + VW * j + e;
            if (d < dim) gp[(size_t)d * Ppad + prob] = g[t][r];
        }
    }
    s_red[0][wave * 2 + h][l31] = bsum;
    s_red[1][wave * 2 + h][l31] = lsum;
    __syncthreads();
    if (tid < kTP) {
        float b = 0.f, l = 0.f;
        for (int q = 0; q < 8; ++q) { b += s_red[0][q][tid]; l += s_red[1][q][tid]; }
        gp[(size_t)dim * Ppad + p0 + tid] = b;
        if (MODE == 0) a.lp[(size_t)part * Ppad + p0 + tid] = l;
    }
}

// sT (N, Ppad) <- s (P, N): a 32 x 32 tile through LDS; problems >= P get cost 0
__global__ __launch_bounds__(256) void probe_costs_kernel(const float* __restrict__ s, int P, int N, int Ppad, float* __restrict__ sT)
{
    __shared__ float t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long long r0 = (long long)blockIdx.x * 32; const int p0 = blockIdx.y * 32;
    for (int j = ty; j < 32; j += 8) {
        const int p = p0 + j; const long long row = r0 + tx;
        t[j][tx] = (p < P && row < N) ? s[(size_t)p * N + row] : 0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const long long row = r0 + j;
        if (row < N) sT[(size_t)row * Ppad + p0 + tx] = t[tx][j];
    }
}

// state of a fit: every vector 0, problems >= P frozen from the start
__global__ void probe_init_kernel(int* __restrict__ is, int P, int Ppad)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= Ppad) return;
    for (int i = 0; i < 8; ++i) is[(size_t)p * 8 + i] = 0;
    is[(size_t)p * 8 + I_FROZEN] = p < P ? 0 : 1;
    is[(size_t)p * 8 + I_ALIVE] = p < P ? 1 : 0;
}

// (P, dim + 1) -> (Ppad, LD), rows >= P and the padding columns zero
__global__ void probe_pack_kernel(const float* __restrict__ w, int P, int dim, int LD, int Ppad, float* __restrict__ W)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)Ppad * LD) return;
    const int p = (int)(i / LD), d = (int)(i % LD);
    W[i] = (p < P && d <= dim) ? w[(size_t)p * (dim + 1) + d] : 0.f;
}

__global__ void probe_finish_kernel(ProbeWs b, float* __restrict__ w, float* __restrict__ stats)
{
    const int p = blockIdx.x;
    for (int d = threadIdx.x; d <= b.dim; d += 256) w[(size_t)p * (b.dim + 1) + d] = b.W[(size_t)p * b.LD + d];
    if (stats && threadIdx.x == 0) {
        stats[4 * p + 0] = b.fs[(size_t)p * 8 + F_F];
        stats[4 * p + 1] = b.fs[(size_t)p * 8 + F_GNORM];
        stats[4 * p + 2] = (float)b.is[(size_t)p * 8 + I_ITER];
        stats[4 * p + 3] = (float)b.is[(size_t)p * 8 + I_STATUS];
    }
}

// ---------------------------------------------------------------- what the two per-problem kernels (probe_vec, probe_l1_vec) share
// NV values per thread reduced over the 256 threads by one fixed binary tree behind one set of barriers; every thread gets the results
struct OpAdd { __device__ double operator()(double a, double b) const { return a + b; } };
struct OpMax { __device__ double operator()(double a, double b) const { return fmax(a, b); } };
template <int NV, class Op>
__device__ __forceinline__ void block_reduce(double (&v)[NV], double (*s)[256])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < NV; ++i) s[i][tid] = v[i];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int i = 0; i < NV; ++i) s[i][tid] = Op()(s[i][tid], s[i][tid + o]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = s[i][0];
    __syncthreads();
}
__device__ __forceinline__ double block_sum(double v, double (*s)[256])
{
    double a[1] = {v};
    block_reduce<1, OpAdd>(a, s);
    return a[0];
}
// the largest of one float per thread (values >= 0; fmax on doubles: a NaN is dropped)
__device__ __forceinline__ float block_max(float v, double (*s)[256])
{
    double a[1] = {v};
    block_reduce<1, OpMax>(a, s);
    return (float)a[0];
}

__device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }

constexpr int kVecPer = 5;      // (1024 + 1 + 255) / 256 elements of a vector per thread

// partial of the last pass for element d of problem p, the parts added in part order; 16 parts' loads are in flight at once (the
// strided loads of one element are independent, only the additions form a chain)
__device__ __forceinline__ float merge_parts(const ProbeWs& b, int p, int d)
{
    const float* src = b.gp + (size_t)d * b.Ppad + p;
    const size_t step = (size_t)b.LD * b.Ppad;
    float s = 0.f;
    int q = 0;
    for (; q + 16 <= b.parts; q += 16) {
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = src[(size_t)(q + i) * step];
#pragma unroll
        for (int i = 0; i < 16; ++i) s += v[i];
    }
    if (q < b.parts) {
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = q + i < b.parts ? src[(size_t)(q + i) * step] : 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (q + i < b.parts) s += v[i];
    }
    return s;
}

// the state words and the vectors of problem p that both methods keep
struct ProbeState { int* is; float* fs; double* ds; float *W, *G, *Dv, *Pv; };
__device__ __forceinline__ ProbeState probe_state(const ProbeWs& b, int p)
{
    const size_t v = (size_t)p * b.LD;
    return ProbeState{b.is + (size_t)p * 8, b.fs + (size_t)p * 8, b.ds + (size_t)p * 8, b.W + v, b.G + v, b.Dv + v, b.Pv + v};
}

// the problem takes no further part in the fit (the caller clears I_CG / I_LS where one is set)
__device__ __forceinline__ void end_problem(int* is, int status) { is[I_STATUS] = status; is[I_FROZEN] = 1; is[I_ALIVE] = 0; }

// after a GRAD pass: -1 go on, else the status the problem ends with -- 2 f or the optimality measure is not finite, 0 the measure
// is within tol of its first value, 1 max_newton iterations are done
__device__ __forceinline__ int newton_stop(float f, float norm, float norm0, float tol, int it, int max_newton)
{
    if (!(f - f == 0.f) || !(norm - norm == 0.f)) return 2;
    if (norm <= tol * norm0) return 0;
    if (it >= max_newton) return 1;
    return -1;
}

// The Armijo scan of trial round k by one thread: slot j's loss sum is the parts' added in part order; slot 0 of round 0 is the step
// length 0 (kept in D_PHI0).  The first step length a with (loss - loss at 0) + reg(j, a, bad) <= rhs(a) is taken; reg is the change
// of the regulariser (it may set bad), rhs the decrease asked for.  take < 0: none of this round; bad: a sum is not finite.
struct ArmijoPick { float take; bool bad; };
template <class Reg, class Rhs>
__device__ __forceinline__ ArmijoPick armijo_scan(const ProbeWs& b, int p, int k, const ProbeAlphas& al, double* ds, Reg reg, Rhs rhs)
{
    float take = -1.f; bool bad = false;
#pragma unroll
    for (int j = 0; j < kNA; ++j) {
        if (j >= al.n || take >= 0.f || bad) break;
        double L = 0.0;
        for (int q = 0; q < b.parts; ++q) L += b.tp[((size_t)q * kNA + j) * b.Ppad + p];
        if (k == 0 && j == 0) { ds[D_PHI0] = L; if (!finite_d(L)) bad = true; continue; }
        const double a = al.a[j];
        bool rbad = false;
        const double r = reg(j, a, rbad);
        if (!finite_d(L) || rbad) { bad = true; break; }
        const double lhs = (L - ds[D_PHI0]) + r;
        if (lhs <= rhs(a)) take = al.a[j];
    }
    return ArmijoPick{take, bad};
}

// what both kernels do with the pick: the problem ends (status 2), moves on to its next Newton iteration, or waits for the next round
__device__ __forceinline__ float armijo_settle(int* is, const ArmijoPick& pk, int last)
{
    if (pk.bad || (pk.take < 0.f && last)) { end_problem(is, 2); is[I_LS] = 0; }
    else if (pk.take >= 0.f) { is[I_LS] = 0; is[I_ITER] += 1; }
    return pk.bad ? -1.f : pk.take;
}

// PHASE 0: after a GRAD pass -- f, g, the stop rule, else the start of CG.  PHASE 1: after the k-th HV pass -- one CG iteration.
// PHASE 2: after trial round k -- the Armijo test of its step lengths.
template <int PHASE>
__global__ __launch_bounds__(256) void probe_vec_kernel(ProbeWs b, int k, int max_newton, int max_cg, float tol, ProbeAlphas al)
{
    __shared__ double s_sum[1][256];
    __shared__ float s_alpha;
    const int p = blockIdx.x, tid = threadIdx.x, n = b.dim + 1;
    const auto [is, fs, ds, W, G, Dv, Pv] = probe_state(b, p);
    float* Rv = b.Rv + (size_t)p * b.LD;

    if (PHASE == 0) {
        if (is[I_FROZEN]) return;
        double ww = 0.0, gg = 0.0;
        for (int d = tid; d < n; d += 256) {
            const float w = W[d], gv = w + merge_parts(b, p, d);
            G[d] = gv;
            ww += (double)w * w; gg += (double)gv * gv;
        }
        ww = block_sum(ww, s_sum); gg = block_sum(gg, s_sum);
        float loss = 0.f;
        for (int q = 0; q < b.parts; ++q) loss += b.lp[(size_t)q * b.Ppad + p];
        const int it = is[I_ITER];
        const float f = (float)(0.5 * ww) + loss, gnorm = (float)sqrt(gg);
        const float g0 = it == 0 ? gnorm : fs[F_G0];
        const int status = newton_stop(f, gnorm, g0, tol, it, max_newton);
        if (status < 0)
            for (int d = tid; d < n; d += 256) { const float gv = G[d]; Pv[d] = 0.f; Rv[d] = -gv; Dv[d] = -gv; }
        if (tid == 0) {
            fs[F_F] = f; fs[F_GNORM] = gnorm; fs[F_G0] = g0;
            if (status >= 0) end_problem(is, status);
            else { ds[D_RR] = gg; is[I_CG] = 1; }
        }
    } else if (PHASE == 1) {
        if (!is[I_CG]) return;
        float hd[kVecPer];
        double dhd = 0.0;
#pragma unroll
        for (int j = 0; j < kVecPer; ++j) {
            const int d = tid + 256 * j;
            hd[j] = 0.f;
            if (d < n) { const float dv = Dv[d]; hd[j] = dv + merge_parts(b, p, d); dhd += (double)dv * hd[j]; }
        }
        dhd = block_sum(dhd, s_sum);
        const double rr = ds[D_RR];
        const bool ok = finite_d(dhd) && dhd > 0.0;
        const float alpha = ok ? (float)(rr / dhd) : 0.f;
        double rrn = 0.0;
#pragma unroll
        for (int j = 0; j < kVecPer; ++j) {
            const int d = tid + 256 * j;
            if (d < n && ok) {
                Pv[d] = fmaf(alpha, Dv[d], Pv[d]);
                const float r = fmaf(-alpha, hd[j], Rv[d]);
                Rv[d] = r; rrn += (double)r * r;
            }
        }
        rrn = block_sum(rrn, s_sum);
        const double gnorm = fs[F_GNORM];
        const bool stop = !ok || !finite_d(rrn) || sqrt(rrn) <= 0.1 * gnorm || k + 1 >= max_cg;
        if (!stop) {
            const float beta = (float)(rrn / rr);
#pragma unroll
            for (int j = 0; j < kVecPer; ++j) {
                const int d = tid + 256 * j;
                if (d < n) Dv[d] = fmaf(beta, Dv[d], Rv[d]);
            }
            if (tid == 0) ds[D_RR] = rrn;
            return;
        }
        // the step is Pv: what the Armijo test needs of it
        double gtp = 0.0, wtp = 0.0, pp = 0.0;
        for (int d = tid; d < n; d += 256) { const double pv = Pv[d]; gtp += (double)G[d] * pv; wtp += (double)W[d] * pv; pp += pv * pv; }
        gtp = block_sum(gtp, s_sum); wtp = block_sum(wtp, s_sum); pp = block_sum(pp, s_sum);
        if (tid == 0) {
            is[I_CG] = 0;
            if (!finite_d(dhd) || !finite_d(rrn) || !finite_d(gtp) || !finite_d(pp)) end_problem(is, 2);
            else { ds[D_GTP] = gtp; ds[D_WTP] = wtp; ds[D_PP] = pp; is[I_LS] = 1; }
        }
    } else {
        if (!is[I_LS]) return;
        if (tid == 0) {
            const ArmijoPick pk = armijo_scan(b, p, k, al, ds, [ds = ds](int, double a, bool&) { return a * ds[D_WTP] + 0.5 * a * a * ds[D_PP]; },
                                              [ds = ds](double a) { return 1e-4 * a * ds[D_GTP]; });
            s_alpha = armijo_settle(is, pk, al.last);
        }
        __syncthreads();
        const float a = s_alpha;
        if (a > 0.f)
            for (int d = tid; d < n; d += 256) W[d] = fmaf(a, Pv[d], W[d]);
    }
}

struct ProbeTrialArgs {
    const float* sT; const float* z; const float* u;      // (N, Ppad)
    double* tp;                                            // (parts, kNA, Ppad)
    const int* flags;
    int N, Ppad, parts, chunk;
    ProbeAlphas al;
};

// sum over the part's rows of |s| softplus(-sgn(s) (z + alpha u)) for every step length of the round, in double: thread (rg, pl)
// adds rows rg, rg + 8, .. of problem p0 + pl in row order, then the 8 row groups are added in order
__global__ __launch_bounds__(256) void probe_trial_kernel(ProbeTrialArgs a)
{
    __shared__ double s_red[kNA][8][kTP];
    const int tid = threadIdx.x, pl = tid & 31, rg = tid >> 5;
    const int part = blockIdx.x % a.parts, p0 = (blockIdx.x / a.parts) * kTP, prob = p0 + pl;
    const int active = a.flags[(size_t)prob * 8 + I_LS];
    if (!__syncthreads_or(active)) return;
    long long c_begin; int c_end;
    part_range(part, a.chunk, a.N, c_begin, c_end);
    double acc[kNA];
#pragma unroll
    for (int j = 0; j < kNA; ++j) acc[j] = 0.0;
    if (active)
        for (int row = (int)c_begin + rg; row < c_end; row += 8) {
            const size_t at = (size_t)row * a.Ppad + prob;
            const float s = a.sT[at];
            if (s == 0.f) continue;
            const double c = fabsf(s), y = s > 0.f ? 1.0 : -1.0, z = a.z[at], u = a.u[at];
#pragma unroll
            for (int j = 0; j < kNA; ++j) {
                if (j >= a.al.n) break;
                const double t = -y * (z + (double)a.al.a[j] * u);
                acc[j] += c * (fmax(t, 0.0) + log1p(exp(-fabs(t))));
            }
        }
#pragma unroll
    for (int j = 0; j < kNA; ++j) s_red[j][rg][pl] = acc[j];
    __syncthreads();
    if (rg == 0 && active)
        for (int j = 0; j < a.al.n; ++j) {
            double t = 0.0;
            for (int q = 0; q < 8; ++q) t += s_red[j][q][pl];
            a.tp[((size_t)part * kNA + j) * a.Ppad + prob] = t;
        }
}

// ---------------------------------------------------------------- the L1 probes (avae_probe_fit_l1)
// The same passes, another per-problem method: proximal Newton, the inner problem by FISTA.  Of the L2 fit's vectors Dv holds the
// FISTA candidate d+ (what the HV pass multiplies), Pv the last accepted d (what the PANEL pass multiplies), Rv is unused.
enum { F_L = 3, F_T = 4, F_RHO = 5, F_MX = 6 };      // fs: L, the momentum t, L / (largest curvature column sum) of the last inner solve, that sum
enum { D_W1 = 0, D_DELTA = 1 };                      // ds: |w|_1, g.d + |w + d|_1 - |w|_1 (D_PHI0 as in the L2 fit)

// sgn(a) max(|a| - t, 0); what it cuts off is an exact +0.0f
__device__ __forceinline__ float soft_thr(float a, float t)
{
    const float m = fabsf(a) - t;
    return m > 0.f ? copysignf(m, a) : 0.f;
}

// |v_j| of the minimum-norm subgradient: |g + sgn(w)| where w != 0, max(|g| - 1, 0) where w = 0 (a NaN stays a NaN)
__device__ __forceinline__ float subgrad_abs(float g, float w)
{
    if (w != 0.f) return fabsf(g + (w > 0.f ? 1.f : -1.f));
    const float e = fabsf(g) - 1.f;
    return e <= 0.f ? 0.f : e;
}

// xs (N, dim) <- x with every row that holds a value that is not finite replaced by zeros, and every problem with a nonzero cost on
// such a row ended with status 2 before the first pass: x~^T (tile) would carry the row's NaN into every problem of the call, 0 cost
// or not.  One wave per row.
__global__ __launch_bounds__(256) void probe_l1_rows_kernel(const float* __restrict__ x, float* __restrict__ xs, const float* __restrict__ sT,
                                                            int* __restrict__ is, int N, int dim, int Ppad)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const float4* src = reinterpret_cast<const float4*>(x + (size_t)row * dim);
    float4* dst = reinterpret_cast<float4*>(xs + (size_t)row * dim);
    const int nv = dim >> 2;                  // <= 256: 4 float4 per lane
    float4 v[4];
    int bad = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = lane + 64 * j;
        v[j] = i < nv ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float t = (v[j].x - v[j].x) + (v[j].y - v[j].y) + (v[j].z - v[j].z) + (v[j].w - v[j].w);
        bad |= !(t == 0.f);
    }
    const bool any = __ballot(bad) != 0ull;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = lane + 64 * j;
        if (i < nv) dst[i] = any ? make_float4(0.f, 0.f, 0.f, 0.f) : v[j];
    }
    if (any)
        for (int p = lane; p < Ppad; p += 64)
            if (sT[(size_t)row * Ppad + p] != 0.f) {          // (every writer stores the same words)
                end_problem(is + (size_t)p * 8, 2);
            }
}

struct ProbeCurvArgs {
    const float* x; const float* D;      // (N, dim), (N, Ppad)
    float* gp;                           // (parts, LD, Ppad)
    const int* flags;
    int N, dim, LD, Ppad, parts, chunk;
};

// the diagonal of H = X~^T D X~ per part: gp[part][j][p] = sum over the part's rows of D_ip x_ij^2, row j = dim the sum of D alone.
// grid = (parts x problem tiles, dim / 32 rounded up); thread (jg, pl) owns dims 32 blockIdx.y + 4 jg .. + 3 of problem p0 + pl and
// adds the rows in row order.
__global__ __launch_bounds__(256) void probe_l1_curv_kernel(ProbeCurvArgs a)
{
    const int tid = threadIdx.x, pl = tid & 31, jg = tid >> 5;
    const int part = blockIdx.x % a.parts, p0 = (blockIdx.x / a.parts) * kTP, prob = p0 + pl;
    const int busy = tid < kTP ? a.flags[(size_t)(p0 + tid) * 8 + I_CG] : 0;
    if (!__syncthreads_or(busy)) return;
    long long c_begin; int c_end;
    part_range(part, a.chunk, a.N, c_begin, c_end);
    const int j = blockIdx.y * 32 + jg * 4;
    const bool jok = j < a.dim, bias = blockIdx.y == 0 && jg == 0;
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, accb = 0.f;
    const float* xj = a.x + (jok ? j : 0);
#pragma unroll 4
    for (int row = (int)c_begin; row < c_end; ++row) {
        const float Dv = a.D[(size_t)row * a.Ppad + prob];
        const float4 xv = *reinterpret_cast<const float4*>(xj + (size_t)row * a.dim);
        acc[0] = fmaf(Dv * xv.x, xv.x, acc[0]); acc[1] = fmaf(Dv * xv.y, xv.y, acc[1]);
        acc[2] = fmaf(Dv * xv.z, xv.z, acc[2]); acc[3] = fmaf(Dv * xv.w, xv.w, acc[3]);
        accb += Dv;
    }
    float* gp = a.gp + (size_t)part * a.LD * a.Ppad;
    if (jok)
#pragma unroll
        for (int e = 0; e < 4; ++e) gp[(size_t)(j + e) * a.Ppad + prob] = acc[e];
    if (bias) gp[(size_t)a.dim * a.Ppad + prob] = accb;
}

// PHASE 0: after a GRAD pass -- F, g, v, the stop rule.  PHASE 3: after the curvature reduction -- L and the first FISTA candidate.
// PHASE 1: after the k-th HV pass -- the accept / reject of L, the momentum with restart, v_q, the next candidate.  PHASE 2: after
// trial round k -- the composite Armijo test of its step lengths.
template <int PHASE>
__global__ __launch_bounds__(256) void probe_l1_vec_kernel(ProbeWs b, int k, int max_newton, int max_inner, float tol, ProbeAlphas al)
{
    __shared__ double s_sum[3][256];
    __shared__ float s_alpha;
    const int p = blockIdx.x, tid = threadIdx.x, n = b.dim + 1;
    const auto [is, fs, ds, W, G, Dv, Pv] = probe_state(b, p);
    float* Yv = b.Yv + (size_t)p * b.LD;
    float* Hd = b.Hd + (size_t)p * b.LD;
    float* Hy = b.Hy + (size_t)p * b.LD;

    if (PHASE == 0) {
        if (is[I_FROZEN]) return;
        const int it = is[I_ITER];
        const float v0_kept = fs[F_G0];
        double w1 = 0.0, vn = 0.0;
        for (int d = tid; d < n; d += 256) {
            const float w = W[d], gv = merge_parts(b, p, d);
            G[d] = gv;
            w1 += (double)fabsf(w); vn += (double)subgrad_abs(gv, w);
        }
        w1 = block_sum(w1, s_sum); vn = block_sum(vn, s_sum);
        float loss = 0.f;
        for (int q = 0; q < b.parts; ++q) loss += b.lp[(size_t)q * b.Ppad + p];
        const float f = (float)w1 + loss, vnorm = (float)vn;
        const float v0 = it == 0 ? vnorm : v0_kept;
        const int status = newton_stop(f, vnorm, v0, tol, it, max_newton);
        if (tid == 0) {
            fs[F_F] = f; fs[F_GNORM] = vnorm; fs[F_G0] = v0;
            if (status >= 0) end_problem(is, status);
            else { ds[D_W1] = w1; is[I_CG] = 1; }
        }
    } else if (PHASE == 3) {
        if (!is[I_CG]) return;
        const float rho = fs[F_RHO];
        float mx = 0.f;
        for (int d = tid; d < n; d += 256) mx = fmaxf(mx, merge_parts(b, p, d));
        mx = block_max(mx, s_sum);
        // L starts at the largest diagonal entry of H (a lower bound of its largest eigenvalue; the backtracking doubles it), from the
        // second inner solve on at half of what the last one ended with, relative to that entry
        float L = mx;
        if (rho > 2.f && rho - rho == 0.f) L = mx * (0.5f * rho);
        if (!(L > 0.f) || !(L - L == 0.f)) {
            if (tid == 0) { is[I_CG] = 0; end_problem(is, 2); }
            return;
        }
        const float iL = 1.f / L;
        for (int d = tid; d < n; d += 256) {
            const float w = W[d];
            Pv[d] = 0.f; Yv[d] = 0.f; Hd[d] = 0.f; Hy[d] = 0.f;
            Dv[d] = soft_thr(fmaf(-G[d], iL, w), iL) - w;
        }
        if (tid == 0) { fs[F_L] = L; fs[F_T] = 1.f; fs[F_MX] = mx; }
    } else if (PHASE == 1) {
        if (!is[I_CG]) return;
        const float L = fs[F_L], t = fs[F_T], vnorm = fs[F_GNORM];
        float hp[kVecPer];
        double dHd = 0.0, dd = 0.0, rs = 0.0;
#pragma unroll
        for (int j = 0; j < kVecPer; ++j) {          // (a loop of loads alone: nothing stored between them, every element's in flight)
            const int d = tid + 256 * j;
            hp[j] = d < n ? merge_parts(b, p, d) : 0.f;
        }
#pragma unroll
        for (int j = 0; j < kVecPer; ++j) {
            const int d = tid + 256 * j;
            if (d < n) {
                const float c = Dv[d], yv = Yv[d], del = c - yv;
                dHd += (double)del * (double)(hp[j] - Hy[d]); dd += (double)del * del; rs += (double)(yv - c) * (double)(c - Pv[d]);
            }
        }
        double sums[3] = {dHd, dd, rs};
        block_reduce<3, OpAdd>(sums, s_sum);
        dHd = sums[0]; dd = sums[1]; rs = sums[2];
        bool bad = !finite_d(dHd) || !finite_d(dd);
        // the backtracking test on the quadratic: q_s(d+) - q_s(y) - grad q_s(y).(d+ - y) = 1/2 (d+ - y).H (d+ - y) <= L/2 |d+ - y|^2
        const bool accept = !bad && dHd <= (double)L * dd;
        const bool last = k + 1 >= max_inner;
        bool stop = last;
        float Ln = L, tn = 1.f;
        if (accept) {
            double vq = 0.0;
#pragma unroll
            for (int j = 0; j < kVecPer; ++j) {
                const int d = tid + 256 * j;
                if (d < n) vq += (double)subgrad_abs(G[d] + hp[j], W[d] + Dv[d]);
            }
            vq = block_sum(vq, s_sum);
            bad = !finite_d(vq);
            stop = last || vq <= 0.1 * (double)vnorm;
            const bool restart = rs > 0.0;          // the momentum points against the step just taken
            tn = restart ? 1.f : 0.5f * (1.f + sqrtf(fmaf(4.f * t, t, 1.f)));
            const float beta = restart ? 0.f : (t - 1.f) / tn, iL = 1.f / L;
#pragma unroll
            for (int j = 0; j < kVecPer; ++j) {
                const int d = tid + 256 * j;
                if (d < n) {
                    const float c = Dv[d], w = W[d];
                    const float yn = fmaf(beta, c - Pv[d], c), hyn = fmaf(beta, hp[j] - Hd[d], hp[j]);
                    Pv[d] = c; Hd[d] = hp[j]; Yv[d] = yn; Hy[d] = hyn;
                    if (!stop) Dv[d] = soft_thr(fmaf(-(G[d] + hyn), iL, w + yn), iL) - w;
                }
            }
        } else if (!bad) {
            // L doubles, the momentum falls back to the last accepted d; this launch was spent
            Ln = 2.f * L;
            const float iL = 1.f / Ln;
#pragma unroll
            for (int j = 0; j < kVecPer; ++j) {
                const int d = tid + 256 * j;
                if (d < n) {
                    const float pd = Pv[d], hd = Hd[d], w = W[d];
                    Yv[d] = pd; Hy[d] = hd;
                    if (!stop) Dv[d] = soft_thr(fmaf(-(G[d] + hd), iL, w + pd), iL) - w;
                }
            }
        }
        if (bad) {
            if (tid == 0) { is[I_CG] = 0; end_problem(is, 2); }
            return;
        }
        if (!stop) {
            if (tid == 0) { fs[F_L] = Ln; fs[F_T] = tn; }
            return;
        }
        // the step is Pv: what the Armijo test needs of it
        double gtd = 0.0, w1d = 0.0;
        for (int d = tid; d < n; d += 256) { const float pv = Pv[d]; gtd += (double)G[d] * pv; w1d += fabs((double)W[d] + (double)pv); }
        gtd = block_sum(gtd, s_sum); w1d = block_sum(w1d, s_sum);
        if (tid == 0) {
            const double delta = gtd + (w1d - ds[D_W1]);
            is[I_CG] = 0;
            if (!finite_d(delta)) end_problem(is, 2);
            else { ds[D_DELTA] = delta; is[I_LS] = 1; fs[F_RHO] = Ln / fs[F_MX]; }
        }
    } else {
        if (!is[I_LS]) return;
        double l1[kNA];
#pragma unroll
        for (int j = 0; j < kNA; ++j) {
            l1[j] = 0.0;
            if (j < al.n) {
                const double a = al.a[j];
                double part = 0.0;
                for (int d = tid; d < n; d += 256) part += fabs((double)W[d] + a * (double)Pv[d]);
                l1[j] = block_sum(part, s_sum);
            }
        }
        if (tid == 0) {
            const ArmijoPick pk = armijo_scan(b, p, k, al, ds, [ds = ds, &l1](int j, double, bool& bad) { bad = !finite_d(l1[j]); return l1[j] - ds[D_W1]; },
                                              [ds = ds](double a) { return 0.01 * a * ds[D_DELTA]; });
            s_alpha = armijo_settle(is, pk, al.last);
        }
        __syncthreads();
        const float a = s_alpha;
        if (a > 0.f)
            for (int d = tid; d < n; d += 256) {
                const float nw = fmaf(a, Pv[d], W[d]);          // at a = 1 and d = 0 - w (the soft-threshold cut it off): exactly 0
                W[d] = nw == 0.f ? 0.f : nw;
            }
    }
}

int pick_dt(int dim) { return dim <= 128 ? 1 : dim <= 256 ? 2 : dim <= 512 ? 4 : 8; }

}  // namespace

// The launch shape, from the problem shape alone.  Problems go in tiles of 32 (one MFMA tile wide).  The rows are cut into parts of
// `chunk` rows, a multiple of the 128-row tile: enough parts for one workgroup per CU on 256 CUs per problem tile, at most
// kProbeMaxParts (the per-problem kernel adds the parts' partials one after the other).  The part count must NOT depend on P (a
// problem's bits may not), so few problem tiles mean few workgroups.  Both figures are a first guess: scripts/probe_bench.py has run
// with these values and no other.  chunk_opt > 0 (option probe_chunk, a test aid) caps the rows of a part instead; it
// is raised where it would give more parts than that.
ProbePlan probe_plan(int N, int P, int dim, int chunk_opt)
{
    ProbePlan p{};
    p.ptiles = (P + kProbeTile - 1) / kProbeTile;
    p.Ppad = p.ptiles * kProbeTile;
    p.LD = dim + 4;
    const RowParts r = row_parts(N, kTR, 256, kProbeMaxParts, chunk_opt);
    p.parts = r.parts; p.chunk = r.chunk;
    return p;
}

hipError_t probe_prepare(hipStream_t st, const ProbeWs& b, const float* s, int P)
{
    hipError_t e = hipMemsetAsync(b.W, 0, (size_t)5 * b.Ppad * b.LD * sizeof(float), st);      // W, G, Dv, Rv, Pv are one run
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(b.fs, 0, (size_t)b.Ppad * 8 * sizeof(float), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(b.ds, 0, (size_t)b.Ppad * 8 * sizeof(double), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(probe_init_kernel, dim3((unsigned)((b.Ppad + 255) / 256)), dim3(256), 0, st, b.is, P, b.Ppad);
    const dim3 grid((unsigned)(((long long)b.N + 31) / 32), (unsigned)(b.Ppad / 32));
    hipLaunchKernelGGL(probe_costs_kernel, grid, dim3(256), 0, st, s, P, b.N, b.Ppad, b.sT);
    return hipGetLastError();
}

hipError_t probe_pass(hipStream_t st, const ProbeWs& b, const float* x, int mode)
{
    ProbePassArgs a{};
    a.x = x; a.sT = b.sT; a.z = b.z; a.D = b.D; a.gp = b.gp; a.lp = b.lp; a.flags = b.is;
    a.N = b.N; a.dim = b.dim; a.LD = b.LD; a.Ppad = b.Ppad; a.parts = b.parts; a.chunk = b.chunk;
    const dim3 grid((unsigned)(b.parts * (b.Ppad / kTP)));
    auto launch = [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (mode == 0) { a.v = b.W; a.flag = I_ALIVE; hipLaunchKernelGGL((probe_pass_kernel<0, DT>), grid, dim3(256), 0, st, a); }
        else { a.v = b.Dv; a.flag = I_CG; hipLaunchKernelGGL((probe_pass_kernel<1, DT>), grid, dim3(256), 0, st, a); }
    };
    if (mode == 2) {
        a.v = b.Pv; a.flag = I_LS; a.out = b.u; a.ldo = b.Ppad; a.pout = b.Ppad;
        hipLaunchKernelGGL((probe_pass_kernel<2, 1>), grid, dim3(256), 0, st, a);
    } else switch (pick_dt(b.dim)) {
        case 1: launch(std::integral_constant<int, 1>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        case 4: launch(std::integral_constant<int, 4>{}); break;
        default: launch(std::integral_constant<int, 8>{}); break;
    }
    return hipGetLastError();
}

// one workgroup per problem of the per-problem kernel of a phase
typedef void (*ProbeVecKernel)(ProbeWs, int, int, int, float, ProbeAlphas);
static hipError_t launch_vec(hipStream_t st, ProbeVecKernel kern, const ProbeWs& b, int P, int k, int max_newton, int inner, float tol, const ProbeAlphas& al)
{
    hipLaunchKernelGGL(kern, dim3((unsigned)P), dim3(256), 0, st, b, k, max_newton, inner, tol, al);
    return hipGetLastError();
}

hipError_t probe_vec(hipStream_t st, const ProbeWs& b, int P, int phase, int k, int max_newton, int max_cg, float tol, const ProbeAlphas& al)
{
    static const ProbeVecKernel kern[3] = {probe_vec_kernel<0>, probe_vec_kernel<1>, probe_vec_kernel<2>};
    if (phase < 0 || phase > 2) return hipErrorInvalidValue;
    return launch_vec(st, kern[phase], b, P, k, max_newton, max_cg, tol, al);
}

hipError_t probe_trial(hipStream_t st, const ProbeWs& b, const ProbeAlphas& al)
{
    ProbeTrialArgs a{};
    a.sT = b.sT; a.z = b.z; a.u = b.u; a.tp = b.tp; a.flags = b.is; a.N = b.N; a.Ppad = b.Ppad; a.parts = b.parts; a.chunk = b.chunk; a.al = al;
    hipLaunchKernelGGL(probe_trial_kernel, dim3((unsigned)(b.parts * (b.Ppad / kTP))), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t probe_finish(hipStream_t st, const ProbeWs& b, int P, float* w, float* stats)
{
    hipLaunchKernelGGL(probe_finish_kernel, dim3((unsigned)P), dim3(256), 0, st, b, w, stats);
    return hipGetLastError();
}

// the state of a fresh L1 fit: that of the L2 fit, then b.xs <- x without the rows that are not finite
hipError_t probe_l1_prepare(hipStream_t st, const ProbeWs& b, const float* x, const float* s, int P)
{
    const hipError_t e = probe_prepare(st, b, s, P);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(probe_l1_rows_kernel, dim3((unsigned)(((long long)b.N + 3) / 4)), dim3(256), 0, st, x, b.xs, b.sT, b.is, b.N, b.dim, b.Ppad);
    return hipGetLastError();
}

hipError_t probe_l1_curv(hipStream_t st, const ProbeWs& b)
{
    ProbeCurvArgs a{};
    a.x = b.xs; a.D = b.D; a.gp = b.gp; a.flags = b.is;
    a.N = b.N; a.dim = b.dim; a.LD = b.LD; a.Ppad = b.Ppad; a.parts = b.parts; a.chunk = b.chunk;
    const dim3 grid((unsigned)(b.parts * (b.Ppad / kTP)), (unsigned)((b.dim + 31) / 32));
    hipLaunchKernelGGL(probe_l1_curv_kernel, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t probe_l1_vec(hipStream_t st, const ProbeWs& b, int P, int phase, int k, int max_newton, int max_inner, float tol, const ProbeAlphas& al)
{
    static const ProbeVecKernel kern[4] = {probe_l1_vec_kernel<0>, probe_l1_vec_kernel<1>, probe_l1_vec_kernel<2>, probe_l1_vec_kernel<3>};
    if (phase < 0 || phase > 3) return hipErrorInvalidValue;
    return launch_vec(st, kern[phase], b, P, k, max_newton, max_inner, tol, al);
}

// out (n, P) = x~ w^T: w packed into W (Ppad, LD) first, then the PANEL pass
hipError_t probe_decision(hipStream_t st, const ProbePlan& p, const float* x, int n, int dim, const float* w, int P, float* W, float* out)
{
    const size_t tot = (size_t)p.Ppad * p.LD;
    hipLaunchKernelGGL(probe_pack_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, w, P, dim, p.LD, p.Ppad, W);
    ProbePassArgs a{};
    a.x = x; a.v = W; a.out = out; a.ldo = P; a.pout = P; a.flags = nullptr;
    a.N = n; a.dim = dim; a.LD = p.LD; a.Ppad = p.Ppad; a.parts = p.parts; a.chunk = p.chunk;
    hipLaunchKernelGGL((probe_pass_kernel<2, 1>), dim3((unsigned)(p.parts * p.ptiles)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace avae
