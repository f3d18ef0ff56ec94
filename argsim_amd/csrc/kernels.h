// kernels.h -- internal launch interface of the gfx950 kernels (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_plan.h"

namespace avae {

// ---------------------------------------------------------------- GEMM (gemm_f32.hip)
// C[M,N] = alpha * op(A) * op(B) (+ bias[n]) (+ C if accumulate), exact fp32 on
// v_mfma_f32_32x32x2_f32.  Row-major storage with leading dimensions:
//   a_mc == false : A[m*lda + k]   (k contiguous)     a_mc == true : A[k*lda + m]
//   b_nc == false : B[n*ldb + k]   (k contiguous)     b_nc == true : B[k*ldb + n]
// The contiguous dimension and every leading dimension must be a multiple of 4 floats and
// every base pointer 16-byte aligned.  M/N/K edges are predicated (zero filled).
// dyn (optional, device): the real row count when it is only known on the device:
//   dyn_kind 1 -> M_eff = min(M, *dyn) (row tiles beyond it exit),  2 -> K_eff = min(K, *dyn).
//   dyn_kind 2 takes [k][x] operands only (a_mc && b_nc, the weight gradients): a k-contiguous tile is staged four k at a time with ONE
//   test of k < K_eff, so a depth that is no multiple of 4 would bring in up to three elements beyond it.  gemm_f32, gemm_f32s and
//   gemm_bf16_direct refuse the other layouts (the conversion passes + gemm_bf16_nt mask per element and take any layout).  With
//   split_k > 1 it takes no bias either: a slice that starts at or beyond K_eff returns before its epilogue.
// split_k > 1: grid.z slices of K, combined with float atomics INTO C (C must hold the value to
// accumulate onto, e.g. zeros); bias is added by slice 0.
struct GemmArgs {
    const float* A; const float* B; float* C; const float* bias;
    int M, N, K, lda, ldb, ldc;
    float alpha;
    int accumulate;      // C += ...
    int split_k;
    const int* dyn; int dyn_kind;
    int dyn_expect;      // dyn_kind 1: the count the host expects (an earlier call's; 0 = unknown) -- launch shaping only, never correctness
    int thin;            // 1: 32x128 block tiles (thin row panels) instead of 128x128; 2: 64x64; 3: skinny form (32x32 per workgroup, K split over its waves)
    // optional second problem of identical shape, layout and scalars, run by the same launch (grid.y = 2): two
    // weight-gradient GEMMs over the same rows then share ONE round of workgroups at half the K split (half the
    // float-atomic traffic each), two small affines share one launch.  Exact-fp32 kernel only.
    const float* A2; const float* B2; float* C2; const float* bias2;
    float* slab = nullptr; size_t slab_floats = 0;      // bf16 TN form, K split: workspace for the slices' partial tiles (summed by a reduce pass instead of float atomics)
    unsigned short* c16 = nullptr;      // bf16 NT form, phased kernel only (gemm_bf16_c16_ok): the result goes HERE as an fp16 panel [M][ldc] INSTEAD of fp32 C (the logits of a
                                        // training step: softmax_ce reads the 2-byte panel and turns it into the bf16 gradient in place); no bias, no accumulate, no K split
    int nt8 = 1;         // bf16 NT form: the phased LDS-DMA kernel (gemm_bf16_p8.hip) where the shape allows; 0: gemm_bf16_nt256_kernel
};
hipError_t gemm_f32(hipStream_t st, bool a_mc, bool b_nc, const GemmArgs& g);
// what gemm_f32 launches for a problem, decided from the arguments alone (host arithmetic, no device): tile 0 128x128, 1 32x128, 2 64x64,
// 3 skinny, -1 nothing to launch (no rows or columns); fast: buffer-load staging; db: double-buffered LDS; persist: the persistent
// 128x128 kernel; the grid; err: the refusal gemm_f32 returns instead of launching
struct GemmF32Form { int tile; bool fast, db, persist; unsigned gx, gy, gz; hipError_t err; };
GemmF32Form gemm_f32_form(bool a_mc, bool b_nc, const GemmArgs& g);
// same contract on the bf16 matrix cores: every fp32 operand element is split into three bf16 in registers and
// six partial products are accumulated in fp32 (gemm_f32s.hip; fp32-accurate, 128x128 tiles only: g.thin ignored)
hipError_t gemm_f32s(hipStream_t st, bool a_mc, bool b_nc, const GemmArgs& g);
// bf16-operand GEMM from fp32 operands in any layout (gemm_f32s.hip, one plane): RNE to bf16 while staging into LDS, one
// product, fp32 accumulate; no conversion pass (g.thin ignored)
hipError_t gemm_bf16_direct(hipStream_t st, bool a_mc, bool b_nc, const GemmArgs& g);

// ---------------------------------------------------------------- bf16-operand GEMM (gemm_bf16.hip)
// fp32 -> bf16 panel: transpose == false: src [rows][cols] (ld) -> dst [rows][ldd];  transpose == true:
// src [K][X] (ld) -> dst [X][ldd] with ldd >= K.  ldd is a multiple of 8; pad columns are zero filled.
hipError_t cvt_bf16(hipStream_t st, const float* src, int ld, bool transpose, int rows_or_K, int cols_or_X,
                    unsigned short* dst, int ldd);
// C = alpha * A B^T (+bias)(+C): A [M][lda], B [N][ldb] bf16 k-contiguous; the other fields as in GemmArgs
hipError_t gemm_bf16_nt(hipStream_t st, const unsigned short* A, int lda, const unsigned short* B, int ldb, const GemmArgs& g);
// the phased 256x256 form of the same contract (gemm_bf16_p8.hip); _ok: K % 64 == 0, N % 4 == 0, aligned C / bias, no device-side K
bool gemm_bf16_p8_ok(const GemmArgs& g, int lda, int ldb);
hipError_t gemm_bf16_p8(hipStream_t st, const unsigned short* A, int lda, const unsigned short* B, int ldb, const GemmArgs& g, int s2);
// would gemm_bf16_nt run this problem on the phased kernel (the only one that writes GemmArgs::c16)?
bool gemm_bf16_c16_ok(const GemmArgs& g, int lda, int ldb);
// the same question from the shape alone: A (M, K), B (N, K) fp32 k-contiguous with K % 8 == 0, C (M, N), rows: the device-side row count or null
bool gemm_bf16_c16_takes(int M, int N, int K, const int* rows, int nt8);
// ... and of gemm_bf16_tn's contract (operands [k][x] row-major, K host- or device-side, any K)
bool gemm_bf16_p8_tn_ok(const GemmArgs& g, int lda, int ldb);
hipError_t gemm_bf16_p8_tn(hipStream_t st, const unsigned short* A, int lda, const unsigned short* B, int ldb, const GemmArgs& g, int s2);
// C = alpha * A^T B (+C): A [K][lda] (m contiguous), B [K][ldb] (n contiguous) bf16, read with transposing LDS loads -- no
// transposed copy of either operand (M, N, lda, ldb multiples of 8; split_k > 1: float atomics into C)
hipError_t gemm_bf16_tn(hipStream_t st, const unsigned short* A, int lda, const unsigned short* B, int ldb, const GemmArgs& g);
// the slices the phased launchers run for a split s2 as gemm_bf16_nt / gemm_bf16_tn derived it (NT: two K tiles or more per slice; TN: the
// split that fills whole rounds of the persistent grid, where the caller asked for one), and whether the TN slices go through GemmArgs::slab
int gemm_bf16_p8_slices(int K, int s2);
int gemm_bf16_p8_tn_slices(const GemmArgs& g, int s2);
bool gemm_bf16_p8_tn_slab(const GemmArgs& g, int s2);
// what gemm_bf16_nt (tn false) / gemm_bf16_tn (tn true) launch for a problem, decided from the arguments alone (host arithmetic, no device):
// the kernel (kBf16None: nothing to launch, or with err the refusal returned instead), s2: the split re-derived for 256x256 tiles, slices: what
// the kernel is launched with, slab: the slices' partial tiles go through GemmArgs::slab and p8_slab_reduce_kernel
enum GemmBf16Kernel { kBf16None = -1, kBf16Nt128 = 0, kBf16Nt256 = 1, kBf16P8Nt = 2, kBf16Tn256 = 3, kBf16P8Tn = 4 };
struct GemmBf16Form { int kernel, s2, slices; bool slab; hipError_t err; };
GemmBf16Form gemm_bf16_form(bool tn, int lda, int ldb, const GemmArgs& g);
// bf16 [K][X] (row stride ld) -> bf16 [X][ldk] (ldk = K rounded up to 8, pad zero-filled)
hipError_t transpose_bf16(hipStream_t st, const unsigned short* src, int ld, int K, int X, unsigned short* dst, int ldk);

// ---------------------------------------------------------------- GRU (gru.hip; kernels in gru_reg.hip, gru_team.hip, gru_rs.hip)
// Gate-interleaved layout ("G16"): the 3D gate rows of W, R, bW, bR and the 3D columns of
// gi / dgi / dgh are stored in the order  c' = ht*48 + u*3 + gate   (ht = unit/16, u = unit%16,
// gate: 0=r 1=u 2=n) so that the 48 values one workgroup owns are contiguous and the three gates of
// one unit are adjacent (one 12-byte access per thread in the gate phase).
constexpr int kMaxGruJobs = 3;
struct GruJob {
    const float* gi;      // + job column offset; row (pos*B + b) at gi + (pos*B+b)*ldg
    const int32_t* gi_rows;   // optional (team kernels only): row gi_rows[pos*B + b] instead -- a layer fed by embedding rows reads
                          // its projection straight out of the per-id table (model.cpp use_table), no per-token copy
    const float* R;       // (3D, D) G16 rows
    const float* bR;      // (3D) G16
    const float* h0;      // (B, D) or nullptr (zeros)
    float* hs;            // output, row (pos*B+b) at hs + (pos*B+b)*ldh (+ column offset applied)
    float* sv;            // saved r,u,n,hn: (S,B,HT,16,4) or nullptr
    float* hp;            // saved h_prev (S,B,D) or nullptr
    int reverse;          // 1: time index map of tf.reverse_sequence (needs lens)
    // optional, bf16 team kernels only: the row-major h (indexed like hs, ldh) / h_prev (S,B,D) copies as bf16 INSTEAD of fp32
    unsigned short* hs16;
    unsigned short* hp16; //   (the backward reads h_prev from here when given)
    // backward only
    const float* dh_out;  // grad wrt hs (same indexing as hs: ldh) or nullptr
    float* dgi;           // (S,B,ldg) G16 columns (+ job offset)
    float* dgh;           // (S,B,ldg)
    unsigned short* dgi16; // optional, bf16 team kernels only: dgi / dgh as bf16 (S,B,ldg) row-major INSTEAD of the fp32 arrays
    unsigned short* dgh16; //   (honoured where gru_plan gives a team form)
    float* dh0;           // (B,D) or nullptr
    float* carry;         // (B,D) scratch: dH_{p+1} * u_{p+1}
    int dgi_by_pos;       // with GruArgs::rowmap: dgi / dgi16 keep the padded (pos * B + row) layout, zeros at padding (a table-fed layer: summed by token id)
    float* dbW;           // (3D) G16 += column sums of dgi (or nullptr)
    float* dbR;           // (3D) G16 += column sums of dgh (or nullptr)
};
struct GruArgs {
    GruJob job[kMaxGruJobs];
    int njobs, S, B, D, ldg, ldh;
    const int* lens;      // (B) or nullptr
    // optional, team kernels only (gru_dev.h "Padding skipped"): steps each SLOT really has and the batch row sitting in it;
    // both or neither.  The other kernel forms ignore them and run every step of every row.
    const int* slens;     // (B) by slot
    const int* perm;      // (B) slot -> batch row
    // optional, team kernels only: COMPACT external arrays.  rowmap[pos * B + row] = the row of gi / hs / sv / hp / dh_out / dgi / dgh
    // that position has among the real (non-padding) positions in time-major order, -1 for a padding position (nothing is read
    // or written for it; it still takes part in the exchange).  gi_rows (a table-fed layer) stays indexed by pos * B + row.
    const int* rowmap;
    // optional, team kernels only, with slens + perm + rowmap: the launch geometry's batch, a multiple of the 16 T-row block above B.
    // Slots hold Bx rows (slens / perm have Bx entries, the exchange scratch and the carry Bx rows); a slot whose perm entry is >= B is
    // a PHANTOM row (slens 1): nothing external is read or written for it.  Every external array keeps B rows per position.  0: B.
    int Bx;
    int G;                // batch groups per job
    int rows_per_group;   // multiple of 16
    int p_begin, p_end;   // steps [p_begin, p_end) of this launch
    unsigned* counters;   // 1664 words (step counters | detection counters | XCD ids), zeroed by the launcher
    int* err;             // device error word (set on spin timeout)
    unsigned long long* stamps;   // 32 words of diagnostic phase sums (ablate bit 32) or nullptr
    int item_pipeline;    // 1: use the software-pipelined D = 512 forward kernel where its geometry applies
    float* xbuf;          // scratch for the team kernels' exchange in MFMA-tile order (see gru_dev.h "tiled exchange"): at least
    size_t xbuf_floats;   // njobs*S*B*D floats (forward) / njobs*S*B*3D (backward); nullptr / too small: register-form kernels
    int stagger;          // 1: delay the second half of the grid by ~half a step (co-resident chains de-phased)
    int force_slow;       // 1: never use the same-XCD L2 fast path
    int sv16;             // 1 (bf16 team kernels, forward AND backward of a layer): the saved gates r, u, n, hn are stored as bf16
    int bf16;             // 1 (compute_dtype 1): the team kernels round both operands of the recurrent product to bf16
    int spec;             // 1 (team kernels, one row block per workgroup): few rows are alive per step -- a consumer loads its operand at once, without a probe round trip in front (speed only)
    int bwd_rs;           // 1: the backward runs the reduce-scatter team kernel (gru_rs.hip) where the team geometry applies and xbuf holds its ring
    int ring;             // 1: the team kernels exchange through a ring of slots where the plan allows it (GruPlan::ring; gru_dev.h "exchange ring"), 0: one slot per position
    int ablate;           // timing experiments only: 1 no MFMA/A loads, 2 no gate-phase loads, 4 no saves, 8 cheap activations, 16 no sync
};
// The kernel form of a launch, from its shape alone (geometry, Bx, xbuf / xbuf_floats, p_begin / p_end, bf16, bwd_rs, ablate,
// item_pipeline): callers plan before they attach slens / perm / rowmap and the job pointers.  gi_rows, slens / perm: team forms only.
constexpr int kGruRing = 4;       // depth of the team kernels' exchange ring (gru_dev.h "exchange ring": why not 3)
enum class GruForm { stepwise, persistent, item, team, team_rs };     // item: forward only (gru_fwd_item_kernel); team_rs: backward only (gru_rs.hip)
struct GruPlan {
    GruForm form;
    int T, C, cpj, Bg;      // team forms: T teams of 16 rows per 16 T-row block, C workgroups per hidden tile (cpj per job); Bg = max(B, Bx)
    bool pipe, diag;        // pipe: several row blocks per workgroup; diag: the DIAG build's timing instantiation (fp32, padded layout)
    int ring;               // slots of the exchange ring (kGruRing; the slot of a value = the iteration that made it, mod ring), 0: one slot per position
    bool team() const { return form == GruForm::team || form == GruForm::team_rs; }
    bool full() const { return team() && !diag; }      // a team form that honours the 16-bit operands, rowmap and phantom rows too
};
GruPlan gru_plan(const GruArgs& a, bool fwd, bool persistent);
hipError_t gru_forward(hipStream_t st, const GruArgs& a, bool persistent);
hipError_t gru_backward(hipStream_t st, const GruArgs& a, bool persistent);
int gru_team_batch(int B);        // smallest row count >= B (within 256) the team kernels have a geometry for with one job and with two; 0: none
bool gru_dim_supported(int D);
// reduce-scatter form of the backward team kernels (gru_rs.hip): floats of exchange scratch it needs for njobs jobs over `rows` slots
size_t gru_bwd_rs_xbuf_floats(int njobs, int rows);
hipError_t gru_bwd_rs_launch(hipStream_t st, const GruArgs& a, const GruPlan& p);
// the launches gru_forward / gru_backward choose between, after planning and preparing the exchange: the team forms (gru_team.hip), the
// register-resident forms (gru_reg.hip; grid = njobs * G * D/16 workgroups, need_resident: a persistent launch) and the item form
hipError_t gru_fwd_team_launch(hipStream_t st, const GruArgs& a, const GruPlan& p);
hipError_t gru_bwd_team_launch(hipStream_t st, const GruArgs& a, const GruPlan& p);
hipError_t gru_reg_launch(hipStream_t st, const GruArgs& a, bool fwd, int grid, bool need_resident);
hipError_t gru_fwd_item_launch(hipStream_t st, const GruArgs& a, int grid);
// one GRU step from a zero state for B rows (the top encoder layer's backward direction: gru_reg.hip "one step from a zero
// state"): gi (B, 3D) / bR G16; h -> h_out[b * ldo + j]; sv (B, D, 4) = r, u, n, hn or nullptr
hipError_t gru_first_step_fwd(hipStream_t st, const float* gi, const float* bR, float* h_out, int ldo, float* sv, int B, int D, const int32_t* lens = nullptr);      // lens: rows of length 0 get h = 0
// its backward: dh[b * ldd + j] -> dgi, dgh (B, 3D) G16
hipError_t gru_first_step_bwd(hipStream_t st, const float* dh, int ldd, const float* sv, float* dgi, float* dgh, int B, int D, const int32_t* lens = nullptr);
bool gru_diag_build();     // true: built with -DAVAE_DIAG (ablation / stamp instantiations present)

// ---------------------------------------------------------------- small kernels (ops.hip)
struct PrepArgs {
    const int32_t* src; const int32_t* tgt;   // (B,Ss),(B,St) row-major
    int B, Ss, St, eos, bos;
    int train; float keepwd; uint64_t seed; const uint8_t* keep_mask;  // (St,B)
    int32_t* src_tm;    // (Ss,B)
    int32_t* lens_src;  // (B)
    int32_t* lens_tgt;  // (B)
    int32_t* lead;      // (St+1,B)
    int32_t* gold;      // (St+1,B)
    int32_t* rank;      // (St+1,B) compact row of (t,b) or -1
    int32_t* cidx;      // (N) flat (t*B+b) of compact row
    int32_t* ntok;      // [0]=N
    float* zero2;       // optional: two floats cleared here (the loss accumulators), saves a memset launch
    int32_t* chunk_counts;   // scratch, kPrepChunks ints: kept positions per chunk of the flat time-major order
};
constexpr int kPrepChunks = 1024;
hipError_t prep_ids(hipStream_t st, const PrepArgs& p);

hipError_t embed_gather(hipStream_t st, const float* E, const int32_t* ids, float* out, int n, int D, int V);
// dE[ids0[t]] += dout0[t], dE[ids1[t]] += dout1[t]; scratch: embed_scatter_scratch_ints(n0 + n1, V) ints
hipError_t embed_scatter_add2(hipStream_t st, float* dE, const int32_t* ids0, const float* dout0, int n0, const int32_t* ids1,
                              const float* dout1, int n1, int D, int V, int32_t* scratch);
// token groups of an id source (ops.hip "token groups"): built once per step, used by the forward gather and the backward sums
bool id_groups_supported(int V);
inline size_t id_groups_ints(size_t n, size_t V) { return 4 * V + 2 + n + (n / 32 + V + 1) + 2 * V + 4; }
hipError_t id_groups_build(hipStream_t st, const int32_t* ids, int n, int V, int32_t* scratch, bool lists);
const int32_t* id_groups_rank(int32_t* scratch, int n, int V);     // [V]  index among the present ids, -1 absent
const int32_t* id_groups_uid(int32_t* scratch, int n, int V);      // [V]  present ids, ascending
const int32_t* id_groups_count(int32_t* scratch, int n, int V);    // [1]  how many
// out[t] = rank[ids[t]]
hipError_t rank_rows(hipStream_t st, int32_t* out, const int32_t* ids, const int32_t* rank, int n, int V);
hipError_t rows_gather_ranked(hipStream_t st, float* dst, const float* src, const int32_t* ids, const int32_t* rank, int n, int W, int V);
hipError_t rows_group_sum(hipStream_t st, float* dst, const int32_t* ids, const float* src, int n, int W, int V, int32_t* scratch);
hipError_t rows_add_indexed(hipStream_t st, float* dst, const float* src, const int32_t* uid, const int32_t* nuniq, int n_max, int D);
inline size_t embed_scatter_scratch_ints(size_t n, size_t V) { return 4 * V + 2 + n + (n / 32 + V + 1); }
// Row order for the padding-skipping team kernels: rows sorted by steps[b] = lens[b] + add (descending, stable) and dealt
// in groups of 16 over the workgroups of a (T, cpj) team geometry so that every workgroup's row blocks get shorter with r
// (slot of sorted group g: ((g % cpj) + (g / cpj / T) * cpj) * T + (g / cpj) % T).  perm[slot] = batch row, slens[slot] =
// its steps.  Up to three geometries in one launch.
struct RowOrder { const int32_t* lens; int add, T, cpj; int32_t* perm; int32_t* slens; };
hipError_t row_order(hipStream_t st, const RowOrder* orders, int n, int Breal, int B, int S, int32_t* steps_sum = nullptr, int sum_rows = 0);      // steps_sum[0..1] <- sum of the first order's steps, sum_rows; B >= Breal slots: the rows beyond Breal are phantom rows of one step
// dst[i,:] = src[idx[i],:] for i < *n_dev
hipError_t rows_gather(hipStream_t st, float* dst, const float* src, const int32_t* idx, const int32_t* n_dev, int n_max, int D, const int32_t* map = nullptr);
// dst[r,:] = rank[r] >= 0 ? src[rank[r],:] : 0   for r < rows
hipError_t rows_expand(hipStream_t st, float* dst, const float* src, const int32_t* rank, int rows, int D, const int32_t* map = nullptr);
// h[b,:] = hs[(len_b-1)*B + b, :]  (model.py:135)
hipError_t pick_last(hipStream_t st, float* h, const float* hs, const int32_t* lens, int B, int W, const int32_t* map = nullptr);      // (map: compact rows, row_map)
// the same from a bf16 source: h[b,:] = float(hs16[(len_b-1)*B + b, :])
hipError_t pick_last16(hipStream_t st, float* h, const unsigned short* hs16, const int32_t* lens, int B, int W, const int32_t* map = nullptr);
// dhs[(len_b-1)*B+b,:] += d[b,:]
hipError_t pick_last_add(hipStream_t st, float* dhs, const float* d, const int32_t* lens, int B, int W, const int32_t* map = nullptr);
// compact row map of an id source (ops.hip "compact row map"): map (S*B), nact (S scratch), count [1]
hipError_t row_map(hipStream_t st, const int32_t* lens, int add, int S, int B, int32_t* map, int32_t* nact, int32_t* count);
hipError_t zero_rows_dyn(hipStream_t st, float* X, const int32_t* count, int rows_max, int W);      // X[r,:] = 0 for r < min(rows_max, *count)
// dhs = 0 everywhere except dhs[(len_b-1)*B+b,:] = dh[b,:]
hipError_t pick_last_bwd(hipStream_t st, float* dhs, const float* dh, const int32_t* lens, int S, int B, int W);

// z = mu (+ exp(lv/2)*eps when train; eps from eps_in or the counter RNG, echoed to eps_out);
// kld[i] = 0.5(mu^2 + e^lv - lv - 1); acc[0] += sum max(kld, free_bits)
hipError_t latent_fwd(hipStream_t st, const float* mu, const float* lv, const float* eps_in, float* eps_out, float* z,
                      float* kld, int n, int train, uint64_t seed, float free_bits, float* acc);
// dmu = dz + c*mu ; dlv = dz*eps*0.5*exp(lv/2) + c*0.5*(exp(lv)-1), c = anneal/(Bg*R) (free-bits gated)
hipError_t latent_bwd(hipStream_t st, const float* dz, const float* mu, const float* lv, const float* eps_used,
                      float* dmu, float* dlv, int B, int R, float coef, float free_bits);

struct CeArgs {
    float* logits;            // (N,V) in: logits, out (if dlogits): (softmax - onehot) * scale
    const int32_t* gold;      // (T,B) flat
    const int32_t* cidx;      // (N) -> flat (t,b)
    const int32_t* n_dev;     // real N
    int n_max, V;
    int write_grad; float inv_n;   // scale; <= 0 -> 1 / *n_dev
    float* loss_samp; float* errt_samp; int32_t* pred;   // (N) optional
    float* loss_acc;          // [0] += sum loss_samp
    unsigned short* grad16;   // optional (N,V) bf16: with write_grad the gradient goes HERE (the bf16 GEMM's operand panel) and the logits stay
    int logits16;             // the logits are the fp16 panel the GEMM left IN grad16 (GemmArgs::c16): read from there, overwritten in place by the bf16 gradient
};
// the kernel form softmax_ce launches for a: 0 the register form (V <= 8192), 1 the fp16-panel form (logits16, V <= 8192, V % 8 == 0),
// 2 the streaming form (V > 8192); -1 where softmax_ce refuses the arguments
int softmax_ce_form(const CeArgs& a);
hipError_t softmax_ce(hipStream_t st, const CeArgs& a);
// pred[i] = argmax_j logits[i, j]  (first max), rows < n
hipError_t argmax_rows(hipStream_t st, const float* logits, int32_t* pred, int n, int V);
// sampled decoding (contract: include/argsim_vae.h, avae_decode_sample), as the kernels take it: inv_t = 1 / temperature (1 at
// temperature 0), top_k = 0 keeps every logit, noise = 0 is the plain first maximum (temperature 0 or top_k 1)
struct SampleParams { float inv_t; int top_k; int noise; uint64_t seed; };
// one token per row of logits (n, V) at step t (row index = batch row): pred (n), logp (n, optional); lead (n, optional): the ids fed
// at this step, a row fed eos at t > 0 is finished (token eos, logp 0)
hipError_t sample_rows(hipStream_t st, const float* logits, int n, int V, int t, const SampleParams& sp, const int32_t* lead, int eos,
                       int32_t* pred, float* logp);
// the same with a nucleus (avae_decode_sample_p): 0 < top_p < 1 and sp.noise != 0; the kept set is the smallest prefix of whole tie
// groups of the top-k set (all of V at top_k 0) that holds top_p of its mass in the fixed-point weights of sample_dev.h;
// nkept (n, optional): its size, 0 for a finished row.  V <= 8192 keeps the row in registers, above that it is re-read per pass
hipError_t sample_rows_p(hipStream_t st, const float* logits, int n, int V, int t, const SampleParams& sp, float top_p, const int32_t* lead,
                         int eos, int32_t* pred, float* logp, int32_t* nkept);

// out[n] (+)= sum_m X[m, n]
hipError_t colsum(hipStream_t st, const float* X, int M, int N, int ldx, float* out, const int32_t* m_dev);
hipError_t add3(hipStream_t st, float* out, const float* a, const float* b, const float* c, int64_t n);
hipError_t zero_fill(hipStream_t st, void* p, size_t bytes);      // a plain kernel instead of the runtime's blit (16-byte aligned p, bytes % 4 == 0)

struct AdamArgs { float* p; const float* g; float* m; float* v; int64_t n; float lr_t, b1, b2, eps;
                  const int* skip_if; };   // device word: non-zero -> the update is a no-op (GRU time-out flag)
hipError_t adam_tf(hipStream_t st, const AdamArgs& a);

// ---------------------------------------------------------------- importance-weighted likelihood (score.hip)
// The k draws of B rows go through the decoder in batches: the rows r are cut into blocks of rc, and a block's draws lie behind
// each other (draw-major), so the pair (kk, r) of the block at r0 (rcb = min(rc, B - r0) rows) is row r0 * k + kk * rcb + (r - r0)
// of z and any run of whole draws of one block is one contiguous decoder batch whose row j carries the ids of row r0 + j % rcb.
struct ScoreDraw {
    const float* mu; const float* lv;   // (B, R)
    const float* eps_in;                // optional (k, B, R): overrides stream 4 of the counter generator
    float* eps_out;                     // optional (k, B, R)
    float* z;                           // (k * B, R) in decoder-batch order (above)
    float* lat;                         // (k, B): 1/2 sum_j (z^2 - eps^2 - lv)
    int* err;                           // device word, set to 1 where an eps is not finite
    int k, B, R, rc; uint64_t seed;
};
hipError_t score_draw(hipStream_t st, const ScoreDraw& a);
// dst (n, S) row j = src (rc, S) row j % rc
hipError_t tile_ids(hipStream_t st, int32_t* dst, const int32_t* src, int n, int rc, int S);
// a decoder batch of n rows whose row j carries the ids of row j % rc: ids0 (T, rc) <- lead (T, n) of the first rc rows, tokrow (T, n) <- t * rc + j % rc
hipError_t lead_rows(hipStream_t st, const int32_t* lead, int T, int n, int rc, int32_t* ids0, int32_t* tokrow);
struct ScoreRows {
    const float* loss;                  // per-token cross-entropy, compacted (prep_ids order)
    const int32_t* rank;                // (T, n): compact row of (t, j) or -1
    int T, n, rc, k0, r0, B;            // batch row j = draw k0 + j / rc of row r0 + j % rc
    float* logpx;                       // (k, B) <- -sum_t loss
    int32_t* ntok;                      // optional (B) <- positions summed (written by the rows of draw 0)
};
hipError_t score_rows(hipStream_t st, const ScoreRows& a);
// logw (k, B, optional) = logpx - lat; bound (B) = logsumexp_k logw - log k, the maximum subtracted
hipError_t score_bound(hipStream_t st, const float* logpx, const float* lat, int k, int B, float* logw, float* bound);

// ---------------------------------------------------------------- beam search (beam.hip)
// One token of the search over n sentences of W hypotheses (contract: include/argsim_vae.h, avae_decode_beam); hypothesis (r, w)
// is row r * W + w of every per-row array.  Win = rows a sentence has going INTO the step (1 at the first token, then W).
// beam_rows: per row of logits (rows, V) its W best candidates cum + logp, best first: cand_sc / cand_tok (rows, W), cand_cnt (rows);
// a finished row (fin, optional) offers (cum, eos) alone; cum null: zeros.  W == 1 ranks by the logit itself (the first maximum).
hipError_t beam_rows(hipStream_t st, const float* logits, int rows, int V, int W, const float* cum, const int32_t* fin, int eos,
                     float* cand_sc, int32_t* cand_tok, int32_t* cand_cnt);
struct BeamStep {
    int n, Win, W, eos;
    const float* cand_sc; const int32_t* cand_tok; const int32_t* cand_cnt;       // (n * Win, W) from beam_rows
    const int32_t* fin_in; const int32_t* len_in;                                 // (n * Win) or null (nothing finished, length 0)
    int32_t* lat_parent; int32_t* lat_token; float* lat_cum;                      // (n * W): the step's lattice entry
    float* cum_out; int32_t* fin_out; int32_t* len_out;                           // (n * W)
    int32_t* live;                                                                // [1] += slots not finished after the step
};
hipError_t beam_select(hipStream_t st, const BeamStep& a);
// state_out (L, n * W, D): row r * W + j of layer l <- row r * Win + parent[r * W + j] of hd[l] (n * Win, D)
hipError_t beam_gather(hipStream_t st, const float* const* hd, int L, int n, int Win, int W, int D, const int32_t* parent, float* state_out);
struct BeamEnd {
    int n, W, n_run, steps, eos;
    const int32_t* lat_parent; const int32_t* lat_token; const float* lat_cum;    // (n_run, n * W)
    const float* cum; const int32_t* len;                                         // (n * W) after the last step
    const float* lenpow;                                                          // [len] = len^alpha as fp32, or null: score = cum
    int32_t* out_ids;                                                             // (n, W, steps), ranked best first, eos beyond n_run
    float* score_out; float* cum_out; int32_t* len_out;                           // (n, W) ranked, optional
    int32_t* o_parent; int32_t* o_token; float* o_cum; size_t out_step;           // optional caller lattice, row stride out_step per step
};
hipError_t beam_backtrack(hipStream_t st, const BeamEnd& a);

// ---------------------------------------------------------------- nearest-neighbour search (knn.hip)
// the k best bank rows per query row under a similarity (contract: include/argsim_vae.h, avae_knn): q (n, dim), bank (N, dim) fp32
// row-major, 16-byte aligned, dim a multiple of 4 in 4..1024; out_idx (n, k) int64, out_score (n, k); carry: the outputs hold an
// earlier call's list, merged in.  N <= 2^31 - 256.
struct KnnArgs {
    const float* q; const float* bank;
    int n, N, dim, k, metric;             // metric: 0 dot, 1 cosine, 2 squared Euclidean (negated)
    int64_t idx_base, self_base; int carry;
    int64_t* out_idx; float* out_score;
};
// the launch shape (knn.hip, knn_plan: a pure host function of the problem shape): query tiles of qrows rows, the bank cut into
// `parts` runs of `chunk` rows (row_parts.h), one workgroup per (query tile, part); chunk_opt > 0 caps chunk (option knn_chunk)
struct KnnPlan { int qrows, qtiles, parts, chunk; };
KnnPlan knn_plan(int n, int N, int k, int chunk_opt);
// workspace laid out by the caller (scoring.cpp): the rows' norms qn (n) and bn (N), the parts' lists (n, parts, k)
struct KnnWs { float *qn, *bn; unsigned long long* lists; };
hipError_t knn_search(hipStream_t st, const KnnArgs& g, const KnnPlan& p, const KnnWs& w);

// ---------------------------------------------------------------- aggregate-posterior diagnostics (agg.hip)
// log q(z_i) under the aggregate posterior of N encoded rows (contract: include/argsim_vae.h, avae_agg_logq): z (n, dim), mu and
// lv (N, dim) fp32 row-major, 16-byte aligned, dim a multiple of 4 in 4..1024, 1 <= N <= 2^31 - 256; logq (n); logqx (n) or null,
// the own pair's density where self_base >= 0 (query i's own bank row is self_base + i)
struct AggArgs {
    const float* z; const float* mu; const float* lv;
    int n, N, dim;
    int64_t self_base;
    float* logq; float* logqx;
};
// the launch shape (agg.hip, agg_plan: a pure host function of the problem shape): query tiles of 128 rows, the bank cut into
// `parts` runs of `chunk` rows (row_parts.h), one workgroup per (query tile, part); chunk_opt > 0 caps chunk (option agg_chunk)
struct AggPlan { int qtiles, parts, chunk; };
AggPlan agg_plan(int n, int N, int dim, int chunk_opt);
// parts_ms: workspace laid out by the caller (scoring.cpp), the parts' (max, sum) pairs (parts, n)
hipError_t agg_logq(hipStream_t st, const AggArgs& g, const AggPlan& p, float2* parts_ms);
// out (4, dim) = per dimension over the N rows: mean mu, unbiased variance of mu (0 for N = 1), mean exp(lv), mean KL term; sums in
// double, fixed order.  Workspace laid out by the caller: mean (dim) and part (moments_blocks(N), 3, dim) doubles
int moments_blocks(int N);
hipError_t latent_moments(hipStream_t st, const float* mu, const float* lv, int N, int dim, float* out, double* mean, double* part);

// ---------------------------------------------------------------- linear probes of latent rows (probe.hip)
// P independent L2 (avae_probe_fit) or L1 (avae_probe_fit_l1) logistic regressions over x (N, dim) in lockstep (contract:
// include/argsim_vae.h).  The host loops (probing.cpp) string these launches together; every buffer is workspace laid out by the caller.
constexpr int kProbeTile = 32;        // problems per tile: P is padded to it with zero-cost problems
constexpr int kProbeAlphas = 7;       // step lengths one probe_trial launch evaluates
constexpr int kProbeMaxParts = 256;
// the launch shape (probe.hip, probe_plan: a pure host function of the problem shape): problem tiles of 32, the rows cut into
// `parts` runs of `chunk` rows, one workgroup per (part, problem tile); chunk_opt > 0 caps chunk (option probe_chunk).  parts and
// chunk do not depend on P.  LD = dim + 4: the row stride of a problem's vectors, the bias at [dim]
struct ProbePlan { int ptiles, Ppad, LD, parts, chunk; };
ProbePlan probe_plan(int N, int P, int dim, int chunk_opt);
struct ProbeWs {
    float *sT, *z, *D, *u;            // (N, Ppad): signed costs, decisions x~ w, curvature, x~ p
    float *W, *G, *Dv, *Rv, *Pv;      // (Ppad, LD), ONE run of 5 Ppad LD floats: iterate, gradient, CG direction, CG residual, Newton step
    float *gp, *lp;                   // (parts, LD, Ppad) and (parts, Ppad): the parts' partials of a pass
    double* tp;                       // (parts, kProbeAlphas, Ppad): the parts' trial loss sums
    int* is; float* fs; double* ds;   // (Ppad, 8) each: per-problem state words (probe.hip)
    int N, dim, LD, Ppad, parts, chunk;
    // the L1 fit alone (null in the L2 fit):
    float *Yv, *Hd, *Hy;              // (Ppad, LD), one run: the FISTA point y, H d of the last accepted d, H y
    float* xs;                        // (N, dim): x with the rows that are not finite zeroed
};
struct ProbeAlphas { int n, last; float a[kProbeAlphas]; };      // a trial round: its step lengths; last: no round follows
hipError_t probe_prepare(hipStream_t st, const ProbeWs& b, const float* s, int P);                 // state of a fresh fit, s (P, N) -> sT
hipError_t probe_pass(hipStream_t st, const ProbeWs& b, const float* x, int mode);                 // 0 GRAD (W), 1 HV (Dv), 2 PANEL (Pv -> u)
hipError_t probe_vec(hipStream_t st, const ProbeWs& b, int P, int phase, int k, int max_newton, int max_cg, float tol, const ProbeAlphas& al);
hipError_t probe_trial(hipStream_t st, const ProbeWs& b, const ProbeAlphas& al);
hipError_t probe_finish(hipStream_t st, const ProbeWs& b, int P, float* w, float* stats);
// the L1 fit (avae_probe_fit_l1) runs probe_pass, probe_trial and probe_finish as they are, on b.xs, with Dv the FISTA candidate and Pv
// the accepted step; its own launches: the state of a fresh fit (probe_prepare + xs), the curvature column sums into gp, and the
// per-problem vector kernel (phase 0 after GRAD, 3 after probe_l1_curv, 1 after the k-th HV pass, 2 after trial round k)
hipError_t probe_l1_prepare(hipStream_t st, const ProbeWs& b, const float* x, const float* s, int P);
hipError_t probe_l1_curv(hipStream_t st, const ProbeWs& b);
hipError_t probe_l1_vec(hipStream_t st, const ProbeWs& b, int P, int phase, int k, int max_newton, int max_inner, float tol, const ProbeAlphas& al);
// out (n, P) = x~ w^T; W: (Ppad, LD) floats of workspace
hipError_t probe_decision(hipStream_t st, const ProbePlan& p, const float* x, int n, int dim, const float* w, int P, float* W, float* out);

// ---------------------------------------------------------------- Ward clustering of latent rows (ward.hip)
// G independent groups per call (contract: include/argsim_vae.h, avae_ward).  A group's buffers are workspace laid out by the caller
// (clustering.cpp); the descriptors themselves live in device memory.
constexpr int kWardOneWgMax = 128;    // planner: the one-workgroup form up to this many rows in the largest group (where the two forms were measured to cross)
struct WardGroup {
    int off, n, mrg, pad;             // first row of x, rows, first merge row of pair / delta / size (= off - g)
    float* D;                         // (n, n): [i][j], i < j, the stored pair values
    double* S;                        // (n, dim) sums of member rows
    int* cnt;                         // (n) member counts, 0 = retired
    unsigned long long* nn;           // (n) nearest-neighbour cache words (ward.hip)
    int* st;                          // (4) the last merge (a, b)
};
struct WardCutGroup { int off, n, mrg, m; };      // m: merges to replay (n - k)
hipError_t ward_init(hipStream_t st, const WardGroup* gs, int G, int nmax, const float* x, int dim);      // sums, counts, every pair value, the row caches
hipError_t ward_tree(hipStream_t st, const WardGroup* gs, int G, int nmax, int dim, int32_t* pair, float* delta, int32_t* size);      // one-workgroup form: all merges
hipError_t ward_round(hipStream_t st, const WardGroup* gs, int G, int nmax, int dim, int t, int32_t* pair, float* delta, int32_t* size);      // launch-per-merge form: merge t of every group
hipError_t ward_cut(hipStream_t st, const WardCutGroup* gs, int G, int nmax, const int32_t* pair, int32_t* p /* (N) workspace */, int32_t* label);

// ---------------------------------------------------------------- affinity propagation of latent rows (affinity.hip)
// One set of N rows per call (contract: include/argsim_vae.h, avae_affinity).  The buffers are workspace laid out by the caller
// (clustering.cpp), or the caller's own s_out / a / r; the state is zero-filled before the first launch.
constexpr int kApMaxN = 1 << 14;
constexpr int kApMaxRB = 16;          // rows per workgroup of the row passes: ap_row_block(N) <= this for N <= kApMaxN
struct ApState {
    int stop_at;                      // 0: running; it + 1: iteration it ended the loop (a launch of a later iteration returns at once)
    int iters, conv, K;               // iterations run, converged, exemplars of the last iteration run
    int cnt[2][2];                    // by iteration parity: columns whose run is shorter than convergence_iter, exemplars
    float pref;                       // the median, where the call asks for it
    unsigned prefix[2], rank[2];      // radix select of the two middle ranks
    unsigned hist[512];
};
struct ApBuffers {
    float *S, *A, *R;                 // (N, N)
    double* part;                     // (row blocks, N) column sums of max(0, R) over a block's rows i != k
    double* cv;                       // (N) R_kk + the column's sum
    int *E, *run, *E2;                // (N) exemplar flags, run lengths, the refined exemplars
    int32_t* c;                       // (N) the first assignment
    unsigned long long* best;         // (N) per exemplar: (order key of the refinement sum) << 32 | ~j
    ApState* st;
};
int ap_row_block(int N);
hipError_t ap_single(hipStream_t st, int32_t* label, int32_t* stat);                        // N = 1
hipError_t ap_similarity(hipStream_t st, const float* x, int N, int dim, int metric, float* S);
hipError_t ap_prepare(hipStream_t st, float* S, int N, int use_pref, float pref, int noise, uint64_t seed, ApState* state);      // median, diagonal, noise
hipError_t ap_iteration(hipStream_t st, const ApBuffers& b, int N, float lam, int it, int conv_iter);      // three launches
hipError_t ap_labels(hipStream_t st, const ApBuffers& b, int N, int32_t* label, int32_t* stat);

// ---------------------------------------------------------------- exact t-SNE of latent rows (tsne.hip)
// One set of N rows per call (contract: include/argsim_vae.h, avae_tsne).  The buffers are workspace laid out by the caller
// (clustering.cpp) or the caller's own outputs; tsne_init writes the state before the first iteration.
constexpr int kTsneMaxN = 1 << 14;
constexpr int kTsneMaxChunk = 4096;   // columns of a part at most: its slice of y is staged in LDS
struct TsneState {
    int stop_at;                      // 0: running; it + 1: iteration it ended phase 2 (a launch of a later iteration returns at once)
    int phase, best_iter;             // 1 or 2; sklearn's best_iter of the phase
    int last_it, how, p1_last;        // the last iteration run, how phase 2 ended, the last iteration of phase 1 in this call or -1
    int pad[2];
    double best_error, last_err, p1_err;      // sklearn's best_error; the last error computed; the error of phase 1's last iteration
};
struct TsnePlan { int rs, parts, chunk; };      // rows per workgroup, column parts, columns per part of the walks
struct TsneArgs {
    const double* P;                  // (N, N) the joint matrix
    float *y, *upd, *gains;           // (N, 2) each
    float* grad;                      // (N, 2) or null
    double* trace;                    // (2, max_iter) or null
    double *part, *errp;              // (N, parts, 5) pair sums; (N, parts) error sums
    TsneState* st;
    int N, rs, parts, chunk;
    int max_iter, X, exag_iter, nic, nwp;      // X = min(exag_iter, max_iter): phase 1's window
    float lr; double ee, min_gn;
};
TsnePlan tsne_plan(int N, int chunk_opt);
hipError_t tsne_conditionals(hipStream_t st, const float* S /* -D: ap_similarity, metric 0 */, int N, double perplexity, double* C, double* beta);
hipError_t tsne_joint(hipStream_t st, double* P /* the conditionals, in place */, int N, double* rowsum /* (N) workspace */);
hipError_t tsne_init(hipStream_t st, const TsneArgs& a, int it0, int warm, int init, uint64_t seed, const double* prog);
hipError_t tsne_iteration(hipStream_t st, const TsneArgs& a, int it);      // two launches, three where the error may be computed
hipError_t tsne_finish(hipStream_t st, const TsneArgs& a, double* kl, int32_t* stat, double* prog);

// ---------------------------------------------------------------- k-means of latent rows (kmeans.hip)
// One set of N rows and R = n_init restarts side by side per call (contract: include/argsim_vae.h, avae_kmeans).  Every buffer is
// workspace laid out by the caller (clustering.cpp); the state, the labels (-1) and the block histograms (0) are filled before the
// first launch.
constexpr int kKmMaxN = 1 << 22;
constexpr int kKmMaxK = 4096, kKmMaxInit = 64, kKmMaxParts = 16, kKmMaxBlocks = 256, kKmMaxTrials = 10;      // trials: 2 + floor(ln 4096)
constexpr int kKmTile = 64;           // rows of a tile of the distance kernel
constexpr int kKmScanRows = 1024;     // rows of a tile of the seeding's cumulative sum
struct KmState {
    int stop_at;                      // 0: running; it + 1: iteration it ended the restart (a launch of a later iteration returns at once)
    int how, reloc;                   // 0 converged, 1 tol, 2 max_iter; relocations so far
    int changed, nempty;              // this iteration: a label differs from the previous iteration's; empty clusters
    int chosen;                       // seeding: the candidate picked in this round
    int pad[2];
    double tol_abs, total;            // the absolute tolerance; seeding: the sum of the closest distances
};
// tile x parts: the distance kernel's grid; slice: sorted positions per workgroup of the member sums; blk: rows per block of the stable
// counting sort; scan: rows per tile of the seeding's cumulative sum
struct KmPlan { int tile, tiles, parts, chunk, slice, slices, blk, blks, scan, scans; };
struct KmArgs {
    const float* x; const double* rnorm;      // rows; their norms (cosine) or null
    int N, dim, k, R, max_iter, T;    // T: seeding trials per centre
    uint64_t seed;
    KmPlan p;
    KmState* st;                      // (R)
    double* C;                        // (R, k, dim) the centres, updated in place
    double* pd; int* pi;              // (R, parts, N) a part's first minimum per row
    int* lab; double* dist;           // (R, N) labels; distance to the own centre as assigned
    int *hist, *off;                  // (R, blks, k) members per row block; their first position inside the cluster's run
    int* start;                       // (R, k + 1) first sorted position of a cluster
    int* order;                       // (R, N) rows by (label, row)
    double* psum;                     // (R, slices + k, dim) member sums of (slice, cluster) at slice + cluster
    int* rel;                         // (R, k, 3) relocations: row or -1, its cluster, the empty cluster
    double *shiftp, *ipart;           // (R, k) squared shift per centre; (R, tiles) inertia partials
    double *vpart, *mean;             // (kKmMaxBlocks, dim), (dim): the column variance
    int* best;                        // (1) the best restart
    double *closest, *D, *candC, *tsum, *ppart;      // seeding: (R, N); (R, T, N); (R, T, dim); (R, scans); (R, T, scans)
    int* cand;                        // (R, T) candidate rows
};
KmPlan km_plan(int N, int k, int R, int chunk_opt);
hipError_t km_prepare(hipStream_t st, const KmArgs& a, double tol);      // row norms (cosine), the absolute tolerance
hipError_t km_load(hipStream_t st, const KmArgs& a, const float* centers_in);      // the given start as doubles into C
hipError_t km_seed(hipStream_t st, const KmArgs& a);                     // greedy k-means++ into C: five launches per centre
hipError_t km_iteration(hipStream_t st, const KmArgs& a, int it);        // seven launches
hipError_t km_finish(hipStream_t st, const KmArgs& a, int32_t* label, float* centers, int32_t* stat, double* inertia, int32_t* label_all,
                     double* centers_all, int32_t* stat_all);

// ---------------------------------------------------------------- Gaussian mixture of latent rows (gmm.hip)
// One set of N rows and R = n_init restarts side by side per call (contract: include/argsim_vae.h, avae_gmm_fit).  Every buffer is
// workspace laid out by the caller (clustering.cpp); the state is zero-filled before the first launch.
constexpr int kGmMaxN = 1 << 22, kGmMaxK = 1024, kGmMaxInit = 16, kGmMaxParts = 16, kGmMaxSlices = 256;
constexpr int kGmTile = 64;           // rows of a tile of the E and M kernels
constexpr int kGmMB = 16;             // components of a workgroup of the M kernel
struct GmState {
    int done, iters, how, pad;        // done: a launch of a later iteration returns at once; how: 0 converged, 1 max_iter, 2 degenerate
    double prev, lower;               // the previous iteration's bound; the last one's (-inf for a degenerate restart)
};
// tile x parts: the E kernel's grid (chunk components per part); slice rows per workgroup of the M kernel
struct GmPlan { int tile, tiles, parts, chunk, slice, slices, blks; };
struct GmArgs {
    const float* x;
    int N, dim, k, R, max_iter, spherical;
    int dreal;                        // dim less the padding columns (option gmm_pad): those have variance 1 and no share in the constants
    double tol, reg;
    GmPlan p;
    GmState* st;                      // (R)
    double *W, *MU, *COV;             // (R, k), (R, k, dim) x 2: the parameters, updated in place
    double *PREC, *HLD, *LC;          // (R, k, dim) 1 / cov; (R, k) half the sum of log cov; (R, k) the constant of t_ic
    double* NC; int* bad;             // (R, k) n_c; a variance of the component is <= 0 or not finite
    double *pm, *ps, *pt; int* pi;    // (R, parts, N) a part's running (max, sum), its first maximum of t
    double* lse;                      // (R, N)
    double* bpart;                    // (R, blks) the bound's partials over blocks of 256 rows
    double* mpart;                    // (R, slices, k, 2 dim + 1) the M-step's partials: sum r, sum r x (dim), sum r x^2 (dim)
    int* best;                        // (1) the best restart
    double* trace;                    // (R, max_iter) the caller's, or null
};
GmPlan gm_plan(int N, int k, int R, int chunk_opt);
// the given parameters into restart slots 0 .. R - 1 with what the E-step derives from them; check: a bad variance ends the restart
hipError_t gm_load(hipStream_t st, const GmArgs& a, const double* w, const double* mu, const double* cov, int check);
hipError_t gm_start_labels(hipStream_t st, const GmArgs& a, const int32_t* label_in);      // init 0: one-hot responsibilities, one M-step
hipError_t gm_iteration(hipStream_t st, const GmArgs& a, int it);        // five launches: E, merge, M, parameters, decide
hipError_t gm_pick(hipStream_t st, const GmArgs& a, int32_t* stat, double* lower, int32_t* stat_all);
// the E-step of restart *a.best (all: of slot 0) under its parameters -> logp, label, resp (each may be null)
hipError_t gm_final(hipStream_t st, const GmArgs& a, double* logp, int32_t* label, double* resp);
hipError_t gm_copy(hipStream_t st, const GmArgs& a, double* weights, double* means, double* covars, double* weights_all, double* means_all,
                   double* covars_all);

// ---------------------------------------------------------------- cluster-quality scores of latent rows (silhouette.hip)
// One set of N rows and L labelings per call (contract: include/argsim_vae.h, avae_silhouette).  Every buffer is workspace laid out by
// the caller (clustering.cpp) or the caller's own output; the counts are zero-filled before the first launch.
constexpr int kSilMaxN = 1 << 18, kSilMaxK = 4096, kSilMaxL = 64;
constexpr int kSilLds = 160 * 1024;   // the LDS one workgroup may take on gfx950
constexpr int kSilTJ = 64;            // columns of a tile of the pair pass
constexpr int kSilDK = 32;            // row elements per LDS stage
// TI rows x TJ columns per tile; the labelings [begin[p], begin[p + 1]) form pass p, whose launch takes bytes[p] of LDS
struct SilPlan { int TI, TJ, npass; int begin[kSilMaxL + 1]; int bytes[kSilMaxL]; };
struct SilArgs {
    const float* x; const double* rnorm;      // rows; their norms (cosine) or null
    const int32_t* label;             // (L, N)
    const int* meta;                  // K (L), then the prefix sums of K (L + 1): where a labeling's clusters start in the (sum K) buffers
    int N, dim, L, metric, Kmax;
    int* cnt;                         // (sum K) members
    double* s;                        // (L, N) silhouette values: the caller's sil, or workspace
    double* ab; int32_t* nearest;     // (L, N, 2), (L, N) or null
    // CH and DB only
    double *msum, *gmean;             // (sum K, dim) member sums, then means; (L, dim) the mean of the labelled rows
    double *e, *r;                    // (L, N) squared distance of a row to its cluster's mean, and its root
    double *Sc, *dbp;                 // (sum K) mean distance to the mean; the largest R of a cluster
    double* tr;                       // (L, 4) trW, trB, non-empty clusters, labelled rows
};
// staging bytes of a pass of nl labelings at TI rows (the bins come on top: TI x sum K x 8)
size_t sil_staging(int TI, int nl);
SilPlan sil_plan(int N, int dim, int L, const int32_t* K, int chunk_opt, int cus);
hipError_t sil_prepare(hipStream_t st, const SilArgs& a);                  // row norms (cosine), the counts
hipError_t sil_pairs(hipStream_t st, const SilArgs& a, const SilPlan& p);  // one launch per pass: s, ab, nearest
hipError_t sil_scores(hipStream_t st, const SilArgs& a, double* score, int32_t* count, double* cluster_mean);
hipError_t sil_indices(hipStream_t st, const SilArgs& a, double* index);   // six launches: CH and DB

// ---------------------------------------------------------------- density clustering of latent rows (dbscan.hip)
// One set of N rows per call (contract: include/argsim_vae.h, avae_dbscan).  Every buffer is workspace laid out by the caller
// (clustering.cpp) or the caller's own output; count, flag and st are zero-filled before the first launch.
constexpr int kDbMaxN = 1 << 17;      // the bit matrix adj[N][ceil(N / 64)] is 2 GiB there
constexpr int kDbTJ = 64;             // columns of a tile of the pair pass: one 64-bit word of adjacency per row
constexpr int kDbDK = 32;             // row elements per LDS stage
constexpr int kDbMaxParts = 65535;    // column parts of the pair pass (grid.y)
constexpr int kDbMaxRounds = 4096;    // of hook and jump
// the default max_rounds is 2 (kDbRoundA ceil(log2 N) + kDbRoundB): twice the fit of tests/dbscan_ref.py's model
constexpr int kDbRoundA = 1, kDbRoundB = 1;
// a workgroup owns TI rows and the column tiles [part * chunk, part * chunk + chunk) of the W = ceil(N / 64)
struct DbPlan { int TI, rtiles, parts, chunk, W, lds, rounds; };
struct DbState { int rounds, nclusters, bad, pad; };
struct DbArgs {
    const float* x; const double* rnorm;      // rows; their norms (cosine) or null
    int N, dim, W, min_samples;
    double thr;                               // a pair is within eps iff p <= thr: eps^2, for the cosine 2 eps
    unsigned long long* adj;                  // (N, W) bit j % 64 of word j / 64 of row i: p(i, j) <= thr
    unsigned long long* cmask;                // (W) the core rows as bits
    int32_t* count;                           // (N) rows within eps, the row itself included: the caller's, or workspace
    int* par[3];                              // (N) each: the parents, and the two arrays the hooks write in turn
    int* num;                                 // (N) a root's cluster number
    int* flag;                                // (max_rounds + 1) flag[t]: round t has work (flag[0] is set by db_core)
    DbState* st;
    int32_t* label;
};
size_t db_pairs_lds(int TI);
DbPlan db_plan(int N, int dim, int chunk_opt, int cus);
hipError_t db_prepare(hipStream_t st, const DbArgs& a);                  // row norms (cosine)
hipError_t db_pairs(hipStream_t st, const DbArgs& a, const DbPlan& p);   // the bit matrix and the counts
hipError_t db_core(hipStream_t st, const DbArgs& a);                     // the core mask, parent[i] = i
hipError_t db_round(hipStream_t st, const DbArgs& a, int t);             // two launches: hook, jump
hipError_t db_finish(hipStream_t st, const DbArgs& a, int32_t* stat);    // verify, number, label, border, stat

// ---------------------------------------------------------------- principal components of latent rows (pca.hip)
// One set of N rows per call (contract: include/argsim_vae.h, avae_pca_fit / avae_pca_transform).  Every buffer is workspace laid out by
// the caller (clustering.cpp) or the caller's own output; st is zero-filled before the first launch.
constexpr int kPcaMaxN = 1 << 22;
constexpr int kPcaT = 64;             // columns of a covariance tile
constexpr int kPcaDK = 16;            // rows per LDS stage of the covariance
constexpr int kPcaResident = 128;     // the largest dreal whose matrix one workgroup keeps in LDS (128 KB of the 160)
constexpr int kPcaMaxSweeps = 256;
// the default max_sweeps: twice the most sweeps tests/pca_ref.py's model of the rule takes over the test cases and a 1024-column case
// (tests/test_pca.py measures it again)
constexpr int kPcaSweeps = 58;
struct PcaPlan { int dreal, tiles, pairs, rows, chunks, form, rounds, sweeps, launches, lds, trows; };
struct PcaState { double thr; int sweeps, converged, rotations, done, rot_sweep, pad; };
struct PcaArgs {
    const float* x; int N, dim, dreal;
    double* msum;                             // (chunks, dim) column sums of the row chunks
    double* mean;                             // (dim) the caller's: the leading dreal are written, and read by the covariance
    double* part;                             // (chunks, pairs, 64, 64) partial tiles of the covariance
    double* A[2];                             // (dreal, dreal) the matrix; the launched solve writes the two in turn
    double* Vt[2];                            // (dreal, dreal) row j = column j of the accumulated rotations
    PcaState* st;
};
size_t pca_resident_lds(int dreal);
PcaPlan pca_plan(int N, int dim, int pad, int chunk_opt, int form_opt, int cus);
hipError_t pca_cov(hipStream_t st, const PcaArgs& a, const PcaPlan& p);                      // mean and covariance: four launches
hipError_t pca_solve(hipStream_t st, const PcaArgs& a, const PcaPlan& p, int max_sweeps);    // init, then one launch or one per round
hipError_t pca_finish(hipStream_t st, const PcaArgs& a, const PcaPlan& p, double* var, double* comp, int32_t* stat);
hipError_t pca_transform(hipStream_t st, const float* x, int n, int dim, const double* mean, const double* comp, const double* scale, int k,
                         float* y, int trows);

// ---------------------------------------------------------------- kernel two-sample test of latent rows (mmd.hip)
// One set of N rows, G comparisons of 1 + P relabelings per call (contract: include/argsim_vae.h, avae_mmd / avae_mmd_relabel).  Every
// buffer is workspace laid out by the caller (scoring.cpp) or the caller's own output.
constexpr int kMmdMaxN = 1 << 17, kMmdMaxG = 64, kMmdMaxQ = 16384, kMmdMaxBw = 8;
constexpr int kMmdLds = 160 * 1024;   // the LDS one workgroup may take on gfx950
constexpr int kMmdDK = 32;            // row elements per LDS stage
// TI rows x 64 columns per tile; pass q covers the relabelings [q nq, q nq + nq) of the G (1 + P); cap = the most slots (relabelings +
// their comparisons) of a pass; lds = the most LDS bytes of a pass
struct MmdPlan { int TI, nq, npass, tiles, W, cap, lds; };
struct MmdArgs {
    const float* x; const double* rnorm;      // rows; their norms (cosine) or null
    const unsigned long long* valid;          // (G, W)
    const unsigned long long* inA;            // (G, 1 + P, W)
    int N, dim, W, G, P, kernel, nbw, cap;
    double gamma[kMmdMaxBw];
    double* part;                             // (row tiles, 2, cap) the row tiles' sums of a pass: A side, B side
    double* sums;                             // (G, 1 + P, 2) U_AA, U_BB: the caller's, or workspace
    double* ull;                              // (G) U_LL: the caller's, or workspace
    const int* counts;                        // (G, 2) m, n of relabeling 0
    double* witness;                          // (G, N) or null
};
size_t mmd_lds(int TI, int slots, int W);
size_t mmd_pass_lds(const MmdPlan& p, int q0, int nq, int P);
MmdPlan mmd_plan(int N, int dim, int G, int P, int chunk_opt, int cus);
hipError_t mmd_relabel(hipStream_t st, const unsigned long long* valid, unsigned long long* inA, int N, int G, int P, uint64_t seed);
hipError_t mmd_prepare(hipStream_t st, const MmdArgs& a, int* counts);     // row norms (cosine), m and n
hipError_t mmd_pairs(hipStream_t st, const MmdArgs& a, const MmdPlan& p);  // two launches per pass: sums, ull
hipError_t mmd_witness(hipStream_t st, const MmdArgs& a, const MmdPlan& p);
hipError_t mmd_stats(hipStream_t st, const MmdArgs& a, double* stat, double* pvalue, unsigned* bad, int32_t* stat_out);

// ---------------------------------------------------------------- greedy decoding (decode.hip)
// the whole loop of model.py:204-219 in one persistent launch; every pointer is device memory
struct DecodeArgs {
    const float* E;                                 // (V, D) tied embedding
    const float *W[8], *R[8], *bW[8], *bR[8];       // decoder GRU layers, G16 row order
    const float *Kout, *bout;                       // out affine: kernel (D, D) as (in, out), bias (D)
    float* state[2];                                // ping-pong (L, b, D); [0] holds state_in on entry
    float* o;                                       // (b, D)
    float* part_val; int32_t* part_idx;             // (G, b) partial argmax per workgroup, G = CU count
    int32_t* ids_tm;                                // (steps + 1, b) time-major ids; row 0 = bos on entry
    int32_t* out_ids;                               // (b, steps) result, eos beyond the kept tokens
    int32_t* kept;                                  // [0] <- tokens kept per row
    unsigned* bar;                                  // grid-barrier counter, zero on entry
    int* err;                                       // error word (spin time-out)
    int b, steps, D, V, L, eos, cache_e; float isd;
    // decode_sample only
    SampleParams sp;
    float *part_x, *part_m, *part_s;                // (G, b) per workgroup: l inv_t of its candidate, running (max, sum exp) of l inv_t
    float* logits;                                  // (b, V), top_k > 0: the step's logits for the row's owner
    float* logp_tm;                                 // (steps, b) time-major log-probabilities, or null
    float* logp_out;                                // (b, steps) result, 0 beyond a row's eos, or null
    // nucleus (decode_sample with 0 < top_p < 1) only
    float top_p;
    int32_t* nkept_tm;                              // (steps, b) time-major sizes of the kept sets, or null
    int32_t* nkept_out;                             // (b, steps) result, 0 where the row had finished, or null
};
// The geometry of one launch of kMode `mode` over G workgroups with lds_max bytes of LDS each: nu = hidden units and vp = vocabulary
// rows per workgroup, cache_e = the workgroup's embedding rows lie in LDS behind the weights (else the logits phase reads E from
// global memory), lds_bytes = the dynamic LDS of the launch.  ok = 0: the launchers refuse (D / G > 2 units per workgroup, L > 8,
// D > 512 or no multiple of 4, the weights alone exceed lds_max, mode < 0).  Host arithmetic only.
struct DecodePlan { int ok, mode, nu, vp, cache_e, lds_bytes, G, lds_max; };      // (G, lds_max: what it was planned for)
DecodePlan decode_plan(int mode, int D, int V, int L, int G, int lds_max);
// the kMode of a call: 0 greedy; sampled: 1 every logit kept (top_k 0 or >= V), 2 top-k, 3 nucleus; -1: top-k or nucleus with V > 8192
int decode_mode(bool sampled, int V, int top_k, bool nucleus);
// G (the CU count: the size of part_val / part_idx rows) and lds_max of the current device as the launchers take them
hipError_t decode_device(int* G, int* lds_max);
// returns hipErrorInvalidValue where decode_plan refuses, the caller runs one launch sequence per token instead (it asks
// decode_plan first); *grid_out = workgroups launched
hipError_t decode_greedy(hipStream_t st, DecodeArgs a, int* grid_out);
// the sampled loop in the same persistent form (a.sp; finished rows emit eos).  Also refuses top_k > 0 or top_p > 0 with V > 8192
hipError_t decode_sample(hipStream_t st, DecodeArgs a, int* grid_out);

// natural <-> G16 row permutation of a (3D, cols) matrix (cols = 1 for biases)
hipError_t g16_permute(hipStream_t st, float* dst, const float* src, int D, int cols, bool to_g16);

// losses[0..2] = loss_gen, loss_kld, loss (model.py:181-185) from the per-token CE (n = min(n_max, *n_dev) entries) and the
// per-element KL terms (nk entries, each floored at free_bits), summed in a fixed order: bit-reproducible
hipError_t finalize_losses(hipStream_t st, float* losses, const float* loss_samp, const int32_t* n_dev, int n_max,
                           const float* kld, int nk, float free_bits, float inv_br, float anneal);

}  // namespace avae
