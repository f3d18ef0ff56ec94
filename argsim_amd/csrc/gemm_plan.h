// gemm_plan.h -- which launches one GEMM product makes, decided from its shape alone (gemm_plan.cpp).  Plain C++: no HIP, no
// handle, no pointer, no environment -- the decision is a value that can be printed and tested without a device
// (avae_debug_gemm_plan, tests/test_gemm_plan.py).
#pragma once

namespace avae {

struct GemmShape {
    bool a_mc, b_nc;          // operand layouts as in GemmArgs
    int M, N, K, ldc;
    int accumulate;
    int split_k;              // a caller's own K split; 0: the plan decides
    int thin;                 // a caller's own tile form (GemmArgs::thin); -1: the plan decides
    int dyn_kind, dyn_expect; // device-side count: 1 rows / 2 K, and what the host expects it to be (0 = unknown)
    bool allow_atomic;        // backward: float atomics into the output are acceptable
    bool rows_are_batch;      // forward: the rows are the batch rows -- the tile form must not depend on how many there are
    bool pair;                // a second problem of the same shape rides in the launch (GemmArgs::A2)
    bool wgrad;               // weight gradient: C += A^T B over K rows, into the zero-filled gradient
    int compute_dtype;        // avae_config::compute_dtype
    bool skinny, dyn_split, dyn_thin;      // the options of the same names
};
enum GemmZero { kZeroNone = 0, kZeroAll = 1, kZeroDynRows = 2 };      // what of the launch's output rows is cleared beforehand: nothing, all, the first *dyn
struct GemmLaunch {
    int row0, rows;           // rows [row0, row0 + rows) of A and C
    int thin, split_k, accumulate;
    int zero;                 // GemmZero
    int dyn;                  // 1: the device-side count applies to this launch; 0: its static bound
};
struct GemmPlan { int n; GemmLaunch launch[2]; };
GemmPlan gemm_plan(const GemmShape& s);

// bf16 mode: does a weight gradient of this shape read both operands row-major through the transposing-LDS-load GEMM (gemm_bf16_tn)?
bool gemm_tn16_shape(int M, int N);
// bf16 layer: K slices of the 256x256-tile kernels for a caller's split_k over `big_tiles` such tiles (bk: their K tile)
int gemm_bf16_slices(int split_k, int big_tiles, int K, int bk);
// bf16 layer: do 256x256 tiles fill the chip, by themselves or through `slices` K slices?
bool gemm_bf16_big_fills(int M, int N, int big_tiles, int slices);

}  // namespace avae
