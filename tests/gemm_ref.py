"""The contract of GemmArgs (argsim_amd/csrc/kernels.h) in plain numpy, and the buffers a GEMM test hands to the device.

    C[:M_eff, :N] = alpha * op(A)[:M_eff, :K_eff] @ op(B)[:K_eff] (+ bias) (+ C0 if accumulate or a K split)

M_eff = min(M, count) under dyn_kind 1, K_eff = min(K, count) under dyn_kind 2; everything else of the C buffer keeps its bits.

build(case) lays the operands out as the model does: leading dimensions wider than the contiguous extent (+ PAD floats), guard rows behind
the last row, and NaN in every float that is not part of the logical operand -- the pad columns, the guard rows, under dyn_kind 1 the rows
of A from the count on, under dyn_kind 2 the rows of a [k][x] operand from the count on (a k-contiguous operand keeps finite values at
k >= count: they are part of rows the kernel does read).  C carries SENT, a NaN with a fixed payload, outside the logical result and in
it too unless the kernel adds into it (accumulate: C0; a K split without accumulate: zeros).

Two data classes.  'exact': operands from {-4..4} without 0, bias and C0 integers, alpha in {1, 0.5, -2}: every partial sum in any order
is a multiple of 1/2 below 2^23, so every kernel family -- the three-way bf16 split, bf16 operands (these integers are exact in bf16), float
atomics -- must return the bits of the exact result; build() asserts the condition.  'rounding': wide-range normal draws, checked against
bound()."""
import dataclasses

import numpy as np

PAD = 8                      # floats between the contiguous extent and the leading dimension
OP_GUARD_ROWS = 2            # NaN rows behind an operand
C_GUARD_ROWS = 4             # sentinel rows behind C
SENT = np.int32(0x7FC5A5A5)  # a quiet NaN with a payload no arithmetic produces
U = 2.0 ** -24               # unit roundoff of fp32
ALPHAS = (1.0, 0.5, -2.0)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    a_mc: int
    b_nc: int
    M: int
    N: int
    K: int
    thin: int = 0
    split_k: int = 1
    alpha: float = 1.0
    bias: bool = False
    accumulate: int = 0
    dyn_kind: int = 0
    count: int = -1           # the device-side count (dyn_kind != 0)
    expect: int = 0           # what the host is told to expect of it
    pair: bool = False
    data: str = 'exact'
    plain_out: bool = False   # ldc = N instead of N + PAD
    reach: tuple = None       # (tile, fast, db, persist) the case claims of gemm_f32_form; None: another kernel family
    dtype: int = 0            # compute_dtype of the handle it runs on
    seed: int = 0
    # ---- 16-bit operands (bf16 mode): see operand16()
    route: int = -1           # avae_debug_gemm16's route (0 gemm_bf16_pre, 1 gemm_tn16); -1: fp32 operands through the other hooks
    ops16: str = ''           # which operands go over as bf16 the way a producer wrote them: 'a', 'b' or 'ab'
    wgrad: int = 0            # route 0: the call is a weight gradient (the plan's K split, C holds the value to add onto)
    nt8: int = 1              # the handle's option bf16_nt8 the case runs with
    round16: bool = False     # the draws are rounded to bf16 (RNE) on the host: both operand forms then hold the same values
    reach16: tuple = None     # (kernel, slices, slab) the case claims of avae_debug_gemm_bf16_form

    @property
    def M_eff(self):
        return min(self.M, self.count) if self.dyn_kind == 1 else self.M

    @property
    def K_eff(self):
        return min(self.K, self.count) if self.dyn_kind == 2 else self.K

    @property
    def lda(self):
        return (self.M if self.a_mc else self.K) + PAD

    @property
    def ldb(self):
        return (self.N if self.b_nc else self.K) + PAD

    @property
    def ldc(self):
        return self.N + (0 if self.plain_out else PAD)

    @property
    def lda16(self):
        """leading dimension of A as a producer's bf16 array: [k][m] twice the logical width (route 1: the logical columns are the SECOND half, as one
        direction's dgh16 out of the 6 D wide array; route 0: + 8), k-contiguous (the panel itself) twice K"""
        return (2 * self.M if self.route == 1 else self.M + PAD) if self.a_mc else 2 * self.K

    @property
    def off16(self):
        return self.M if self.a_mc and self.route == 1 else 0

    @property
    def ldb16(self):
        return self.N + PAD

    @property
    def id(self):
        return '%s-%d%d-%dx%dx%d' % (self.name, self.a_mc, self.b_nc, self.M, self.N, self.K)


def case(name, lay, M, N, K, **kw):
    """a Case with the contiguous extents of [k][x] operands rounded up to 4 floats"""
    a_mc, b_nc = lay
    if a_mc:
        M = (M + 3) // 4 * 4
    if b_nc:
        N = (N + 3) // 4 * 4
    return Case(name, a_mc, b_nc, M, N, K, **kw)


@dataclasses.dataclass
class Problem:
    """one problem's host buffers: A, B, C as the device gets them (2-D, float32, row stride = leading dimension), bias or None, and the
    logical operands a (M, K), b (K, N) in float64"""
    A: np.ndarray
    B: np.ndarray
    C: np.ndarray
    bias: np.ndarray
    a: np.ndarray
    b: np.ndarray


def sentinel(shape):
    return np.full(shape, SENT, np.int32).view(np.float32)


def _operand(logical, x_contig):
    """logical: (X, K).  -> the padded buffer, [k][x] where x_contig else [x][k], NaN outside the logical operand"""
    src = logical.T if x_contig else logical
    buf = np.full((src.shape[0] + OP_GUARD_ROWS, src.shape[1] + PAD), np.nan, np.float32)
    buf[:src.shape[0], :src.shape[1]] = src
    return buf


def _draw(rng, shape, data):
    if data == 'exact':
        return (rng.integers(1, 5, shape) * rng.choice((-1, 1), shape)).astype(np.float64)
    return (rng.standard_normal(shape) * np.exp(rng.standard_normal(shape))).astype(np.float32).astype(np.float64)


def _draw_add(rng, shape, data):
    if data == 'exact':
        return rng.integers(-8, 9, shape).astype(np.float64)
    return rng.standard_normal(shape).astype(np.float32).astype(np.float64)


def exact_limit(c):
    """the largest magnitude any partial result of an 'exact' case can reach, from the case alone: it must stay below 2^23 (multiples of 1/2)"""
    return abs(c.alpha) * 16.0 * c.K + 8.0 + 8.0


def build(c):
    """-> [Problem] (two of them for a pair), deterministic in the case"""
    assert c.data in ('exact', 'rounding') and (c.data != 'exact' or c.alpha in ALPHAS)
    assert (c.dyn_kind != 0) == (c.count >= 0)
    rng = np.random.default_rng([c.M, c.N, c.K, c.a_mc, c.b_nc, c.thin, c.split_k, c.seed])
    out = []
    for _ in range(2 if c.pair else 1):
        a, b = _draw(rng, (c.M, c.K), c.data), _draw(rng, (c.K, c.N), c.data)
        if c.round16:
            a, b = bf16_round(a), bf16_round(b)
        A, B = _operand(a, c.a_mc), _operand(b.T, c.b_nc)
        if c.dyn_kind == 1:
            if c.a_mc:
                A[:, c.M_eff:] = np.nan
            else:
                A[c.M_eff:] = np.nan
        if c.dyn_kind == 2:
            if c.a_mc:
                A[c.K_eff:] = np.nan
            if c.b_nc:
                B[c.K_eff:] = np.nan
        bias = _draw_add(rng, c.N, c.data).astype(np.float32) if c.bias else None
        C = sentinel((c.M + C_GUARD_ROWS, c.ldc)).copy()
        if c.accumulate:
            C[:c.M, :c.N] = _draw_add(rng, (c.M, c.N), c.data)
        elif c.split_k > 1:
            C[:c.M, :c.N] = 0.0
        p = Problem(A, B, C, bias, a, b)
        if c.data == 'exact':
            assert 2.0 * magnitude(c, p).max(initial=0.0) < 2.0 ** 24, c
        out.append(p)
    return out


def _adds_into(c):
    return bool(c.accumulate) or c.split_k > 1


def magnitude(c, p):
    """|alpha| |a| |b| + |bias| + |C0| over the logical result: what every rounding of the computation is relative to"""
    m = abs(c.alpha) * (np.abs(p.a[:c.M_eff, :c.K_eff]) @ np.abs(p.b[:c.K_eff]))
    if p.bias is not None:
        m = m + np.abs(p.bias.astype(np.float64))
    if _adds_into(c):
        m = m + np.abs(p.C[:c.M_eff, :c.N].astype(np.float64))
    return m


def product(c, p, a=None, b=None):
    """the logical result in float64 (exact for the 'exact' class: integers far below 2^53)"""
    a = p.a if a is None else a
    b = p.b if b is None else b
    r = c.alpha * (a[:c.M_eff, :c.K_eff] @ b[:c.K_eff])
    if p.bias is not None:
        r = r + p.bias.astype(np.float64)
    if _adds_into(c):
        r = r + p.C[:c.M_eff, :c.N].astype(np.float64)
    return r


def reference(c, problems=None):
    """-> per problem the expected FULL C buffer (float32; guard rows, pad columns and the rows from M_eff on as build() left them)"""
    problems = build(c) if problems is None else problems
    out = []
    for p in problems:
        want = p.C.copy()
        r = product(c, p)
        r32 = r.astype(np.float32)
        if c.data == 'exact':
            assert np.array_equal(r32.astype(np.float64), r), c
        want[:c.M_eff, :c.N] = r32
        out.append(want)
    return out


def untouched(c, got, before):
    """indices of the floats outside the logical result whose bits moved"""
    g, w = got.view(np.int32).copy(), before.view(np.int32).copy()
    g[:c.M_eff, :c.N] = 0
    w[:c.M_eff, :c.N] = 0
    return np.argwhere(g != w)


def bf16_round(x):
    """float64 / float32 values -> rounded to bf16 (RNE), as float64"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


NAN16 = np.uint16(0x7FC1)     # a bf16 NaN: what a 16-bit operand buffer holds wherever a correct kernel does not read


def bf16_bits(x):
    """values -> their bf16 bit patterns (RNE) as uint16"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def operand16(rows, ld, off=0, valid=None):
    """rows: the (R, X) array as a producer wrote it row-major (a [k][x] operand: R = K; the k-contiguous panel: R = M).  -> the uint16 buffer
    (R + OP_GUARD_ROWS, ld) holding bf16(rows) in the columns from off on, NAN16 in every other column, in the guard rows and in the rows from
    `valid` on (the rows behind a device-side count)"""
    R, X = rows.shape
    assert off + X <= ld
    buf = np.full((R + OP_GUARD_ROWS, ld), NAN16, np.uint16)
    v = R if valid is None else min(R, valid)
    buf[:v, off:off + X] = bf16_bits(rows[:v])
    return buf


def operands16(c, p):
    """-> (A16, B16) of a case with Case.ops16, None where the operand goes over as fp32; the count cuts the rows as in build()"""
    a16 = b16 = None
    if 'a' in c.ops16:
        if c.a_mc:
            a16 = operand16(p.a.T, c.lda16, c.off16, c.K_eff if c.dyn_kind == 2 else None)
        else:
            a16 = operand16(p.a, c.lda16, c.off16, c.M_eff if c.dyn_kind == 1 else None)
    if 'b' in c.ops16:
        assert c.b_nc
        b16 = operand16(p.b, c.ldb16, 0, c.K_eff if c.dyn_kind == 2 else None)
    return a16, b16


def bound(c, p, family):
    """elementwise error bound of a 'rounding' case and the float64 result it applies to.
    family 'f32' (exact-fp32 kernel; also the bf16-operand kernels against products of the bf16-rounded operands): K_eff fused adds in
    any order, alpha, bias, accumulate and the slices' adds, each at most u of the magnitude: (K_eff + split_k + 3) u magnitude.
    family 'f32s' (three-way bf16 split): no derivation in the code: the ceiling of test_gemm_split_bf16_is_fp32_accurate, 2e-6 (|alpha| |A| |B| + 1)"""
    if family == 'f32s':
        return product(c, p), 2e-6 * (abs(c.alpha) * (np.abs(p.a[:c.M_eff, :c.K_eff]) @ np.abs(p.b[:c.K_eff])) + 1.0)
    if family == 'bf16':
        a, b = bf16_round(p.a), bf16_round(p.b)
        q = dataclasses.replace(p, a=a, b=b)
        return product(c, p, a, b), (c.K_eff + c.split_k + 3) * U * magnitude(c, q)
    assert family == 'f32'
    return product(c, p), (c.K_eff + c.split_k + 3) * U * magnitude(c, p)
