"""tests/gemm_ref.py against numpy on examples small enough to check by hand, and the case table of tests/test_gpu_gemm.py against the
library's own dispatch (avae_debug_gemm_f32_form: the function gemm_f32() itself launches from).  No GPU."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import gemm_ref as R
import test_gpu_gemm as G


def _lib():
    from argsim_amd import lib
    return lib, lib.load()


def test_reference_is_numpy_matmul_on_a_padded_transposed_pair():
    c = R.case('example', (1, 1), 10, 6, 5, alpha=0.5, bias=True, accumulate=1, pair=True)
    assert (c.M, c.N) == (12, 8) and (c.lda, c.ldb, c.ldc) == (12 + R.PAD, 8 + R.PAD, 8 + R.PAD)
    ps = R.build(c)
    assert len(ps) == 2 and not np.array_equal(ps[0].a, ps[1].a) and not np.array_equal(ps[0].bias, ps[1].bias)
    for p, want in zip(ps, R.reference(c, ps)):
        # the device buffers hold the transposes, padded: read the operands back out of THEM
        a, b = p.A[:c.K, :c.M].T.astype(np.float64), p.B[:c.K, :c.N].astype(np.float64)
        assert np.array_equal(a, p.a) and np.array_equal(b, p.b)
        ref = 0.5 * np.matmul(a, b) + p.bias + p.C[:c.M, :c.N]
        assert np.array_equal(want[:c.M, :c.N], ref.astype(np.float32))
        assert R.untouched(c, want, p.C).size == 0


@pytest.mark.parametrize('lay', G.L4)
def test_operand_layouts_and_nan_outside(lay):
    c = R.case('layout', lay, 8, 12, 4)
    p = R.build(c)[0]
    A = p.A[:c.K, :c.M].T if c.a_mc else p.A[:c.M, :c.K]
    B = p.B[:c.K, :c.N] if c.b_nc else p.B[:c.N, :c.K].T
    assert np.array_equal(A, p.a) and np.array_equal(B, p.b)
    assert p.A.shape == ((c.K if c.a_mc else c.M) + R.OP_GUARD_ROWS, c.lda) and p.B.shape == ((c.K if c.b_nc else c.N) + R.OP_GUARD_ROWS, c.ldb)
    for buf, logical in ((p.A, A), (p.B, B)):
        assert np.isnan(buf).sum() == buf.size - logical.size and np.isfinite(logical).all()


def test_guards_and_sentinels_survive_the_reference():
    for c in (R.case('g', (0, 0), 7, 5, 8, bias=True),
              R.case('g', (0, 1), 7, 8, 8, split_k=2),
              R.case('g', (0, 0), 7, 5, 8, accumulate=1, dyn_kind=1, count=3),
              R.case('g', (1, 1), 8, 8, 8, dyn_kind=2, count=5, split_k=2, plain_out=True)):
        p = R.build(c)[0]
        before = p.C.copy()
        want = R.reference(c, [p])[0]
        assert np.array_equal(p.C.view(np.int32), before.view(np.int32))              # the reference leaves its input alone
        v, b = want.view(np.int32), before.view(np.int32)
        assert (v[c.M:] == R.SENT).all() and (v[:, c.N:] == R.SENT).all()
        assert np.array_equal(v[c.M_eff:c.M], b[c.M_eff:c.M])                         # rows beyond the device-side count keep C0 / zeros / the sentinel
        assert np.isfinite(want[:c.M_eff, :c.N]).all()
        assert R.untouched(c, want, before).size == 0
        want[c.M_eff, 0] = 1.0
        assert R.untouched(c, want, before).tolist() == [[c.M_eff, 0]]
    # the count cuts the operands: rows of A, or the depth
    c = R.case('g', (0, 0), 7, 5, 8, dyn_kind=1, count=3)
    p = R.build(c)[0]
    assert np.isnan(p.A[3:]).all() and np.array_equal(R.reference(c, [p])[0][:3, :5], (p.a[:3] @ p.b).astype(np.float32))
    c = R.case('g', (1, 1), 8, 8, 8, dyn_kind=2, count=5)
    p = R.build(c)[0]
    assert np.isnan(p.A[5:]).all() and np.isnan(p.B[5:]).all()
    assert np.array_equal(R.reference(c, [p])[0][:8, :8], (p.a[:, :5] @ p.b[:5]).astype(np.float32))


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0, np.nextafter(np.float32(1.00390625), np.float32(2))], np.float32)      # 1 + 2^-8 ties to even (down), 1 + 3 * 2^-8 ties up
    assert R.bf16_round(x).tolist() == [1.0, 1.0, 1.015625, -3.0, 1.0078125]


def test_exactness_condition_holds_for_every_gpu_case():
    ids = [c.id + repr(c) for c in G.ALL_CASES]
    assert len(set(ids)) == len(ids)
    for c in G.ALL_CASES:
        if c.data == 'exact':
            assert c.alpha in R.ALPHAS and R.exact_limit(c) < 2.0 ** 23, c
            if c.M * c.N <= 1 << 17:
                for p in R.build(c):                    # (build asserts the condition on the data itself)
                    assert 2.0 * R.magnitude(c, p).max(initial=0.0) <= 2.0 * R.exact_limit(c) < 2.0 ** 24


def test_hooks_are_exported_and_typed():
    lib, l = _lib()
    header = open(lib.CSRC + '/../../include/argsim_vae.h').read()
    for name in ('avae_debug_gemm_forced', 'avae_debug_gemm_f32_form', 'avae_debug_gemm16', 'avae_debug_gemm_bf16_form'):
        assert name in lib.SIGNATURES and hasattr(l, name)
        assert name not in header


def form(l, c, **kw):
    c = dataclasses.replace(c, **kw)
    out = (C.c_int32 * 8)()
    assert l.avae_debug_gemm_f32_form(c.a_mc, c.b_nc, c.M, c.N, c.K, c.lda, c.ldb, c.ldc, c.accumulate, c.thin, c.split_k, c.dyn_kind, c.expect, int(c.pair), out) == 0
    return list(out)


def test_every_fp32_case_reaches_the_form_it_claims():
    """the proof that the shapes of tests/test_gpu_gemm.py hit the code they are meant to hit"""
    lib, l = _lib()
    assert G.env_clean()
    seen = set()
    for c in G.F32_CASES:
        for expect in {0, c.expect}:
            f = form(l, c, expect=expect)
            assert tuple(f[:4]) == c.reach and f[7] == 0, (c.id, f)
        tile, fast, db, persist, gx, gy, gz, _ = f
        bm, bn = {0: (128, 128), 1: (32, 128), 2: (64, 64), 3: (32, 32)}[tile]
        tiles = -(-c.M // bm) * -(-c.N // bn)
        assert (gx, gy, gz) == ((768, 1, 1) if persist else (tiles, 2 if c.pair else 1, c.split_k)), (c.id, f)
        seen.add((tile, fast, db, persist, c.a_mc, c.b_nc))
    # every launch form on the layouts it is instantiated for
    for lay in G.L4:
        for reach in (G.PRED, G.T32, G.T64):
            assert reach + lay in seen, (reach, lay)
    for reach, lays in ((G.FAST, G.L4), (G.SKINNY, ((0, 0), (0, 1))), (G.DB_FAST, ((0, 1),)), (G.DB_PRED, ((0, 0), (1, 1))), (G.PERSIST, ((0, 0), (0, 1)))):
        for lay in lays:
            assert reach + lay in seen, (reach, lay)


def test_16bit_operand_buffers_hold_nan_wherever_a_kernel_must_not_read():
    c = R.case('o16', (1, 1), 16, 24, 10, dtype=1, route=1, ops16='ab', round16=True, data='rounding', dyn_kind=2, count=7)
    p = R.build(c)[0]
    assert np.array_equal(R.bf16_round(p.a), p.a) and np.array_equal(R.bf16_round(p.b), p.b)          # the draws are bf16 values already
    a16, b16 = R.operands16(c, p)
    assert (c.lda16, c.off16, c.ldb16) == (32, 16, 32) and a16.shape == (10 + R.OP_GUARD_ROWS, 32) and b16.shape == (10 + R.OP_GUARD_ROWS, 32)
    widen = lambda u: (u.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    assert np.array_equal(widen(a16[:7, 16:]), p.a.T[:7]) and np.array_equal(widen(b16[:7, :24]), p.b[:7])
    for buf, logical in ((a16, 7 * 16), (b16, 7 * 24)):
        assert (buf == R.NAN16).sum() == buf.size - logical and np.isnan(widen(buf)).sum() == buf.size - logical
    # a rows count cuts the k-contiguous panel's rows
    c = R.case('o16', (0, 0), 9, 8, 16, dtype=1, route=0, ops16='a', round16=True, dyn_kind=1, count=4)
    a16, b16 = R.operands16(c, R.build(c)[0])
    assert b16 is None and c.lda16 == 32 and (a16[4:] == R.NAN16).all() and (a16[:4, 16:] == R.NAN16).all() and (a16[:4, :16] != R.NAN16).all()
    assert R.bf16_bits(np.array([1.0, 1.00390625, 1.01171875, -3.0], np.float32)).tolist() == [0x3F80, 0x3F80, 0x3F82, 0xC040]


def test_every_16bit_case_reaches_the_form_it_claims():
    """the proof for the bf16-mode cases: avae_debug_gemm_bf16_form returns gemm_bf16_form, the value gemm_bf16_nt / gemm_bf16_tn launch from"""
    lib, l = _lib()
    seen = set()
    for c in G.CASES16:
        kernel, slices, slab, refused, s2, asked = G.form16(l, c)
        assert (kernel, slices, slab) == c.reach16 and refused == 0, (c.id, kernel, slices, slab, refused)
        seen.add((c.route, kernel, slices > 1, slab, c.dyn_kind))
    for want in ((1, G.P8TN, False, 0, 0), (1, G.TN256, False, 0, 0), (1, G.P8TN, True, 1, 0), (1, G.TN256, True, 0, 0), (1, G.P8TN, True, 1, 2),
                 (1, G.TN256, True, 0, 2), (1, G.P8TN, False, 0, 2), (0, G.NT128, False, 0, 0), (0, G.NT128, False, 0, 1), (0, G.NT128, True, 0, 0),
                 (0, G.NT128, True, 0, 2), (-1, G.P8NT, True, 0, 0), (-1, G.NT256, True, 0, 0), (-1, G.P8NT, False, 0, 0), (-1, G.NT256, False, 0, 0)):
        assert want in seen, want
    # the cases that claim a re-derived split say which: 3 asked -> 6, and -> 1 (the launch then accumulates)
    for c in G.NT_SPLIT_CASES:
        assert G.form16(l, c)[4:] == [c.reach16[1], 3], c.id
    # a slab too small for the slices' tiles: float atomics instead
    c = [c for c in G.TN16_CASES if c.reach16 == (G.P8TN, 2, 1)][0]
    assert G.form16(l, c, slab_floats=(8 << 16) - 1)[:3] == [G.P8TN, 2, 0] and G.form16(l, c, slab_floats=8 << 16)[:3] == [G.P8TN, 2, 1]


def test_bf16_form_refusals_and_the_unreachable_clamp():
    lib, l = _lib()
    c = [c for c in G.TN16_CASES if c.reach16 == (G.P8TN, 1, 0)][0]
    assert G.form16(l, c)[3] == 0
    assert G.form16(l, c, dyn_kind=1)[3] == 1 and G.form16(l, c, bias=1)[3] == 1 and G.form16(l, c, lda=c.lda16 - 4)[3] == 1 and G.form16(l, c, M=c.M - 4)[3] == 1
    p = G.PRE_CASES[0]
    assert G.form16(l, p, M=0)[:4] == [-1, 1, 0, 0] and G.form16(l, c, wgrad=0, split_k=2, M=0)[:4] == [-1, 1, 0, 0]
    assert G.form16(l, p, lda=p.lda16 - 4)[3] == 1 and G.form16(l, p, dyn_kind=2, split_k=3)[3] == 1 and G.form16(l, p, dyn_kind=2, split_k=3, bias=0)[3] == 0
    # gemm_bf16_p8 clamps its split to two K tiles per slice; gemm_bf16_slices has left four already, so the phased NT kernel always runs the
    # re-derived split as it stands (no case can reach the clamp), and a device-side depth keeps the phased NT kernel out
    for M, N in ((1300, 1300), (5000, 2500), (4100, 4100)):
        for K in range(128, 4097, 64):
            for split in (1, 2, 3, 8, 40):
                kernel, slices, slab, refused, s2, asked = G.form16(l, dataclasses.replace(G.NT_SPLIT_CASES[0], M=M, N=N, K=K, split_k=split))
                if kernel == G.NT128:                   # (the caller's split as it stands)
                    assert refused == 0 and slices == split and s2 * -(-M // 256) * -(-N // 256) < 200, (M, N, K, split)
                else:
                    assert refused == 0 and kernel == G.P8NT and slices == s2, (M, N, K, split)
    assert G.form16(l, dataclasses.replace(G.NT_SPLIT_CASES[0], dyn_kind=2, bias=False))[0] == G.NT256


def test_form_refusals_and_empty_problems():
    lib, l = _lib()
    c = R.case('r', (0, 0), 200, 72, 52)
    assert form(l, c)[7] == 0
    assert form(l, c, K=54)[7] == 1 and form(l, dataclasses.replace(c, a_mc=1), M=202)[7] == 1 and form(l, dataclasses.replace(c, b_nc=1), N=74)[7] == 1
    assert form(l, c, M=0) == [-1, 0, 0, 0, 0, 0, 0, 0]
    # a device-side depth: [k][x] operands only (kernels.h)
    for lay in G.L4:
        assert form(l, R.case('r', lay, 128, 132, 1024, dyn_kind=2, count=5))[7] == (lay != G.KX)
