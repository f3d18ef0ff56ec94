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
    for name in ('avae_debug_gemm_forced', 'avae_debug_gemm_f32_form'):
        assert name in lib.SIGNATURES and hasattr(l, name)
    header = open(lib.CSRC + '/../../include/argsim_vae.h').read()
    assert 'avae_debug_gemm_forced' not in header and 'avae_debug_gemm_f32_form' not in header


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


def test_form_refusals_and_empty_problems():
    lib, l = _lib()
    c = R.case('r', (0, 0), 200, 72, 52)
    assert form(l, c)[7] == 0
    assert form(l, c, K=54)[7] == 1 and form(l, dataclasses.replace(c, a_mc=1), M=202)[7] == 1 and form(l, dataclasses.replace(c, b_nc=1), N=74)[7] == 1
    assert form(l, c, M=0) == [-1, 0, 0, 0, 0, 0, 0, 0]
    # a device-side depth: [k][x] operands only (kernels.h)
    for lay in G.L4:
        assert form(l, R.case('r', lay, 128, 132, 1024, dyn_kind=2, count=5))[7] == (lay != G.KX)
