"""nearest-neighbour search, the part that needs no GPU: the entry is declared and bound, VAE.neighbors' argument rules, the float64
reference of tests/knn_ref.py against a brute-force argsort, and the condition on the inputs of tests/test_gpu_knn.py."""
import os
import re

import numpy as np
import pytest

import knn_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_signature():
    from argsim_amd import lib
    src = open(os.path.join(ROOT, 'include', 'argsim_vae.h')).read()
    assert re.search(r'\bavae_knn\s*\(', src) and 'avae_knn_config' in src
    assert 'avae_knn' in lib.SIGNATURES and len(lib.SIGNATURES['avae_knn'][1]) == 9
    names = [f[0] for f in lib.AvaeKnnConfig._fields_]
    assert names == ['k', 'metric', 'idx_base', 'self_base', 'carry', 'reserved']
    import ctypes
    assert ctypes.sizeof(lib.AvaeKnnConfig) == 32
    for word in ('order_key', 'carry', 'idx_base', 'self_base', 'cancellation', 'knn_chunk'):
        assert word in src, word
    assert hasattr(lib.load(), 'avae_knn')


def test_argument_checks():
    import torch
    from argsim_amd.model import _check_knn_args, neighbors, VAE
    q, b = np.zeros((3, 8), np.float32), np.zeros((5, 8), np.float32)
    assert _check_knn_args(q, b, 5, 'cos') == (5, 1, -1, None)
    assert _check_knn_args(q, b, 32, 'euc', True, 2) == (32, 2, 0, 2)
    assert _check_knn_args(torch.zeros(3, 8), torch.zeros(0, 8), 1, 'dot', (4,)) == (1, 0, 4, None)
    assert _check_knn_args(q, b, 1, 'dot', 7)[2] == 7
    bad = [dict(k=0), dict(k=33), dict(k=2.5), dict(k=True), dict(metric='l1'), dict(metric=1),
           dict(queries=np.zeros((3, 6), np.float32), bank=np.zeros((5, 6), np.float32)),            # dim % 4
           dict(queries=np.zeros((3, 1028), np.float32), bank=np.zeros((5, 1028), np.float32)),      # dim > 1024
           dict(bank=np.zeros((5, 12), np.float32)),                                                 # mismatched dims
           dict(queries=q.astype(np.float64)), dict(bank=b.astype(np.float16)), dict(bank=torch.zeros(5, 8, dtype=torch.float64)),
           dict(queries=np.zeros(8, np.float32)), dict(queries=np.zeros((0, 8), np.float32)), dict(queries=[[0.0] * 8]),
           dict(exclude_self=-1), dict(exclude_self=(1, 2)), dict(exclude_self=1.5), dict(block=0), dict(block=1.5)]
    for kw in bad:
        args = dict(queries=q, bank=b, k=5, metric='cos', exclude_self=False, block=None)
        args.update(kw)
        with pytest.raises(ValueError):
            _check_knn_args(**args)
    assert callable(neighbors) and callable(VAE.neighbors)


def _brute(q, bank, k, metric):
    s = kr.scores64(q, bank, metric)
    idx = np.argsort(-s, axis=1, kind='stable')[:, :k]
    return idx, np.take_along_axis(s, idx, 1)


def test_reference_agrees_with_brute_force():
    rng = np.random.default_rng(5)
    for n, N, dim, k in ((2, 9, 4, 3), (4, 17, 8, 17), (1, 6, 12, 1)):
        q, bank = rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((N, dim)).astype(np.float32)
        for metric in kr.METRICS:
            s = kr.scores64(q, bank, metric)
            # the scores themselves, element by element
            for i in range(n):
                for c in range(N):
                    a, b = q[i].astype(np.float64), bank[c].astype(np.float64)
                    want = {'dot': a @ b, 'cos': a @ b / (np.linalg.norm(a) * np.linalg.norm(b)), 'euc': -((a - b) ** 2).sum()}[metric]
                    assert abs(s[i, c] - want) <= 1e-12 * max(1.0, abs(want))
            bi, bs = _brute(q, bank, k, metric)
            ri, rs = kr.topk(s, k)
            assert np.array_equal(ri, bi) and np.array_equal(rs, bs)
            # idx_base shifts the indices; self_base removes one row per query; a short bank pads with -1 / -inf
            ri2, _ = kr.topk(s, k, idx_base=100)
            assert np.array_equal(ri2, ri + 100)
            ri3, rs3 = kr.topk(s, N, self_base=1)
            for i in range(n):
                keep = [c for c in np.argsort(-s[i], kind='stable') if c != 1 + i]
                assert ri3[i, :len(keep)].tolist() == keep and (ri3[i, len(keep):] == -1).all() and np.isneginf(rs3[i, len(keep):]).all()
            # carry: two halves merged = the whole
            h = N // 3
            c1 = kr.topk(s[:, :h], k)
            c2 = kr.topk(s[:, h:], k, idx_base=h, carry=c1)
            assert np.array_equal(c2[0], ri) and np.array_equal(c2[1], rs)
    # ties go to the lower index; NaN below -inf; +0 and -0 equal
    s = np.array([[1.0, np.nan, -np.inf, 1.0, -0.0, 0.0]])
    ri, rs = kr.topk(s, 6)
    assert ri.tolist() == [[0, 3, 4, 5, 2, 1]]
    assert kr.order_key(np.array([0.0, -0.0, np.nan, -np.inf, np.inf, 1.0, -1.0], np.float32)).tolist() == \
        [0x80000000, 0x80000000, 0, 0x007fffff, 0xff800000, 0xbf800000, 0x407fffff]
    # the judge accepts the reference itself and refuses a wrong list
    q, bank = kr.make_inputs(3, 40, 8)
    s = kr.scores64(q, bank, 'cos')
    ri, rs = kr.topk(s, 5)
    assert kr.judge(ri, rs.astype(np.float32), s, 5, 1e-6) <= 1e-6
    wrong = ri.copy()
    wrong[1, 4] = int(np.argmin(s[1]))
    with pytest.raises(AssertionError):
        kr.judge(wrong, rs.astype(np.float32), s, 5, 1e-6)
    with pytest.raises(AssertionError):
        kr.judge(ri[:, ::-1].copy(), rs[:, ::-1].astype(np.float32), s, 5, 1e-6)


def test_inputs_plant_what_the_gpu_tests_look_for():
    for case in kr.CASES:
        n, N, dim, k = case
        q, bank = kr.case_inputs(case)
        assert q.dtype == bank.dtype == np.float32 and q.shape == (n, dim) and bank.shape == (N, dim)
        assert np.array_equal(bank[N // 2], bank[1]) and np.array_equal(bank[N - 1], bank[1]) and not bank[3].any()
        assert np.array_equal(q[0], bank[1])
        norms = np.linalg.norm(np.delete(bank, 3, 0).astype(np.float64), axis=1)
        assert 0.5 < norms.min() and norms.max() < 2.0 and abs(norms.mean() - 1.0) < 0.15 if dim >= 20 else True


@pytest.mark.parametrize('metric', kr.METRICS)
def test_input_condition(metric):
    """at most 5 % of the queries of any GPU case have a k-th / (k+1)-th float64 gap that is positive and <= 1e-5 (exact ties come
    from the planted duplicates only, where the index order decides)"""
    for case in kr.CASES:
        share = kr.small_gaps(kr.case_scores(case, metric), case[3])
        print(case, metric, "share of queries with a gap in (0, 1e-5]: %.4f" % share)
        assert share <= 0.05, (case, metric, share)
