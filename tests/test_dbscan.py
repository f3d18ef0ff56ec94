"""Density clustering without a device: the float64 reference of tests/dbscan_ref.py against scikit-learn and against the textbook loop,
the margins of the cases the GPU tests rely on, the CPU model of the device's round rule against the planner's default, the launch planner
(avae_debug_dbscan_plan, host arithmetic), and the parts of the Python layer that need no device (a stand-in for the C entry)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dbscan_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM = [(n, dim, m) for n, dim in dr.RANDOM_SHAPES for m in (0, 1)]


# ---------------------------------------------------------------- the reference
def textbook(x, metric, eps, min_samples):
    """DBSCAN as Ester et al. wrote it: rows in ascending order, a cluster grown from each unvisited core row"""
    A = dr.pair_values(x, metric) <= dr.threshold(metric, eps)
    n = len(A)
    label = np.full(n, -2)                                  # -2: not visited
    c = 0
    for s in range(n):
        if label[s] != -2:
            continue
        near = np.flatnonzero(A[s])
        if len(near) < min_samples:
            label[s] = -1
            continue
        label[s] = c
        seeds = list(near)
        while seeds:
            j = seeds.pop(0)
            if label[j] == -1:
                label[j] = c                                # noise so far: a border row of this cluster
            if label[j] != -2:
                continue
            label[j] = c
            nj = np.flatnonzero(A[j])
            if len(nj) >= min_samples:
                seeds += list(nj)
        c += 1
    return label


def _all_cases():
    for n, dim, m in RANDOM:
        x, eps, ms = dr.random_case(n, dim, m)
        yield 'random-%d-%d-%s' % (n, dim, dr.METRICS[m]), x, m, eps, ms
    for name, (x, m, eps, ms) in dr.EXACT.items():
        yield name, x, m, eps, ms
    x, eps, ms = dr.bridge()[:3]
    yield 'bridge', x, 0, eps, ms
    x, eps, ms = dr.numbering()[:3]
    yield 'numbering', x, 0, eps, ms


def test_every_random_case_has_the_margin():
    """|p - thr| >= 1e-9 thr for every pair, against a summation error below (dim + 3) 2^-52 <= 2.3e-13: any correct double evaluation
    decides every pair the same way.  And the cases are not trivial: together they have core, border and noise rows and several clusters"""
    seen = np.zeros(4, np.int64)
    for n, dim, m in RANDOM:
        x, eps, ms = dr.random_case(n, dim, m)
        assert x.shape == (n, dim) and dr.margin(x, m, eps) >= dr.MARGIN, (n, dim, m)
        seen += dr.dbscan(x, m, eps, ms)['stat']
        if n >= 63:
            assert dr.dbscan(x, m, eps, ms)['stat'][1] > 0, (n, dim, m)
    assert (dim + 3) * 2.0 ** -52 < 1e-3 * dr.MARGIN and (seen > 20).all(), seen


def test_the_exact_cases_are_exact_and_touch_eps():
    for name, (x, m, eps, ms) in dr.EXACT.items():
        assert m == 0 and (x == np.round(x)).all() and np.abs(x).max() < 1024, name
        thr = dr.threshold(m, eps)
        assert thr == round(thr), name                      # eps * eps is an integer in double
        p = dr.pair_values(x, m)
        assert (p == np.round(p)).all(), name
        if name != 'all_noise':
            assert (p[~np.eye(len(p), dtype=bool)] == thr).any(), name      # pairs at exactly eps, which are inside
    assert (dr.dbscan(*dr.EXACT['all_core'])['core']).all() and dr.dbscan(*dr.EXACT['all_core'])['stat'][0] == 5
    assert (dr.dbscan(*dr.EXACT['all_noise'])['label'] == -1).all()
    r = dr.dbscan(*dr.EXACT['grid_at_eps'])
    assert r['stat'].tolist() == [1, 35, 24, 4]             # the interior is core, the edges are border, the corners noise


def test_the_reference_on_the_named_cases():
    x, eps, ms, labels, counts = dr.bridge()
    r = dr.dbscan(x, 0, eps, ms)
    assert r['label'].tolist() == labels and r['count'].tolist() == counts and r['stat'].tolist() == [2, 10, 1, 0]
    x, eps, ms, labels = dr.numbering()
    r = dr.dbscan(x, 0, eps, ms)
    assert r['label'].tolist() == labels and not r['core'][0] and r['core'].tolist() == [False, False, True, False, True, True, False]
    for name, o in dr.orders(256).items():
        r = dr.dbscan(dr.chain(256, o), 0, 1.0, 3)
        ends = [int(o[0]), int(o[255])]
        assert (r['label'] == 0).all() and sorted(np.flatnonzero(~r['core']).tolist()) == sorted(ends), name
        r = dr.dbscan(dr.ring(256, o), 0, 1.0, 3)
        assert (r['label'] == 0).all() and r['core'].all() and (r['count'] == 3).all(), name
    # cosine: a zero row is at distance 1 from every other row; scaled copies of a row have p = 0
    x = dr.cosine_rows()
    p = dr.pair_values(x, 1)
    assert (p[1, [0, 2, 3, 4]] == 2).all() and p[1, 1] == 0 and p[0, 2] == 0 and p[0, 3] == 0 and np.array_equal(p, p.T)
    assert dr.dbscan(x, 1, 0.5, 2)['label'].tolist() == [0, -1, 0, 0, -1] and dr.dbscan(x, 1, 0.999, 2)['count'].tolist() == [4, 1, 4, 4, 4]
    assert dr.dbscan(x, 1, 1.0, 5)['count'].tolist() == [5] * 5 and dr.dbscan(x, 1, 1.0, 5)['label'].tolist() == [0] * 5


def test_the_reference_against_the_textbook_loop():
    for name, x, m, eps, ms in _all_cases():
        assert np.array_equal(dr.dbscan(x, m, eps, ms)['label'], textbook(x, m, eps, ms)), name


def test_the_reference_against_sklearn():
    cluster = pytest.importorskip('sklearn.cluster')
    for name, x, m, eps, ms in _all_cases():
        if name.startswith('random') or name in ('bridge', 'numbering'):
            assert name in ('bridge', 'numbering') or dr.margin(x, m, eps) >= dr.MARGIN
            sk = cluster.DBSCAN(eps=eps, min_samples=ms, metric=dr.METRICS[m], algorithm='brute').fit(x.astype(np.float64))
            r = dr.dbscan(x, m, eps, ms)
            assert np.array_equal(sk.labels_, r['label']), name
            assert np.array_equal(sk.core_sample_indices_, np.flatnonzero(r['core'])), name


# ---------------------------------------------------------------- the rounds
def test_the_round_model_stays_within_the_default():
    """the model of hook and jump over the adversarial family: the worst count is ceil(log2 n) + 1 (the bit-reversed chain); the
    planner's default is twice that"""
    worst = dr.family_rounds()
    for n, (t, where) in worst.items():
        lg = int(n - 1).bit_length()
        assert t <= lg + 1 and 2 * t <= dr.default_rounds(n), (n, t, where)
    assert worst[4096][0] == 13 and worst[1024][0] == 11


def test_the_round_model_finds_the_lowest_row_of_each_component():
    r = np.random.default_rng(3)
    for n in (5, 60, 300):
        e = r.integers(0, n, (n // 2, 2))
        src, dst = dr._both(e)
        P, t = dr.round_model(n, src, dst)
        want = np.arange(n)
        for _ in range(n):
            np.minimum.at(want, src, want[dst])
        assert np.array_equal(P, want) and t <= dr.default_rounds(n)


# ---------------------------------------------------------------- the planner
def _plan(N, dim=128, chunk=0, cus=256):
    from argsim_amd import lib
    out = np.full(9, -1, np.int32)
    assert lib.load().avae_debug_dbscan_plan(N, dim, chunk, cus, out.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    ti, rtiles, parts, tiles, W, lds, rounds, lo, hi = out.tolist()
    return dict(TI=ti, rtiles=rtiles, parts=parts, chunk=tiles, W=W, lds=lds, rounds=rounds, ws=(lo & 0xffffffff) | (hi << 32))


def test_the_plan_covers_every_tile_once():
    for N in (1, 2, 5, 63, 64, 65, 257, 3000, 1 << 16, (1 << 17) - 1, 1 << 17):
        for chunk in (0, 4, 16 | (1 << 8), 64 | (3 << 8), 2 << 8, 200 | (5000 << 8)):
            for cus in (1, 256):
                p = _plan(N, 128, chunk, cus)
                assert p['TI'] in (4, 8, 16, 32, 64) and p['W'] == -(-N // 64) and p['rtiles'] == -(-N // p['TI'])
                assert 1 <= p['parts'] <= 65535 and (p['parts'] - 1) * p['chunk'] < p['W'] <= p['parts'] * p['chunk']
                assert p['lds'] == 8 * (32 * p['TI'] + 32 * 64 + p['TI'] + 64) + 8 * p['TI'] <= 64 * 1024
                assert p['rounds'] == dr.default_rounds(N) == 2 * (int(N - 1).bit_length() + 1)
                if chunk & 255:
                    assert p['TI'] == max(t for t in (4, 8, 16, 32, 64) if t <= max(chunk & 255, 4))
                else:
                    assert p['TI'] == 64 or (p['TI'] >= min(N, 4) and p['TI'] // 2 < max(N, 4) <= max(p['TI'], 4))
                if chunk >> 8:
                    assert p['chunk'] == min(chunk >> 8, 0x7fffff80) or p['parts'] == 65535
                else:                                       # the fewest tiles per part that keep the parts within what two per CU ask for
                    assert p['chunk'] == max(1, -(-p['W'] // -(-2 * cus // p['rtiles'])))
                n, W = N, p['W']
                need = 8 * n * W + 8 * W + 16 * n + 4 * n + 8 * n + 4 * (p['rounds'] + 1) + 16
                assert need <= p['ws'] <= need + 10 * 256
    assert _plan(1 << 17)['ws'] >= 1 << 31 and _plan(1 << 17)['rounds'] == 36 and _plan(3000)['TI'] == 64 and _plan(3)['TI'] == 4
    from argsim_amd import lib
    out = np.zeros(9, np.int32)
    for bad in ((0, 128, 0, 256), ((1 << 17) + 1, 128, 0, 256), (10, 6, 0, 256), (10, 1028, 0, 256), (10, 128, -1, 256), (10, 128, 0, 0)):
        assert lib.load().avae_debug_dbscan_plan(*bad, out.ctypes.data_as(C.POINTER(C.c_int32))) == 1


def test_the_declaration_matches_the_header():
    from argsim_amd import lib
    res, args = lib.SIGNATURES['avae_dbscan']
    assert res is C.c_int and len(args) == 8 and args[4] == C.POINTER(lib.AvaeDbscanConfig)
    with open(os.path.join(ROOT, 'include', 'argsim_vae.h')) as f:
        text = f.read()
    body = re.search(r'typedef struct avae_dbscan_config \{(.*?)\} avae_dbscan_config;', text, re.S).group(1)
    fields = re.findall(r'^\s*(int32_t|double)\s+(\w+);', body, re.M)
    ctype = {'int32_t': C.c_int32, 'double': C.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(lib.AvaeDbscanConfig._fields_) and C.sizeof(lib.AvaeDbscanConfig) == 24
    decl = re.search(r'int\s+avae_dbscan\((.*?)\);', text, re.S).group(1)
    assert len(re.sub(r'/\*.*?\*/', '', decl, flags=re.S).split(',')) == 8
    assert hasattr(lib.load(), 'avae_dbscan') and hasattr(lib.load(), 'avae_debug_dbscan_plan')


# ---------------------------------------------------------------- the Python layer without a device
def _ref_raw(calls, flag=0, rounds=3):
    """dbscan_raw's stand-in: the float64 reference on what the wrapper hands to the C entry"""
    def raw(vae, x, cfg, want_count=True):
        calls.append(dict(x=np.array(x), cfg=(cfg.metric, cfg.min_samples, cfg.max_rounds, cfg.reserved, cfg.eps), want_count=want_count))
        r = dr.dbscan(x, cfg.metric, cfg.eps, cfg.min_samples)
        stat = np.array(r['stat'].tolist() + [rounds, flag, 0, 0], np.int32)
        return dict(label=r['label'].astype(np.int32), count=r['count'].astype(np.int32), stat=stat)
    return raw


def test_the_wrapper_pads_and_reports():
    from argsim_amd import dbscan as D
    x, eps, ms = dr.random_case(65, 4, 0)
    z = np.ascontiguousarray(np.concatenate([x, x[:, :2]], 1))          # 6 columns: padded with zeros to 8
    calls = []
    res = D.dbscan(None, z, 0.5, 3, 'cosine', max_rounds=7, raw=_ref_raw(calls))
    (c,) = calls
    assert c['x'].shape == (65, 8) and c['x'].dtype == np.float32 and (c['x'][:, 6:] == 0).all() and np.array_equal(c['x'][:, :6], z)
    assert c['cfg'] == (1, 3, 7, 0, 0.5) and c['want_count'] is True
    r = dr.dbscan(c['x'], 1, 0.5, 3)
    assert res['labels'].dtype == np.int64 and np.array_equal(res['labels'], r['label']) and np.array_equal(res['counts'], r['count'])
    assert np.array_equal(res['core_sample_indices'], np.flatnonzero(r['core'])) and res['rounds'] == 3
    assert [res['n_clusters'], len(res['core_sample_indices']), res['n_border'], res['n_noise']] == r['stat'].tolist()
    assert set(res) == {'labels', 'core_sample_indices', 'n_clusters', 'n_noise', 'n_border', 'counts', 'rounds'}
    calls.clear()
    import torch
    D.dbscan(None, torch.as_tensor(x), eps, raw=_ref_raw(calls))         # a host tensor, the defaults
    assert calls[0]['cfg'] == (0, 5, 0, 0, eps) and isinstance(calls[0]['x'], np.ndarray) and calls[0]['x'].shape == (65, 4)


def test_the_wrapper_checks_its_arguments_and_the_verify_flag():
    from argsim_amd import dbscan as D
    z = dr.random_case(64, 4, 0)[0]
    raw = _ref_raw([])
    bad = [dict(z=[[1.0]]), dict(z=z.astype(np.float64)), dict(z=np.zeros((8,), np.float32)), dict(z=np.zeros((0, 8), np.float32)),
           dict(z=np.zeros((20, 1025), np.float32)), dict(metric='sqeuclidean'), dict(eps=0.0), dict(eps=-1.0), dict(eps=float('inf')),
           dict(eps=float('nan')), dict(eps='1'), dict(min_samples=0), dict(min_samples=2.5), dict(min_samples=True), dict(max_rounds=-1),
           dict(max_rounds=4097), dict(max_rounds=1.5)]
    for kw in bad:
        args = dict(z=z, eps=1.0, min_samples=5, metric='euclidean', max_rounds=0)
        args.update(kw)
        with pytest.raises(ValueError):
            D.dbscan(None, raw=raw, **args)
    with pytest.raises(RuntimeError, match='max_rounds'):
        D.dbscan(None, z, 1.0, raw=_ref_raw([], flag=1))
    for kw in (dict(k=0), dict(k=64), dict(k=33), dict(k=1.0), dict(metric='dot'), dict(z=z[:1])):
        args = dict(z=z, k=4, metric='euclidean')
        args.update(kw)
        with pytest.raises(ValueError):
            D.kdist(None, **args)


class _Stub:
    """dbscan by the reference, the scores recorded"""
    def __init__(self):
        self.db, self.sil = [], []

    def dbscan(self, x, eps, min_samples=5, metric='euclidean', max_rounds=0):
        from argsim_amd import dbscan as D
        self.db.append((eps, min_samples, metric))
        return D.dbscan(None, x, eps, min_samples, metric, max_rounds, raw=_ref_raw([]))

    def silhouette(self, x, labels, metric, return_samples=False):
        import sil_ref as sr
        from argsim_amd import silhouette as S
        from test_silhouette import _ref_raw as sil_raw
        self.sil.append(np.array(labels))
        assert sr is not None
        return S.silhouette(None, x, labels, metric, return_samples, raw=sil_raw([]))

    def sweep_eps(self, x, eps_list, min_samples=5, metric='euclidean'):
        from argsim_amd import dbscan as D
        return D.sweep_eps(self, x, eps_list, min_samples, metric)

    def affinity(self, x, metric, max_iter, seed):
        return dict(labels=np.arange(len(x)) % 2, converged=True, n_iter=3)

    def neighbors(self, q, bank, k, metric, exclude_self, return_distance):
        d2 = ((q[:, None, :].astype(np.float64) - bank[None].astype(np.float64)) ** 2).sum(2)
        np.fill_diagonal(d2, np.inf)
        idx = np.argsort(d2, 1, kind='stable')[:, :k]
        assert metric == 'euc' and exclude_self is True and return_distance is True and q is bank and q.shape[1] % 4 == 0
        return idx, np.take_along_axis(d2, idx, 1).astype(np.float32)


def test_sweep_eps_makes_one_silhouette_call_and_passes_noise_on():
    from argsim_amd import dbscan as D
    x, eps, ms = dr.random_case(129, 4, 0)
    v = _Stub()
    grid = [1e-3, eps * 0.7, eps, eps * 1.3, 100.0]                      # all noise .. one cluster: the ends cannot be scored
    t = D.sweep_eps(v, x, grid, ms, 'euclidean')
    assert v.db == [(e, ms, 'euclidean') for e in grid] and len(v.sil) == 1
    ok = [i for i in range(5) if 2 <= t['n_clusters'][i] <= int((t['labels'][i] >= 0).sum()) - 1]
    assert 0 not in ok and 4 not in ok and len(ok) >= 2 and t['n_clusters'][0] == 0 and t['n_clusters'][4] == 1
    assert np.array_equal(v.sil[0], t['labels'][ok]) and (v.sil[0] == -1).any() and v.sil[0].min() == -1      # noise stays at -1
    assert np.isnan(t['score'][[0, 4]]).all() and np.isfinite(t['score'][ok]).all() and np.isfinite(t['ch'][ok]).all()
    assert t['best'] == grid[ok[int(np.argmax(t['score'][ok]))]] and t['labels'].shape == (5, 129) and t['eps'].tolist() == grid
    assert t['n_noise'][0] == 129 and t['n_noise'][4] == 0
    none = D.sweep_eps(v, x, [1e-3], ms)
    assert none['best'] is None and len(v.sil) == 1 and np.isnan(none['score']).all()
    with pytest.raises(ValueError):
        D.sweep_eps(v, x, [1.0] * 65)
    with pytest.raises(ValueError):
        D.sweep_eps(v, x, [])


def test_kdist_is_the_sorted_kth_neighbour_distance():
    from argsim_amd import dbscan as D
    x = dr.blobs(50, 6, 9)
    v = _Stub()
    d = np.sqrt(((x[:, None].astype(np.float64) - x[None]) ** 2).sum(2))
    np.fill_diagonal(d, np.inf)
    assert np.allclose(D.kdist(v, x, 4), np.sort(np.sort(d, 1)[:, 3]), rtol=1e-6)
    u = x.astype(np.float64) / np.sqrt((x.astype(np.float64) ** 2).sum(1))[:, None]
    c = 1.0 - u @ u.T
    np.fill_diagonal(c, np.inf)
    assert np.allclose(D.kdist(v, x, 2, 'cosine'), np.sort(np.sort(c, 1)[:, 1]), atol=1e-6)


def test_eval_explore_flags():
    from argsim_amd import eval_explore as ee
    ap = ee.build_parser()
    base = ['--inputs', 'a.npy', '--labels', 'b.npy']
    A = ap.parse_args(base)
    assert A.dbscan is None and A.dbscan_min == 5 and A.dbscan_sweep is None
    A = ap.parse_args(base + ['--dbscan', '0.25', '--dbscan-min', '3', '--dbscan-sweep', '0.1,0.2,1e-1'])
    assert A.dbscan == 0.25 and A.dbscan_min == 3 and A.dbscan_sweep == [0.1, 0.2, 0.1]
    for flag, bad in (('--dbscan', '0'), ('--dbscan', '-1'), ('--dbscan', 'x'), ('--dbscan', 'inf'), ('--dbscan-min', '0'), ('--dbscan-sweep', '0.1,,2'),
                      ('--dbscan-sweep', '1,0'), ('--dbscan-sweep', ','.join(['1'] * 65))):
        with pytest.raises(SystemExit):
            ap.parse_args(base + [flag, bad])
    x, eps, ms = dr.random_case(65, 4, 0)
    labels = np.array(['t%d-pro-x' % (i % 2) for i in range(65)])
    cols0, lines0 = ee.evaluate(_Stub(), x, None, labels)
    assert list(cols0) == ['cls_euc', 'dist_euc', 'cls_cos', 'dist_cos'] and not any('noise' in line for line in lines0)      # as before
    cols, lines = ee.evaluate(_Stub(), x, None, labels, dbscan=eps, dbscan_min=ms, quality=True)
    assert list(cols)[:4] == list(cols0) and list(cols)[4:] == ['cls_db_euc', 'dist_db_euc', 'cls_db_cos', 'dist_db_cos']
    r = dr.dbscan(x, 0, eps, ms)
    assert np.array_equal(cols['cls_db_euc'], r['label']) and np.array_equal(np.isnan(cols['dist_db_euc']), r['label'] < 0)
    assert "%d clusters, %d noise rows" % (r['stat'][0], r['stat'][3]) in lines
    counts = [i for i, line in enumerate(lines) if line.endswith('noise rows')]
    assert len(counts) == 2 and all(lines[i + 1].startswith('silhouette') for i in counts)
    plain = ee.evaluate(_Stub(), x, None, labels, quality=True)[1]
    assert lines[:len(plain)] == plain
    cols, lines = ee.evaluate(_Stub(), x, None, labels, dbscan_sweep=[eps * 0.8, eps, 50.0], dbscan_min=ms)
    tail = lines[len(lines0):]
    assert lines[:len(lines0)] == lines0 and tail[0] == 'dbscan sweep euc' and tail[1] == 'eps clusters noise silhouette CH DB' and tail[5] == 'dbscan sweep cos'
    rows = [line.split() for line in tail[2:5]]
    assert len(tail) == 10 and [float(r[0]) for r in rows] == [float('%g' % (eps * 0.8)), eps, 50.0] and sum(r[-1] == '*' for r in rows) == 1
    assert rows[2][1:4] == ['1', '0', 'nan']
