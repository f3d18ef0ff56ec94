"""The float64 reference of avae_silhouette (tests/sil_ref.py) against a brute-force restatement, scikit-learn and scipy, the margins of
the cases the GPU tests rely on, the launch planner (avae_debug_sil_plan, host arithmetic), and the parts of the Python layer that need no
device: label compaction, the ValueErrors, the padding, sweep_k's single silhouette call, eval_explore's flags."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sil_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize('metric', [0, 1, 2], ids=['euc', 'cos', 'sqeuc'])
def test_the_reference_equals_three_plain_loops(metric):
    x = sr.pad4(sr.gaussian(37, 6, 2))
    lab = sr.labels_of(37, 6, 4, empty=(2,))
    lab[::9] = -1                                            # unlabelled rows
    lab[5] = 6                                               # ... and one by a label >= K
    ref = sr.run(x, metric, lab[None], [6])[0]
    a, b, s, near = sr.brute(x, metric, lab, 6)
    bd = sr.bounds(x, metric, ref)
    assert np.array_equal(near, ref['nearest']) and ref['count'][2] == 0 and ref['count'].sum() == (sr._valid(lab, 6) >= 0).sum()
    assert (np.abs(a - ref['a']) <= 2 * bd['a']).all() and (np.abs(b - ref['b']) <= 2 * bd['b']).all() and (np.abs(s - ref['sil']) <= 2 * bd['s']).all()
    off = sr._valid(lab, 6) < 0
    assert (ref['sil'][off] == 0).all() and (ref['a'][off] == 0).all() and (ref['nearest'][off] == -1).all()
    assert abs(ref['score'] - s[~off].mean()) <= 2 * bd['score']
    cm = np.array([s[lab == c].mean() if (lab == c).any() else 0.0 for c in range(6)])
    assert (np.abs(cm - ref['cluster_mean']) <= 2 * bd['cluster_mean']).all() and ref['cluster_mean'][2] == 0


def test_a_nan_row_that_is_unlabelled_enters_nothing():
    x = sr.gaussian(20, 4, 1)
    lab = sr.labels_of(20, 3, 2)
    lab[4] = -1
    xn = x.copy()
    xn[4] = np.nan
    for metric in (0, 1, 2):
        got = sr.run(xn, metric, lab[None], [3])[0]
        keep = np.arange(20) != 4
        want = sr.run(x[keep], metric, lab[keep][None], [3])[0]
        assert np.isfinite(got['sil']).all() and np.isfinite([got['score'], got['ch'], got['db']]).all()
        assert np.allclose(got['sil'][keep], want['sil'], rtol=0, atol=1e-14) and abs(got['ch'] - want['ch']) < 1e-12 and abs(got['db'] - want['db']) < 1e-12


@pytest.mark.parametrize('metric', [0, 1, 2], ids=['euc', 'cos', 'sqeuc'])
@pytest.mark.parametrize('k', [3, 7])
def test_the_reference_equals_sklearn(metric, k):
    """silhouette_samples on the reference's own distance matrix, CH and DB on its rows: within twice the bounds (130 x 12; at K = 3 the
    differences are 0 and 4e-16)"""
    metrics = pytest.importorskip('sklearn.metrics')
    x = sr.pad4(sr.gaussian(130, 12, 4))
    lab = sr.labels_of(130, k, 5)
    ref = sr.run(x, metric, lab[None], [k])[0]
    bd = sr.bounds(x, metric, ref)
    D = sr.distances(x, metric)
    np.fill_diagonal(D, 0.0)
    s = metrics.silhouette_samples(D, lab, metric='precomputed')
    assert (np.abs(s - ref['sil']) <= 2 * bd['s']).all()
    assert abs(metrics.silhouette_score(D, lab, metric='precomputed') - ref['score']) <= 2 * bd['score']
    X = sr.rows_of(x, 1 if metric == 1 else 0)
    ch, db = metrics.calinski_harabasz_score(X, lab), metrics.davies_bouldin_score(X, lab)
    print("CH %.3g (bound %.3g), DB %.3g (bound %.3g)" % (abs(ch - ref['ch']), bd['ch'], abs(db - ref['db']), bd['db']))
    assert abs(ch - ref['ch']) <= 2 * bd['ch'] and abs(db - ref['db']) <= 2 * bd['db']


def test_the_distances_equal_scipy():
    dist = pytest.importorskip('scipy.spatial.distance')
    x = sr.pad4(sr.gaussian(40, 12, 3))
    X = x.astype(np.float64)
    for metric, name in ((0, 'euclidean'), (1, 'cosine'), (2, 'sqeuclidean')):
        D = sr.distances(x, metric)
        assert np.allclose(D, dist.cdist(X, X, name), rtol=1e-12, atol=1e-14)
    x[3] = x[17]                                             # duplicate rows: exactly 0 by differences
    assert sr.distances(x, 0)[3, 17] == 0 and sr.distances(x, 2)[17, 3] == 0
    z = x.copy()
    z[5] = 0                                                 # a zero row stays zero: cosine distance 1 to every row
    assert (np.delete(sr.distances(z, 1)[5], 5) == 1).all()


def test_degenerate_labelings():
    x = sr.gaussian(12, 8, 4)
    one = sr.run(x, 0, np.zeros((1, 12), np.int64), [1])[0]
    assert (one['sil'] == 0).all() and one['score'] == 0 and (one['nearest'] == -1).all() and np.isnan(one['ch']) and np.isnan(one['db'])
    each = sr.run(x, 0, np.arange(12)[None], [12])[0]
    assert (each['sil'] == 0).all() and (each['a'] == 0).all() and np.isnan(each['ch']) and each['db'] == 0
    pts = sr.gaussian(3, 8, 6)
    dup = sr.run(np.repeat(pts, 4, axis=0), 0, np.repeat(np.arange(3), 4)[None], [3])[0]
    assert (dup['a'] == 0).all() and (dup['sil'] == 1).all() and dup['trW'] == 0 and dup['ch'] == 1.0
    none = sr.run(x, 0, np.full((1, 12), -1), [3])[0]
    assert none['score'] == 0 and (none['count'] == 0).all() and np.isnan(none['ch'])


@pytest.mark.parametrize('case', sr.CASES, ids=sr.CASE_IDS)
def test_the_cases_have_margins(case):
    x, labels, K = sr.case_labels(case)
    for metric in (0, 1, 2):
        for l, ref in enumerate(sr.run(x, metric, labels, K)):
            assert sr.has_margins(ref), (case[0], metric, l)
            bd = sr.bounds(x, metric, ref)
            assert bd['s'].max() < 1e-11 and bd['score'] < 1e-11 and not bd['ch'] > 1e-9 and not bd['db'] > 1e-9


def test_bounds_cover_a_reordered_sum():
    x, labels, K = sr.case_labels(sr.CASES[3])
    for metric in (0, 1, 2):
        ref = sr.run(x, metric, labels[:1], K[:1])[0]
        flip = sr.run(x[::-1], metric, labels[:1, ::-1], K[:1])[0]           # every sum in the opposite row order
        bd = sr.bounds(x, metric, ref)
        assert (np.abs(flip['sil'][::-1] - ref['sil']) <= bd['s']).all() and abs(flip['score'] - ref['score']) <= bd['score']
        assert abs(flip['ch'] - ref['ch']) <= bd['ch'] and abs(flip['db'] - ref['db']) <= bd['db']


# ---------------------------------------------------------------- the planner
def _plan(N, dim, K, chunk=0, cus=256):
    from argsim_amd import lib
    K = np.ascontiguousarray(K, np.int32)
    out = np.full(2 * len(K) + 5, -1, np.int32)
    rc = lib.load().avae_debug_sil_plan(N, dim, len(K), K.ctypes.data_as(C.POINTER(C.c_int32)), chunk, cus, out.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0
    ti, tj, npass, limit, staging = out[:5].tolist()
    begin = out[5:5 + 2 * npass:2].tolist()
    nbytes = out[6:6 + 2 * npass:2].tolist()
    return dict(TI=ti, TJ=tj, npass=npass, limit=limit, staging=staging, begin=begin, bytes=nbytes)


def test_the_plan_fits_the_lds_and_covers_every_labeling_once():
    r = np.random.default_rng(1)
    for N in (2, 65, 3000, 1 << 16, 1 << 18):
        for dim in (4, 128, 1024):
            for L in (1, 5, 32, 64):
                for kmax in (2, 33, 700, 4096):
                    for chunk in (0, 4, 24, 100):
                        for cus in (1, 256):
                            K = r.integers(1, kmax + 1, L)
                            K[r.integers(0, L)] = kmax
                            p = _plan(N, dim, K, chunk, cus)
                            assert p['TI'] in (4, 8, 16, 32, 64) and 1 <= p['TJ'] <= 64 and p['limit'] == 160 * 1024
                            assert p['begin'][0] == 0 and p['begin'] == sorted(set(p['begin'])) and p['begin'][-1] < L      # contiguous passes
                            ends = p['begin'][1:] + [L]
                            for b, e, nb in zip(p['begin'], ends, p['bytes']):
                                cols = int(K[b:e].sum())
                                assert p['TI'] * cols * 8 < nb <= p['limit'], (N, L, kmax, chunk)                          # bins + staging fit
                                if chunk:
                                    assert cols <= chunk or e - b == 1
                            if chunk:
                                assert p['TI'] <= max(chunk, 4) and p['TJ'] == min(chunk, 64)
                            else:
                                assert p['TJ'] == 64 and (p['TI'] == 4 or -(-N // p['TI']) >= cus)                          # enough row tiles for the CUs


def test_the_plan_at_k_4096_and_at_a_pass_boundary():
    p = _plan(260, 12, [4096])
    assert p['TI'] == 4 and p['npass'] == 1 and p['bytes'][0] == 4 * 4096 * 8 + p['staging']
    assert _plan(1 << 18, 128, [4096], cus=1)['TI'] == 4
    # two labelings at TI = 4: the staging of a two-labeling pass from a small plan, then sum K at the last column that fits and one more
    small = _plan(16, 12, [2, 2], cus=1 << 20)
    assert small['TI'] == 4 and small['npass'] == 1
    staging = small['bytes'][0] - 4 * 4 * 8
    cols = (small['limit'] - staging) // (4 * 8)
    assert cols > 4096
    fit = _plan(1 << 16, 128, [4096, cols - 4096])
    assert fit['TI'] == 4 and fit['npass'] == 1 and fit['bytes'][0] <= fit['limit'] < fit['bytes'][0] + 32
    over = _plan(1 << 16, 128, [4096, cols - 4095])
    assert over['TI'] == 4 and over['npass'] == 2 and over['begin'] == [0, 1]
    # a larger row tile wherever it costs no further pass: 32 labelings of a k sweep in one pass
    sweep = _plan(1 << 16, 128, list(range(2, 34)))
    assert sweep['npass'] == 1 and sweep['TI'] == 16
    assert _plan(1 << 16, 128, [16])['TI'] == 64 and _plan(3000, 128, [16])['TI'] == 8


# ---------------------------------------------------------------- the Python layer without a device
def _ref_raw(calls):
    """silhouette_raw's stand-in: the float64 reference on what the wrapper hands to the C entry"""
    def raw(vae, x, cfg, label, K, want=()):
        calls.append(dict(x=np.array(x), cfg=(cfg.metric, cfg.L, cfg.reserved, cfg.reserved2), label=np.array(label), K=np.array(K), want=tuple(want)))
        refs = sr.run(x, cfg.metric, label, K)
        L, N, kmax = len(refs), x.shape[0], int(np.max(K))
        out = dict(score=np.array([r['score'] for r in refs]), index=np.array([[r['ch'], r['db']] for r in refs]), count=np.zeros((L, kmax), np.int32),
                   sil=np.stack([r['sil'] for r in refs]), ab=np.stack([np.stack([r['a'], r['b']], -1) for r in refs]),
                   nearest=np.stack([r['nearest'] for r in refs]).astype(np.int32))
        for l, r in enumerate(refs):
            out['count'][l, :K[l]] = r['count']
        return {k: v for k, v in out.items() if k == 'score' or k in want}
    return raw


def test_the_wrapper_compacts_labels_and_maps_them_back():
    from argsim_amd import silhouette as S
    z = sr.gaussian(40, 10, 3)                              # 10 columns: padded with zeros to 12
    labels = np.stack([sr.labels_of(40, 3, 1), sr.labels_of(40, 5, 2)]).astype(np.int64) * 7 + 100
    labels[1, ::6] = -2
    calls = []
    res = S.silhouette(None, z, labels, 'cosine', return_samples=True, raw=_ref_raw(calls))
    (c,) = calls
    assert c['x'].shape == (40, 12) and (c['x'][:, 10:] == 0).all() and np.array_equal(c['x'][:, :10], z) and c['cfg'] == (1, 2, 0, 0)
    assert c['label'].dtype == np.int32 and c['K'].tolist() == [3, 5] and set(c['want']) == {'count', 'index', 'sil', 'ab', 'nearest'}
    assert np.array_equal(c['label'], np.where(labels >= 0, (labels - 100) // 7, -1))
    assert [v.tolist() for v in res['clusters']] == [[100, 107, 114], [100, 107, 114, 121, 128]] and res['n_clusters'].tolist() == [3, 5]
    refs = sr.run(sr.pad4(z), 1, c['label'], c['K'])
    for l, ref in enumerate(refs):
        assert res['score'][l] == ref['score'] and res['ch'][l] == ref['ch'] and res['db'][l] == ref['db']
        assert np.array_equal(res['counts'][l], ref['count']) and np.array_equal(res['samples'][l], ref['sil'])
        assert np.array_equal(res['a'][l], ref['a']) and np.array_equal(res['b'][l], ref['b'])
        assert np.array_equal(res['nearest'][l], np.where(ref['nearest'] >= 0, ref['nearest'] * 7 + 100, -1))
    assert (res['nearest'][1][::6] == -1).all() and (res['samples'][1][::6] == 0).all()
    calls.clear()
    one = S.silhouette(None, z, labels[0], raw=_ref_raw(calls))                        # (N,) labels: no leading axis, no samples asked for
    assert set(calls[0]['want']) == {'count', 'index'} and calls[0]['cfg'] == (0, 1, 0, 0) and 'samples' not in one
    assert np.ndim(one['score']) == 0 and one['clusters'].tolist() == [100, 107, 114] and one['counts'].sum() == 40


def test_the_wrapper_checks_its_arguments():
    import torch
    from argsim_amd import silhouette as S
    z = np.zeros((20, 8), np.float32)
    lab = np.arange(20) % 3
    raw = _ref_raw([])
    S.silhouette(None, sr.gaussian(20, 8, 1), lab, raw=raw)
    S.silhouette(None, torch.as_tensor(sr.gaussian(20, 8, 1)), torch.as_tensor(lab), 'sqeuclidean', raw=raw)
    bad = [dict(z=[[1.0]]), dict(z=z.astype(np.float64)), dict(z=np.zeros((8,), np.float32)), dict(z=np.zeros((1, 8), np.float32), labels=np.zeros(1, int)),
           dict(z=np.zeros((20, 1025), np.float32)), dict(metric='manhattan'), dict(labels=lab.astype(np.float64)), dict(labels=lab[:19]),
           dict(labels=np.zeros((2, 3, 20), int)), dict(labels=np.zeros((65, 20), int)),
           dict(labels=np.zeros(20, int)),                  # one cluster
           dict(labels=np.arange(20)),                      # as many clusters as rows
           dict(labels=np.where(np.arange(20) < 3, np.arange(20), -1)),      # ... as labelled rows
           dict(labels=np.full(20, -1)),                    # nothing labelled
           dict(labels=np.stack([lab, np.zeros(20, int)]))]                  # the second labeling has one cluster
    for kw in bad:
        args = dict(z=z, labels=lab, metric='euclidean')
        args.update(kw)
        with pytest.raises(ValueError):
            S.silhouette(None, args['z'], args['labels'], args['metric'], raw=raw)


def test_sweep_k_makes_one_silhouette_call():
    from argsim_amd import silhouette as S
    z = sr.planted(60, 8, 3, 2)

    class Stub:
        def __init__(self):
            self.km, self.sil = [], []

        def kmeans(self, x, k, metric, n_init, seed):
            self.km.append((k, metric, n_init, seed))
            return dict(labels=np.arange(len(x)) % k, inertia=100.0 / k)

        def silhouette(self, x, labels, metric):
            self.sil.append(np.array(labels))
            return S.silhouette(None, x, labels, metric, raw=_ref_raw([]))

    v = Stub()
    t = S.sweep_k(v, z, range(2, 7), 'cosine', n_init=3, seed=5)
    assert v.km == [(k, 'cosine', 3, 5) for k in range(2, 7)] and len(v.sil) == 1 and v.sil[0].shape == (5, 60)
    assert t['k'].tolist() == [2, 3, 4, 5, 6] and t['best'] == t['k'][int(np.argmax(t['score']))] and t['labels'].shape == (5, 60)
    assert t['score'].shape == t['ch'].shape == t['db'].shape == t['inertia'].shape == (5,)
    with pytest.raises(ValueError):
        S.sweep_k(v, z, range(2, 67))


def test_the_declaration_matches_the_header():
    from argsim_amd import lib
    res, args = lib.SIGNATURES['avae_silhouette']
    assert res is C.c_int and len(args) == 14 and args[4] == C.POINTER(lib.AvaeSilhouetteConfig) and args[6] == C.POINTER(C.c_int32)
    with open(os.path.join(ROOT, 'include', 'argsim_vae.h')) as f:
        text = f.read()
    body = re.search(r'typedef struct avae_silhouette_config \{(.*?)\} avae_silhouette_config;', text, re.S).group(1)
    fields = re.findall(r'^\s*(int32_t)\s+(\w+);', body, re.M)
    assert [(n, C.c_int32) for t, n in fields] == list(lib.AvaeSilhouetteConfig._fields_) and C.sizeof(lib.AvaeSilhouetteConfig) == 16
    decl = re.search(r'int\s+avae_silhouette\((.*?)\);', text, re.S).group(1)
    assert len(re.sub(r'/\*.*?\*/', '', decl, flags=re.S).split(',')) == 14
    assert hasattr(lib.load(), 'avae_debug_sil_plan')


# ---------------------------------------------------------------- eval_explore
class _Vae:
    """affinity and k-means by fixed rules, the scores by the reference"""
    def affinity(self, x, metric, max_iter, seed):
        return dict(labels=np.arange(len(x)) % 2, converged=True, n_iter=3)

    def kmeans(self, x, k, metric, n_init, seed):
        return dict(labels=np.arange(len(x)) % k, stop='converged', n_iter=2, inertia=1.0 / k)

    def silhouette(self, x, labels, metric, return_samples=False):
        from argsim_amd import silhouette as S
        return S.silhouette(None, x, labels, metric, return_samples, raw=_ref_raw([]))

    def sweep_k(self, x, ks, metric, n_init=10, seed=0):
        from argsim_amd import silhouette as S
        return S.sweep_k(self, x, ks, metric, n_init, seed)


def test_eval_explore_flags():
    from argsim_amd import eval_explore as ee
    ap = ee.build_parser()
    base = ['--inputs', 'a.npy', '--labels', 'b.npy']
    A = ap.parse_args(base)
    assert A.quality is False and A.sweep is None
    A = ap.parse_args(base + ['--quality', '--sweep', '2:10:4'])
    assert A.quality is True and A.sweep == [2, 6, 10] and ap.parse_args(base + ['--sweep', '3:5']).sweep == [3, 4, 5]
    for bad in ('1:5', '5:3', '2', '2:5:0', 'a:b', '2:100'):
        with pytest.raises(SystemExit):
            ap.parse_args(base + ['--sweep', bad])
    z = sr.gaussian(12, 4, 1)
    labels = np.array(['t%d-pro-x' % (i % 2) for i in range(12)])
    cols0, lines0 = ee.evaluate(_Vae(), z, z, labels, kmeans=3, kmeans_init=2)
    assert not any('silhouette' in line or 'sweep' in line for line in lines0)                          # without the flags: as before
    assert (cols0, lines0)[1] == ee.evaluate(_Vae(), z, z, labels, 0, 200, 3, 2, False, None)[1]
    cols, lines = ee.evaluate(_Vae(), z, z, labels, kmeans=3, kmeans_init=2, quality=True)
    assert list(cols) == list(cols0) and [line for line in lines if not line.startswith('silhouette')] == lines0
    qual = [i for i, line in enumerate(lines) if line.startswith('silhouette')]
    assert len(qual) == 8 and all(lines[i - 1].endswith('clusters') for i in qual)                       # one behind every run
    euc = sr.run(sr.pad4(z), 0, (np.arange(12) % 2)[None], [2])[0]
    assert lines[qual[0]] == "silhouette %.4f  CH %.2f  DB %.4f" % (euc['score'], euc['ch'], euc['db'])
    cos = sr.run(sr.pad4(z), 1, (np.arange(12) % 3)[None], [3])[0]
    assert lines[qual[6]] == "silhouette %.4f  CH %.2f  DB %.4f" % (cos['score'], cos['ch'], cos['db'])
    cols, lines = ee.evaluate(_Vae(), z, None, labels, sweep=[2, 3, 4])
    assert lines[:len(ee.evaluate(_Vae(), z, None, labels)[1])] == ee.evaluate(_Vae(), z, None, labels)[1]
    tail = lines[len(ee.evaluate(_Vae(), z, None, labels)[1]):]
    assert tail[0] == 'sweep euc' and tail[1] == 'k silhouette CH DB' and tail[5] == 'sweep cos' and len(tail) == 10
    rows = [line.split() for line in tail[2:5]]
    assert [r[0] for r in rows] == ['2', '3', '4'] and sum(len(r) == 5 and r[4] == '*' for r in rows) == 1
    best = max(rows, key=lambda r: float(r[1]))
    assert best[-1] == '*'
    one = ee.quality_line(_Vae(), z, np.zeros(12, int), 'euclidean')
    assert one == "silhouette n/a (1 clusters)"
