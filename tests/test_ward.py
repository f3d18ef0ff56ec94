"""the float64 reference of the Ward clustering (tests/ward_ref.py) and the host side of argsim_amd/cluster.py, without a GPU: the
reference reproduces scipy's linkage and scikit-learn's AgglomerativeClustering, the two scores reproduce scikit-learn's and two
values worked out by hand, the inputs of tests/test_gpu_ward.py are what it says (every merge of an exact case decided by a gap
>= 2^-20), rows are gathered by group as avae_ward takes them, and the command line prints the reference's lines."""
import numpy as np
import pytest

import ward_ref as wr
from argsim_amd import cluster, eval_cluster

_REF = {}


def _ref(case):
    if case not in _REF:
        _REF[case] = wr.ward(wr.case_inputs(case))
    return _REF[case]


@pytest.mark.parametrize('case', wr.CASES, ids=wr.CASE_IDS)
def test_reference_is_scipy_and_sklearn(case):
    hier = pytest.importorskip('scipy.cluster.hierarchy')
    sk = pytest.importorskip('sklearn.cluster')
    x, ref = wr.case_inputs(case), _ref(case)
    n = x.shape[0]
    Z = hier.linkage(x.astype(np.float64), 'ward')
    mine = cluster.linkage_matrix(ref['pair'], ref['delta'], ref['size'])
    assert np.array_equal(mine[:, [0, 1, 3]], Z[:, [0, 1, 3]])
    assert np.abs(mine[:, 2] - Z[:, 2]).max() <= 2.0 ** -23 * Z[:, 2].max()          # sqrt of a value rounded once to fp32
    labels = sk.AgglomerativeClustering(n_clusters=5).fit(x).labels_
    assert cluster.adjusted_rand(labels, wr.cut(ref['pair'], n, 5)) == 1.0
    # the certificate holds for the reference's own tree, and follow's values are the tree's
    chosen, least = wr.follow(x, ref['pair'])
    assert (chosen <= (1 + 2.0 ** -21) * least).all() and (np.abs(ref['delta'] - chosen) <= 2.0 ** -24 * chosen).all()
    # .. and tells a wrong tree: swap in a pair that is not the nearest
    wrong = ref['pair'].copy()
    wrong[0] = (0, 1) if tuple(wrong[0]) != (0, 1) else (0, 2)
    chosen, least = wr.follow(x, wrong[:1])
    assert chosen[0] > (1 + 2.0 ** -21) * least[0]


@pytest.mark.parametrize('case', wr.CASES, ids=wr.CASE_IDS)
def test_exact_cases_are_decided_by_a_gap(case):
    ref = _ref(case)
    print("minimum gap %.3g" % ref['gap'].min())
    assert ref['gap'].min() >= wr.MIN_GAP and ref['unique'].all()


def test_cases_hold_what_the_gpu_test_says():
    assert sorted(c[1] for c in wr.CASES) == [4, 36, 128, 1024]
    ns = [c[0] for c in wr.CASES]
    assert any(n < 64 for n in ns) and any(64 < n < 256 for n in ns) and any(n > 256 for n in ns) and all(n <= 300 for n in ns)
    assert wr.BIG[0] > 1024 and wr.BIG[1] == 36 and wr.GROUP_SIZES == [1, 2, 3, 64, 65, 200]
    for case in wr.CASES + [wr.NEAR_TIES, wr.BIG]:
        x = wr.case_inputs(case)
        assert x.dtype == np.float32 and np.isfinite(x).all() and x.shape == (case[-3], case[-2])
    near = wr.ward(wr.case_inputs(wr.NEAR_TIES))
    assert near['gap'].min() < 2.0 ** -22 or not near['unique'].all()          # the lattice has near-ties: no exact case
    m = 9
    x = wr.tie_inputs(m)
    assert x.shape == (4 * m, 4) and len(np.unique(x, axis=0)) == m and np.array_equal(x, np.round(x)) and np.abs(x).max() <= 3
    ref = wr.ward(x)
    assert not ref['delta'][:3 * m].any() and ref['delta'][3 * m] > 0 and not ref['unique'][0]
    assert (ref['pair'][:3, 0] == 0).all()                                      # ties go to the lowest a: row 0's copies first
    assert (np.diff(ref['pair'][:3 * m, 0]) >= 0).all()


def test_cut_and_relabel():
    pair = np.array([[1, 3], [0, 2], [0, 1]])
    assert list(wr.cut(pair, 4, 4)) == [0, 1, 2, 3] and list(wr.cut(pair, 4, 3)) == [0, 1, 2, 1]
    assert list(wr.cut(pair, 4, 2)) == [0, 1, 0, 1] and list(wr.cut(pair, 4, 1)) == [0, 0, 0, 0]
    assert list(cluster.relabel([5, 5, 2, 9, 2, 5])) == [0, 0, 1, 2, 1, 0]
    Z = cluster.linkage_matrix(pair, np.array([0.5, 2.0, 8.0], np.float32), [2, 2, 4])
    assert np.array_equal(Z, [[1, 3, 1.0, 2], [0, 2, 2.0, 2], [4, 5, 4.0, 4]])


def test_scores_by_hand_and_against_sklearn():
    # a = {0,1,2 | 3,4,5}, b = {0,1 | 2,3 | 4,5}: contingency [[2,1,0],[0,1,2]].  Pairs together in both: 2; in a: 6; in b: 3; of 15.
    # ARI = (2 - 6 * 3 / 15) / ((6 + 3) / 2 - 6 * 3 / 15) = 0.8 / 3.3 = 8 / 33
    a, b = [0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 2, 2]
    assert abs(cluster.adjusted_rand(a, b) - 8 / 33) <= 1e-15
    # H(a) = ln 2, H(b) = ln 3, H(a | b) = (1 / 3) ln 2 (only b's middle cluster is mixed): MI = (2 / 3) ln 2;
    # homogeneity 2 / 3, completeness (2 / 3) ln 2 / ln 3, V = their harmonic mean
    h, c = 2 / 3, 2 / 3 * np.log(2) / np.log(3)
    assert abs(cluster.v_measure(a, b) - 2 * h * c / (h + c)) <= 1e-15
    assert cluster.adjusted_rand(a, [7, 7, 7, 3, 3, 3]) == 1.0 and abs(cluster.v_measure(a, [7, 7, 7, 3, 3, 3]) - 1.0) <= 1e-15
    assert cluster.adjusted_rand([0, 0, 0], [0, 0, 0]) == 1.0 and cluster.v_measure([0, 0, 0], [0, 0, 0]) == 1.0
    assert cluster.v_measure([0, 0, 1, 1], [0, 0, 0, 0]) == 0.0
    metrics = pytest.importorskip('sklearn.metrics')
    r = np.random.default_rng(0)
    for n, ka, kb in ((50, 3, 4), (400, 7, 7), (1000, 30, 2), (30, 30, 5), (200, 1, 6)):
        u, v = r.integers(0, ka, n), r.integers(0, kb, n)
        v[: n // 2] = u[: n // 2] % kb
        assert abs(cluster.adjusted_rand(u, v) - metrics.adjusted_rand_score(u, v)) <= 1e-12
        assert abs(cluster.v_measure(u, v) - metrics.v_measure_score(u, v)) <= 1e-12
    names = np.array(['x-%d' % i for i in u])
    assert cluster.adjusted_rand(names, v) == cluster.adjusted_rand(u, v)


def test_rows_are_gathered_by_group():
    groups = np.array(['t2', 't1', 't2', 't1', 't1', 't3'])
    keys, rows, off = cluster.gather_groups(groups, 6)
    assert keys == ['t2', 't1', 't3'] and [list(r) for r in rows] == [[0, 2], [1, 3, 4], [5]] and list(off) == [0, 2, 5, 6] and off.dtype == np.int32
    keys, rows, off = cluster.gather_groups(None, 4)
    assert keys == [0] and list(rows[0]) == [0, 1, 2, 3] and list(off) == [0, 4]
    keys, rows, off = cluster.gather_groups({('a', 'p'): np.array([3, 1]), 'all': np.arange(5)}, 5)
    assert keys == [('a', 'p'), 'all'] and list(rows[0]) == [3, 1] and list(off) == [0, 2, 7]
    z = np.arange(30, dtype=np.float32).reshape(5, 6)
    x = cluster.gathered(z, rows)
    assert x.shape == (7, 8) and x.flags['C_CONTIGUOUS'] and np.array_equal(x[:, :6], z[[3, 1, 0, 1, 2, 3, 4]]) and not x[:, 6:].any()
    for bad in (dict(groups=np.zeros(5)), dict(groups={'a': np.array([6])}), dict(groups={'a': np.array([], np.int64)}), dict(groups={'a': np.array([0.5])}),
                dict(groups={})):
        with pytest.raises(ValueError):
            cluster.gather_groups(bad['groups'], 6)

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("the device was touched: %s" % name)
    for bad in (z.astype(np.float64), np.zeros(6, np.float32), np.zeros((3, 1028), np.float32), [[0.0] * 4]):
        with pytest.raises(ValueError):
            cluster.ward(NoDevice(), bad)
    with pytest.raises(ValueError):
        cluster.cluster_eval(NoDevice(), z, np.zeros(4))


def _stub_raw(vae, x, group_off):
    """avae_ward's outputs from the reference"""
    outs = [wr.ward(x[group_off[g]:group_off[g + 1]]) for g in range(len(group_off) - 1)]
    return tuple(np.concatenate([o[k] for o in outs], axis=0) for k in ('pair', 'delta', 'size'))


def _stub_cut(vae, pair, group_off, k):
    out = []
    for g in range(len(group_off) - 1):
        n = group_off[g + 1] - group_off[g]
        out.append(wr.cut(pair[group_off[g] - g:group_off[g + 1] - g - 1], n, k[g]))
    return np.concatenate(out).astype(np.int32)


class _StubVAE:
    """VAE.ward / ward_cut / cluster_eval with the device call stubbed by the reference"""

    def ward(self, z, groups=None):
        return cluster.ward(self, z, groups, raw=_stub_raw)

    def ward_cut(self, res, k):
        return cluster.ward_cut(self, res, k, raw=_stub_cut)

    def cluster_eval(self, z, gold, groups=None):
        return cluster.cluster_eval(self, z, gold, groups, raw=_stub_raw, raw_cut=_stub_cut)


def _labelled():
    r = np.random.default_rng(9)
    names = np.array(['%s-%s-%d' % (t, s, q) for t in ('gun', 'abortion') for s in ('p', 'c') for q in (1, 2) for _ in range(10)])
    names = names[r.permutation(len(names))]
    _, ids = np.unique(names, return_inverse=True)
    z = (30.0 * r.standard_normal((8, 12))[ids] + r.standard_normal((len(names), 12))).astype(np.float32)
    return z, names


def test_cluster_eval_and_the_command_line_with_the_device_stubbed(tmp_path, capsys, monkeypatch):
    sk = pytest.importorskip('sklearn.cluster')
    metrics = pytest.importorskip('sklearn.metrics')
    z, names = _labelled()
    vae = _StubVAE()
    parts = eval_cluster.split_labels(names)
    sel = eval_cluster.selections(parts, 'stance')
    assert list(sel) == [('abortion', 'c'), ('abortion', 'p'), ('gun', 'c'), ('gun', 'p')]
    assert list(eval_cluster.selections(parts, 'topic')) == ['abortion', 'gun'] and ('gun', '2') in eval_cluster.selections(parts, 'reason')
    for key, rows in sel.items():
        assert all(parts[i][:2] == key for i in rows) and len(rows) == 20
    scores, lines = eval_cluster.evaluate(vae, z, names, 'stance')
    # the reference's own computation (eval_clustering.py:95-103), selection by selection
    want = []
    for key, rows in sel.items():
        y = names[rows]
        pred = sk.AgglomerativeClustering(n_clusters=len(set(y))).fit(z[rows]).labels_
        want.append("{:<20s}\tARS: {:.4F}\tV_MSR: {:.4f}".format(str(key), metrics.adjusted_rand_score(y, pred), metrics.v_measure_score(y, pred)))
    assert lines == want and lines[0].startswith("('abortion', 'c')   \tARS: 1.0000\tV_MSR: 1.0000")
    # --by all: eval_clustering_explorative.py:138-176
    scores, lines = eval_cluster.evaluate(vae, z, names, 'all')
    topics = np.array([p[0] for p in parts])
    order = list(dict.fromkeys(topics.tolist()))
    pred_t = sk.AgglomerativeClustering(n_clusters=2).fit(z).labels_
    pred_r = sk.AgglomerativeClustering(n_clusters=8).fit(z).labels_
    want = ["TOPIC:  ARS: {:.4F}\tV_MSR: {:.4f}".format(metrics.adjusted_rand_score(topics, pred_t), metrics.v_measure_score(topics, pred_t)),
            "REASON: ARS: {:.4F}\tV_MSR: {:.4f}".format(metrics.adjusted_rand_score(names, pred_r), metrics.v_measure_score(names, pred_r))]
    for t in order:
        rows = np.flatnonzero(topics == t)
        pred = sk.AgglomerativeClustering(n_clusters=4).fit(z[rows]).labels_
        want.append("{:<20s}: ARS: {:.4F}\tV_MSR: {:.4f}".format(t, metrics.adjusted_rand_score(names[rows], pred), metrics.v_measure_score(names[rows], pred)))
    assert lines == want
    # the command line: files in, lines out, --dims selects columns
    monkeypatch.setattr(eval_cluster, 'make_vae', lambda device: vae)
    np.save(str(tmp_path / 'z.npy'), np.concatenate([z, np.zeros((len(z), 3), np.float32)], axis=1))
    np.save(str(tmp_path / 'l.npy'), names)
    np.save(str(tmp_path / 'd.npy'), np.arange(12))
    got = eval_cluster.main(['--inputs', str(tmp_path / 'z.npy'), '--labels', str(tmp_path / 'l.npy'), '--by', 'all', '--dims', str(tmp_path / 'd.npy')])
    assert capsys.readouterr().out.strip().split('\n') == want and got == scores
    with pytest.raises(ValueError):
        eval_cluster.split_labels(['a-b'])
    # ward_cut: one k, one per group, a dict; a k out of range raises
    res = vae.ward(z, topics)
    assert res['keys'] == order and list(res['group_off']) == [0, 40, 80]
    for k in (4, [4, 4], {order[0]: 4, order[1]: 4}):
        labels = vae.ward_cut(res, k)
        assert all(cluster.adjusted_rand(names[res['groups'][t]['rows']], labels[t]) == 1.0 for t in order)
    with pytest.raises(ValueError):
        vae.ward_cut(res, 41)
