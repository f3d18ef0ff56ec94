"""The float64 reference of affinity propagation (tests/ap_ref.py) against scikit-learn and against its own fp32 emulation, the margin
conditions that make the GPU test's exact comparisons legitimate, the teeth of the step bounds, and the host side of
argsim_amd/affinity.py and eval_explore.py.  No GPU."""
import csv
import warnings

import numpy as np
import pytest

import ap_ref as ar
from argsim_amd import affinity as af

_RUNS = {}


def _case(i):
    """(S, float64 run, fp32 run) of margin case i, computed once and never modified"""
    if i not in _RUNS:
        name, make, metric = ar.CASES[i]
        S, _ = ar.prepared(ar.pad4(make()), metric)
        S.setflags(write=False)
        _RUNS[i] = (S, ar.run(S), ar.run(S.astype(np.float32), one=ar.step_fp32))
    return _RUNS[i]


@pytest.mark.parametrize('i', range(len(ar.CASES)), ids=ar.CASE_IDS)
def test_margin_cases_have_their_margins_and_fp32_agrees(i):
    S, ref, r32 = _case(i)
    print(ar.CASE_IDS[i], ref['n_iter'], ref['K'], ref['margins'])
    assert ref['converged'] == 1 and ref['K'] > 1 and ar.has_margins(ref)
    assert r32['n_iter'] == ref['n_iter'] and r32['converged'] == ref['converged']
    assert np.array_equal(r32['exemplars'], ref['exemplars']) and np.array_equal(r32['label'], ref['label'])
    assert np.array_equal(r32['E'], ref['E'])


@pytest.mark.parametrize('i', range(len(ar.CASES)), ids=ar.CASE_IDS)
def test_reference_agrees_with_sklearn(i):
    cluster = pytest.importorskip('sklearn.cluster')
    S, ref, _ = _case(i)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ap = cluster.AffinityPropagation(affinity='precomputed', random_state=0).fit(S.copy())
    assert np.array_equal(ap.cluster_centers_indices_, ref['exemplars'])
    assert np.array_equal(ap.cluster_centers_indices_[ap.labels_], ref['label'])
    assert abs(ap.n_iter_ - ref['n_iter']) <= 1                  # sklearn perturbs S by its own noise


def test_reference_follows_sklearns_lines_iteration_by_iteration():
    S, ref, _ = _case(1)
    A, R = np.zeros_like(S), np.zeros_like(S)
    A2, R2 = np.zeros_like(S), np.zeros_like(S)
    scale = np.abs(S).max()
    for it in range(ref['n_iter']):
        A, R, E = ar.step(S, A, R, 0.5)
        E2 = ar.sklearn_step(S, A2, R2, 0.5)
        assert np.abs(A - A2).max() <= 1e-12 * scale and np.abs(R - R2).max() <= 1e-12 * scale, it
        assert np.array_equal(E, E2) and np.array_equal(E, ref['E'][it]), it
    assert np.array_equal(A, ref['A'])


def test_stopping_rule_and_the_short_runs():
    S, ref, _ = _case(1)
    E = ref['E']
    n = ref['n_iter']
    assert n > 15 and (E[n - 15:] == E[n - 1]).all() and not (E[n - 16:n - 1] == E[n - 2]).all()      # the first full window that held
    for mi in (1, 2):
        short = ar.run(S, max_iter=mi, convergence_iter=1)
        assert short['K'] == 0 and (short['label'] == -1).all() and short['converged'] == 0
    x = ar.pad4(ar.CASES[1][1]())
    low = ar.run(ar.prepared(x, 1, preference=-1e6)[0], max_iter=40)
    assert (low['n_iter'], low['converged'], low['K']) == (40, 0, 0)


def test_median_and_similarity():
    x = ar.pad4(ar.gaussian(5, 12, 1))
    for metric in (0, 1):
        S = ar.similarity(x, metric)
        assert np.array_equal(S, S.T) and not np.diag(S).any()
        for i in range(5):
            for k in range(5):
                a, b = x[i].astype(np.float64), x[k].astype(np.float64)
                want = -((a - b) ** 2).sum() if metric == 0 else -(1 - a @ b / np.sqrt((a @ a) * (b @ b)))
                assert i == k or abs(S[i, k] - want) <= 1e-12 * abs(want)
        P, pref = ar.prepared(x, metric)
        assert (np.diag(P) == pref).all() and pref == np.sort(S.astype(np.float32).ravel())[12]          # 25 entries: the middle one
    P, pref = ar.prepared(x[:2], 0)
    s = np.float32(ar.similarity(x[:2], 0)[0, 1])
    assert pref == s / np.float32(2)                                                                     # (s + 0) / 2


def test_generator_copy_and_noise_bound():
    idx = np.arange(1 << 16)
    u = ar.uniform01(7, 5, idx)
    assert 0 < u.min() and u.max() < 1 and abs(u.mean() - 0.5) < 0.01
    assert not np.array_equal(u, ar.uniform01(8, 5, idx)) and not np.array_equal(u, ar.uniform01(7, 4, idx))
    n = ar.normal01(7, 5, idx)
    assert abs(n.mean()) < 0.02 and abs(n.std() - 1) < 0.02 and np.abs(n).max() <= ar.NORMAL_MAX < 6
    assert int(ar.mix64(np.uint64(0))) == 0xE220A8397B1DCDAF                                            # splitmix64's first output for state 0


def _state(N, seed):
    r = np.random.default_rng(seed)
    S, _ = ar.prepared(ar.pad4(ar.gaussian(N, 12, seed)), 0)
    A = (-np.abs(r.standard_normal((N, N))) * 3).astype(np.float32)
    R = (r.standard_normal((N, N)) * 3).astype(np.float32)
    np.fill_diagonal(R, 60.0)                                # exemplar-like columns: R_kk stays positive through the step
    return S, A, R


def _inside(S, A, R, An, Rn, lam):
    """a step's result against float64 within the bounds, the way the GPU test checks the device's"""
    S, A, R = (np.asarray(v, np.float64) for v in (S, A, R))
    okR = np.abs(Rn.astype(np.float64) - ar.responsibilities(S, A, R, lam)) <= ar.bound_R(S, A, R)
    okA = np.abs(An.astype(np.float64) - ar.availabilities(A, Rn.astype(np.float64), lam)) <= ar.bound_A(A, Rn)
    return okR.all(), okA.all()


def test_step_bounds_hold_for_the_emulation_and_catch_the_two_mistakes():
    for N, seed, lam in ((37, 1, 0.5), (96, 2, 0.8125)):
        S, A, R = _state(N, seed)
        An, Rn, _ = ar.step_fp32(S, A, R, lam)
        assert _inside(S, A, R, An, Rn, lam) == (True, True)
        An, Rn, _ = ar.step_fp32(S, A, R, lam, bug='second')
        assert not _inside(S, A, R, An, Rn, lam)[0]
        An, Rn, _ = ar.step_fp32(S, A, R, lam, bug='diag')
        assert _inside(S, A, R, An, Rn, lam) == (True, False)
    for i in range(len(ar.CASES)):                           # and along every margin case's own trajectory
        S, ref, _ = _case(i)
        A, R = np.zeros(S.shape, np.float32), np.zeros(S.shape, np.float32)
        for it in range(min(ref['n_iter'], 12)):
            An, Rn, _ = ar.step_fp32(S, A, R, 0.5)
            assert _inside(S, A, R, An, Rn, 0.5) == (True, True), (i, it)
            A, R = An, Rn


def test_labels_tail():
    S = -np.array([[0, 1, 4, 9.], [1, 0, 1, 4], [4, 1, 0, 1], [9, 4, 1, 0]])
    np.fill_diagonal(S, -2.0)
    label, ex, _ = ar.labels(S, np.array([True, False, False, True]))
    # first assignment: 1 -> 0 (S -1 against -4), 2 -> 3; clusters {0, 1} and {2, 3} tie within themselves: the lowest member stays
    assert ex.tolist() == [0, 2] and label.tolist() == [0, 0, 2, 2]
    label, ex, _ = ar.labels(S, np.zeros(4, bool))
    assert (label == -1).all() and len(ex) == 0


def test_centroids_distances_and_purity():
    r = np.random.default_rng(0)
    z = r.standard_normal((24, 6)).astype(np.float32)
    labels = r.integers(0, 4, 24)
    labels[:4] = np.arange(4)
    ids, ctr = af.centroids(z, labels)
    assert ids.tolist() == [0, 1, 2, 3]
    for c in ids:
        assert np.allclose(ctr[c], z[labels == c].astype(np.float64).mean(0), rtol=1e-14)
    de, dc = af.dist_to_centroids(z, labels, 'sqeuclidean'), af.dist_to_centroids(z, labels, 'cosine')
    for i in range(24):
        c, v = ctr[labels[i]], z[i].astype(np.float64)
        assert np.isclose(de[i], ((v - c) ** 2).sum(), rtol=1e-13) and np.isclose(dc[i], 1 - v @ c / np.sqrt((v @ v) * (c @ c)), rtol=1e-13)
    with pytest.raises(ValueError):
        af.dist_to_centroids(z, labels, 'manhattan')
    # purity, restated directly: per cluster in order of first appearance (members, share inside the mask), sorted by descending share
    pred = np.array([3, 3, 1, 1, 1, 2, 2, 0, 3, 2])
    mask = np.array([1, 1, 1, 0, 0, 1, 1, 1, 0, 1], bool)
    want = []
    for c in (3, 1, 2, 0):
        n, hit = int((pred == c).sum()), int((pred[mask] == c).sum())
        want.append((c, n, hit / n))
    want.sort(key=lambda t: -t[2])
    assert af.purity(pred, mask) == [t for t in want if t[2] >= 0.5 and t[1] >= 2] == [(2, 3, 1.0), (3, 3, 2 / 3)]
    assert af.purity(pred, mask, min_acc=0.0, min_cnt=1) == want


class _FakeVAE:
    """VAE.affinity from the float64 reference: what argsim_amd.affinity.affinity does with the raw call's result"""
    device = 'cpu'

    def raw(self, vae, x, cfg, want_s=False, messages=False, a=None, r=None):
        self.seen = (x, cfg)
        S, _ = ar.prepared(x, cfg.metric, cfg.preference if cfg.use_preference else None)
        res = ar.run(S, cfg.damping, cfg.max_iter, cfg.convergence_iter)
        out = dict(label=res['label'].astype(np.int32), stat=np.array([res['n_iter'], res['converged'], res['K'], 0], np.int32))
        if want_s:
            out.update(s=S.astype(np.float32), a=res['A'].astype(np.float32), r=res['R'].astype(np.float32))
        return out

    def affinity(self, z, metric='euclidean', **kw):
        return af.affinity(self, z, metric, raw=self.raw, **kw)


def test_affinity_relabels_and_checks_its_arguments():
    fake = _FakeVAE()
    z = ar.CASES[1][1]()                                     # 37 x 12
    res = fake.affinity(z, 'cosine', return_messages=True)
    _, ref, _ = _case(1)
    assert np.array_equal(res['exemplars'], ref['exemplars']) and np.array_equal(res['exemplars'][res['labels']], ref['label'])
    assert res['n_iter'] == ref['n_iter'] and res['converged'] is True and res['s'].shape == (37, 37)
    x, cfg = fake.seen
    assert x.shape == (37, 12) and x.dtype == np.float32 and (cfg.metric, cfg.max_iter, cfg.convergence_iter, cfg.use_preference, cfg.noise) == (1, 200, 15, 0, 1)
    fake.affinity(z[:, :10], 'euclidean', preference=-3.5, noise=False, seed=11, damping=0.75)
    x, cfg = fake.seen
    assert x.shape == (37, 12) and not x[:, 10:].any()       # 10 columns: padded with zeros to 12
    assert (cfg.metric, cfg.use_preference, cfg.preference, cfg.noise, cfg.seed, cfg.damping) == (0, 1, -3.5, 0, 11, 0.75)
    none = fake.affinity(z, 'cosine', max_iter=1, convergence_iter=1)
    assert (none['labels'] == -1).all() and len(none['exemplars']) == 0 and none['converged'] is False
    bad = [dict(z=z.astype(np.float64)), dict(z=[[1.0]]), dict(z=z[0]), dict(z=np.zeros((0, 4), np.float32)), dict(z=np.zeros((3, 1028), np.float32)),
           dict(metric='manhattan'), dict(z=z, metric='precomputed'), dict(preference=float('nan')), dict(damping=0.4), dict(damping=1.0),
           dict(max_iter=0), dict(max_iter=10001), dict(max_iter=2.5), dict(convergence_iter=0), dict(convergence_iter=201), dict(seed=-1)]
    for kw in bad:
        args = dict(dict(z=z, metric='euclidean'), **kw)
        with pytest.raises(ValueError):
            fake.affinity(args.pop('z'), args.pop('metric'), **args)


def test_eval_explore_lines_and_csv(tmp_path, capsys, monkeypatch):
    from argsim_amd import eval_cluster, eval_explore
    r = np.random.default_rng(9)
    names = np.array(['%s-%s-%d' % (t, s, q) for t in ('abortion', 'gun') for s in ('p', 'c') for q in (1, 2) for _ in range(3)])      # 24 rows
    _, ids = np.unique(names, return_inverse=True)
    z = (8.0 * r.standard_normal((8, 6))[ids] + r.standard_normal((24, 6))).astype(np.float32)
    np.save(str(tmp_path / 'z.npy'), z)
    np.save(str(tmp_path / 'l.npy'), names)
    np.save(str(tmp_path / 'p.npy'), np.array(['post %d, "quoted"' % i for i in range(24)]))
    monkeypatch.setattr(eval_cluster, 'make_vae', lambda device: _FakeVAE())
    out = tmp_path / 'c.csv'
    cols = eval_explore.main(['--inputs', str(tmp_path / 'z.npy'), '--labels', str(tmp_path / 'l.npy'), '--posts', str(tmp_path / 'p.npy'), '--csv', str(out)])
    lines = capsys.readouterr().out.strip().split('\n')
    topics = np.array([n.split('-')[0] for n in names])
    want = []
    for run, dist in (('euc', 'sqeuclidean'), ('cos', 'cosine')):
        pred = cols['cls_' + run]
        assert pred.min() == 0 and len(set(pred.tolist())) == pred.max() + 1 > 1
        for t in ('abortion', 'gun'):
            want.append(" ".join([t.ljust(9)] + ["{:.3f}|{:03d}|{:03d}".format(a, n, c) for c, n, a in af.purity(pred, topics == t)]))
        want.append("%d clusters" % (pred.max() + 1))
        assert np.array_equal(cols['dist_' + run], af.dist_to_centroids(z, pred, dist))
    assert lines == want and any('|' in line for line in lines)
    with open(str(out), newline='') as f:
        rows = list(csv.reader(f))
    assert rows[0] == ['id', 'post', 'topic', 'labels', 'cls_euc', 'dist_euc', 'cls_cos', 'dist_cos'] and len(rows) == 25
    assert rows[3][:5] == ['2', 'post 2, "quoted"', 'abortion', str(names[2]), str(cols['cls_euc'][2])] and float(rows[3][5]) == cols['dist_euc'][2]
    # with the sampled embeddings: four runs, the reference's column order
    np.save(str(tmp_path / 's.npy'), z + np.float32(0.01))
    eval_explore.main(['--inputs', str(tmp_path / 'z.npy'), '--labels', str(tmp_path / 'l.npy'), '--inputs-sp', str(tmp_path / 's.npy'), '--csv', str(out)])
    capsys.readouterr()
    with open(str(out), newline='') as f:
        assert next(csv.reader(f)) == ['id'] + eval_explore.COLUMNS
