"""The float64 reference of avae_kmeans (tests/kmeans_ref.py) against scikit-learn and against brute-force restatements, the margins of
the cases the GPU tests rely on, and the parts of the Python layer that need no device: argument checks, the ctypes declaration against
the header, eval_explore's options."""
import math
import os
import re

import numpy as np
import pytest

import kmeans_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sklearn(x, c0, max_iter=300, tol=0.0):
    cluster = pytest.importorskip('sklearn.cluster')
    km = cluster.KMeans(n_clusters=c0.shape[0], init=np.asarray(c0, np.float64), n_init=1, algorithm='lloyd', max_iter=max_iter, tol=tol)
    return km.fit(np.asarray(x, np.float64))


@pytest.mark.parametrize('case', kr.CASES, ids=kr.CASE_IDS)
def test_lloyd_equals_sklearn(case):
    name, make, k = case
    x = make()
    inits = list(kr.random_init(x, k, 11, 3)) + [kr.case_inits(x, k)["far"][0]]           # the last one relocates
    for j, c0 in enumerate(inits):
        ref = kr.run(x, k, 0, max_iter=300, init=c0[None])
        km = _sklearn(x, c0)
        assert np.array_equal(ref['labels'], km.labels_) and ref['n_iter'] == km.n_iter_, (name, j)
        assert np.allclose(ref['centers'], km.cluster_centers_, rtol=1e-12, atol=1e-13)
        assert abs(ref['inertia'] - km.inertia_) <= 1e-12 * km.inertia_
        assert (ref['relocations'] > 0) == (j == 3)


def test_tol_and_max_iter_stops_equal_sklearn():
    x = kr.gaussian(200, 16, 3)
    c0 = kr.random_init(x, 8, 5, 1)[0]
    full = kr.run(x, 8, 0, max_iter=300, init=c0[None])
    assert full['stop'] == 0 and full['n_iter'] > 4
    cut = kr.run(x, 8, 0, max_iter=3, init=c0[None])
    km = _sklearn(x, c0, max_iter=3)
    assert cut['stop'] == 2 and cut['n_iter'] == km.n_iter_ == 3 and np.array_equal(cut['labels'], km.labels_)
    assert abs(cut['inertia'] - km.inertia_) <= 1e-12 * km.inertia_
    tol = kr.run(x, 8, 0, max_iter=300, tol=0.5, init=c0[None])
    km = _sklearn(x, c0, tol=0.5)
    assert tol['stop'] == 1 and tol['n_iter'] == km.n_iter_ < full['n_iter'] and np.array_equal(tol['labels'], km.labels_)
    assert np.allclose(tol['centers'], km.cluster_centers_, rtol=1e-12, atol=1e-13)
    assert math.isclose(tol['tol_abs'], 0.5 * np.asarray(x, np.float64).var(0).mean(), rel_tol=1e-15)


def test_seeding_against_a_brute_force_restatement():
    x = kr.planted(96, 8, 6, 1)
    X = kr.rows_of(x, 0)
    N, k, seed = 96, 6, 5
    T = kr.trials(k)
    assert T == 3 and kr.trials(1) == 2 and kr.trials(4096) == 10
    for r in range(3):
        got = kr.seeding(X, k, seed, r)['rows']
        u0 = float(kr.uniform01(seed, 7, kr.seed_index(r, 0, 0)))
        assert 0 < u0 < 1 and got[0] == int(u0 * N)
        rows = [int(u0 * N)]
        for c in range(1, k):
            closest = [min(sum((X[i, j] - X[q, j]) ** 2 for j in range(8)) for q in rows) for i in range(N)]
            total = math.fsum(closest)
            best, best_pot = None, None
            for t in range(T):
                u = float(kr.uniform01(seed, 7, kr.seed_index(r, c, t)))
                run, cand = 0.0, N - 1
                for i in range(N):
                    run += closest[i]
                    if run >= u * total:
                        cand = i
                        break
                pot = math.fsum(min(closest[i], sum((X[i, j] - X[cand, j]) ** 2 for j in range(8))) for i in range(N))
                if best is None or pot < best_pot:
                    best, best_pot = cand, pot
            rows.append(best)
        assert got.tolist() == rows, r


def test_the_uniforms_are_the_device_s_fp32_values():
    u = kr.uniform01(3, 7, np.arange(4096))
    assert ((u > 0) & (u <= 1)).all() and (u.astype(np.float32).astype(np.float64) == u).all()
    assert kr.seed_index(2, 3, 1) == ((2 << 20) + 3 << 20) + 1


def test_restarts_do_not_depend_on_n_init():
    x = kr.pad4(kr.gaussian(37, 12, 2))
    three, five = kr.run(x, 5, 0, n_init=3, max_iter=60, seed=9), kr.run(x, 5, 0, n_init=5, max_iter=60, seed=9)
    for r in range(3):
        assert np.array_equal(three['seeds'][r], five['seeds'][r]) and np.array_equal(three['runs'][r]['labels'], five['runs'][r]['labels'])
        assert three['runs'][r]['inertia'] == five['runs'][r]['inertia']
    assert five['best'] == int(np.argmin(five['inertias'])) and five['inertia'] == five['inertias'].min()


def test_cosine_is_the_euclidean_reference_on_unit_rows_plus_the_projection():
    x = kr.planted(257, 16, 9, 3, spread=2.0)
    z = x.copy()
    z[7] = 0                                                 # a zero row stays zero
    Z = kr.rows_of(z, 1)
    assert (Z[7] == 0).all() and np.allclose((np.delete(Z, 7, 0) ** 2).sum(1), 1.0, atol=1e-14)
    assert (kr.project(np.array([[0.0, 0.0], [3.0, 4.0]])) == np.array([[0.0, 0.0], [0.6, 0.8]])).all()      # and a zero centre
    X = kr.rows_of(x, 1)
    c0 = X[[3, 30, 60, 90, 120, 150, 180, 210, 240]]
    cos = kr.lloyd(X, c0, 60, 0.0, metric=1)
    C, prev = c0.copy(), None                                # Euclidean steps on X with the projection in between
    for it in range(60):
        lab = kr.sqdist(X, C).argmin(1)
        C = kr.project(kr.update(X, lab, kr.sqdist(X, C)[np.arange(257), lab], 9, 0)[0])
        if prev is not None and np.array_equal(lab, prev):
            break
        prev = lab
    assert it + 1 == cos['n_iter'] and np.array_equal(lab, cos['labels']) and np.array_equal(C, cos['centers'])
    assert np.allclose((cos['centers'] ** 2).sum(1), 1.0, atol=1e-14)
    dots = (X * cos['centers'][cos['labels']]).sum(1)
    assert math.isclose(cos['inertia'], (2 * (1 - dots)).sum(), rel_tol=1e-12)      # sum 2 (1 - cos)


def test_repeated_points_and_k_equal_to_N():
    pts = kr.gaussian(4, 8, 5)
    x = np.tile(pts, (6, 1))
    dup = kr.run(x, 3, 0, max_iter=1, init=np.stack([pts[0], pts[0], pts[2]])[None])
    assert dup['relocations'] == 1 and dup['stop'] == 2
    full = kr.run(x, 4, 0, max_iter=30, init=pts[None])
    assert np.array_equal(full['labels'], np.tile(np.arange(4), 6)) and full['inertia'] == 0.0 and full['n_iter'] == 1
    x = kr.gaussian(20, 4, 1)
    each = kr.run(x, 20, 0, max_iter=30, seed=2)
    assert sorted(each['labels'].tolist()) == list(range(20)) and each['inertia'] == 0.0
    one = kr.run(x, 1, 0, max_iter=30, seed=2)
    assert (one['labels'] == 0).all() and np.allclose(one['centers'][0], np.asarray(x, np.float64).mean(0), rtol=1e-14, atol=1e-15)


@pytest.mark.parametrize('case', kr.CASES, ids=kr.CASE_IDS)
def test_the_margin_cases_have_margins(case):
    name, make, k = case
    x = make()
    worst = np.inf
    for metric in (0, 1):
        for init in kr.case_inits(x, k).values():
            ref = kr.run(x, k, metric, n_init=init.shape[0], max_iter=30, init=init)
            assert kr.restarts_have_margins(ref), (name, metric, ref['margin'])
            for c0 in init:                                   # each start as a call of its own: the best restart is decided too
                assert kr.has_margins(kr.run(x, k, metric, max_iter=30, init=c0[None]))
            if name.startswith('gauss'):                      # and in the three-restart calls of the Gaussian cases
                assert kr.has_margins(ref), (name, metric, ref['best_margin'])
            worst = min(worst, ref['margin'])
        for max_iter in (1, 30):
            ref = kr.run(x, k, metric, n_init=5, max_iter=max_iter, seed=5)
            assert kr.restarts_have_margins(ref), (name, metric, ref['margin'])
            worst = min(worst, ref['margin'])
    far = kr.run(x, k, 0, max_iter=30, init=kr.case_inits(x, k)['far'])
    assert far['relocations'] >= 1
    print(name, "smallest relative margin %.3g (needed %.3g)" % (worst, kr.MARGIN))


def test_bounds_are_small_and_cover_a_reordered_sum():
    x = kr.gaussian(200, 128, 4)
    X = kr.rows_of(x, 0)
    ref = kr.run(x, 70, 0, max_iter=30, init=kr.random_init(x, 70, 11, 1))
    e = kr.centre_bound(X, ref['labels'], ref['centers'], 0)
    assert e.max() < 1e-12
    other = np.stack([X[ref['labels'] == c][::-1].sum(0) / max((ref['labels'] == c).sum(), 1) for c in range(70)])      # members in descending order
    assert (np.abs(other - ref['centers']) <= e).all()
    D = kr.sqdist(X, ref['centers'])
    flipped = ((X[:, None, ::-1] - ref['centers'][None, :, ::-1]) ** 2).sum(-1)
    assert (np.abs(D - flipped) <= kr.dist_bound(X, ref['centers'])).all()
    assert kr.inertia_bound(X, ref['labels'], ref['centers'], e) < 1e-9 * ref['inertia']


# ---------------------------------------------------------------- the Python layer without a device
def test_check_kmeans_args():
    from argsim_amd.model import _check_kmeans_args as check
    z = np.zeros((20, 8), np.float32)
    check(z, 3)
    check(z, 20, 'cosine', 64, 10000, 0.0, (1 << 64) - 1, np.zeros((64, 20, 8), np.float32))
    check(z, 3, init=np.zeros((3, 8), np.float32), n_init=1)
    bad = [dict(z=[[1.0]]), dict(z=z.astype(np.float64)), dict(z=np.zeros((8,), np.float32)), dict(z=np.zeros((0, 8), np.float32)),
           dict(z=np.zeros((4, 1025), np.float32)), dict(k=0), dict(k=21), dict(k=2.0), dict(metric='manhattan'), dict(n_init=0), dict(n_init=65),
           dict(max_iter=0), dict(max_iter=10001), dict(max_iter=1.5), dict(tol=-1e-3), dict(tol=float('nan')), dict(tol='x'), dict(seed=-1),
           dict(seed=1 << 64), dict(init='random'), dict(init=np.zeros((4, 8), np.float32)), dict(init=np.zeros((2, 3, 8), np.float32), n_init=3)]
    for kw in bad:
        args = dict(z=z, k=3)
        args.update(kw)
        with pytest.raises(ValueError):
            check(**args)


def test_the_declaration_matches_the_header():
    import ctypes as C
    from argsim_amd import lib
    assert 'avae_kmeans' in lib.SIGNATURES
    res, args = lib.SIGNATURES['avae_kmeans']
    assert res is C.c_int and len(args) == 13 and args[4] == C.POINTER(lib.AvaeKmeansConfig)
    with open(os.path.join(ROOT, 'include', 'argsim_vae.h')) as f:
        text = f.read()
    body = re.search(r'typedef struct avae_kmeans_config \{(.*?)\} avae_kmeans_config;', text, re.S).group(1)
    fields = re.findall(r'^\s*(int32_t|double|uint64_t)\s+(\w+);', body, re.M)
    ctype = {'int32_t': C.c_int32, 'double': C.c_double, 'uint64_t': C.c_uint64}
    assert [(n, ctype[t]) for t, n in fields] == list(lib.AvaeKmeansConfig._fields_)
    assert C.sizeof(lib.AvaeKmeansConfig) == 40 and lib.AvaeKmeansConfig.tol.offset == 24 and lib.AvaeKmeansConfig.seed.offset == 32
    decl = re.search(r'int\s+avae_kmeans\((.*?)\);', text, re.S).group(1)
    assert len(re.sub(r'/\*.*?\*/', '', decl, flags=re.S).split(',')) == 13


def test_eval_explore_options():
    from argsim_amd import eval_explore as ee
    ap = ee.build_parser()
    base = ['--inputs', 'a.npy', '--labels', 'b.npy']
    A = ap.parse_args(base)
    assert A.kmeans is None and A.kmeans_init == 10 and A.max_iter == 200 and A.perplexity == 40.0 and A.tsne is None and A.seed == 0
    A = ap.parse_args(base + ['--kmeans', '12', '--kmeans-init', '3'])
    assert A.kmeans == 12 and A.kmeans_init == 3
    for args in (['--kmeans', '0'], ['--kmeans', '-2'], ['--kmeans', 'x'], ['--kmeans', '5', '--kmeans-init', '0']):
        with pytest.raises(SystemExit):
            ap.parse_args(base + args)
    assert ee.COLUMNS == "post topic labels cls_euc dist_euc cls_euc_sp dist_euc_sp cls_cos dist_cos cls_cos_sp dist_cos_sp".split()
    assert ee.KM_COLUMNS == "cls_km_euc dist_km_euc cls_km_euc_sp dist_km_euc_sp cls_km_cos dist_km_cos cls_km_cos_sp dist_km_cos_sp".split()


def test_eval_explore_kmeans_runs_with_a_stub():
    """evaluate() with --kmeans adds the k-means runs behind the affinity runs and leaves those as they are"""
    from argsim_amd import eval_explore as ee

    class Stub:
        def affinity(self, x, metric, max_iter, seed):
            return dict(labels=np.arange(len(x)) % 2, converged=True, n_iter=3)

        def kmeans(self, x, k, metric, n_init, seed):
            return dict(labels=np.arange(len(x)) % k, stop='converged', n_iter=2)

    z = kr.gaussian(12, 4, 1)
    labels = np.array(['t%d-pro-x' % (i % 2) for i in range(12)])
    cols0, lines0 = ee.evaluate(Stub(), z, None, labels)
    cols, lines = ee.evaluate(Stub(), z, z, labels, kmeans=3, kmeans_init=2)
    assert list(cols0) == ['cls_euc', 'dist_euc', 'cls_cos', 'dist_cos'] and lines[:len(lines0)] != [] and lines0 == ee.evaluate(Stub(), z, None, labels, kmeans=None)[1]
    assert [c for c in cols if '_km_' in c] == ['cls_km_euc', 'dist_km_euc', 'cls_km_euc_sp', 'dist_km_euc_sp', 'cls_km_cos', 'dist_km_cos',
                                                 'cls_km_cos_sp', 'dist_km_cos_sp']
    assert lines.count('3 clusters') == 4 and cols['dist_km_cos'].shape == (12,)
