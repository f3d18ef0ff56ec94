"""the float64 reference of the linear probes (tests/probe_ref.py) and the host side of argsim_amd/probe.py, without a GPU: the
reference reproduces scikit-learn's liblinear, probe_costs builds liblinear's weights, the argument checks raise before anything
touches the device, the certificate |w - w*| <= |grad f(w)| holds, and the inputs of tests/test_gpu_probe.py are what it says."""
import numpy as np
import pytest

import probe_ref as pr
from argsim_amd import probe


def _blobs(K, n=120, dim=6, seed=0):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, K, n)
    y[:K] = np.arange(K)
    x = (rng.standard_normal((K, dim))[y] * 1.5 + rng.standard_normal((n, dim))).astype(np.float32)
    return x, y


@pytest.mark.parametrize('K,C', [(2, 0.001), (3, 0.001), (5, 0.001), (2, 1.0), (4, 0.1)])
def test_reference_is_liblinear(K, C):
    sk = pytest.importorskip('sklearn.linear_model')
    x, y = _blobs(K, seed=K)
    classes, costs = probe.probe_costs(y, None, C, 'balanced')
    w = np.stack([pr.newton64(x, costs[p].astype(np.float64)) for p in range(costs.shape[0])])
    model = sk.LogisticRegression(C=C, penalty='l2', solver='liblinear', class_weight='balanced', tol=1e-12, max_iter=10000).fit(x.astype(np.float64), y)
    assert list(classes) == list(model.classes_)
    assert np.abs(w[:, :-1] - model.coef_).max() <= 1e-6 and np.abs(w[:, -1] - model.intercept_).max() <= 1e-6
    dec = pr.tilde(x) @ w.T
    assert (probe.labels_from_decision(classes, dec) == model.predict(x.astype(np.float64))).all()


def test_probe_costs_by_hand():
    labels = np.array(['a', 'b', 'b', 'c', 'c', 'c', 'a', 'zz'])
    train = np.array([0, 1, 2, 3, 4, 5])                  # a x 1, b x 2, c x 3: w = 6 / (3 n_k) = 2, 1, 2/3
    classes, costs = probe.probe_costs(labels, train, 0.5, 'balanced')
    assert list(classes) == ['a', 'b', 'c'] and costs.dtype == np.float32 and costs.shape == (3, 8)
    want = np.array([[1.0, -.5, -.5, -.5, -.5, -.5, 0, 0], [-.5, .5, .5, -.5, -.5, -.5, 0, 0], [-.5, -.5, -.5, 1 / 3, 1 / 3, 1 / 3, 0, 0]])
    assert np.array_equal(costs, want.astype(np.float32))
    _, plain = probe.probe_costs(labels, train, 0.5, None)
    assert np.array_equal(np.abs(plain[:, :6]), np.full((3, 6), 0.5, np.float32)) and np.array_equal(np.sign(plain), np.sign(costs))
    # two classes: one problem, positive on the larger class; weights 5 / (2 x 2) and 5 / (2 x 3)
    classes, costs = probe.probe_costs(labels, np.array([1, 2, 3, 4, 5]), 2.0, 'balanced')
    assert list(classes) == ['b', 'c'] and costs.shape == (1, 8)
    assert np.allclose(costs[0], [0, -2.5, -2.5, 5 / 3, 5 / 3, 5 / 3, 0, 0], rtol=1e-7, atol=0)
    # a boolean mask is the same rows; one class: no problem
    mask = np.zeros(8, bool)
    mask[[1, 2, 3, 4, 5]] = True
    assert np.array_equal(probe.probe_costs(labels, mask, 2.0, 'balanced')[1], costs)
    classes, costs = probe.probe_costs(labels, np.array([3, 4]), 1.0)
    assert list(classes) == ['c'] and costs.shape == (0, 8)
    assert (probe.labels_from_decision(classes, np.zeros((4, 0))) == 'c').all()
    # the prediction rules: first maximum; the positive side at K = 2
    assert list(probe.labels_from_decision(np.array([3, 5, 9]), np.array([[1., 1., 0.], [0., 2., 2.], [-1., -2., -.5]]))) == [3, 5, 9]
    assert list(probe.labels_from_decision(np.array([3, 5]), np.array([[1.], [0.], [-1.]]))) == [5, 3, 3]


def test_argument_checks_raise_before_the_device():
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("the device was touched: %s" % name)
    v = NoDevice()
    z = np.zeros((6, 8), np.float32)
    y = np.array([0, 1, 2, 0, 1, 2])
    s = np.ones((2, 6), np.float32)
    for bad in (dict(z=z.astype(np.float64)), dict(z=np.zeros((6, 6), np.float32)), dict(z=np.zeros((6, 1028), np.float32)), dict(z=np.zeros(6, np.float32)),
                dict(z=[[0.0] * 8] * 6), dict(costs=s.astype(np.float64)), dict(costs=np.ones((2, 5), np.float32)), dict(costs=np.ones((0, 6), np.float32)),
                dict(tol=-1e-3), dict(tol=float('nan')), dict(max_newton=0), dict(max_cg=0), dict(max_cg=1.5)):
        with pytest.raises(ValueError):
            probe.fit_raw(v, **dict(dict(z=z, costs=s), **bad))
    for bad in (dict(labels=y[:5]), dict(C=0), dict(C=float('inf')), dict(class_weight='other'), dict(train=np.array([0, 0, 1])), dict(train=np.array([7])),
                dict(train=np.array([], np.int64)), dict(train=np.array([0.5])), dict(tol=-1.0), dict(z=z[:, :6])):
        with pytest.raises(ValueError):
            probe.fit(v, **dict(dict(z=z, labels=y), **bad))
    for bad in (dict(folds=np.zeros(5, int)), dict(groups=np.zeros(7, int)), dict(labels=y[:5]), dict(max_newton=0)):
        with pytest.raises(ValueError):
            probe.cross_validate(v, **dict(dict(z=z, labels=y, folds=np.arange(6) % 2), **bad))
    with pytest.raises(ValueError):
        probe.decision_raw(v, z, np.zeros((2, 8), np.float32))


def test_cv_problems():
    labels = np.array(['x', 'y', 'x', 'y', 'p', 'q', 'r', 'p', 'q', 'r', 'p'])
    groups = np.array(['t2'] * 4 + ['t1'] * 7)
    folds = np.array([0, 0, 1, 1, 0, 0, 0, 1, 1, 1, 1])
    jobs, costs = probe.cv_problems(labels, folds, groups, C=1.0, class_weight=None)
    assert [(j['group'], j['fold'], j['lo'], j['hi']) for j in jobs] == [('t2', 0, 0, 1), ('t2', 1, 1, 2), ('t1', 0, 2, 5), ('t1', 1, 5, 8)]
    assert costs.shape == (8, 11)
    assert np.array_equal(costs[0], [0, 0, -1, 1, 0, 0, 0, 0, 0, 0, 0]) and np.array_equal(costs[2], [0, 0, 0, 0, 0, 0, 0, 1, -1, -1, 1])
    dec = np.zeros((11, 8))
    dec[:, 0] = dec[:, 1] = 1.0               # t2: always 'y'
    dec[:, 2] = dec[:, 5] = 1.0               # t1: always 'p'
    res = probe.cv_predictions(jobs, labels, dec)
    assert res['scores'] == {'t2': 0.5, 't1': (1 / 3 + 2 / 4) / 2} and res['mean'] == (0.5 + (1 / 3 + 2 / 4) / 2) / 2
    from argsim_amd.eval_probe import report, split_labels
    t, c = split_labels(['abortion-pro-3', 'gun-con-1'])
    assert list(t) == ['abortion', 'gun'] and list(c) == ['pro-3', 'con-1'] and list(split_labels(['a-pro-3'], True)[1]) == ['pro']
    assert report(res)[:2] == ['t2 50.00', 't1 41.67']


def test_certificate_on_perturbed_points():
    case = pr.CASES[1]
    x, s = pr.case_inputs(case)
    rng = np.random.default_rng(3)
    for p in (0, 1, 2, 3, 5):
        w = pr.newton64(x, s[p])
        assert np.linalg.norm(pr.grad64(x, s[p], w)) <= 1e-12
        for scale in (1e-6, 1e-3, 0.1, 3.0):
            v = w + scale * rng.standard_normal(w.shape)
            assert np.linalg.norm(v - w) <= np.linalg.norm(pr.grad64(x, s[p], v)) * (1 + 1e-9)
    assert not pr.newton64(x, s[2]).any()


def test_cases_hold_what_the_gpu_test_says():
    assert sorted(c[2] for c in pr.CASES) == [4, 36, 128, 1024]
    assert {c[0] % 128 for c in pr.CASES} >= {1, 127} and {c[1] % 32 for c in pr.CASES} >= {1, 31}
    assert any(c[0] > 128 for c in pr.CASES) and any(c[1] > 64 for c in pr.CASES) and 129 in [c[0] for c in pr.CASES] and 33 in [c[1] for c in pr.CASES]
    assert all(c[0] <= 400 and c[1] <= 70 for c in pr.CASES)
    for case in pr.CASES:
        x, s = pr.case_inputs(case)
        assert x.dtype == np.float32 and s.dtype == np.float32 and x.shape == (case[0], case[2]) and s.shape == (case[1], case[0])
        assert (s[1] > 0).all() and not s[2].any() and (s[3] < 0).all()
        zero = s[0] == 0
        assert 0 < zero.sum() < case[0] and (zero[:-1] != zero[1:]).sum() > 4          # held-out rows scattered among the others
        assert {0.001, 1.0} <= {0.001 if p % 2 == 0 else 1.0 for p in range(case[1])}
        assert np.abs(s[4]).max() < 0.01 and np.abs(s[5]).max() > 0.1


def test_reference_predictions_stay_within_the_exclusion_cap():
    """the worst case the GPU test allows a device: |w - w*| <= 2 tol g0 for every problem.  Under it at most 5 % of the rows of
    the cross-validation case may be too close to call"""
    z, labels, folds, groups = pr.cv_inputs()
    jobs, costs = probe.cv_problems(labels, folds, groups, pr.CV_C, 'balanced')
    assert costs.shape[0] == 25 and len(jobs) == 10
    w = np.stack([pr.newton64(z, costs[p]) for p in range(25)])
    worst = 2 * pr.CV_TOL * pr.g0_64(z, costs)
    dec, dbound = pr.tilde(z) @ w.T, pr.decision_bound(z, w)
    skip = np.zeros(pr.CV_N, bool)
    for j in jobs:
        v, sl = j['valid'], slice(j['lo'], j['hi'])
        skip[v] = pr.undecided(z[v], j['classes'], dec[v, sl], worst[sl], dbound[v, sl])
    res = probe.cv_predictions(jobs, labels, dec)
    print("too close to call under the worst-case bound: %d of %d; scores %s" % (skip.sum(), pr.CV_N, res['scores']))
    assert skip.mean() <= 0.05
    assert all(0.5 < v < 1.0 for v in res['scores'].values())       # neither chance nor a problem too easy to tell a wrong model
