"""the float64 reference of the L1 probes (tests/probe_l1_ref.py) and the host side of the selection, without a GPU: the reference
reproduces scikit-learn's liblinear L1 model (the penalised bias, the C scaling, the support), every case the GPU test compares
supports on has decided coordinates, l1_costs is its definition, the union rule of select_dims, the argument checks raise before
anything touches the device, and eval_cluster's --select and --dims exclude each other."""
import numpy as np
import pytest

import probe_l1_ref as pl
from argsim_amd import eval_cluster, probe


@pytest.mark.parametrize('case', pl.SK_CASES, ids=pl.CASE_ID)
def test_reference_is_liblinear(case):
    sk = pytest.importorskip('sklearn.linear_model')
    x, cls = pl.case_labels(case)
    K, C = case[2], case[5]
    assert C <= 0.1                                     # (liblinear's own L1 solver takes minutes at large C and tol 1e-10)
    classes, costs = probe.l1_costs(cls, C=C)
    assert np.array_equal(costs, pl.case_inputs(case)[1]) and list(classes) == list(range(K))
    ref = pl.case_ref(case)
    x64 = x.astype(np.float64)
    fit = lambda y: sk.LogisticRegression(penalty='l1', C=C, solver='liblinear', tol=1e-10, max_iter=100000).fit(x64, y)
    # one-vs-rest by hand (what liblinear does for K >= 3); at K = 2 the one model of classes[1]
    models = [fit(cls)] if K == 2 else [fit((cls == k).astype(int)) for k in range(K)]
    coef = np.concatenate([m.coef_ for m in models])
    icpt = np.concatenate([m.intercept_ for m in models])
    assert np.abs(ref[:, :-1] - coef).max() <= 1e-6 and np.abs(ref[:, -1] - icpt).max() <= 1e-6
    assert np.array_equal(ref[:, :-1] != 0, coef != 0) and np.array_equal(ref[:, -1] != 0, icpt != 0)
    assert np.array_equal(pl.useful_dims(ref[:, :-1]), probe.useful_dims(coef))
    # the reference is optimal by its own measure too
    for p in range(costs.shape[0]):
        assert np.abs(pl.v64(x, costs[p], ref[p])).sum() <= 1e-9 * pl.v0_64(x, costs[p:p + 1])[0]


@pytest.mark.parametrize('case', pl.GPU_CASES + pl.SK_CASES, ids=pl.CASE_ID)
def test_cases_have_decided_coordinates(case):
    x, s = pl.case_inputs(case)
    N, dim, K, P = case[:4]
    assert x.shape == (N, dim) and s.shape == (P, N) and x.dtype == np.float32 and s.dtype == np.float32
    ref, dec = pl.case_ref(case), pl.case_decided(case)
    v0 = pl.v0_64(x, s)
    for p in range(P):
        assert np.abs(pl.v64(x, s[p], ref[p])).sum() <= 1e-9 * v0[p]
        assert (~dec[p]).sum() <= pl.CAP * (dim + 1), (p, int((~dec[p]).sum()))
        assert (ref[p] != 0).any()
    # what the GPU test of the selection relies on
    if case == pl.GPU_CASES[1]:
        assert dec.all() and set(range(6)) <= set(pl.useful_dims(ref[:, :-1]).tolist())


def test_the_reference_pieces_by_hand():
    # one row x = (2), cost +c: F(w, b) = |w| + |b| + c softplus(-(2 w + b)); g(0) = -c / 2 (2, 1)
    x = np.array([[2.0]], np.float32)
    s = np.array([[3.0]], np.float32)
    assert np.allclose(pl.grad64(x, s[0], np.zeros(2)), [-3.0, -1.5])
    assert np.allclose(pl.v64(x, s[0], np.zeros(2)), [-2.0, -0.5]) and np.isclose(pl.v0_64(x, s)[0], 2.5)
    assert np.isclose(pl.objective64(x, s[0], np.array([0.5, -0.25])), 0.75 + 3.0 * np.log1p(np.exp(-0.75)))
    assert np.allclose(pl.v64(x, s[0], np.array([0.5, 0.0])), [1 - 6 / (1 + np.e), 0.0])       # |g_b| = 3 / (1 + e) <= 1
    w = pl.prox_newton64(x, s[0])
    assert w[1] == 0 and np.isclose(6.0 / (1.0 + np.exp(2 * w[0])), 1.0)       # the bias stays out: |g_b| = 1/2 <= 1
    assert not pl.prox_newton64(x, 0.3 * s[0]).any()                            # |g(0)| <= 1 everywhere: w = 0
    assert np.array_equal(pl.soft(np.array([2.0, -2.0, 0.5, -0.5]), 1.0), [1.0, -1.0, 0.0, 0.0])
    assert not np.signbit(pl.soft(np.array([-0.5]), 1.0)).any()


def test_l1_costs_by_hand():
    labels = np.array(['a', 'b', 'b', 'c', 'c', 'c', 'a', 'zz'])
    train = np.array([0, 1, 2, 3, 4, 5])
    classes, costs = probe.l1_costs(labels, train)
    assert list(classes) == ['a', 'b', 'c'] and costs.dtype == np.float32 and costs.shape == (3, 8)
    want = 0.1 * np.array([[1, -1, -1, -1, -1, -1, 0, 0], [-1, 1, 1, -1, -1, -1, 0, 0], [-1, -1, -1, 1, 1, 1, 0, 0]])
    assert np.array_equal(costs, want.astype(np.float32))
    assert np.array_equal(probe.l1_costs(labels, train, 0.5, 'balanced')[1], probe.probe_costs(labels, train, 0.5, 'balanced')[1])
    classes, costs = probe.l1_costs(labels[:6], np.array([1, 2, 3, 4, 5]), 2.0)
    assert list(classes) == ['b', 'c'] and np.array_equal(costs, np.array([[0, -2, -2, 2, 2, 2]], np.float32))
    assert probe.l1_costs(labels, np.array([3, 4]))[1].shape == (0, 8)
    with pytest.raises(ValueError):
        probe.l1_costs(labels, C=0)


def test_select_dims_union_rule():
    coef = np.zeros((3, 8), np.float32)
    coef[0, 5] = 1e-30
    coef[2, 1] = -2.0
    coef[1, 5] = 0.5
    coef[1, 7] = -0.0
    dims = probe.useful_dims(coef)
    assert dims.dtype == np.int64 and dims.tolist() == [1, 5]
    assert probe.useful_dims(np.zeros((0, 8), np.float32)).tolist() == [] and probe.useful_dims(np.zeros((2, 4))).shape == (0,)
    with pytest.raises(ValueError):
        probe.useful_dims(np.zeros(8))

    class OneClass:                                     # a single class: no problem, no device call, no column
        def __getattr__(self, name):
            raise AssertionError("the device was touched: %s" % name)
    dims, model = probe.select_dims(OneClass(), np.zeros((4, 8), np.float32), np.array([1, 1, 1, 1]))
    assert dims.tolist() == [] and model.coef_.shape == (0, 8) and list(model.classes_) == [1]


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
                dict(tol=-1e-3), dict(tol=float('nan')), dict(max_newton=0), dict(max_inner=0), dict(max_inner=1.5)):
        with pytest.raises(ValueError):
            probe.fit_l1_raw(v, **dict(dict(z=z, costs=s), **bad))
    with pytest.raises(ValueError, match='max_inner'):
        probe.fit_l1_raw(v, z, s, max_inner=0)
    for fn in (probe.fit_l1, probe.select_dims):
        for bad in (dict(labels=y[:5]), dict(C=0), dict(C=float('inf')), dict(class_weight='other'), dict(train=np.array([0, 0, 1])), dict(train=np.array([7])),
                    dict(tol=-1.0), dict(max_inner=0), dict(z=z[:, :6])):
            with pytest.raises(ValueError):
                fn(v, **dict(dict(z=z, labels=y), **bad))
    with pytest.raises(TypeError):
        probe.fit_l1(v, z, y, max_cg=3)                 # the L2 fit's knob is not the L1 fit's


def test_eval_cluster_flags(tmp_path, capsys):
    parse = eval_cluster.build_parser().parse_args
    base = ['--inputs', 'z.npy', '--labels', 'l.npy']
    A = parse(base)
    assert A.select is None and A.dims is None and A.save_dims is None and A.by == 'stance'
    assert parse(base + ['--select', 'stance', '--save-dims', 'd.npy']).save_dims == 'd.npy'
    for which in ('topic', 'stance', 'reason', 'labels'):
        assert parse(base + ['--select', which]).select == which
    for bad in (['--select', 'stance', '--dims', 'd.npy'], ['--select', 'other'], ['--select']):
        with pytest.raises(SystemExit):
            parse(base + bad)
    assert 'not allowed with' in capsys.readouterr().err
    np.save(str(tmp_path / 'z.npy'), np.zeros((4, 8), np.float32))
    np.save(str(tmp_path / 'l.npy'), np.array(['a-pro-1', 'a-con-2', 'b-pro-1', 'b-con-3']))
    with pytest.raises(SystemExit):                      # --save-dims alone; refused before a handle is made
        eval_cluster.main(['--inputs', str(tmp_path / 'z.npy'), '--labels', str(tmp_path / 'l.npy'), '--save-dims', str(tmp_path / 'd.npy')])
    parts = eval_cluster.split_labels(['a-pro-1', 'a-con-2', 'b-pro-1'])
    assert eval_cluster.partition(parts, 'topic').tolist() == ['a', 'a', 'b']
    assert eval_cluster.partition(parts, 'stance').tolist() == ['a-pro', 'a-con', 'b-pro']
    assert eval_cluster.partition(parts, 'reason').tolist() == ['a-1', 'a-2', 'b-1']
    assert eval_cluster.partition(parts, 'labels').tolist() == ['a-pro-1', 'a-con-2', 'b-pro-1']

    class Keeps:                                        # a selection that keeps no column, or did not converge, is an error with text
        def __init__(self, dims, status):
            self.dims, self.status = dims, status

        def select_dims(self, z, labels, C=0.1):
            return np.array(self.dims, np.int64), probe.Probe(None, np.unique(labels), np.zeros((1, 9), np.float32), np.array([[0, 0, 0, self.status]], np.float32))
    z, labels = np.zeros((3, 8), np.float32), ['a-pro-1', 'a-con-2', 'b-pro-1']
    with pytest.raises(RuntimeError, match='keeps no column'):
        eval_cluster.select(Keeps([], 0), z, labels, 'stance')
    with pytest.raises(RuntimeError, match='did not converge'):
        eval_cluster.select(Keeps([1], 1), z, labels, 'stance')
    assert eval_cluster.select(Keeps([1, 4], 0), z, labels, 'stance').tolist() == [1, 4]
