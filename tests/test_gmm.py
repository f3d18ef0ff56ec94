"""The float64 reference of the Gaussian mixture (tests/gmm_ref.py) against scikit-learn's GaussianMixture, the margins of every case the
GPU tests rely on, the derived bounds, and the Python layer without a device (argument rules, the declaration against the header, BIC /
AIC, the draw from a mixture prior, eval_explore's options).

The sklearn tolerance: the largest deviation of gmm_ref from sklearn 1.7.2 over the cases below, measured on one CPU, was 5.8e-13 relative
(a variance of gauss200x128, 'diag', tol 1e-3; sklearn forms q_ic by the Gram trick and sums through BLAS).  SK_TOL is ten times that, to
cover another BLAS's summation order, and stays under the cap of 1e-9 beyond which the reference would be wrong."""
import os
import re
import types

import numpy as np
import pytest

import gmm_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SK_TOL = min(10 * 5.8e-13, 1e-9)


# ---------------------------------------------------------------- the reference against sklearn
@pytest.mark.parametrize('tol', [1e-3, 1e-6])
@pytest.mark.parametrize('covariance', ['diag', 'spherical'])
@pytest.mark.parametrize('case', gr.CASES, ids=gr.CASE_IDS)
def test_reference_against_sklearn(case, covariance, tol):
    import warnings
    from sklearn.mixture import GaussianMixture
    name, make, k = case
    x = make()
    X = x.astype(np.float64)
    lab = gr.start_labels(x.shape[0], k)
    ref = gr.run(x, k, covariance, 1, 100, tol, 1e-6, lab)
    w, mu, cov = ref['starts'][0]
    g = GaussianMixture(k, covariance_type=covariance, tol=tol, reg_covar=1e-6, max_iter=100, weights_init=w, means_init=mu,
                        precisions_init=1.0 / cov if covariance == 'diag' else 1.0 / cov[:, 0])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        g.fit(X)
    assert (ref['n_iter'], ref['stop'] == 0) == (g.n_iter_, g.converged_)
    assert np.array_equal(ref['labels'], g.predict(X))
    gcov = g.covariances_ if covariance == 'diag' else np.repeat(g.covariances_[:, None], x.shape[1], 1)
    rel = lambda a, b: float((np.abs(a - b) / np.abs(b)).max())
    dev = max(rel(ref['weights'], g.weights_), rel(ref['covars'], gcov), float(np.abs(ref['means'] - g.means_).max() / np.abs(g.means_).max()),
              rel(np.array([ref['lower']]), np.array([g.lower_bound_])), rel(ref['logp'], g.score_samples(X)))
    print("%s %s tol %g: %d iterations, deviation from sklearn %.3g, stop margin %.3g, label gap %.3g"
          % (name, covariance, tol, ref['n_iter'], dev, ref['stop_margin'], ref['label_gap']))
    assert dev <= SK_TOL
    assert gr.has_margins(ref)
    npar, bic, aic = gr.bic_aic(ref['logp'].mean(), x.shape[0], k, x.shape[1], covariance)
    assert npar == g._n_parameters() and abs(bic - g.bic(X)) <= SK_TOL * abs(bic) and abs(aic - g.aic(X)) <= SK_TOL * abs(aic)
    from argsim_amd import gmm as G
    assert G.n_parameters(k, x.shape[1], covariance) == npar


# ---------------------------------------------------------------- margins of the cases the GPU tests rely on
@pytest.mark.parametrize('covariance', ['diag', 'spherical'])
@pytest.mark.parametrize('name', gr.CASE_IDS)
def test_the_margin_cases_have_margins(name, covariance):
    x, k, lab, ref = gr.whole_run(name, covariance)
    assert gr.restarts_have_margins(ref), (ref['stop_margin'], ref['label_gap'])
    assert all(q['stop'] == 0 and 1 < q['n_iter'] < 100 for q in ref['runs'])
    assert len({tuple(l) for l in lab.tolist()}) == 3                          # three different starts
    print(name, covariance, "margins: stop %.3g, label %.3g, best %.3g (needed %.3g)" % (ref['stop_margin'], ref['label_gap'], ref['best_margin'], gr.MARGIN))


def test_the_other_gpu_cases_have_margins():
    x = gr.planted(96, 8, 6, 1)
    ref = gr.run(x, 6, 'diag', 1, 100, 1e-3, 1e-6, gr.start_labels(96, 6, 1))
    assert gr.has_margins(ref) and ref['stop'] == 0 and 3 < ref['n_iter'] < 100
    z = gr.planted(200, 10, 4, 8, spread=4.0)
    for covariance in ('diag', 'spherical'):
        assert gr.has_margins(gr.run(z, 4, covariance, 1, 100, 1e-3, 1e-6, gr.start_labels(200, 4, 1, seed=9)))
    x, lab = gr.repeated_points()
    assert gr.run(x, 4, 'diag', 1, 10, 1e-3, 0.0, lab[None])['stop'] == 2
    ok = gr.run(x, 4, 'diag', 1, 10, 1e-3, 1e-6, lab[None])
    assert ok['stop'] == 0 and ok['stop_margin'] > gr.MARGIN and np.array_equal(ok['labels'], lab)


# ---------------------------------------------------------------- the reference itself
def test_reference_conventions():
    x = gr.planted(96, 8, 6, 1)
    lab = gr.start_labels(96, 6, 1)[0].copy()
    lab[10:14] = [-1, 6, 1000, -7]
    lab[lab == 3] = -1
    r = gr.onehot(lab, 6)
    assert r.sum() == (lab >= 0).sum() - 2 and r[:, 3].sum() == 0
    w, mu, cov = gr.start_from_labels(x, lab, 6, 1e-6, 0)
    assert (mu[3] == 0).all() and (cov[3] == 1e-6).all() and abs(w.sum() - 1) < 1e-15 and 0 < w[3] < 1e-15
    # padding: a padded column has variance 1 and no share in the constants; the other columns are those of the unpadded rows
    xp = np.pad(x[:, :6], ((0, 0), (0, 2)))
    for sph in (0, 1):
        a = gr.mstep(x[:, :6], r, 1e-6, sph)
        b = gr.mstep(xp, r, 1e-6, sph, pad=2)
        assert np.array_equal(a[1], b[1][:, :6]) and np.array_equal(a[2], b[2][:, :6]) and (b[2][:, 6:] == 1).all()
        ea, eb = gr.estep(x[:, :6], *a[:3]), gr.estep(xp, *b[:3], pad=2)
        assert np.array_equal(ea['t'], eb['t'])
    # max_iter 0 and the degenerate start
    zero = gr.run(x, 6, 'diag', 1, 0, 1e-3, 1e-6, gr.start_labels(96, 6, 1))
    assert zero['n_iter'] == 0 and zero['stop'] == 1 and zero['lower'] == -np.inf and zero['trace'].size == 0
    both = gr.run(*[gr.repeated_points()[0], 4, 'diag', 2, 5, 1e-3, 0.0, np.stack([gr.repeated_points()[1], gr.start_labels(24, 4)[0]])])
    assert both['runs'][0]['stop'] == 2 and both['lowers'][0] == -np.inf
    assert both['best'] == (1 if both['runs'][1]['stop'] != 2 else 0)


def test_bounds_are_small_and_cover_a_reordered_sum():
    x = gr.gaussian(200, 128, 4)
    w, mu, cov = gr.start_from_labels(x, gr.start_labels(200, 5)[0], 5, 1e-6, 0)
    s = gr.step_bounds(x, w, mu, cov, 1e-6, 0)
    # small: the margin argument of the GPU tests needs every one-step bound far below 2^-30
    assert max(s['eb']['t'].max(), s['eb']['lse'].max(), s['mb']['means'].max(), s['mb']['covars'].max(), s['mb']['weights'].max()) < gr.MARGIN / 8
    X = x.astype(np.float64)
    q = ((X[:, None, ::-1] - mu[None, :, ::-1]) ** 2 / cov[None, :, ::-1]).sum(-1)          # the columns in descending order
    assert (np.abs(q - s['e']['q']) <= s['eb']['t']).all()
    r = s['e']['resp']
    mu2 = (r[::-1].T @ X[::-1]) / (r[::-1].sum(0) + gr.TEN_EPS)[:, None]                     # the rows in descending order
    assert (np.abs(mu2 - s['means']) <= s['mb']['means']).all()
    # EM does not decrease the bound
    ref = gr.run(x, 5, 'diag', 1, 30, 0.0, 0.0, gr.start_labels(200, 5))
    assert (np.diff(ref['trace']) >= -1e-12).all()


# ---------------------------------------------------------------- the Python layer without a device
def test_check_gmm_args():
    from argsim_amd.model import _check_gmm_args as check
    z = np.zeros((20, 10), np.float32)
    check(z, 3)
    check(z, 20, 'spherical', 16, 10000, 0.0, 0.0, (1 << 63) - 1, np.zeros((16, 20), np.int32))
    check(z, 3, max_iter=0, init=np.zeros(20, np.int64))
    check(z, 3, init=dict(weights=np.ones(3) / 3, means=np.zeros((3, 10)), covariances=np.ones((3, 10))))
    check(z, 3, 'spherical', 2, init=dict(weights=np.ones((2, 3)) / 3, means=np.zeros((2, 3, 10)), covariances=np.ones((2, 3))))
    bad = [dict(z=[[1.0]]), dict(z=z.astype(np.float64)), dict(z=np.zeros((8,), np.float32)), dict(z=np.zeros((1, 8), np.float32)),
           dict(z=np.zeros((4, 1025), np.float32)), dict(k=0), dict(k=21), dict(k=2.0), dict(covariance='full'), dict(covariance='tied'),
           dict(n_init=0), dict(n_init=17), dict(max_iter=-1), dict(max_iter=10001), dict(max_iter=1.5), dict(tol=-1e-3), dict(tol=float('nan')),
           dict(tol='x'), dict(reg_covar=-1e-9), dict(reg_covar=float('nan')), dict(seed=-1), dict(seed=1 << 63), dict(init='random'),
           dict(init=np.zeros(19, np.int32)), dict(init=np.zeros((2, 20), np.int32)), dict(init=np.zeros(20, np.float32)),
           dict(init=dict(weights=np.ones(3), means=np.zeros((3, 10)))), dict(init=dict(weights=np.ones(3), means=np.zeros((3, 9)), covariances=np.ones((3, 10)))),
           dict(init=dict(weights=np.ones(3), means=np.zeros((3, 10)), covariances=np.ones(3)))]
    for kw in bad:
        args = dict(z=z, k=3)
        args.update(kw)
        with pytest.raises(ValueError):
            check(**args)


def test_the_declaration_matches_the_header():
    import ctypes as C
    from argsim_amd import lib
    res, args = lib.SIGNATURES['avae_gmm_fit']
    assert res is C.c_int and len(args) == 22 and args[4] == C.POINTER(lib.AvaeGmmConfig)
    res, args = lib.SIGNATURES['avae_gmm_score']
    assert res is C.c_int and len(args) == 11
    with open(os.path.join(ROOT, 'include', 'argsim_vae.h')) as f:
        text = f.read()
    body = re.search(r'typedef struct avae_gmm_config \{(.*?)\} avae_gmm_config;', text, re.S).group(1)
    fields = re.findall(r'^\s*(int32_t|double|uint64_t)\s+(\w+);', body, re.M)
    ctype = {'int32_t': C.c_int32, 'double': C.c_double, 'uint64_t': C.c_uint64}
    assert [(n, ctype[t]) for t, n in fields] == list(lib.AvaeGmmConfig._fields_)
    assert C.sizeof(lib.AvaeGmmConfig) == 40 and lib.AvaeGmmConfig.tol.offset == 24 and lib.AvaeGmmConfig.reg_covar.offset == 32
    for name, n in (('avae_gmm_fit', 22), ('avae_gmm_score', 11)):
        decl = re.search(r'int\s+%s\((.*?)\);' % name, text, re.S).group(1)
        assert len(re.sub(r'/\*.*?\*/', '', decl, flags=re.S).split(',')) == n


def test_mixture_prior_draw():
    from argsim_amd import gmm as G
    from argsim_amd.model import VAE
    me = types.SimpleNamespace(cfg=dict(dim_rep=8))
    z0 = VAE.prior_draw(me, 5, 3)
    assert np.array_equal(z0, np.random.default_rng(3).standard_normal((5, 8)).astype(np.float32))          # without prior: today's z
    prior = dict(weights=np.array([0.2, 0.8]), means=np.stack([np.full(8, -3.0), np.full(8, 3.0)]), covariances=np.full((2, 8), 0.01))
    z = VAE.prior_draw(me, 400, 3, prior)
    assert z.shape == (400, 8) and z.dtype == np.float32
    rng = np.random.default_rng(3)
    comp = rng.choice(2, size=400, p=prior['weights'])
    assert np.array_equal(z, (prior['means'][comp] + 0.1 * rng.standard_normal((400, 8))).astype(np.float32))
    assert abs((z[:, 0] > 0).mean() - 0.8) < 0.1 and np.array_equal(G.sample(prior, 400, 3)[1], comp)
    sph = dict(prior, covariances=np.array([0.01, 0.01]))
    assert np.array_equal(G.sample(sph, 400, 3)[0], z)
    for bad in (dict(prior, means=np.zeros((2, 7))), dict(weights=prior['weights'], means=prior['means']), dict(prior, covariances=np.ones((3, 8)))):
        with pytest.raises(ValueError):
            VAE.prior_draw(me, 5, 3, bad)


def test_eval_explore_options():
    from argsim_amd import eval_explore as ee
    ap = ee.build_parser()
    base = ['--inputs', 'a.npy', '--labels', 'b.npy']
    A = ap.parse_args(base)
    assert A.gmm is None and A.gmm_cov == 'diag' and A.gmm_init == 1 and A.gmm_sweep is None
    A = ap.parse_args(base + ['--gmm', '12', '--gmm-cov', 'spherical', '--gmm-init', '3', '--gmm-sweep', '2:8:2'])
    assert (A.gmm, A.gmm_cov, A.gmm_init, A.gmm_sweep) == (12, 'spherical', 3, [2, 4, 6, 8])
    for args in (['--gmm', '0'], ['--gmm', 'x'], ['--gmm-cov', 'full'], ['--gmm', '5', '--gmm-init', '0'], ['--gmm-sweep', '5'], ['--gmm-sweep', '1:4']):
        with pytest.raises(SystemExit):
            ap.parse_args(base + args)
    assert ee.GMM_COLUMNS == "cls_gmm_z logp_gmm_z cls_gmm_z_sp logp_gmm_z_sp".split()


def test_eval_explore_gmm_runs_with_a_stub(tmp_path):
    """evaluate() with --gmm adds the mixture's runs behind the others and leaves those as they are"""
    from argsim_amd import eval_explore as ee
    calls = []

    class Stub:
        def affinity(self, x, metric, max_iter, seed):
            return dict(labels=np.arange(len(x)) % 2, converged=True, n_iter=3)

        def gmm(self, x, k, covariance, n_init, seed):
            calls.append((k, covariance, n_init, seed))
            return dict(labels=np.arange(len(x)) % k, logp=-np.arange(len(x), dtype=np.float64), converged=len(calls) > 1, n_iter=7, lower_bound=-1.5,
                        bic=10.0, aic=8.0)

        def sweep_gmm(self, x, ks, covariance, n_init, seed):
            return dict(k=ks, bic=np.array([3.0, 1.0, 2.0]), aic=np.array([3.0, 2.0, 1.0]), lower_bound=np.array([-3.0, -2.0, -1.0]), best=ks[1])

    z = gr.gaussian(12, 4, 1)
    labels = np.array(['t%d-pro-x' % (i % 2) for i in range(12)])
    cols0, lines0 = ee.evaluate(Stub(), z, None, labels)
    cols, lines = ee.evaluate(Stub(), z, z, labels, gmm=3, gmm_cov='spherical', gmm_init=2, gmm_sweep=[2, 3, 4], seed=5)
    assert list(cols0) == ['cls_euc', 'dist_euc', 'cls_cos', 'dist_cos'] and not any('gmm' in l for l in lines0)
    assert [c for c in cols if 'gmm' in c] == ee.GMM_COLUMNS and calls == [(3, 'spherical', 2, 5)] * 2
    assert "gmm_z: stopped after 7 iterations" in lines and "gmm_z_sp: stopped after 7 iterations" not in lines
    assert lines.count("gmm_z: lower bound -1.500000  BIC 10.00  AIC 8.00") == 1 and lines.count('3 clusters') == 2
    at = lines.index("gmm sweep z")
    assert lines[at + 1:at + 5] == ["k BIC AIC lower_bound", "2 3.00 3.00 -3.000000", "3 1.00 2.00 -2.000000 *", "4 2.00 1.00 -1.000000"]
    assert "gmm sweep z_sp" in lines and cols['logp_gmm_z'].shape == (12,)
    path = str(tmp_path / 'c.csv')
    ee.write_csv(path, [''] * 12, ['t'] * 12, [str(v) for v in labels], cols)
    with open(path) as f:
        head = f.readline().strip().split(',')
    assert head[-4:] == ee.GMM_COLUMNS
