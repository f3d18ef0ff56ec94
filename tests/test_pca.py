"""Principal components without a device: the float64 restatement of tests/pca_ref.py against numpy's eigh and scikit-learn, the
convergence of the rotation rule on the rank-deficient cases, the planner's default sweep count against the measured counts, the launch
planner (avae_debug_pca_plan, host arithmetic) and the parts of the Python layer that need no device (a stand-in for the C entries)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pca_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FITS = {}


def _fits():
    """every test case's reference model, computed once"""
    if not _FITS:
        for name, (x, pad) in pr.test_cases().items():
            _FITS[name] = (x, pad, pr.fit(x, pad))
    return _FITS


# ---------------------------------------------------------------- the reference
def test_the_reference_against_eigh():
    """certificates from the rows themselves: residual, orthogonality, eigenvalues; the order, the clip and the signs"""
    for name, (x, pad, m) in _fits().items():
        d = x.shape[1] - pad
        c = pr.certificates(x, m, pad)
        assert m['converged'] and max(c.values()) <= 64 * d * pr.EPS, (name, c)
        assert (np.diff(m['var']) <= 0).all() and (m['var'] >= 0).all() and pr.signs_ok(m['comp']), name
        assert m['rank'] == int((m['var'] > m['thr']).sum()) <= d, name


def test_the_round_robin_order_meets_every_pair_once():
    for n in (1, 2, 3, 4, 5, 8, 33, 36, 129):
        seen = set()
        for r in range(pr.rounds(n)):
            p = pr.partners(n, r)
            live = np.flatnonzero(p < n)
            assert (p[p[live]] == live).all() and (p[live] != live).all() and len(live) == 2 * (n // 2)
            pairs = {(int(min(j, p[j])), int(max(j, p[j]))) for j in live}
            assert not pairs & seen
            seen |= pairs
        assert len(seen) == n * (n - 1) // 2


def test_the_exact_cases_in_the_reference():
    m = pr.fit(pr.axis_rows([1.0, 3.0, 2.0, 3.0]))
    assert m['sweeps'] == 1 and m['rotations'] == 0 and m['var'].tolist() == [18.0 / 7, 18.0 / 7, 8.0 / 7, 2.0 / 7]
    assert np.array_equal(m['comp'], np.eye(4)[[1, 3, 2, 0]])
    m = pr.fit(pr.block_rows())
    r = np.sqrt(0.5)
    assert m['rotations'] == 1 and m['sweeps'] == 2 and np.allclose(m['var'], [6.0, 2.0 / 3, 0, 0], atol=1e-15)
    assert np.allclose(m['comp'][:2], [[r, r, 0, 0], [r, -r, 0, 0]], atol=1e-15)
    m = pr.fit(np.full((5, 4), 7.0, np.float32))
    assert m['rank'] == 0 and m['sweeps'] == 1 and np.array_equal(m['comp'], np.eye(4)) and (m['var'] == 0).all()
    assert pr.fit(pr.random_rows(2, 4))['rank'] == 1


def test_the_reference_against_sklearn():
    skd = pytest.importorskip('sklearn.decomposition')
    x = pr.random_rows(257, 36)
    m = pr.fit(x)
    for solver in ('covariance_eigh', 'full'):
        try:
            sk = skd.PCA(svd_solver=solver).fit(x.astype(np.float64))
        except ValueError:
            pytest.skip("this scikit-learn has no svd_solver=%r" % solver)
        top = sk.explained_variance_[0]
        assert np.abs(sk.explained_variance_ - m['var']).max() <= 1e-12 * top and np.abs(sk.mean_ - m['mean']).max() <= 1e-13
        assert np.allclose(sk.explained_variance_ratio_, m['var'] / m['var'].sum(), atol=1e-13)
        assert np.allclose(sk.singular_values_, np.sqrt(m['var'] * 256), rtol=1e-10)
        keep = m['var'] > 1e-6 * top                            # directions are conditioned by the gaps: the well-separated ones
        assert np.abs(sk.components_[keep] - m['comp'][keep]).max() <= 1e-6         # the same signs
    from argsim_amd import pca as P
    raw = _ref_raw([])
    for frac in (0.5, 0.9, 0.999):
        sk = skd.PCA(n_components=frac, svd_solver='full').fit(x.astype(np.float64))
        assert len(P.pca(None, x, frac, raw=raw)['explained_variance']) == sk.n_components_
    sk = skd.PCA(n_components=5, whiten=True, svd_solver='full').fit(x.astype(np.float64))
    mod = P.pca(None, x, 5, whiten=True, raw=raw)
    y = P.transform(None, x, mod, raw=_ref_transform)
    assert np.abs(y - sk.transform(x.astype(np.float64))).max() <= 1e-5 and np.allclose(mod['noise_variance'], sk.noise_variance_)


def test_the_rule_settles_on_the_rank_deficient_cases():
    for name in ('rankdef-64x36', 'rankdef-256x132', 'collapsed-257x132', 'few-40x64', 'few-7x8', 'random-2x132-0', 'random-3x132-3'):
        x, pad, m = _fits()[name]
        assert m['converged'] and m['sweeps'] <= pr.DEFAULT_SWEEPS // 2, (name, m['sweeps'])
    m = _fits()['rankdef-64x36'][2]
    assert m['rank'] <= 35 and m['var'][-1] == 0.0


def test_the_default_is_twice_the_measured_sweeps():
    worst = max(m['sweeps'] for _, _, m in _fits().values())
    print("most sweeps over the test cases: %d; recorded %s" % (worst, pr.MEASURED))
    assert worst == pr.MEASURED['tests'] and pr.DEFAULT_SWEEPS == 2 * max(pr.MEASURED.values())
    assert _plan(300, 1024)['sweeps'] == pr.DEFAULT_SWEEPS
    with open(os.path.join(ROOT, 'argsim_amd', 'csrc', 'kernels.h')) as f:
        assert int(re.search(r'constexpr int kPcaSweeps = (\d+);', f.read()).group(1)) == pr.DEFAULT_SWEEPS


# ---------------------------------------------------------------- the plan
def _plan(N, dim, pad=0, chunk=0, form=0, cus=256):
    from argsim_amd import lib
    out = np.full(13, -1, np.int32)
    assert lib.load().avae_debug_pca_plan(N, dim, pad, chunk, form, cus, out.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    names = 'dreal tiles pairs rows chunks form rounds sweeps launches lds trows'.split()
    p = dict(zip(names, out.tolist()))
    p['ws'] = (int(out[11]) & 0xffffffff) | (int(out[12]) << 32)
    return p


def _plan_py(N, dim, pad, chunk, form, cus):
    """the planner restated"""
    d = dim - pad
    tiles = -(-d // 64)
    pairs = tiles * (tiles + 1) // 2
    want = max(1, -(-4 * cus // pairs))
    rows = max(64, -(--(-N // want) // 16) * 16)
    if chunk:
        rows = min(rows, chunk)
    rows = max(rows, -(-N // min(1024, max(1, (1 << 25) // (pairs * 4096)))))
    f = form if form else (1 if d <= 128 else 2)
    rounds = d + (d & 1) - 1
    lds = 8 * (d * d + 3 * d) + 8 * d + 2 * (d * (d + 1) // 2) if f == 1 else 32 * 32
    trows = 16 if not chunk or chunk >= 16 else 8 if chunk >= 8 else 4
    return dict(dreal=d, tiles=tiles, pairs=pairs, rows=rows, chunks=-(-N // rows), form=f, rounds=rounds, sweeps=pr.DEFAULT_SWEEPS,
                launches=6 + (1 if f == 1 else pr.DEFAULT_SWEEPS * (rounds + 1)), lds=lds, trows=trows)


def test_the_plan_against_its_restatement():
    for N in (2, 3, 64, 257, 3000, 65536, 131072, 1 << 22):
        for dim, pad in ((4, 0), (4, 3), (36, 3), (128, 0), (132, 3), (132, 0), (260, 0), (1024, 0)):
            for chunk in (0, 1, 7, 16, 100):
                for form in (0, 2):
                    for cus in (1, 256):
                        p = _plan(N, dim, pad, chunk, form, cus)
                        ws = p.pop('ws')
                        assert p == _plan_py(N, dim, pad, chunk, form, cus), (N, dim, pad, chunk, form, cus)
                        assert p['lds'] <= 160 * 1024 and 1 <= p['chunks'] <= 1024 and (p['chunks'] - 1) * p['rows'] < N <= p['chunks'] * p['rows']
                        assert p['chunks'] * p['pairs'] * 4096 * 8 <= (1 << 28) + 4096 * 8 * p['pairs']
                        nn = p['dreal'] ** 2
                        need = 32 + 8 * (p['chunks'] * dim + p['chunks'] * p['pairs'] * 4096 + (4 if p['form'] == 2 else 3) * nn)
                        assert need <= ws <= need + 8 * 256
    # the form switch at dreal 128, the resident solve's LDS, the launch counts
    assert _plan(3000, 128)['form'] == 1 and _plan(3000, 132, 3)['form'] == 2 and _plan(3000, 132, 0)['form'] == 2 and _plan(3000, 128, form=2)['form'] == 2
    assert _plan(3000, 128)['lds'] == 151680 and _plan(3000, 128)['launches'] == 7
    assert _plan(300, 1024)['launches'] == 6 + pr.DEFAULT_SWEEPS * 1024 and _plan(300, 1024)['rounds'] == 1023 and _plan(300, 8, 3)['rounds'] == 5
    from argsim_amd import lib
    out = np.zeros(13, np.int32)
    for bad in ((1, 128, 0, 0, 0, 256), ((1 << 22) + 1, 128, 0, 0, 0, 256), (10, 6, 0, 0, 0, 256), (10, 1028, 0, 0, 0, 256), (10, 128, 4, 0, 0, 256),
                (10, 128, -1, 0, 0, 256), (10, 128, 0, -1, 0, 256), (10, 128, 0, 0, 3, 256), (10, 128, 0, 0, 0, 0), (10, 132, 0, 0, 1, 256)):
        assert lib.load().avae_debug_pca_plan(*bad, out.ctypes.data_as(C.POINTER(C.c_int32))) == 1


def test_the_declarations_match_the_header():
    from argsim_amd import lib
    res, args = lib.SIGNATURES['avae_pca_fit']
    assert res is C.c_int and len(args) == 9 and args[4] == C.POINTER(lib.AvaePcaConfig) and len(lib.SIGNATURES['avae_pca_transform'][1]) == 9
    with open(os.path.join(ROOT, 'include', 'argsim_vae.h')) as f:
        text = f.read()
    body = re.search(r'typedef struct avae_pca_config \{(.*?)\} avae_pca_config;', text, re.S).group(1)
    fields = re.findall(r'^\s*(int32_t)\s+(\w+);', body, re.M)
    assert [(n, C.c_int32) for t, n in fields] == list(lib.AvaePcaConfig._fields_) and C.sizeof(lib.AvaePcaConfig) == 16
    for name in ('avae_pca_fit', 'avae_pca_transform'):
        decl = re.search(r'int\s+%s\((.*?)\);' % name, text, re.S).group(1)
        assert len(re.sub(r'/\*.*?\*/', '', decl, flags=re.S).split(',')) == 9
        assert hasattr(lib.load(), name)
    assert hasattr(lib.load(), 'avae_debug_pca_plan')


# ---------------------------------------------------------------- the Python layer without a device
def _ref_raw(calls, converged=True):
    """pca_raw's stand-in: the float64 reference on what the wrapper hands to the C entry"""
    def raw(vae, x, cfg):
        x = np.array(x)
        calls.append(dict(x=x, cfg=(cfg.pad, cfg.max_sweeps, cfg.reserved, cfg.reserved2)))
        m = pr.fit(x, cfg.pad)
        dim, d = x.shape[1], x.shape[1] - cfg.pad
        mean, var, comp = np.zeros(dim), np.zeros(dim), np.zeros((dim, dim))
        mean[:d], var[:d], comp[:d, :d] = m['mean'], m['var'], m['comp']
        return dict(mean=mean, var=var, comp=comp, stat=np.array([m['sweeps'], int(converged), m['rotations'], m['rank'], 0, 0, 0, 0], np.int32))
    return raw


def _ref_transform(vae, x, mean, comp, scale):
    return pr.transform(np.asarray(x), mean, comp, len(comp), scale).astype(np.float32)


def test_the_wrapper_pads_and_reports():
    import torch
    from argsim_amd import pca as P
    z = np.ascontiguousarray(pr.random_rows(65, 8)[:, :6])              # 6 columns: padded with zeros to 8, pad = 2
    calls = []
    mod = P.pca(None, z, max_sweeps=9, raw=_ref_raw(calls))
    (c,) = calls
    assert c['x'].shape == (65, 8) and c['x'].dtype == np.float32 and (c['x'][:, 6:] == 0).all() and c['cfg'] == (2, 9, 0, 0)
    ref = pr.fit(z)
    assert set(mod) == {'mean', 'components', 'explained_variance', 'explained_variance_ratio', 'singular_values', 'noise_variance',
                        'effective_dim', 'n_samples', 'rank', 'sweeps', 'whiten'}
    assert mod['components'].shape == (6, 6) and np.array_equal(mod['explained_variance'], ref['var']) and np.array_equal(mod['mean'], ref['mean'])
    assert mod['n_samples'] == 65 and mod['rank'] == ref['rank'] and mod['sweeps'] == ref['sweeps'] and mod['whiten'] is False
    assert np.allclose(mod['effective_dim'], ref['var'].sum() ** 2 / (ref['var'] ** 2).sum()) and mod['noise_variance'] == 0.0
    calls.clear()
    two = P.pca(None, torch.as_tensor(z), 2, raw=_ref_raw(calls))         # a host tensor
    assert isinstance(calls[0]['x'], np.ndarray) and two['components'].shape == (2, 6) and np.allclose(two['noise_variance'], ref['var'][2:].mean())
    assert np.allclose(two['singular_values'], np.sqrt(ref['var'][:2] * 64))
    ratio = np.cumsum(ref['var'] / ref['var'].sum())
    for frac in (0.3, 0.8, 0.99):
        assert len(P.pca(None, z, frac, raw=_ref_raw([]))['explained_variance']) == int(np.searchsorted(ratio, frac, side='right')) + 1


def test_the_wrapper_checks_its_arguments_and_the_flag():
    from argsim_amd import pca as P
    z = pr.random_rows(64, 8)
    raw = _ref_raw([])
    bad = [dict(z=[[1.0]]), dict(z=z.astype(np.float64)), dict(z=np.zeros((8,), np.float32)), dict(z=np.zeros((1, 8), np.float32)),
           dict(z=np.zeros((20, 1025), np.float32)), dict(n_components=0), dict(n_components=9), dict(n_components=1.0), dict(n_components=0.0),
           dict(n_components=-0.5), dict(n_components=True), dict(n_components='2'), dict(whiten=1), dict(max_sweeps=-1), dict(max_sweeps=257),
           dict(max_sweeps=1.5), dict(z=z[:5], n_components=5)]
    for kw in bad:
        args = dict(z=z, n_components=None, whiten=False, max_sweeps=0)
        args.update(kw)
        with pytest.raises(ValueError):
            P.pca(None, raw=raw, **args)
    assert P.pca(None, z[:5], 4, raw=raw)['components'].shape == (4, 8)
    with pytest.raises(RuntimeError, match='max_sweeps'):
        P.pca(None, z, raw=_ref_raw([], converged=False))
    mod = P.pca(None, z, 3, raw=raw)
    for zz in (z[:, :4], z.astype(np.float64), np.zeros((0, 8), np.float32)):
        with pytest.raises(ValueError):
            P.transform(None, zz, mod, raw=_ref_transform)
    with pytest.raises(ValueError):
        P.transform(None, z, dict(mean=mod['mean']), raw=_ref_transform)
    with pytest.raises(ValueError):
        P.inverse_transform(mod, np.zeros((3, 4)))
    flat = np.ascontiguousarray(np.concatenate([z[:, :2], np.zeros((64, 2), np.float32)], 1))      # two zero columns: rank 2
    wm = P.pca(None, flat, whiten=True, raw=raw)
    with pytest.raises(ValueError, match='rank'):
        P.transform(None, flat, wm, raw=_ref_transform)


def test_inverse_of_transform_on_a_full_model():
    from argsim_amd import pca as P
    z = np.ascontiguousarray(pr.random_rows(65, 8)[:, :6])
    for whiten in (False, True):
        mod = P.pca(None, z, whiten=whiten, raw=_ref_raw([]))
        y = pr.transform(z, mod['mean'], mod['components'], 6, 1.0 / np.sqrt(mod['explained_variance']) if whiten else None)
        assert np.abs(P.inverse_transform(mod, y) - z).max() <= 1e-12
        y32 = P.transform(None, z, mod, raw=_ref_transform)
        assert y32.dtype == np.float32 and y32.shape == (65, 6) and np.abs(P.inverse_transform(mod, y32) - z).max() <= 1e-5
    part = P.pca(None, z, 2, raw=_ref_raw([]))
    back = P.inverse_transform(part, pr.transform(z, part['mean'], part['components'], 2))
    assert np.allclose(((back - z) ** 2).sum() / 64, part['noise_variance'] * 4)       # what is lost is the dropped variance


class _Stub:
    """the analyses eval_explore calls, pca by the reference"""
    def __init__(self):
        self.seen = []

    def pca(self, z, n_components=None, whiten=False, max_sweeps=0):
        from argsim_amd import pca as P
        return P.pca(None, z, n_components, whiten, max_sweeps, raw=_ref_raw([]))

    def pca_transform(self, z, model):
        from argsim_amd import pca as P
        return P.transform(None, z, model, raw=_ref_transform)

    def pca_reduce(self, z, k, whiten=False):
        from argsim_amd import pca as P
        return P.reduce(self, z, k, whiten)

    def affinity(self, x, metric, max_iter, seed):
        self.seen.append(('affinity', x.shape))
        return dict(labels=np.arange(len(x)) % 2, converged=True, n_iter=3)

    def kmeans(self, x, k, metric, n_init, seed):
        self.seen.append(('kmeans', x.shape))
        return dict(labels=np.arange(len(x)) % k, stop='converged', n_iter=2)


def test_eval_explore_flags():
    from argsim_amd import eval_explore as ee
    ap = ee.build_parser()
    base = ['--inputs', 'a.npy', '--labels', 'b.npy']
    A = ap.parse_args(base)
    assert A.pca is None and A.pca_whiten is False
    A = ap.parse_args(base + ['--pca', '3', '--pca-whiten'])
    assert A.pca == 3 and isinstance(A.pca, int) and A.pca_whiten is True
    assert ap.parse_args(base + ['--pca', '0.95']).pca == 0.95
    for bad in ('0', '-1', '1.0', '1.5', 'x', '0.0'):
        with pytest.raises(SystemExit):
            ap.parse_args(base + ['--pca', bad])
    x = pr.random_rows(65, 8)
    labels = np.array(['t%d-pro-x' % (i % 2) for i in range(65)])
    v0 = _Stub()
    cols0, lines0 = ee.evaluate(v0, x, None, labels, kmeans=2)
    assert v0.seen == [('affinity', (65, 8))] * 2 + [('kmeans', (65, 8))] * 2 and not any(line.startswith('pca') for line in lines0)
    v = _Stub()
    cols, lines = ee.evaluate(v, x, x[:, ::-1].copy(), labels, kmeans=2, pca=3, pca_whiten=True)
    assert v.seen == [('affinity', (65, 3))] * 4 + [('kmeans', (65, 3))] * 4          # every run on the reduced rows
    ref = pr.fit(x)
    assert lines[:2] == ['pca z', 'component variance ratio cumulative'] and lines[6] == 'pca z_sp'
    assert [float(t) for t in lines[2].split()] == [0.0, float('%.6g' % ref['var'][0]), float('%.4f' % (ref['var'][0] / ref['var'].sum())),
                                                    float('%.4f' % (ref['var'][0] / ref['var'].sum()))]
    assert lines[5] == "effective dimension %.2f of 8, rank %d, kept 3" % (ref['var'].sum() ** 2 / (ref['var'] ** 2).sum(), ref['rank'])
    assert list(cols)[:4] == ['cls_euc', 'dist_euc', 'cls_euc_sp', 'dist_euc_sp']
