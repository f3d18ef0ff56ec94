"""Principal components on the device (avae_pca_fit, avae_pca_transform, VAE.pca) against the float64 restatement of tests/pca_ref.py.

The fit is judged by certificates measured against float64 numpy from the rows themselves (pca_ref.certificates): the residual
max|C V^T - V^T L| / l_max, the orthogonality max|V V^T - I|, the eigenvalue error against eigvalsh / l_max and the mean error.  Each must
be at most 4 x what pca_ref attains on the same case, with a floor of dreal eps (the device may order the covariance sums otherwise, and both
sides obey the same sweeps x dim x eps growth), and below the hard cap 1e-10.  The transform is judged against float64 from the DEVICE's
model: one rounding to fp32.  Rows are padded with NaN rows, and every output is guarded by a sentinel, the untouched padding tail of mean,
var and comp included."""
import ctypes as C

import numpy as np
import pytest

import pca_ref as pr
from test_gpu_kmeans import _model, _ptr

pytestmark = pytest.mark.gpu

SENT = -77.0
CAP = 1e-10
_REF = {}


def _cfg(pad=0, max_sweeps=0, reserved=0, reserved2=0):
    from argsim_amd import lib
    return lib.AvaePcaConfig(pad=pad, max_sweeps=max_sweeps, reserved=reserved, reserved2=reserved2)


def _fit(x, pad=0, max_sweeps=0, chunk=0, form=0):
    """avae_pca_fit on NaN-padded rows and sentinel-guarded outputs -> dict(mean, var (dreal,), comp (dreal, dreal), stat, raw bytes)"""
    import torch
    m = _model()
    dev = m.device
    x = np.ascontiguousarray(x, np.float32)
    N, dim = x.shape
    d = dim - pad
    dx = torch.full((N + 3, dim), float('nan'), dtype=torch.float32, device=dev)
    dx[:N] = torch.as_tensor(x).to(dev)
    mean = torch.full((dim + 8,), SENT, dtype=torch.float64, device=dev)
    var = torch.full((dim + 8,), SENT, dtype=torch.float64, device=dev)
    comp = torch.full((dim * dim + 8,), SENT, dtype=torch.float64, device=dev)
    stat = torch.full((16,), int(SENT), dtype=torch.int32, device=dev)
    cfg = _cfg(pad, max_sweeps)
    assert m._l.avae_set_option(m._h, b'pca_chunk', chunk) == 0 and m._l.avae_set_option(m._h, b'pca_form', form) == 0
    m._stream()
    try:
        m._ck(m._l.avae_pca_fit(m._h, _ptr(dx), N, dim, C.byref(cfg), _ptr(mean), _ptr(var), _ptr(comp), _ptr(stat)))
    finally:
        m._l.avae_set_option(m._h, b'pca_chunk', 0)
        m._l.avae_set_option(m._h, b'pca_form', 0)
    mean, var, comp, stat = mean.cpu().numpy(), var.cpu().numpy(), comp.cpu().numpy(), stat.cpu().numpy()
    assert (mean[d:] == SENT).all() and (var[d:] == SENT).all() and (comp[dim * dim:] == SENT).all() and (stat[8:] == int(SENT)).all()
    cm = comp[:dim * dim].reshape(dim, dim)
    assert (cm[d:] == SENT).all() and (cm[:, d:] == SENT).all()                 # the padding tail is left untouched
    assert (stat[4:8] == 0).all()
    return dict(mean=mean[:d], var=var[:d], comp=cm[:d, :d].copy(), stat=stat[:8], bytes=(mean.tobytes(), var.tobytes(), comp.tobytes(), stat.tobytes()))


def _ref(key, x, pad):
    """the reference model of a case and its certificates, computed once"""
    if key not in _REF:
        model = pr.fit(x, pad)
        _REF[key] = (model, pr.certificates(x, model, pad))
    return _REF[key]


def _judge(out, x, pad, key, what):
    """the device's certificates against 4 x the reference's (floor dreal eps), the hard cap, the flag and the sweeps"""
    ref, rc = _ref(key, x, pad)
    d = x.shape[1] - pad
    dc = pr.certificates(x, out, pad)
    for name in ('res', 'orth', 'eig', 'mean'):
        bound = 4.0 * max(rc[name], d * pr.EPS)
        print("%s: %s device %.3g reference %.3g bound %.3g" % (what, name, dc[name], rc[name], bound))
        assert dc[name] <= bound and dc[name] <= CAP, (what, name)
    print("%s: stat %s reference sweeps %d rank %d" % (what, out['stat'].tolist(), ref['sweeps'], ref['rank']))
    assert out['stat'][1] == 1 and 1 <= out['stat'][0] <= pr.DEFAULT_SWEEPS, what
    assert pr.signs_ok(out['comp']) and (np.diff(out['var']) <= 0).all() and (out['var'] >= 0).all(), what
    return ref


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize('shape', pr.SHAPES, ids=['%dx%d-pad%d' % s for s in pr.SHAPES])
def test_shapes_against_the_reference(shape):
    """N in {2, 3, 63, 64, 65, 257} x dim in {4, 36, 132} x pad in {0, 3}: odd dreal and the bye, the resident solve up to dreal 36 and at
    129 / 132 the launched one, one to three column tiles"""
    N, dim, pad = shape
    x = pr.random_rows(N, dim, pad)
    out = _fit(x, pad)
    _judge(out, x, pad, ('random', shape), 'random %s' % (shape,))
    assert 1 <= out['stat'][3] <= dim - pad


def test_300_by_260_the_launched_solve_over_several_tile_pairs():
    x = pr.dense(300, 260)
    out = _fit(x)
    ref = _judge(out, x, 0, 'dense-300x260', '300x260')
    assert out['stat'][3] == ref['rank'] == 260


# ---------------------------------------------------------------- directions
@pytest.mark.parametrize('case', ['200x36', '300x132'])
def test_directions_on_designed_spectra(case):
    """neighbouring eigenvalues a factor >= 2 apart: every component above the noise is eigh's direction"""
    N, dim, spec = (200, 36, 2.0 ** -np.arange(12)) if case == '200x36' else (300, 132, 3.0 ** -np.arange(10))
    x = pr.designed(N, dim, spec)
    out = _fit(x)
    _judge(out, x, 0, ('designed', case), 'designed ' + case)
    lam, Q = np.linalg.eigh(pr.covariance(x)[1])
    lam, Q = lam[::-1], Q[:, ::-1]
    for c in range(len(spec)):
        dot = abs(float(out['comp'][c] @ Q[:, c]))
        assert dot >= 1 - 1e-9, (c, dot)
    assert np.allclose(out['var'][:len(spec)], spec, rtol=1e-5) and out['var'][len(spec)] < 1e-10 * spec[-1]


# ---------------------------------------------------------------- exact cases
def test_axis_rows_need_no_rotation():
    """rows +-s_j e_j: C is diagonal -- one sweep, no rotation, var exactly the variances in descending order, the components the unit
    vectors, ties in ascending column order"""
    scales = [1.0, 3.0, 2.0, 3.0, 0.5, 2.0, 4.0, 1.0]
    x = pr.axis_rows(scales)
    out = _fit(x)
    assert out['stat'][:3].tolist() == [1, 1, 0] and out['stat'][3] == 8
    want = sorted(range(8), key=lambda j: (-scales[j], j))
    assert out['var'].tolist() == [2.0 * scales[j] ** 2 / 15.0 for j in want]
    assert np.array_equal(out['comp'], np.eye(8)[want]) and (out['mean'] == 0).all()


def test_a_two_by_two_block():
    """[[a, b], [b, a]] -> (1, 1) / sqrt 2 and (1, -1) / sqrt 2, each with its first entry of largest magnitude positive"""
    out = _fit(pr.block_rows())
    r = np.sqrt(0.5)
    assert out['stat'][:4].tolist() == [2, 1, 1, 2]
    assert np.allclose(out['var'], [6.0, 2.0 / 3.0, 0.0, 0.0], rtol=0, atol=1e-15)
    assert np.allclose(out['comp'][0], [r, r, 0, 0], rtol=0, atol=1e-15) and np.allclose(out['comp'][1], [r, -r, 0, 0], rtol=0, atol=1e-15)
    assert np.array_equal(out['comp'][2:], np.eye(4)[2:])


def test_constant_rows_two_rows_and_deficient_columns():
    x = np.full((9, 8), 2.5, np.float32)
    out = _fit(x)
    assert out['stat'][:4].tolist() == [1, 1, 0, 0] and (out['var'] == 0).all() and np.array_equal(out['comp'], np.eye(8)) and (out['mean'] == 2.5).all()
    x = pr.random_rows(2, 4)
    out = _fit(x)
    assert out['stat'][1] == 1 and out['stat'][3] == 1 and (out['var'][1:] <= 1e-15 * out['var'][0]).all()      # N = 2: rank 1
    for key in ('rankdef-64x36', 'rankdef-256x132'):                       # a duplicate and a zero column: exact covariance (pca_ref.rank_deficient)
        x, pad = pr.test_cases()[key]
        out = _fit(x)
        ref = _judge(out, x, 0, key, key)
        assert out['stat'][3] == ref['rank'] < x.shape[1] and out['var'][-1] == 0.0
    x, pad = pr.test_cases()['collapsed-257x132']
    _judge(_fit(x), x, 0, 'collapsed-257x132', 'collapsed')


def test_offset_rows_need_the_two_pass_covariance():
    """rows + 1000 against float64: E[xx] - E[x]E[x] would lose seven digits here"""
    x = pr.offset(257, 36)
    out = _fit(x)
    _judge(out, x, 0, 'offset-257x36', 'offset')
    lam = np.linalg.eigvalsh(pr.covariance(x)[1])[::-1]
    assert np.abs(out['var'] - np.maximum(lam, 0)).max() <= 1e-12 * lam[0]


# ---------------------------------------------------------------- forms and plans
@pytest.mark.parametrize('shape', [(64, 36, 0), (64, 36, 3), (257, 128, 0), (257, 128, 3)], ids=lambda s: '%dx%d-pad%d' % s)
def test_both_forms_give_the_same_bytes(shape):
    """the resident and the launched solve: identical bytes of mean, var, comp, stat; two calls likewise.  The larger shape is 257 x 128
    (dreal 128 and 125), the most the resident solve takes: at 257 x 132 its dreal is 132 or 129 and pca_form 1 is refused, which
    test_the_refusals asserts for both paddings."""
    N, dim, pad = shape
    x = pr.random_rows(N, dim, pad)
    one = _fit(x, pad, form=1)
    two = _fit(x, pad, form=2)
    assert one['bytes'] == two['bytes']
    assert _fit(x, pad, form=1)['bytes'] == one['bytes'] and _fit(x, pad)['bytes'] == one['bytes']
    assert one['stat'][1] == 1


def test_chunks_stay_within_the_bound():
    x = pr.dense(257, 132, 3)
    key = 'dense-257x132'
    base = _judge(_fit(x, 3), x, 3, key, 'chunk 0')
    assert base['rank'] == 129
    for chunk in (1, 7, 16, 100):
        out = _fit(x, 3, chunk=chunk)
        _judge(out, x, 3, key, 'chunk %d' % chunk)
        assert out['stat'][3] == base['rank'] and out['stat'][1] == 1
        assert _fit(x, 3, chunk=chunk)['bytes'] == out['bytes']


def test_not_converged_is_a_refusal():
    """one sweep on a dense case: flag 0, VAE.pca raises naming max_sweeps, the default then succeeds"""
    m = _model()
    x = pr.random_rows(65, 36)
    out = _fit(x, max_sweeps=1)
    assert out['stat'][0] == 1 and out['stat'][1] == 0 and out['stat'][2] > 0
    out = _fit(x, max_sweeps=1, form=2)
    assert out['stat'][0] == 1 and out['stat'][1] == 0
    with pytest.raises(RuntimeError, match='max_sweeps'):
        m.pca(x, max_sweeps=1)
    assert m.pca(x)['sweeps'] <= pr.DEFAULT_SWEEPS


# ---------------------------------------------------------------- transform
def _transform(x, mean, comp, scale, k, chunk=0):
    import torch
    m = _model()
    dev = m.device
    n, dim = x.shape
    dx = torch.full((n + 3, dim), float('nan'), dtype=torch.float32, device=dev)
    dx[:n] = torch.as_tensor(x).to(dev)
    up = lambda v: torch.as_tensor(np.ascontiguousarray(v, np.float64)).to(dev)
    dm, dc = up(mean), up(comp)
    ds = up(scale) if scale is not None else None
    y = torch.full((n * k + 8,), SENT, dtype=torch.float32, device=dev)
    assert m._l.avae_set_option(m._h, b'pca_chunk', chunk) == 0
    m._stream()
    try:
        m._ck(m._l.avae_pca_transform(m._h, _ptr(dx), n, dim, _ptr(dm), _ptr(dc), _ptr(ds) if ds is not None else None, k, _ptr(y)))
    finally:
        m._l.avae_set_option(m._h, b'pca_chunk', 0)
    y = y.cpu().numpy()
    assert (y[n * k:] == SENT).all()
    return y[:n * k].reshape(n, k)


@pytest.mark.parametrize('dim,pad', [(36, 0), (132, 3)])
def test_transform_rounds_once(dim, pad):
    """against float64 (x - mean) comp^T scale from the DEVICE's model: |d| <= 2^-23 max(|y|, 2^-126); k in {1, 2, dreal}, with and
    without scale, n in {1, 65}; the same bytes for several pca_chunk.  The rows are well-conditioned (pca_ref.dense, more rows than
    columns): the bound is relative to |y|, and a y that is the cancelled sum of terms 10^9 times larger (a null direction of N < dreal
    rows) is below what ANY float64 evaluation, the reference's included, resolves -- dim 2^-52 sum|terms| -- so it cannot be judged"""
    x = pr.dense(257, dim, pad)
    d = dim - pad
    out = _fit(x, pad)
    mean = np.zeros(dim)
    mean[:d] = out['mean']
    comp = np.zeros((dim, dim))
    comp[:d, :d] = out['comp']
    scale = 1.0 / np.sqrt(np.maximum(out['var'], 1e-300))
    scale = np.where(out['var'] > out['var'][0] * 1e-12, scale, 1.0)
    for k in (1, 2, d):
        for sc in (None, scale[:k]):
            for n in (1, 65):
                want = pr.transform(x[:n], mean[:d], comp[:d, :d], k, sc)
                got = _transform(x[:n], mean, comp[:k], sc, k)
                err = np.abs(got.astype(np.float64) - want)
                print("transform dim %d k %d scale %s n %d: worst %.3g of bound" % (dim, k, sc is not None, n, (err / (2.0 ** -23 * np.maximum(np.abs(want), 2.0 ** -126))).max()))
                assert (err <= 2.0 ** -23 * np.maximum(np.abs(want), 2.0 ** -126)).all()
                for chunk in (1, 4, 9):
                    assert _transform(x[:n], mean, comp[:k], sc, k, chunk=chunk).tobytes() == got.tobytes()


# ---------------------------------------------------------------- refusals
def test_the_refusals():
    import torch
    m = _model()
    dev = m.device
    dx = torch.zeros((8, 8), dtype=torch.float32, device=dev)
    big = torch.zeros((4, 132), dtype=torch.float32, device=dev)
    d8 = lambda n: torch.zeros((n,), dtype=torch.float64, device=dev)
    mean, var, comp, st = d8(132), d8(132), d8(132 * 132), torch.zeros((8,), dtype=torch.int32, device=dev)
    y = torch.zeros((64,), dtype=torch.float32, device=dev)
    good = dict(x=_ptr(dx), N=8, dim=8, cfg=_cfg(), mean=_ptr(mean), var=_ptr(var), comp=_ptr(comp), stat=_ptr(st))
    bad = [(dict(x=None), 'x is null'), (dict(mean=None), 'mean is null'), (dict(var=None), 'var is null'), (dict(comp=None), 'comp is null'),
           (dict(stat=None), 'stat is null'), (dict(N=1), 'N must be in [2, 2^22]'), (dict(N=(1 << 22) + 1), 'N must be in [2, 2^22]'),
           (dict(dim=6), 'dim must be a multiple of 4 in [4, 1024]'), (dict(dim=1028), 'dim must be'), (dict(cfg=_cfg(pad=4)), 'pad must be'),
           (dict(cfg=_cfg(pad=-1)), 'pad must be'), (dict(cfg=_cfg(max_sweeps=-1)), 'max_sweeps must be'), (dict(cfg=_cfg(max_sweeps=257)), 'max_sweeps must be'),
           (dict(x=_ptr(dx, 4)), '16-byte aligned'), (dict(cfg=_cfg(reserved=1)), 'reserved'), (dict(cfg=_cfg(reserved2=1)), 'reserved')]
    for kw, text in bad:
        a = dict(good)
        a.update(kw)
        rc = m._l.avae_pca_fit(m._h, a['x'], a['N'], a['dim'], C.byref(a['cfg']), a['mean'], a['var'], a['comp'], a['stat'])
        assert rc != 0 and text in m._l.avae_last_error(m._h).decode(), (kw, m._l.avae_last_error(m._h))
    assert m._l.avae_pca_fit(m._h, good['x'], 8, 4, C.byref(_cfg(pad=3)), good['mean'], good['var'], good['comp'], good['stat']) == 0     # pad < dim
    assert m._l.avae_pca_fit(m._h, good['x'], 8, 8, None, good['mean'], good['var'], good['comp'], good['stat']) != 0
    assert 'config is null' in m._l.avae_last_error(m._h).decode()
    for key, v in ((b'pca_chunk', -1), (b'pca_form', -1), (b'pca_form', 3)):
        assert m._l.avae_set_option(m._h, key, v) != 0 and key.decode() in m._l.avae_last_error(m._h).decode()
    assert m._l.avae_set_option(m._h, b'pca_form', 1) == 0
    try:
        for pad in (0, 3):                                              # dreal 132 and 129
            rc = m._l.avae_pca_fit(m._h, _ptr(big), 4, 132, C.byref(_cfg(pad=pad)), good['mean'], good['var'], good['comp'], good['stat'])
            assert rc != 0 and 'pca_form 1' in m._l.avae_last_error(m._h).decode()
    finally:
        m._l.avae_set_option(m._h, b'pca_form', 0)
    tgood = dict(x=_ptr(dx), n=8, dim=8, mean=_ptr(mean), comp=_ptr(comp), k=2, y=_ptr(y))
    tbad = [(dict(x=None), 'x is null'), (dict(mean=None), 'mean is null'), (dict(comp=None), 'comp is null'), (dict(y=None), 'y is null'),
            (dict(n=0), 'n must be'), (dict(n=(1 << 22) + 1), 'n must be'), (dict(dim=6), 'dim must be'), (dict(dim=1028), 'dim must be'),
            (dict(k=0), 'k must be in [1, dim]'), (dict(k=9), 'k must be in [1, dim]'), (dict(x=_ptr(dx, 4)), '16-byte aligned')]
    for kw, text in tbad:
        a = dict(tgood)
        a.update(kw)
        rc = m._l.avae_pca_transform(m._h, a['x'], a['n'], a['dim'], a['mean'], a['comp'], None, a['k'], a['y'])
        assert rc != 0 and text in m._l.avae_last_error(m._h).decode(), (kw, m._l.avae_last_error(m._h))


# ---------------------------------------------------------------- through the Python layer
def test_vae_pca_on_host_and_device_rows():
    import torch
    from argsim_amd import pca as P
    from argsim_amd.model import pca, pca_reduce, pca_transform
    m = _model()
    z = np.ascontiguousarray(pr.random_rows(129, 8)[:, :6])                        # 6 columns: no multiple of 4
    ref = pr.fit(z)
    models = [m.pca(arg) for arg in (z, torch.as_tensor(z), torch.as_tensor(z).to(m.device))]
    for mod in models:
        assert mod['components'].shape == (6, 6) and mod['mean'].shape == (6,) and mod['n_samples'] == 129 and mod['rank'] == 6
        assert np.allclose(mod['explained_variance'], ref['var'], rtol=1e-12) and np.allclose(np.abs(mod['components'] @ ref['comp'].T), np.eye(6), atol=1e-9)
        assert np.allclose(mod['explained_variance_ratio'].sum(), 1.0) and mod['noise_variance'] == 0.0 and mod['whiten'] is False
        assert np.allclose(mod['singular_values'], np.sqrt(ref['var'] * 128)) and np.allclose(mod['effective_dim'], ref['var'].sum() ** 2 / (ref['var'] ** 2).sum())
        assert all(np.array_equal(mod[n], models[0][n]) for n in ('mean', 'components', 'explained_variance'))
    x8 = torch.as_tensor(pr.random_rows(129, 8)).to(m.device)                     # 8 columns on the device: taken as it is
    full = pca(m, x8)
    assert np.allclose(full['explained_variance'], pr.fit(x8.cpu().numpy())['var'], rtol=1e-12)
    two = m.pca(z, n_components=2)
    assert two['components'].shape == (2, 6) and np.allclose(two['noise_variance'], ref['var'][2:].mean())
    ratio = ref['var'] / ref['var'].sum()
    frac = m.pca(z, n_components=0.9)
    assert len(frac['explained_variance']) == int(np.searchsorted(np.cumsum(ratio), 0.9, side='right')) + 1
    # whitening: unit variances, in float64 within the transform's rounding
    wm = m.pca(z, n_components=4, whiten=True)
    y = m.pca_transform(z, wm)
    assert isinstance(y, np.ndarray) and y.shape == (129, 4) and y.dtype == np.float32
    want = pr.transform(z, wm['mean'], wm['components'], 4, 1.0 / np.sqrt(wm['explained_variance']))
    assert (np.abs(y - want) <= 2.0 ** -23 * np.maximum(np.abs(want), 2.0 ** -126)).all()
    assert np.allclose(want.var(0, ddof=1), 1.0, rtol=1e-9) and np.allclose(y.astype(np.float64).var(0, ddof=1), 1.0, rtol=1e-5)
    yd = pca_transform(m, torch.as_tensor(z).to(m.device), wm)
    assert isinstance(yd, torch.Tensor) and yd.is_cuda and np.array_equal(yd.cpu().numpy(), y)
    back = P.inverse_transform(full, m.pca_transform(x8, full))
    assert np.abs(back - x8.cpu().numpy()).max() <= 1e-5
    # reduce, then k-means on the reduced rows
    yk, mod = pca_reduce(m, z, 3)
    assert yk.shape == (129, 3) and mod['components'].shape == (3, 6)
    km = m.kmeans(np.ascontiguousarray(np.pad(yk, [(0, 0), (0, 1)])), 2, 'euclidean', n_init=1, seed=0)
    assert km['labels'].shape == (129,)


def test_eval_explore_with_and_without_pca(capsys):
    """--pca 2 prints the table and runs --kmeans 2 on the reduced rows; without --pca two runs of the present flags print the same bytes"""
    from argsim_amd import eval_explore as ee
    m = _model()
    rng = np.random.RandomState(3)
    x = np.ascontiguousarray(np.concatenate([rng.standard_normal((20, 8)) * 0.1 + 3, rng.standard_normal((20, 8)) * 0.1 - 3]), np.float32)
    labels = np.array(['t%d-pro-x' % (i // 20) for i in range(40)])
    cols0, lines0 = ee.evaluate(m, x, None, labels, kmeans=2, kmeans_init=2)
    cols1, lines1 = ee.evaluate(m, x, None, labels, kmeans=2, kmeans_init=2)
    assert '\n'.join(lines0).encode() == '\n'.join(lines1).encode() and not any(line.startswith('pca') for line in lines0)
    cols, lines = ee.evaluate(m, x, None, labels, kmeans=2, kmeans_init=2, pca=2)
    assert lines[0] == 'pca z' and lines[1] == 'component variance ratio cumulative' and len(lines[2].split()) == 4 and lines[3].startswith('1 ')
    assert lines[4].startswith('effective dimension ') and lines[4].endswith('of 8, rank 8, kept 2')
    assert list(cols) == list(cols0) and len(set(cols['cls_km_euc'].tolist())) == 2
    assert np.array_equal(cols['cls_km_euc'] == cols['cls_km_euc'][0], cols0['cls_km_euc'] == cols0['cls_km_euc'][0])      # the same split
    y, _ = m.pca_reduce(x, 2)
    from argsim_amd import affinity
    assert np.allclose(cols['dist_km_euc'], affinity.dist_to_centroids(y, cols['cls_km_euc'], 'sqeuclidean'))
