"""The Gaussian mixture on the device (avae_gmm_fit, avae_gmm_score, VAE.gmm) against the float64 reference of tests/gmm_ref.py.

No tolerance here is measured.  ONE EM step from given parameters must agree with the reference's step within twice the bounds gmm_ref
derives from operation counts (twice: the reference errs as well).  A call of T iterations must equal, bit for bit, T chained calls of one
iteration that feed the parameters back in, and every link of the chain is checked against the reference step from the same inputs: so every
iteration of the device's trajectory is a correct EM step within a derived bound, and no tolerance over a whole run is invented.  On the
margin cases (gmm_ref.CASES; the margins are asserted on the reference alone, here and in tests/test_gmm.py) every decision of a run -- the
stop against tol, a row's component, the best restart -- has a relative margin of 2^-30, so iterations, stop codes and labels must equal the
reference's exactly and the parameters agree within 2^-30 of their magnitude (the cap the margin argument needs, not an accuracy claim; the
observed ratio is printed).  For ANY input the result carries a certificate that is evaluated in float64 from the outputs alone.  Rows are
followed by NaN rows and every output is guarded by a sentinel.  (The refusal of a workspace the device cannot give is not provoked.)"""
import ctypes as C

import numpy as np
import pytest

import gmm_ref as gr

pytestmark = pytest.mark.gpu

KEYS = ('dim_tgt', 'dim_emb', 'dim_rep', 'rnn_layers', 'accelerate', 'learn_rate', 'bos', 'eos')
SENT_I, SENT_F = -77, 123.0
_STATE = {}


def _model():
    if 'm' not in _STATE:
        from helpers import make_case
        from argsim_amd.model import VAE
        cfg, P, ids, keep, eps = make_case('tiny')
        m = VAE('infer', init=False, **{k: cfg[k] for k in KEYS})
        m.set_params(P)
        _STATE['m'] = m
    return _STATE['m']


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _cfg(k, n_init=1, max_iter=1, covariance=0, init=1, reserved=0, tol=0.0, reg_covar=1e-6):
    from argsim_amd import lib
    return lib.AvaeGmmConfig(k=k, n_init=n_init, max_iter=max_iter, covariance=covariance, init=init, reserved=reserved, tol=tol, reg_covar=reg_covar)


OUTS = ('weights', 'means', 'covars', 'label', 'stat', 'lower', 'logp', 'resp', 'weights_all', 'means_all', 'covars_all', 'stat_all', 'trace')


def _buffers(N, dim, k, R, T):
    import torch
    f, i = torch.float64, torch.int32
    return dict(weights=((k,), f), means=((k, dim), f), covars=((k, dim), f), label=((N,), i), stat=((4,), i), lower=((R,), f), logp=((N,), f),
                resp=((N, k), f), weights_all=((R, k), f), means_all=((R, k, dim), f), covars_all=((R, k, dim), f), stat_all=((R, 4), i),
                trace=((R, T), f))


def _guarded(bufs, dev):
    import torch
    return {n: torch.full((int(np.prod(s)) + 8,), SENT_I if dt == torch.int32 else SENT_F, dtype=dt, device=dev) for n, (s, dt) in bufs.items()}


def _unguard(t, bufs):
    import torch
    out = {}
    for n, (s, dt) in bufs.items():
        v = t[n].cpu().numpy()
        size = int(np.prod(s))
        assert (v[size:] == (SENT_I if dt == torch.int32 else SENT_F)).all(), n
        out[n] = v[:size].reshape(s)
    return out


def _rows(x):
    """the rows on the device, followed by three NaN rows"""
    import torch
    dev = _model().device
    x = np.ascontiguousarray(x, np.float32)
    dx = torch.full((x.shape[0] + 3, x.shape[1]), float('nan'), dtype=torch.float32, device=dev)
    dx[:x.shape[0]] = torch.as_tensor(x).to(dev)
    return dx


def _fit(x, k, labels=None, params=None, chunk=0, pad=0, **kw):
    """avae_gmm_fit on NaN-followed rows and sentinel-guarded outputs -> dict of numpy arrays.  labels (R, N) or params = (w (R, k), mu,
    cov (R, k, dim))"""
    import torch
    m = _model()
    dev = m.device
    N, dim = x.shape
    if params is not None:
        params = [np.ascontiguousarray(p, np.float64) for p in params]
        R = params[0].shape[0]
    else:
        labels = np.ascontiguousarray(labels, np.int32).reshape(-1, N)
        R = labels.shape[0]
    cfg = _cfg(k, n_init=R, init=0 if params is None else 1, **kw)
    dx = _rows(x)
    dl = None if params is not None else torch.as_tensor(labels).to(dev)
    dp = [None] * 3 if params is None else [torch.as_tensor(p).to(dev) for p in params]
    bufs = _buffers(N, dim, k, R, cfg.max_iter)
    t = _guarded(bufs, dev)
    assert m._l.avae_set_option(m._h, b'gmm_chunk', chunk) == 0 and m._l.avae_set_option(m._h, b'gmm_pad', pad) == 0
    m._stream()
    try:
        m._ck(m._l.avae_gmm_fit(m._h, _ptr(dx), N, dim, C.byref(cfg), _ptr(dl), *[_ptr(p) for p in dp], *[_ptr(t[n]) for n in OUTS]))
    finally:
        m._l.avae_set_option(m._h, b'gmm_chunk', 0)
        m._l.avae_set_option(m._h, b'gmm_pad', 0)
    return _unguard(t, bufs)


def _score(x, w, mu, cov, chunk=0, pad=0):
    import torch
    m = _model()
    dev = m.device
    n, dim = x.shape
    k = w.shape[0]
    dx = _rows(x)
    dp = [torch.as_tensor(np.ascontiguousarray(p, np.float64)).to(dev) for p in (w, mu, cov)]
    bufs = dict(logp=((n,), torch.float64), label=((n,), torch.int32), resp=((n, k), torch.float64))
    t = _guarded(bufs, dev)
    assert m._l.avae_set_option(m._h, b'gmm_chunk', chunk) == 0 and m._l.avae_set_option(m._h, b'gmm_pad', pad) == 0
    m._stream()
    try:
        m._ck(m._l.avae_gmm_score(m._h, _ptr(dx), n, dim, k, *[_ptr(p) for p in dp], *[_ptr(t[n_]) for n_ in ('logp', 'label', 'resp')]))
    finally:
        m._l.avae_set_option(m._h, b'gmm_chunk', 0)
        m._l.avae_set_option(m._h, b'gmm_pad', 0)
    return _unguard(t, bufs)


def _same_bits(p, q, names=OUTS):
    return [n for n in names if p[n].tobytes() != q[n].tobytes()]


def _ratio(d, b):
    return float((np.abs(d) / (2 * b + 1e-300)).max())


def _check_estep(x, w, mu, cov, logp, resp, label, pad=0, what=''):
    """logp, resp and label are the E-step of (w, mu, cov) within the bounds; label is the first maximum"""
    e = gr.estep(x, w, mu, cov, pad)
    eb = gr.estep_bounds(x, w, mu, cov, e, pad)
    rl, rr = _ratio(logp - e['lse'], eb['lse']), _ratio(resp - e['resp'], eb['resp'])
    print("%s E-step: logp error / bound %.3g, resp error / bound %.3g" % (what, rl, rr))
    assert rl <= 1 and rr <= 1
    N = x.shape[0]
    assert ((label >= 0) & (label < w.shape[0])).all()
    own = e['t'][np.arange(N), label]
    assert (own + eb['t'][np.arange(N), label] >= (e['t'] - eb['t']).max(1)).all()                  # a maximum (the first: test_score's tie)
    return e, eb


def _check_step(x, params, out, r, reg, sph, pad=0, what=''):
    """restart r of a one-iteration call from params against the reference's step within twice the derived bounds"""
    w, mu, cov = (p[r] for p in params)
    s = gr.step_bounds(x, w, mu, cov, reg, sph, pad)
    rat = dict(weights=_ratio(out['weights_all'][r] - s['weights'], s['mb']['weights']), means=_ratio(out['means_all'][r] - s['means'], s['mb']['means']),
               covars=_ratio(out['covars_all'][r] - s['covars'], s['mb']['covars']), lower=_ratio(out['lower'][r] - s['e']['lower'], s['eb']['lower']))
    print("%s restart %d: error / bound %s" % (what, r, ' '.join('%s %.3g' % kv for kv in rat.items())))
    assert max(rat.values()) <= 1, rat
    assert out['trace'][r, 0] == out['lower'][r] and out['stat_all'][r].tolist() == [1, 1, 0, 0]
    return s


def _chunk_for(k):
    """a gmm_chunk that gives at least 3 component parts (k >= 3), and with the cases' N >= 37 many row tiles and slices"""
    return max(1, k // 3)


# ---------------------------------------------------------------- one EM step
@pytest.mark.parametrize('covariance', ['diag', 'spherical'])
@pytest.mark.parametrize('chunked', [False, True])
@pytest.mark.parametrize('name', gr.CASE_IDS)
def test_one_step(name, chunked, covariance):
    _, make, k = gr.CASES[gr.CASE_IDS.index(name)]
    x = make()
    sph = gr.COVS[covariance]
    lab = gr.start_labels(x.shape[0], k, 2)
    params = [np.stack(p) for p in zip(*[gr.start_from_labels(x, l, k, 1e-6, sph) for l in lab])]
    out = _fit(x, k, params=params, chunk=_chunk_for(k) if chunked else 0, max_iter=1, covariance=sph)
    for r in range(2):
        _check_step(x, params, out, r, 1e-6, sph, what=name)
    b = int(out['stat'][0])
    assert out['stat'].tolist() == [b, 1, 1, 0] and b == int(np.argmax(out['lower']))
    _check_estep(x, out['weights'], out['means'], out['covars'], out['logp'], out['resp'], out['label'], what=name)


# ---------------------------------------------------------------- the induction
@pytest.mark.parametrize('covariance', ['diag', 'spherical'])
@pytest.mark.parametrize('chunk', [0, 3])
def test_call_of_T_iterations_is_T_chained_steps(chunk, covariance):
    x = gr.planted(257, 16, 9, 3, spread=2.0)
    k, T, sph = 9, 4, gr.COVS[covariance]
    lab = gr.start_labels(257, k, 2)
    params = [np.stack(p) for p in zip(*[gr.start_from_labels(x, l, k, 1e-6, sph) for l in lab])]
    whole = _fit(x, k, params=params, chunk=chunk, max_iter=T, covariance=sph)
    assert whole['stat_all'].tolist() == [[T, 1, 0, 0]] * 2
    for t in range(T):
        link = _fit(x, k, params=params, chunk=chunk, max_iter=1, covariance=sph)
        for r in range(2):
            _check_step(x, params, link, r, 1e-6, sph, what='link %d' % t)
        assert link['lower'].tobytes() == whole['trace'][:, t].tobytes(), t
        params = [link['weights_all'], link['means_all'], link['covars_all']]
    assert not _same_bits(whole, link, ('weights_all', 'means_all', 'covars_all', 'lower', 'weights', 'means', 'covars', 'logp', 'resp', 'label'))


# ---------------------------------------------------------------- whole runs on the margin cases
@pytest.mark.parametrize('covariance', ['diag', 'spherical'])
@pytest.mark.parametrize('name', gr.CASE_IDS)
def test_whole_runs(name, covariance):
    x, k, lab, ref = gr.whole_run(name, covariance)
    assert gr.restarts_have_margins(ref), (ref['stop_margin'], ref['label_gap'])
    out = _fit(x, k, labels=lab, covariance=gr.COVS[covariance], **{n: v for n, v in gr.RUN_KW.items() if n != 'n_init'})
    worst = 0.0
    for r, q in enumerate(ref['runs']):
        assert out['stat_all'][r].tolist() == [q['n_iter'], q['stop'], 0, 0], (r, out['stat_all'][r], q['n_iter'], q['stop'])
        for n, a in (('weights_all', q['weights']), ('means_all', q['means']), ('covars_all', q['covars']), ('lower', np.array(q['lower'])),
                     ('trace', q['trace'][:q['n_iter']])):
            got = out[n][r] if n != 'trace' else out[n][r, :q['n_iter']]
            worst = max(worst, float(np.abs(got - a).max() / np.abs(a).max()))
        assert (out['trace'][r, q['n_iter']:] == -np.inf).all()
    print("%s %s: largest deviation / magnitude %.3g = %.3g of 2^-30" % (name, covariance, worst, worst / gr.MARGIN))
    assert worst <= gr.MARGIN
    b = int(out['stat'][0])
    assert out['stat'][1:3].tolist() == out['stat_all'][b, :2].tolist()
    if gr.has_margins(ref):
        assert b == ref['best']
    if b == ref['best']:
        assert np.array_equal(out['label'], ref['labels'])
        assert np.abs(out['logp'] - ref['logp']).max() <= gr.MARGIN * np.abs(ref['logp']).max()


# ---------------------------------------------------------------- shapes
SHAPES = [(2, 1, 4, 0), (2, 2, 4, 0), (63, 63, 12, 2), (64, 64, 128, 0), (65, 65, 4, 0), (65, 2, 1024, 0), (257, 130, 128, 0), (257, 63, 12, 2),
          (64, 1, 1024, 0), (257, 65, 4, 0)]


@pytest.mark.parametrize('N,k,dim,pad', SHAPES)
def test_shapes(N, k, dim, pad):
    """one step from three different starts, both covariances; a restart run alone is that restart within the larger call"""
    x = gr.gaussian(N, dim, 31)
    x[:, dim - pad:] = 0.0
    rng = np.random.default_rng(32)
    lab = np.stack([rng.permutation(N) % k for _ in range(3)]).astype(np.int32)
    for sph in (0, 1):
        params = [np.stack(p) for p in zip(*[gr.start_from_labels(x, l, k, 1e-2, sph, pad) for l in lab])]
        out = _fit(x, k, params=params, pad=pad, max_iter=1, covariance=sph, reg_covar=1e-2)
        for r in range(3):
            _check_step(x, params, out, r, 1e-2, sph, pad, what='%dx%d k %d' % (N, dim, k))
        if pad:
            assert (out['covars_all'][:, :, dim - pad:] == 1.0).all() and (out['means_all'][:, :, dim - pad:] == 0.0).all()
        if sph:
            assert (out['covars_all'][:, :, :dim - pad] == out['covars_all'][:, :, :1]).all()
        _check_estep(x, out['weights'], out['means'], out['covars'], out['logp'], out['resp'], out['label'], pad)
        alone = _fit(x, k, params=[p[1:2] for p in params], pad=pad, max_iter=1, covariance=sph, reg_covar=1e-2)
        for n in ('weights_all', 'means_all', 'covars_all', 'lower', 'stat_all', 'trace'):
            assert alone[n][0].tobytes() == out[n][1].tobytes(), n
        two = _fit(x, k, labels=lab, pad=pad, max_iter=2, covariance=sph, reg_covar=1e-2)          # the start from labels, two iterations
        assert two['stat_all'][:, 0].tolist() == [2, 2, 2] and np.isfinite(two['lower']).all()


# ---------------------------------------------------------------- the start from labels
def test_start_from_labels_leaves_out_of_range_rows_out():
    x = gr.planted(96, 8, 6, 1)
    k = 6
    lab = gr.start_labels(96, k, 2)
    lab[0, 10:20] = [-1, k, 1000, -5, k + 1, -1, -2 ** 31, 2 ** 31 - 1, -1, k]
    lab[1][lab[1] == 3] = -1                                         # component 3 of restart 1 starts empty
    for sph in (0, 1):
        out = _fit(x, k, labels=lab, max_iter=0, covariance=sph)
        assert out['stat_all'].tolist() == [[0, 1, 0, 0]] * 2 and out['stat'].tolist() == [0, 0, 1, 0] and (out['lower'] == -np.inf).all()
        for r in range(2):
            w, mu, cov = gr.start_from_labels(x, lab[r], k, 1e-6, sph)
            resp = gr.onehot(lab[r], k)
            mb = gr.mstep_bounds(x, resp, np.zeros_like(resp), 1e-6, sph)
            assert _ratio(out['weights_all'][r] - w, mb['weights']) <= 1 and _ratio(out['means_all'][r] - mu, mb['means']) <= 1
            assert _ratio(out['covars_all'][r] - cov, mb['covars']) <= 1
        n3 = gr.TEN_EPS / 96
        assert abs(out['weights_all'][1, 3] - n3 / (n3 + (lab[1] >= 0).sum() / 96)) <= 1e-12 * n3
        assert (out['means_all'][1, 3] == 0.0).all() and (np.abs(out['covars_all'][1, 3] - 1e-6) <= 16 * gr.EPS * 1e-6 * sph).all()
        assert np.array_equal(out['weights'], out['weights_all'][0])
        _check_estep(x, out['weights'], out['means'], out['covars'], out['logp'], out['resp'], out['label'])


# ---------------------------------------------------------------- degenerate restarts
def test_degenerate():
    x, lab = gr.repeated_points()
    ref = gr.run(x, 4, 'diag', 1, 10, 1e-3, 0.0, lab[None])
    assert ref['stop'] == 2
    out = _fit(x, 4, labels=lab, max_iter=10, tol=1e-3, reg_covar=0.0)
    assert out['stat'].tolist() == [0, 0, 2, 0] and out['lower'][0] == -np.inf and (out['trace'] == -np.inf).all()
    with pytest.raises(ValueError, match='ill-defined empirical covariance'):
        _model().gmm(x, 4, init=lab, reg_covar=0.0)
    # a healthy restart beside it is the best one
    lab2 = np.stack([lab, gr.start_labels(24, 4)[0]])
    out = _fit(x, 4, labels=lab2, max_iter=1, reg_covar=0.0)
    assert out['stat_all'][0].tolist() == [0, 2, 0, 0] and out['lower'][0] == -np.inf
    if out['stat_all'][1, 1] != 2:
        assert out['stat'][0] == 1
    out = _fit(x, 4, labels=lab, max_iter=10, tol=1e-3, reg_covar=1e-6)
    ref = gr.run(x, 4, 'diag', 1, 10, 1e-3, 1e-6, lab[None])
    assert out['stat'].tolist() == [0, ref['n_iter'], ref['stop'], 0] and ref['stop'] == 0
    for n in ('weights', 'means', 'covars', 'logp', 'resp', 'lower'):
        assert np.isfinite(out[n]).all(), n
    assert np.array_equal(out['label'], lab)
    res = _model().gmm(x, 4, init=lab, reg_covar=1e-6)
    assert res['converged'] and np.array_equal(res['labels'], lab)


# ---------------------------------------------------------------- stops
def test_stops():
    x = gr.planted(96, 8, 6, 1)
    lab = gr.start_labels(96, 6, 1)
    ref = gr.run(x, 6, 'diag', 1, 100, 1e-3, 1e-6, lab)
    assert ref['stop'] == 0 and 3 < ref['n_iter'] < 100 and ref['stop_margin'] > gr.MARGIN
    out = _fit(x, 6, labels=lab, max_iter=3, tol=0.0)                            # max_iter reached
    assert out['stat'].tolist() == [0, 3, 1, 0] and np.isfinite(out['trace']).all() and out['trace'][0, 2] == out['lower'][0]
    out = _fit(x, 6, labels=lab, max_iter=100, tol=1e-3)                         # tol reached
    assert out['stat'].tolist() == [0, ref['n_iter'], 0, 0]
    assert np.isfinite(out['trace'][0, :ref['n_iter']]).all() and (out['trace'][0, ref['n_iter']:] == -np.inf).all()
    assert out['trace'][0, ref['n_iter'] - 1] == out['lower'][0]
    out = _fit(x, 6, labels=lab, max_iter=100, tol=1e300)                        # the second iteration's change is below any such tol
    assert out['stat'].tolist() == [0, 2, 0, 0]
    out = _fit(x, 6, labels=lab, max_iter=0)
    assert out['stat'].tolist() == [0, 0, 1, 0] and out['lower'][0] == -np.inf and out['trace'].size == 0
    _check_estep(x, out['weights'], out['means'], out['covars'], out['logp'], out['resp'], out['label'])


# ---------------------------------------------------------------- the certificate, on data without margins
@pytest.mark.parametrize('reg', [1e-6, 0.0])
def test_certificate(reg):
    x = gr.gaussian(300, 32, 21)
    k, R, T = 17, 4, 40
    lab = gr.start_labels(300, k, R, seed=22)
    out = _fit(x, k, labels=lab, max_iter=T, tol=1e-3, reg_covar=reg)
    b = int(out['stat'][0])
    ok = [r for r in range(R) if out['stat_all'][r, 1] != 2]
    assert ok and b == min(ok, key=lambda r: (-out['lower'][r], r))
    assert out['stat'].tolist() == [b] + out['stat_all'][b, :2].tolist() + [0] and (out['stat_all'][:, 2:] == 0).all()
    for n in ('weights', 'means', 'covars'):
        assert out[n].tobytes() == out[n + '_all'][b].tobytes(), n
    for r in range(R):
        it, how = out['stat_all'][r, :2]
        assert 1 <= it <= T and how in (0, 1, 2)
        tr = out['trace'][r]
        assert (tr[it:] == -np.inf).all() and np.isfinite(tr[:it]).all()
        if how == 2:
            assert out['lower'][r] == -np.inf
            continue
        assert out['lower'][r] == tr[it - 1]
        w, cov = out['weights_all'][r], out['covars_all'][r]
        assert (w > 0).all() and abs(w.sum() - 1) <= (k + 4) * 2 * gr.EPS and (cov > 0).all() and np.isfinite(cov).all()
        if how == 0:
            assert abs(tr[it - 1] - tr[it - 2]) < 1e-3
        else:
            assert it == T
        if it > 1:
            assert (np.abs(np.diff(tr[:it]))[:-1] >= 1e-3).all()              # no earlier iteration met the stop
        if reg == 0.0:                                                         # EM does not decrease the likelihood
            e = gr.estep(x, w, out['means_all'][r], cov)
            slack = 2 * gr.estep_bounds(x, w, out['means_all'][r], cov, e)['lower']
            assert (np.diff(tr[:it]) >= -slack).all(), (r, np.diff(tr[:it]).min(), slack)
    _check_estep(x, out['weights'], out['means'], out['covars'], out['logp'], out['resp'], out['label'], what='certificate')
    assert (np.abs(out['resp'].sum(1) - 1) <= (k + 8) * 4 * gr.EPS + 2 * gr.estep_bounds(x, out['weights'], out['means'], out['covars'],
            gr.estep(x, out['weights'], out['means'], out['covars']))['resp'].sum(1)).all()


# ---------------------------------------------------------------- avae_gmm_score
@pytest.mark.parametrize('chunk', [0, 3])
def test_score(chunk):
    x = gr.planted(257, 16, 9, 3, spread=2.0)
    lab = gr.start_labels(257, 9, 1)
    fit = _fit(x, 9, labels=lab, chunk=chunk, max_iter=5)
    sc = _score(x, fit['weights'], fit['means'], fit['covars'], chunk=chunk)
    assert not _same_bits(fit, sc, ('logp', 'label', 'resp'))                   # on the fitted rows: the fit's own bits
    other = gr.planted(70, 16, 9, 4, spread=2.0)
    sc = _score(other, fit['weights'], fit['means'], fit['covars'], chunk=chunk)
    _check_estep(other, fit['weights'], fit['means'], fit['covars'], sc['logp'], sc['resp'], sc['label'], what='score')
    one = _score(other[:1], fit['weights'], fit['means'], fit['covars'])
    assert one['logp'][0] == _score(other, fit['weights'], fit['means'], fit['covars'])['logp'][0]
    # components 2 and 5 made copies of component 7: the label of a row nearest to them is the FIRST maximum, 2
    w, mu, cov = (np.array(fit[n]) for n in ('weights', 'means', 'covars'))
    for c in (2, 5):
        w[c], mu[c], cov[c] = w[7], mu[7], cov[7]
    tie = _score(x, w, mu, cov, chunk=chunk)
    assert (tie['label'] != 5).all() and (tie['label'] != 7).all() and (tie['label'] == 2).sum() >= (fit['label'] == 7).sum() > 0
    assert (tie['resp'][:, 2] == tie['resp'][:, 5]).all() and (tie['resp'][:, 2] == tie['resp'][:, 7]).all()


def test_same_call_same_bits():
    x = gr.gaussian(300, 32, 21)
    lab = gr.start_labels(300, 17, 3, seed=22)
    for chunk in (0, 7):
        p = _fit(x, 17, labels=lab, chunk=chunk, max_iter=6, covariance=1)
        q = _fit(x, 17, labels=lab, chunk=chunk, max_iter=6, covariance=1)
        assert not _same_bits(p, q)


def test_chunk_never_changes_a_score():
    """gmm_chunk moves last bits of sums only: from the same parameters the final E-step's label is the same and logp agrees to rounding"""
    x = gr.gaussian(200, 128, 4)
    w, mu, cov = gr.start_from_labels(x, gr.start_labels(200, 5)[0], 5, 1e-6, 0)
    p, q = _score(x, w, mu, cov), _score(x, w, mu, cov, chunk=2)
    assert np.array_equal(p['label'], q['label'])
    assert (np.abs(p['logp'] - q['logp']) <= (5 * 5 + 100) * 2 * gr.EPS * np.maximum(np.abs(p['logp']), 1)).all()


# ---------------------------------------------------------------- errors
def test_errors_have_text_and_touch_nothing():
    import torch
    m = _model()
    dev = m.device
    x = gr.planted(96, 8, 6, 1)
    N, dim, k = 96, 8, 6
    dx = _rows(x)
    lab = torch.as_tensor(gr.start_labels(N, k, 2)).to(dev)
    par = [torch.ones(s, dtype=torch.float64, device=dev) for s in ((2, k), (2, k, dim), (2, k, dim))]
    bufs = _buffers(N, dim, k, 2, 3)

    def call(cfg=None, x_=dx, N_=N, dim_=dim, label_in=lab, params=(None, None, None), drop=(), null_cfg=False):
        t = _guarded(bufs, dev)
        cfg = cfg or _cfg(k, n_init=2, max_iter=3, init=0)
        outs = [None if n in drop else _ptr(t[n]) for n in OUTS]
        rc = m._l.avae_gmm_fit(m._h, _ptr(x_) if x_ is not None else None, N_, dim_, None if null_cfg else C.byref(cfg), _ptr(label_in),
                               *[_ptr(p) for p in params], *outs)
        text = m._l.avae_last_error(m._h).decode()
        for n, (s, dt) in bufs.items():
            v = t[n].cpu().numpy()
            assert (v == (SENT_I if dt == torch.int32 else SENT_F)).all(), (n, text)
        return rc, text

    bad = [dict(null_cfg=True), dict(x_=None)] + [dict(drop=(n,)) for n in ('weights', 'means', 'covars', 'label', 'stat', 'lower')]
    bad += [dict(N_=1), dict(N_=(1 << 22) + 1), dict(dim_=0), dict(dim_=6), dict(dim_=1028)]
    bad += [dict(x_=dx.view(-1)[1:])]                                           # not 16-byte aligned
    bad += [dict(cfg=_cfg(k_, n_init=2, max_iter=3, init=0)) for k_ in (0, 97, 1025)]
    bad += [dict(cfg=_cfg(k, n_init=r, max_iter=3, init=0)) for r in (0, 17)]
    bad += [dict(cfg=_cfg(k, n_init=2, max_iter=t, init=0)) for t in (-1, 10001)]
    bad += [dict(cfg=_cfg(k, n_init=2, max_iter=3, init=i)) for i in (-1, 2)]
    bad += [dict(cfg=_cfg(k, n_init=2, max_iter=3, init=0, covariance=c)) for c in (-1, 2)]
    bad += [dict(label_in=None)]
    bad += [dict(cfg=_cfg(k, n_init=2, max_iter=3, init=1), params=p) for p in ((None, par[1], par[2]), (par[0], None, par[2]), (par[0], par[1], None))]
    bad += [dict(drop=d) for d in (('weights_all',), ('means_all',), ('covars_all', 'means_all'))]
    bad += [dict(cfg=_cfg(k, n_init=2, max_iter=3, init=0, tol=v)) for v in (-1.0, float('nan'))]
    bad += [dict(cfg=_cfg(k, n_init=2, max_iter=3, init=0, reg_covar=v)) for v in (-1e-9, float('nan'))]
    bad += [dict(cfg=_cfg(k, n_init=2, max_iter=3, init=0, reserved=1))]
    texts = set()
    for kw in bad:
        rc, text = call(**kw)
        assert rc != 0 and 'gmm' in text, (kw, rc, text)
        texts.add(text)
    assert len(texts) >= 14
    for key, v in ((b'gmm_chunk', -1), (b'gmm_pad', 4), (b'gmm_pad', -1)):
        assert m._l.avae_set_option(m._h, key, v) != 0
    # the score entry's
    t = _guarded(dict(logp=((N,), torch.float64)), dev)
    for args in ((None, N, dim, k), (dx, 0, dim, k), (dx, N, 6, k), (dx, N, dim, 0), (dx, N, dim, 1025)):
        rc = m._l.avae_gmm_score(m._h, _ptr(args[0]) if args[0] is not None else None, *args[1:], _ptr(par[0]), _ptr(par[1]), _ptr(par[2]),
                                 _ptr(t['logp']), None, None)
        assert rc != 0 and 'gmm score' in m._l.avae_last_error(m._h).decode()
    assert m._l.avae_gmm_score(m._h, _ptr(dx), N, dim, k, _ptr(par[0]), _ptr(par[1]), _ptr(par[2]), None, None, None) != 0
    assert (t['logp'].cpu().numpy() == SENT_F).all()
    # the handle is usable afterwards: the optional outputs may all be absent
    rc, text = 0, ''
    t = _guarded(bufs, dev)
    cfg = _cfg(k, n_init=2, max_iter=3, init=0)
    opt = ('logp', 'resp', 'weights_all', 'means_all', 'covars_all', 'stat_all', 'trace')
    m._ck(m._l.avae_gmm_fit(m._h, _ptr(dx), N, dim, C.byref(cfg), _ptr(lab), None, None, None, *[None if n in opt else _ptr(t[n]) for n in OUTS]))
    got = _unguard({n: t[n] for n in OUTS if n not in opt}, {n: bufs[n] for n in OUTS if n not in opt})
    full = _fit(x, k, labels=lab.cpu().numpy(), max_iter=3)
    assert not _same_bits(got, full, ('weights', 'means', 'covars', 'label', 'stat', 'lower'))


# ---------------------------------------------------------------- the Python layer
def test_python_layer_with_padded_columns():
    m = _model()
    z = gr.planted(200, 10, 4, 8, spread=4.0)                                   # 10 columns: padded to 12 for the device
    lab = gr.start_labels(200, 4, 1, seed=9)
    for covariance in ('diag', 'spherical'):
        ref = gr.run(z, 4, covariance, 1, 100, 1e-3, 1e-6, lab)
        assert gr.has_margins(ref)
        res = m.gmm(z, 4, covariance=covariance, init=lab, return_resp=True, return_all=True)
        assert res['means'].shape == (4, 10) and res['covariances'].shape == ((4, 10) if covariance == 'diag' else (4,))
        assert res['resp'].shape == (200, 4) and res['trace'].shape == (1, 100) and res['weights_all'].shape == (1, 4)
        assert (res['best'], res['n_iter'], res['stop'], res['converged']) == (ref['best'], ref['n_iter'], 'converged', True)
        assert np.array_equal(res['labels'], ref['labels'])
        cov = res['covariances'] if covariance == 'diag' else np.repeat(res['covariances'][:, None], 10, 1)
        for got, want in ((res['weights'], ref['weights']), (res['means'], ref['means']), (cov, ref['covars']), (res['logp'], ref['logp']),
                          (np.array(res['lower_bound']), np.array(ref['lower']))):
            assert np.abs(got - want).max() <= gr.MARGIN * np.abs(want).max()
        npar, bic, aic = gr.bic_aic(ref['logp'].mean(), 200, 4, 10, covariance)
        assert res['n_parameters'] == npar and abs(res['bic'] - bic) <= 2 * gr.MARGIN * abs(bic) and abs(res['aic'] - aic) <= 2 * gr.MARGIN * abs(aic)
        sc = m.gmm_score(z, res, return_resp=True)
        assert sc['logp'].tobytes() == res['logp'].tobytes() and np.array_equal(sc['labels'], res['labels']) and sc['resp'].tobytes() == res['resp'].tobytes()
        again = m.gmm(z, 4, covariance=covariance, init=dict(weights=res['weights'], means=res['means'], covariances=res['covariances']), max_iter=0)
        assert again['logp'].tobytes() == res['logp'].tobytes() and again['n_iter'] == 0
    km = m.gmm(z, 4, n_init=2, seed=3)                                          # the k-means start
    assert km['converged'] and km['lower_bounds'].shape == (2,) and np.isfinite(km['logp']).all()
    sw = m.sweep_gmm(z, [2, 4, 6], seed=3)
    assert sw['k'] == [2, 4, 6] and sw['best'] == sw['k'][int(np.argmin(sw['bic']))] and len(sw['models']) == 3 and sw['best'] == 4
    from argsim_amd import gmm as G
    R = m.cfg['dim_rep']
    prior = dict(weights=np.array([0.25, 0.75]), means=np.stack([np.full(R, -2.0), np.full(R, 2.0)]), covariances=np.array([0.01, 0.04]))
    zz, comp = G.sample(prior, 5, seed=4)
    assert np.array_equal(m.prior_draw(5, 4, prior), zz) and zz.shape == (5, R) and zz.dtype == np.float32
    assert np.array_equal(m.prior_draw(5, 4), np.random.default_rng(4).standard_normal((5, R)).astype(np.float32))
    ids = m.generate(5, steps=6, seed=4, prior=prior)
    assert np.array_equal(np.asarray(ids), np.asarray(m.sample(zz, 6, 1.0, 0, 4)))
    with pytest.raises(ValueError):
        m.generate(5, steps=6, prior=dict(weights=np.ones(1), means=np.zeros((1, R + 1)), covariances=np.ones(1)))
