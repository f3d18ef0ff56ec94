"""Affinity propagation on the device (avae_affinity, VAE.affinity) against the float64 reference of tests/ap_ref.py.

No tolerance here is measured.  A similarity is ONE rounding to fp32 of a double result (within one fp32 ulp of the float64 value; the
double summation order may differ from numpy's), the median is an exact selection, the noise is bounded by the generator's range
(|normal01| < 6), one step stays inside the derived step bounds of ap_ref, and on the margin cases (ap_ref.CASES; asserted on the CPU
by tests/test_affinity.py and again here on the device's own S) every decision of the run has a margin far above the fp32 error, so
that stat, exemplars and labels equal the float64 reference's exactly.  For ANY input the result carries a certificate that is
evaluated from the returned s, a and r.  Operands are padded with NaN rows and outputs guarded by a sentinel.  (The refusal of a
workspace the device cannot give is not provoked: within N <= 2^14 the call needs 3.3 GB at the most.)"""
import ctypes as C
import math

import numpy as np
import pytest

import ap_ref as ar

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


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else None


def _cfg(metric=0, max_iter=200, convergence_iter=15, preference=None, noise=0, warm=0, damping=0.5, seed=0, reserved=(0, 0)):
    from argsim_amd import lib
    return lib.AvaeAffinityConfig(metric=metric, max_iter=max_iter, convergence_iter=convergence_iter, use_preference=0 if preference is None else 1,
                                  noise=noise, warm=warm, damping=damping, preference=0.0 if preference is None else preference, seed=seed,
                                  reserved=(C.c_int32 * 2)(*reserved))


def _ap(x, a=None, r=None, messages=True, want_s=True, **kw):
    """avae_affinity on NaN-padded rows and sentinel-guarded outputs -> dict(label, stat, s, a, r) numpy"""
    import torch
    m = _model()
    dev = m.device
    x = np.ascontiguousarray(x, np.float32)
    N, dim = x.shape
    dx = torch.full((N + 3, dim), float('nan'), dtype=torch.float32, device=dev)
    dx[:N] = torch.as_tensor(x).to(dev)
    label = torch.full((N + 4,), SENT_I, dtype=torch.int32, device=dev)
    stat = torch.full((8,), SENT_I, dtype=torch.int32, device=dev)
    mats = {}
    for name, init, on in (('s', None, want_s), ('a', a, messages), ('r', r, messages)):
        if on:
            mats[name] = torch.full((N * N + 8,), SENT_F, dtype=torch.float32, device=dev)
            if init is not None:
                mats[name][:N * N] = torch.as_tensor(np.ascontiguousarray(init, np.float32).ravel()).to(dev)
    cfg = _cfg(**kw)
    m._stream()
    m._ck(m._l.avae_affinity(m._h, _ptr(dx), N, dim, C.byref(cfg), _ptr(label), _ptr(stat), _ptr(mats.get('s')), _ptr(mats.get('a')),
                             _ptr(mats.get('r'))))
    label, stat = label.cpu().numpy(), stat.cpu().numpy()
    assert (label[N:] == SENT_I).all() and (stat[4:] == SENT_I).all()
    out = dict(label=label[:N], stat=stat[:4])
    for name, t in mats.items():
        v = t.cpu().numpy()
        assert (v[N * N:] == SENT_F).all(), name
        out[name] = v[:N * N].reshape(N, N)
    return out


def _same_bits(p, q, names=('label', 'stat', 'a', 'r', 's')):
    return all(np.array_equal(p[n].view(np.uint32), q[n].view(np.uint32)) for n in names if n in p)


def _certificate(out):
    """what any result must satisfy, from the returned s, a and r alone"""
    s, a, r, label, stat = out['s'].astype(np.float64), out['a'], out['r'], out['label'], out['stat']
    N = s.shape[0]
    E = (np.diag(a) + np.diag(r)) > np.float32(0)                     # fp32, as the device forms it
    assert stat[2] == E.sum() and stat[3] == 0
    if not E.any():
        assert (label == -1).all()
        return
    ex = np.unique(label)
    assert len(ex) == E.sum() and (label[ex] == ex).all()              # every label is an exemplar's row; exemplars label themselves
    assert np.array_equal(label, ar.assign(s, ex))                     # stored fp32 values: the maximum over the final exemplars, exactly
    first = ar.assign(s, np.flatnonzero(E))
    worst = 0.0
    for e in np.flatnonzero(E):
        ii = np.flatnonzero(first == e)
        sums = np.array([math.fsum(s[ii, j]) for j in ii])
        mine = [t for t, j in enumerate(ii) if j in set(ex.tolist())]
        assert len(mine) == 1, (e, ii, ex)
        best = sums.max()
        worst = max(worst, (best - sums[mine[0]]) / max(abs(best), 1e-300))
        assert sums[mine[0]] >= best - 2.0 ** -22 * abs(best), (e, sums)
    print("worst refinement shortfall %.3g" % worst)


@pytest.mark.parametrize('N', [2, 3, 37, 96, 200, 257])
def test_similarity_diagonal_and_median(N):
    """both metrics at dim 4, 12 (padded to 16) and 128: within one ulp of float64, symmetric, the diagonal exactly the median of the
    fp32 matrix (N^2 odd and even)"""
    for dim in (4, 12, 128):
        x = ar.pad4(ar.gaussian(N, dim, 10 * N + dim))
        for metric in (0, 1):
            out = _ap(x, metric=metric, max_iter=1, convergence_iter=1, messages=False)
            s = out['s']
            ref = ar.similarity(x, metric)
            off = ~np.eye(N, dtype=bool)
            err = np.abs(s.astype(np.float64) - ref)[off]
            assert (err <= np.spacing(np.abs(ref.astype(np.float32)))[off]).all(), (N, dim, metric, err.max())
            assert np.array_equal(s.view(np.uint32), s.T.copy().view(np.uint32))
            clean = s.copy()
            np.fill_diagonal(clean, 0)
            pref = np.median(clean)
            assert pref.dtype == np.float32 and (np.diag(s).view(np.uint32) == pref.view(np.uint32)).all(), (N, dim, metric, pref, s[0, 0])


def test_given_preference_and_precomputed():
    x = ar.pad4(ar.gaussian(37, 12, 2))
    S = ar.similarity(x, 1).astype(np.float32)
    pre = _ap(S, metric=2, preference=-0.75, max_iter=1, convergence_iter=1, messages=False)['s']
    want = S.copy()
    np.fill_diagonal(want, np.float32(-0.75))
    assert np.array_equal(pre.view(np.uint32), want.view(np.uint32))
    own = _ap(S, metric=2, max_iter=1, convergence_iter=1, messages=False)['s']       # the median takes the matrix's own diagonal
    assert (np.diag(own) == np.median(S)).all() and np.array_equal(own[~np.eye(37, dtype=bool)], S[~np.eye(37, dtype=bool)])
    full = _ap(S, metric=2)
    ref = ar.run(full['s'].astype(np.float64))
    assert ar.has_margins(ref)
    assert full['stat'].tolist() == [ref['n_iter'], ref['converged'], ref['K'], 0] and np.array_equal(full['label'], ref['label'])


def test_one_row():
    out = _ap(np.ones((1, 4), np.float32))
    assert out['label'].tolist() == [0] and out['stat'].tolist() == [0, 1, 1, 0]
    assert out['s'][0, 0] == SENT_F and out['a'][0, 0] == SENT_F                    # nothing else runs


def test_noise():
    x = ar.pad4(ar.gaussian(37, 12, 2))
    kw = dict(metric=0, max_iter=1, convergence_iter=1, messages=False)
    clean = _ap(x, **kw)['s']
    one, again, other = _ap(x, noise=1, seed=1, **kw)['s'], _ap(x, noise=1, seed=1, **kw)['s'], _ap(x, noise=1, seed=2, **kw)['s']
    for noisy in (one, other):
        d = np.abs(noisy.astype(np.float64) - clean.astype(np.float64))
        assert (d <= 6 * ar.noise_scale(clean) + np.spacing(np.abs(clean)).astype(np.float64)).all()
        assert d.max() > 0
    assert ar.NORMAL_MAX < 6
    assert np.array_equal(one.view(np.uint32), again.view(np.uint32)) and not np.array_equal(one, other)


def _check_step(S, A0, R0, out, lam):
    """the device's step from (S, A0, R0) against float64 within the derived bounds; A from the device's own new R"""
    S, A0, R0 = (np.asarray(v, np.float64) for v in (S, A0, R0))
    Rn = ar.responsibilities(S, A0, R0, lam)
    dR = np.abs(out['r'].astype(np.float64) - Rn)
    bR = ar.bound_R(S, A0, R0)
    An = ar.availabilities(A0, out['r'].astype(np.float64), lam)
    dA = np.abs(out['a'].astype(np.float64) - An)
    bA = ar.bound_A(A0, out['r'])
    print("R: worst error / bound %.3g   A: %.3g" % ((dR / bR).max(), (dA / np.where(bA > 0, bA, 1)).max()))
    assert (dR <= bR).all() and (dA <= bA).all()
    E = (np.diag(out['a']) + np.diag(out['r'])) > np.float32(0)
    assert out['stat'].tolist() == [1, 0, int(E.sum()), 0]


@pytest.mark.parametrize('shape', [(96, 8), (257, 4), (1024, 64)], ids=lambda s: '%dx%d' % s)
def test_one_step_from_a_given_state(shape):
    """warm = 1, max_iter = 1 from random messages; 1024 rows reach 128 blocks of column partials"""
    N, dim = shape
    r = np.random.default_rng(N)
    x = ar.pad4(ar.gaussian(N, dim, N + 1))
    A0 = (-np.abs(r.standard_normal((N, N))) * 3).astype(np.float32)
    R0 = (r.standard_normal((N, N)) * 3).astype(np.float32)
    for lam in (0.5, 0.8125):
        out = _ap(x, a=A0, r=R0, warm=1, max_iter=1, convergence_iter=1, damping=lam)
        _check_step(out['s'], A0, R0, out, lam)


def test_steps_from_zero():
    x = ar.pad4(ar.planted(96, 8, 6, 1))
    N = 96
    A, R = np.zeros((N, N), np.float32), np.zeros((N, N), np.float32)
    cold = _ap(x, max_iter=1, convergence_iter=1)
    _check_step(cold['s'], A, R, cold, 0.5)
    out = cold
    for _ in range(2):
        A, R = out['a'], out['r']
        out = _ap(x, a=A, r=R, warm=1, max_iter=1, convergence_iter=1)
        _check_step(out['s'], A, R, out, 0.5)
    three = _ap(x, max_iter=3, convergence_iter=3)            # the same three steps in one call: the same bits
    assert _same_bits(three, out, ('a', 'r', 's'))


def test_two_equal_maxima():
    """a row whose two largest A + S are equal: the second maximum IS the first, so both columns get S - Y; exact in fp32"""
    S = -np.array([[0, 2, 2, 5], [2, 0, 3, 4], [2, 3, 0, 1], [5, 4, 1, 0]], np.float32)
    out = _ap(S, metric=2, preference=-3.0, max_iter=1, convergence_iter=1)
    P = S.astype(np.float64)
    np.fill_diagonal(P, -3.0)
    An, Rn, E = ar.step(P, np.zeros((4, 4)), np.zeros((4, 4)), 0.5)
    assert np.array_equal(out['r'], Rn.astype(np.float32)) and np.array_equal(out['a'], An.astype(np.float32))
    assert out['r'][0, 1] == 0 and out['r'][0, 2] == 0


@pytest.mark.parametrize('case', ar.CASES, ids=ar.CASE_IDS)
def test_exact_cases(case):
    name, make, metric = case
    out = _ap(ar.pad4(make()), metric=metric)
    ref = ar.run(out['s'].astype(np.float64))
    print(name, "iterations %d, K %d, margins %s" % (ref['n_iter'], ref['K'], ref['margins']))
    assert ar.has_margins(ref)
    assert out['stat'].tolist() == [ref['n_iter'], ref['converged'], ref['K'], 0]
    assert np.array_equal(np.unique(out['label']), ref['exemplars']) and np.array_equal(out['label'], ref['label'])
    _certificate(out)


def test_one_iteration_has_no_exemplar_and_a_low_preference_never_converges():
    x = ar.pad4(ar.gaussian(37, 12, 2))
    out = _ap(x, metric=1, max_iter=1, convergence_iter=1)
    assert out['stat'].tolist() == [1, 0, 0, 0] and (out['label'] == -1).all()
    out = _ap(x, metric=1, preference=-1e6, max_iter=40)
    assert out['stat'].tolist() == [40, 0, 0, 0] and (out['label'] == -1).all()
    _certificate(out)


@pytest.mark.parametrize('which', ['n2', 'n3', 'n257', 'repeated', 'noisy', 'unconverged', 'big'])
def test_certificate(which):
    if which[1:].isdigit():          # whole runs at the smallest sizes and one row past a row block and a wave
        N = int(which[1:])
        out = _ap(ar.gaussian(N, 4, N), metric=0, noise=1, seed=N)
    elif which == 'repeated':          # 4 points 6 times, noise off: ties everywhere, fp32 and float64 may part
        out = _ap(ar.repeated_points(), metric=0)
    elif which == 'noisy':
        out = _ap(ar.repeated_points(), metric=0, noise=1, seed=3)
    elif which == 'unconverged':     # stopped by max_iter with exemplars: labels all the same
        out = _ap(ar.pad4(ar.gaussian(200, 16, 3)), metric=1, max_iter=20, convergence_iter=15)
        assert out['stat'][0] == 20
    else:
        out = _ap(ar.pad4(ar.planted(1024, 64, 12, 8)), metric=0, noise=1, seed=5)
        assert out['stat'][2] > 0
    _certificate(out)


def test_errors_have_text():
    import torch
    m = _model()
    dev = m.device
    N = 8
    x = torch.ones((N, 8), dtype=torch.float32, device=dev)
    label = torch.full((N,), SENT_I, dtype=torch.int32, device=dev)
    stat = torch.full((4,), SENT_I, dtype=torch.int32, device=dev)
    s, a, r = (torch.full((N * N,), SENT_F, dtype=torch.float32, device=dev) for _ in range(3))

    def call(x=x, N=N, dim=8, label=label, stat=stat, s=s, a=a, r=r, off=0, null_cfg=False, **kw):
        cfg = _cfg(**kw)
        return m._l.avae_affinity(m._h, _ptr(x, off), N, dim, None if null_cfg else C.byref(cfg), _ptr(label), _ptr(stat), _ptr(s), _ptr(a), _ptr(r))

    bad = [dict(null_cfg=True), dict(x=None), dict(label=None), dict(stat=None), dict(N=0), dict(N=(1 << 14) + 1), dict(dim=6), dict(dim=0),
           dict(dim=1028), dict(max_iter=0), dict(max_iter=10001), dict(convergence_iter=0), dict(convergence_iter=201), dict(damping=0.25),
           dict(damping=1.0), dict(damping=float('nan')), dict(metric=3), dict(metric=-1), dict(metric=2, dim=12), dict(off=4), dict(a=None),
           dict(r=None), dict(warm=1, a=None, r=None), dict(reserved=(1, 0)), dict(reserved=(0, 1))]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert len(m._l.avae_last_error(m._h)) > 5, kw
    torch.cuda.synchronize(dev)
    assert (label == SENT_I).all() and (stat == SENT_I).all() and all((t == SENT_F).all() for t in (s, a, r))      # outputs untouched
    assert call() == 0                                     # the handle stays usable
    assert call(s=None, a=None, r=None) == 0               # the matrices are optional
    torch.cuda.synchronize(dev)
    assert (label != SENT_I).all() and (stat != SENT_I).all()


def test_rows_that_are_not_finite_give_complete_labels():
    base = ar.pad4(ar.gaussian(37, 12, 2))
    for bad in (np.nan, np.inf):
        for metric in (0, 1):
            x = base.copy()
            x[5] = bad
            x[20, 3] = bad
            out = _ap(x, metric=metric, max_iter=30)
            label = out['label']
            assert 1 <= out['stat'][0] <= 30 and ((label >= -1) & (label < 37)).all()
            ex = np.unique(label[label >= 0])
            assert (label[ex] == ex).all()


def test_the_same_call_twice_gives_the_same_bits():
    x = ar.pad4(ar.gaussian(200, 16, 3))
    for kw in (dict(metric=1), dict(metric=0, noise=1, seed=9)):
        assert _same_bits(_ap(x, **kw), _ap(x, **kw))


def test_python_layer():
    from argsim_amd import affinity as af
    from argsim_amd import model
    m = _model()
    z = ar.gaussian(37, 12, 2)                              # 12 columns: padded with zeros
    raw = _ap(ar.pad4(z), metric=1, noise=1, seed=4)
    res = m.affinity(z, 'cosine', seed=4)
    ex = np.unique(raw['label'])
    assert np.array_equal(res['exemplars'], ex) and np.array_equal(res['labels'], np.searchsorted(ex, raw['label']))
    assert res['n_iter'] == raw['stat'][0] and res['converged'] == bool(raw['stat'][1])
    fn = model.affinity(m, z, 'cosine', seed=4, return_messages=True)
    assert np.array_equal(fn['labels'], res['labels']) and np.array_equal(fn['s'].view(np.uint32), raw['s'].view(np.uint32))
    none = m.affinity(z, 'euclidean', max_iter=1, convergence_iter=1)
    assert (none['labels'] == -1).all() and len(none['exemplars']) == 0 and not none['converged']
    pre = m.affinity(raw['s'], 'precomputed', preference=float(raw['s'][0, 0]), noise=False)
    assert len(pre['exemplars']) > 0 and af.dist_to_centroids(z, pre['labels'], 'cosine').shape == (37,)
