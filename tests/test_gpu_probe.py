"""linear probes on the device (avae_probe_fit, avae_probe_decision, VAE.probe_fit, VAE.probe_cv) against the float64 reference of
tests/probe_ref.py.

No tolerance here is measured.  Every problem is strongly convex with modulus 1, so a returned w carries its own certificate,
|w - w*| <= |grad f(w)|, whose right-hand side the test evaluates in float64; the stop rule is held to |grad f(w)| <= 2 tol |grad f(0)|
in float64 (the device's own gradient must be within a factor 2 of the real one), the loss to the summation bound of N + dim
fp32 terms, the decisions to the standard dot-product bound.  Shapes: probe_ref.CASES (remainders 1, tile - 1, tile + 1 on the row
tile of 128 and the problem tile of 32; dims 4, 36, 128, 1024), whose inputs tests/test_probe.py checks on the CPU.  Operands are
padded with NaN rows and outputs guarded by a sentinel."""
import ctypes as C

import numpy as np
import pytest

import probe_ref as pr

pytestmark = pytest.mark.gpu

TOL, MAX_NEWTON, MAX_CG = 1e-4, 50, 30
KEYS = ('dim_tgt', 'dim_emb', 'dim_rep', 'rnn_layers', 'accelerate', 'learn_rate', 'bos', 'eos')
SENTINEL = 123.0
_STATE = {}
_RUNS = {}


def _model():
    if 'm' not in _STATE:
        from helpers import make_case
        from argsim_amd.model import VAE
        cfg, P, ids, keep, eps = make_case('tiny')
        m = VAE('infer', init=False, **{k: cfg[k] for k in KEYS})
        m.set_params(P)
        _STATE['m'] = m
    return _STATE['m']


def _padded(x, extra=3):
    """the rows of x on the device with `extra` NaN rows behind them: a read beyond the array shows in the result"""
    import torch
    x = np.asarray(x, np.float32)
    t = torch.full((x.shape[0] + extra, x.shape[1]), float('nan'), dtype=torch.float32, device=_model().device)
    t[:x.shape[0]] = torch.as_tensor(np.array(x, order='C')).to(t.device)
    return t


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else None


def _raw_fit(x, N, dim, s, P, w, stats, tol=TOL, max_newton=MAX_NEWTON, max_cg=MAX_CG, reserved=0, null_cfg=False):
    """the C entry as it stands -> its return code"""
    from argsim_amd import lib
    m = _model()
    pc = lib.AvaeProbeConfig(max_newton, max_cg, tol, reserved)
    m._stream()
    return m._l.avae_probe_fit(m._h, x, N, dim, s, P, None if null_cfg else C.byref(pc), w, stats)


def _fit(x, s, tol=TOL, max_newton=MAX_NEWTON, max_cg=MAX_CG):
    """avae_probe_fit on NaN-padded inputs and sentinel-guarded outputs -> (w (P, dim + 1), stats (P, 4)) numpy"""
    import torch
    m = _model()
    (N, dim), P = x.shape, s.shape[0]
    dx, ds = _padded(x), _padded(s)
    w = torch.full((P * (dim + 1) + 4,), SENTINEL, dtype=torch.float32, device=m.device)
    st = torch.full((P * 4 + 4,), SENTINEL, dtype=torch.float32, device=m.device)
    m._ck(_raw_fit(_ptr(dx), N, dim, _ptr(ds), P, _ptr(w), _ptr(st), tol, max_newton, max_cg))
    w, st = w.cpu().numpy(), st.cpu().numpy()
    assert (w[P * (dim + 1):] == SENTINEL).all() and (st[P * 4:] == SENTINEL).all()
    return w[:P * (dim + 1)].reshape(P, dim + 1), st[:P * 4].reshape(P, 4)


def _decision(x, w):
    import torch
    m = _model()
    (n, dim), P = x.shape, w.shape[0]
    dx, dw = _padded(x), _padded(w)
    out = torch.full((n * P + 4,), SENTINEL, dtype=torch.float32, device=m.device)
    m._stream()
    m._ck(m._l.avae_probe_decision(m._h, _ptr(dx), n, dim, _ptr(dw), P, _ptr(out)))
    out = out.cpu().numpy()
    assert (out[n * P:] == SENTINEL).all()
    return out[:n * P].reshape(n, P)


def _same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)) for x, y in zip(a, b))


def _run(case):
    """the default-plan fit of a case (cached and shared: never modified)"""
    if case not in _RUNS:
        out = _fit(*pr.case_inputs(case))
        for a in out:
            a.setflags(write=False)
        _RUNS[case] = out
    return _RUNS[case]


def _check_certificate(case, w, st, tol=TOL):
    x, s = pr.case_inputs(case)
    N, P, dim = case
    ref, g0 = pr.case_ref(case), pr.g0_64(x, s)
    worst = 0.0
    for p in range(P):
        g = float(np.linalg.norm(pr.grad64(x, s[p], w[p])))
        err = float(np.linalg.norm(w[p].astype(np.float64) - ref[p]))
        f = pr.objective64(x, s[p], w[p])
        if g0[p] > 0:
            worst = max(worst, g / (tol * g0[p]))
        assert st[p, 3] == 0, (p, st[p])                                       # converged
        assert g <= 2 * tol * g0[p], (p, g, tol * g0[p], st[p])                # the stop rule is truthful
        assert err <= g, (p, err, g)                                           # the theorem: a wrong objective fails here
        assert abs(st[p, 0] - f) <= 2 * (N + dim) * 2.0 ** -24 * abs(f), (p, st[p, 0], f)
        assert 0 <= st[p, 2] <= MAX_NEWTON and st[p, 2] == int(st[p, 2])
        if not s[p].any():
            assert not w[p].any() and st[p, 2] == 0 and st[p, 0] == 0 and st[p, 1] == 0, (p, st[p])
    print("worst |grad f|_64 / (tol g0) = %.3f, most Newton iterations %d" % (worst, int(st[:, 2].max())))


@pytest.mark.parametrize('case', pr.CASES, ids=pr.CASE_IDS)
def test_certificate(case):
    w, st = _run(case)
    assert np.isfinite(w).all() and np.isfinite(st).all()
    _check_certificate(case, w, st)


@pytest.mark.parametrize('case', pr.CASES, ids=pr.CASE_IDS)
def test_a_problem_does_not_depend_on_its_companions(case):
    x, s = pr.case_inputs(case)
    w, st = _run(case)
    P = s.shape[0]
    # the same call again: the same bits
    assert _same_bits(_fit(x, s), (w, st))
    # all problems in another order
    perm = np.random.default_rng(5).permutation(P)
    w2, st2 = _fit(x, np.ascontiguousarray(s[perm]))
    assert _same_bits((w2, st2), (w[perm], st[perm]))
    # every problem alone
    for p in range(P):
        w1, st1 = _fit(x, np.ascontiguousarray(s[p:p + 1]))
        assert _same_bits((w1, st1), (w[p:p + 1], st[p:p + 1])), p


@pytest.mark.parametrize('case', pr.CASES, ids=pr.CASE_IDS)
def test_parts_meet_the_certificate(case):
    x, s = pr.case_inputs(case)
    m = _model()
    try:
        m.set_option('probe_chunk', 50)           # 3 (N 127, 129), 4 (N 200) and 6 (N 257) parts, none a multiple of the tile
        w, st = _fit(x, s)
        assert _same_bits(_fit(x, s), (w, st))
    finally:
        m.set_option('probe_chunk', 0)
    _check_certificate(case, w, st)
    assert _same_bits(_fit(x, s), _run(case))


@pytest.mark.parametrize('case', pr.CASES, ids=pr.CASE_IDS)
def test_decision(case):
    x, _ = pr.case_inputs(case)
    w = pr.case_ref(case).astype(np.float32)
    want = pr.tilde(x) @ w.astype(np.float64).T
    bound = pr.decision_bound(x, w)
    got = _decision(x, w)
    assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) - bound).max())
    m = _model()
    try:
        m.set_option('probe_chunk', 50)
        got2 = _decision(x, w)
    finally:
        m.set_option('probe_chunk', 0)
    assert _same_bits([got2], [got])              # a row's decision does not depend on the part it falls in
    from argsim_amd import probe
    assert _same_bits([probe.decision_raw(m, x, w)], [got])


def test_cross_validation_predicts_what_the_reference_predicts():
    from argsim_amd import probe
    m = _model()
    z, labels, folds, groups = pr.cv_inputs()
    res = m.probe_cv(z, labels, folds, groups, C=pr.CV_C, tol=pr.CV_TOL, max_newton=MAX_NEWTON, max_cg=MAX_CG, return_parts=True)
    jobs, costs, w = res['jobs'], res['costs'], res['w']
    assert costs.shape[0] == 25 and (res['stats'][:, 3] == 0).all()
    ref_w = np.stack([pr.newton64(z, costs[p]) for p in range(costs.shape[0])])
    cert = np.array([np.linalg.norm(pr.grad64(z, costs[p], w[p])) for p in range(costs.shape[0])])
    assert (np.linalg.norm(w - ref_w, axis=1) <= cert).all()
    dec64 = pr.tilde(z) @ ref_w.T
    dbound = pr.decision_bound(z, w)
    ref = probe.cv_predictions(jobs, labels, dec64)
    skip = np.zeros(len(labels), bool)
    for j in jobs:
        v, sl = j['valid'], slice(j['lo'], j['hi'])
        skip[v] = pr.undecided(z[v], j['classes'], dec64[v, sl], cert[sl], dbound[v, sl])
    print("rows too close to call: %d of %d" % (skip.sum(), len(labels)))
    assert skip.mean() <= 0.05
    assert (res['pred'][~skip] == ref['pred'][~skip]).all()
    for g in ref['scores']:
        in_g = groups == g
        # a group's score is a mean over folds of accuracies: an excluded row moves it by at most 1 / (its fold's size)
        room = sum(skip[j['valid']].sum() / len(j['valid']) for j in jobs if j['group'] == g) / sum(1 for j in jobs if j['group'] == g)
        assert abs(res['scores'][g] - ref['scores'][g]) <= room + 1e-12, (g, res['scores'][g], ref['scores'][g], room, in_g.sum())
    # probe_fit on one job's training rows is that job's model, bit for bit
    j = jobs[0]
    train = np.flatnonzero((groups == j['group']) & (folds != j['fold']))
    one = m.probe_fit(z, labels, C=pr.CV_C, train=train, tol=pr.CV_TOL, max_newton=MAX_NEWTON, max_cg=MAX_CG)
    assert list(one.classes_) == list(j['classes'])
    assert _same_bits([one.coef_, one.intercept_], [w[j['lo']:j['hi'], :-1], w[j['lo']:j['hi'], -1]])
    assert (one.predict(z[j['valid']]) == res['pred'][j['valid']]).all()


def test_eval_probe_prints_the_reference_format(tmp_path, capsys):
    from argsim_amd import eval_probe
    z, labels, folds, groups = pr.cv_inputs()
    names = np.array(['%s-%s-%s' % (g, 'pro' if c in ('c0', 'c1') else 'con', c) for g, c in zip(groups, labels)])
    for name, a in (('z', z), ('l', names), ('f', folds)):
        np.save(str(tmp_path / (name + '.npy')), a)
    args = ['--inputs', str(tmp_path / 'z.npy'), '--labels', str(tmp_path / 'l.npy'), '--folds', str(tmp_path / 'f.npy')]
    res = eval_probe.main(args)
    lines = capsys.readouterr().out.strip().split('\n')
    want = _model().probe_cv(z, labels, folds, groups)              # the class is stance-reason: the same partition of the rows as labels
    assert res['scores'] == want['scores'] and lines == ['a %.2f' % (100 * want['scores']['a']), 'b %.2f' % (100 * want['scores']['b']), str(want['mean'])]
    eval_probe.main(args + ['--stance'])
    lines = capsys.readouterr().out.strip().split('\n')
    assert len(lines) == 4 and 0.0 <= float(lines[0]) <= 1.0 and lines[1].startswith('a ') and lines[2].startswith('b ')


def test_values_that_are_not_finite_end_their_problem_alone():
    case = pr.CASES[1]
    x, s = pr.case_inputs(case)
    w, st = _run(case)
    s2 = s.copy()
    s2[4, 17] = np.nan
    s2[6, 3] = np.inf
    w2, st2 = _fit(x, s2)
    keep = np.ones(s.shape[0], bool)
    keep[[4, 6]] = False
    assert st2[4, 3] == 2 and st2[6, 3] == 2
    assert _same_bits((w2[keep], st2[keep]), (w[keep], st[keep]))
    # an infinite row: every problem that holds it ends with status 2; the call returns
    x2 = x.copy()
    x2[9, 1] = np.inf
    _, st3 = _fit(x2, s)
    assert (st3[s[:, 9] != 0, 3] == 2).all()
    # max_newton reached: status 1 after exactly that many iterations
    _, st4 = _fit(x, s[:2], tol=1e-6, max_newton=1)
    assert (st4[:, 3] == 1).all() and (st4[:, 2] == 1).all()


def test_errors_have_text():
    import torch
    m = _model()
    dev = m.device
    x = torch.ones((8, 8), dtype=torch.float32, device=dev)
    s = torch.ones((2, 8), dtype=torch.float32, device=dev)
    w = torch.full((2, 12), SENTINEL, dtype=torch.float32, device=dev)
    st = torch.full((2, 4), SENTINEL, dtype=torch.float32, device=dev)
    out = torch.full((8, 2), SENTINEL, dtype=torch.float32, device=dev)
    ok = dict(x=_ptr(x), N=8, dim=8, s=_ptr(s), P=2, w=_ptr(w), stats=_ptr(st))
    bad = [dict(x=None), dict(s=None), dict(w=None), dict(null_cfg=True), dict(N=0), dict(P=0), dict(N=(1 << 31) - 255), dict(P=(1 << 20) + 1), dict(max_newton=0),
           dict(max_cg=0), dict(tol=-1.0), dict(tol=float('nan')), dict(reserved=1), dict(dim=6), dict(dim=0), dict(dim=1028),
           dict(x=_ptr(x, 4)), dict(w=_ptr(w, 4)), dict(N=1 << 30, dim=1024, P=1 << 20)]
    for kw in bad:
        assert _raw_fit(**dict(ok, **kw)) != 0, kw
        assert len(m._l.avae_last_error(m._h)) > 5, kw
    assert b'bytes' in m._l.avae_last_error(m._h)        # the workspace refusal names its size
    call = lambda *a: m._l.avae_probe_decision(m._h, *a)
    for args in ((None, 8, 8, _ptr(w), 2, _ptr(out)), (_ptr(x), 8, 8, None, 2, _ptr(out)), (_ptr(x), 8, 8, _ptr(w), 2, None),
                 (_ptr(x), 0, 8, _ptr(w), 2, _ptr(out)), (_ptr(x), 8, 8, _ptr(w), 0, _ptr(out)), (_ptr(x), 8, 6, _ptr(w), 2, _ptr(out)),
                 (_ptr(x, 4), 4, 8, _ptr(w), 2, _ptr(out)), (_ptr(x), 8, 8, _ptr(w, 4), 2, _ptr(out))):
        assert call(*args) != 0, args
        assert len(m._l.avae_last_error(m._h)) > 5, args
    torch.cuda.synchronize(dev)
    for t in (w, st, out):
        assert (t == SENTINEL).all()                      # outputs untouched
    assert _raw_fit(**ok) == 0
    with pytest.raises(RuntimeError):
        m.set_option('probe_chunk', -1)
