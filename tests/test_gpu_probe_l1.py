"""L1 probes on the device (avae_probe_fit_l1, VAE.probe_fit_l1, VAE.select_dims, eval_cluster --select) against the float64 reference
of tests/probe_l1_ref.py.

No tolerance here is measured.  The objective is not strongly convex, so there is no bound on |w - w*|; what a returned w carries is
its optimality measure |v(w)|_1, which the test evaluates in float64 and holds to 2 tol |v(0)|_1 (the factor 2 of
tests/test_gpu_probe.py: the device's own measure must be within tol |v(0)|_1 of the real one), the objective to the summation bound
of N + dim fp32 terms.  The support is compared on the coordinates that the reference optimum decides with a margin
(probe_l1_ref.GAP_G, GAP_W; tests/test_probe_l1.py holds the cases to at most 5 % undecided ones on the CPU).  Shapes:
probe_l1_ref.GPU_CASES.  Operands are padded with NaN rows and outputs guarded by a sentinel."""
import ctypes as C

import numpy as np
import pytest

import probe_l1_ref as pl
import probe_ref as pr
from test_gpu_probe import SENTINEL, _fit as _fit_l2, _model, _padded, _ptr, _same_bits

pytestmark = pytest.mark.gpu

TOL, MAX_NEWTON, MAX_INNER = 1e-4, 50, 50
_RUNS = {}


def _raw_fit(x, N, dim, s, P, w, stats, tol=TOL, max_newton=MAX_NEWTON, max_inner=MAX_INNER, reserved=0, null_cfg=False):
    """the C entry as it stands -> its return code"""
    from argsim_amd import lib
    m = _model()
    pc = lib.AvaeProbeL1Config(max_newton, max_inner, tol, reserved)
    m._stream()
    return m._l.avae_probe_fit_l1(m._h, x, N, dim, s, P, None if null_cfg else C.byref(pc), w, stats)


def _fit(x, s, tol=TOL, max_newton=MAX_NEWTON, max_inner=MAX_INNER):
    """avae_probe_fit_l1 on NaN-padded inputs and sentinel-guarded outputs -> (w (P, dim + 1), stats (P, 4)) numpy"""
    import torch
    m = _model()
    (N, dim), P = x.shape, s.shape[0]
    dx, ds = _padded(x), _padded(s)
    w = torch.full((P * (dim + 1) + 4,), SENTINEL, dtype=torch.float32, device=m.device)
    st = torch.full((P * 4 + 4,), SENTINEL, dtype=torch.float32, device=m.device)
    m._ck(_raw_fit(_ptr(dx), N, dim, _ptr(ds), P, _ptr(w), _ptr(st), tol, max_newton, max_inner))
    w, st = w.cpu().numpy(), st.cpu().numpy()
    assert (w[P * (dim + 1):] == SENTINEL).all() and (st[P * 4:] == SENTINEL).all()
    return w[:P * (dim + 1)].reshape(P, dim + 1), st[:P * 4].reshape(P, 4)


def _run(case):
    """the default-plan fit of a case (cached and shared: never modified)"""
    if case not in _RUNS:
        out = _fit(*pl.case_inputs(case))
        for a in out:
            a.setflags(write=False)
        _RUNS[case] = out
    return _RUNS[case]


def _zeros_are_plus_zero(w):
    return (np.ascontiguousarray(w).view(np.uint32)[w == 0] == 0).all()


def _check_certificate(x, s, w, st, tol=TOL):
    N, dim = x.shape
    v0 = pl.v0_64(x, s)
    worst = 0.0
    assert np.isfinite(w).all() and np.isfinite(st).all()
    assert _zeros_are_plus_zero(w)
    for p in range(s.shape[0]):
        v = float(np.abs(pl.v64(x, s[p], w[p])).sum())
        f = pl.objective64(x, s[p], w[p])
        if v0[p] > 0:
            worst = max(worst, v / (tol * v0[p]))
        print("problem %d: |v|_1 %.3e (device %.3e), tol |v(0)|_1 %.3e, F %.9g (device %.9g), iterations %d, status %d"
              % (p, v, st[p, 1], tol * v0[p], f, st[p, 0], st[p, 2], st[p, 3]))
        assert st[p, 3] == 0, (p, st[p])                                       # converged
        assert v <= 2 * tol * v0[p], (p, v, tol * v0[p], st[p])                # the stop rule is truthful
        assert abs(st[p, 1] - v) <= tol * v0[p] + 1e-6 * v, (p, st[p, 1], v)   # the device's own measure: within the other factor
        assert abs(st[p, 0] - f) <= 2 * (N + dim) * 2.0 ** -24 * abs(f), (p, st[p, 0], f)
        assert 0 <= st[p, 2] <= MAX_NEWTON and st[p, 2] == int(st[p, 2])
    print("worst |v|_1 / (tol |v(0)|_1) = %.3f, most outer iterations %d" % (worst, int(st[:, 2].max())))


@pytest.mark.parametrize('case', pl.GPU_CASES, ids=pl.CASE_ID)
def test_certificate(case):
    x, s = pl.case_inputs(case)
    w, st = _run(case)
    _check_certificate(x, s, w, st)


@pytest.mark.parametrize('case', pl.GPU_CASES, ids=pl.CASE_ID)
def test_support(case):
    w, _ = _run(case)
    ref, dec = pl.case_ref(case), pl.case_decided(case)
    assert ((~dec).mean(axis=1) <= pl.CAP).all()
    got, want = w != 0, ref != 0
    assert (got[dec] == want[dec]).all(), np.argwhere(dec & (got != want))
    assert want.any(axis=1).all()                       # no case is the empty model


def test_the_selection(tmp_path, capsys):
    from argsim_amd import eval_cluster, model
    case = pl.GPU_CASES[1]
    x, cls = pl.case_labels(case)
    assert pl.case_decided(case).all()                  # every coordinate decided: the selection must be the reference's exactly
    want = pl.useful_dims(pl.case_ref(case)[:, :-1])
    assert set(range(6)) <= set(want.tolist())          # the planted columns, two per class
    m = _model()
    dims, probe = m.select_dims(x, cls)
    assert dims.dtype == np.int64 and dims.tolist() == want.tolist()
    assert list(probe.classes_) == [0, 1, 2] and (probe.stats[:, 3] == 0).all()
    assert _same_bits([probe.coef_, probe.intercept_], [_run(case)[0][:, :-1], _run(case)[0][:, -1]])
    dims2, _ = model.select_dims(m, x, cls)
    assert dims2.tolist() == dims.tolist()
    assert (probe.predict(x) == cls).mean() > 0.8
    # the command line: the same columns written as int64, then the score lines of a clustering on those columns
    labels = np.array(['t-s%d-r%d' % (c, c) for c in cls])
    np.save(str(tmp_path / 'z.npy'), x)
    np.save(str(tmp_path / 'l.npy'), labels)
    args = ['--inputs', str(tmp_path / 'z.npy'), '--labels', str(tmp_path / 'l.npy'), '--by', 'topic']
    eval_cluster.main(args + ['--select', 'stance', '--save-dims', str(tmp_path / 'd.npy')])
    lines = capsys.readouterr().out.strip().split('\n')
    saved = np.load(str(tmp_path / 'd.npy'))
    assert saved.dtype == np.int64 and saved.tolist() == want.tolist()
    _, ref_lines = eval_cluster.evaluate(m, np.ascontiguousarray(x[:, want]), labels, 'topic')
    assert lines == ['useful dimensions: %d of %d' % (len(want), x.shape[1])] + ref_lines
    eval_cluster.main(args + ['--dims', str(tmp_path / 'd.npy')])
    assert capsys.readouterr().out.strip().split('\n') == ref_lines


@pytest.mark.parametrize('case', pl.GPU_CASES, ids=pl.CASE_ID)
def test_a_problem_does_not_depend_on_its_companions(case):
    x, s = pl.case_inputs(case)
    w, st = _run(case)
    P = s.shape[0]
    assert _same_bits(_fit(x, s), (w, st))
    perm = np.random.default_rng(5).permutation(P)
    w2, st2 = _fit(x, np.ascontiguousarray(s[perm]))
    assert _same_bits((w2, st2), (w[perm], st[perm]))
    for p in range(P):
        w1, st1 = _fit(x, np.ascontiguousarray(s[p:p + 1]))
        assert _same_bits((w1, st1), (w[p:p + 1], st[p:p + 1])), p


@pytest.mark.parametrize('case', pl.GPU_CASES, ids=pl.CASE_ID)
def test_parts_meet_the_certificate(case):
    x, s = pl.case_inputs(case)
    m = _model()
    P = s.shape[0]
    perm = np.random.default_rng(6).permutation(P)
    try:
        m.set_option('probe_chunk', 50)           # 3 (N 127, 129), 4 (N 200) and 6 (N 257) parts, none a multiple of the tile
        w, st = _fit(x, s)
        assert _same_bits(_fit(x, np.ascontiguousarray(s[perm])), (w[perm], st[perm]))
        assert _same_bits(_fit(x, np.ascontiguousarray(s[P - 1:])), (w[P - 1:], st[P - 1:]))
    finally:
        m.set_option('probe_chunk', 0)
    _check_certificate(x, s, w, st)
    assert _same_bits(_fit(x, s), _run(case))


def test_edge_cases():
    case = pl.SK_CASES[0]
    x, cls = pl.case_labels(case)
    from argsim_amd import probe
    # costs so small that w = 0 is optimal
    _, tiny = probe.l1_costs(cls, C=1e-3)
    assert (pl.v0_64(x, tiny) == 0).all()
    w, st = _fit(x, tiny)
    assert (np.ascontiguousarray(w).view(np.uint32) == 0).all() and (st[:, 3] == 0).all() and (st[:, 2] == 0).all() and (st[:, 1] == 0).all()
    # a problem whose costs are all 0, and one whose training rows all have one sign (the bias alone fits it)
    _, s = pl.case_inputs(case)
    s2 = np.array(s)
    s2[1] = 0.0
    s2[2] = 0.1
    w, st = _fit(x, s2)
    _check_certificate(x, s2, w, st)
    assert not w[1].any() and st[1, 2] == 0 and st[1, 0] == 0
    assert w[2, -1] > 0
    assert _same_bits((w[:1], st[:1]), _fit(x, s[:1]))
    # max_newton reached: status 1 after exactly that many iterations, a finite w
    w, st = _fit(x, s, tol=1e-6, max_newton=1)
    assert (st[:, 3] == 1).all() and (st[:, 2] == 1).all() and np.isfinite(w).all() and w.any(axis=1).all()
    # one Hessian product per iteration: slower, never a failure
    w, st = _fit(x, s, max_inner=1)
    assert np.isin(st[:, 3], (0, 1)).all() and np.isfinite(w).all() and _zeros_are_plus_zero(w)


def test_values_that_are_not_finite_end_their_problem_alone():
    case = pl.GPU_CASES[1]
    x, s = pl.case_inputs(case)
    s2 = np.array(s)
    s2[1, 9] = 0.0                                   # problem 1 leaves row 9 out
    w, st = _fit(x, s2)
    assert (st[:, 3] == 0).all()
    x2 = np.array(x)
    x2[9, 1] = np.nan
    w2, st2 = _fit(x2, s2)
    assert st2[0, 3] == 2 and st2[2, 3] == 2
    assert _same_bits((w2[1:2], st2[1:2]), (w[1:2], st[1:2]))
    # a cost that is not finite ends its own problem
    s3 = np.array(s)
    s3[0, 17] = np.nan
    s3[2, 3] = np.inf
    w3, st3 = _fit(x, s3)
    assert st3[0, 3] == 2 and st3[2, 3] == 2
    assert _same_bits((w3[1:2], st3[1:2]), (_run(case)[0][1:2], _run(case)[1][1:2]))


def test_the_l2_fit_keeps_its_bits_after_an_l1_fit():
    case = pr.CASES[1]
    x, s = pr.case_inputs(case)
    before = _fit_l2(x, s)
    _fit(*pl.case_inputs(pl.GPU_CASES[2]))
    assert _same_bits(_fit_l2(x, s), before)


def test_errors_have_text():
    import torch
    m = _model()
    dev = m.device
    x = torch.ones((8, 8), dtype=torch.float32, device=dev)
    s = torch.ones((2, 8), dtype=torch.float32, device=dev)
    w = torch.full((2, 12), SENTINEL, dtype=torch.float32, device=dev)
    st = torch.full((2, 4), SENTINEL, dtype=torch.float32, device=dev)
    ok = dict(x=_ptr(x), N=8, dim=8, s=_ptr(s), P=2, w=_ptr(w), stats=_ptr(st))
    bad = [dict(x=None), dict(s=None), dict(w=None), dict(null_cfg=True), dict(N=0), dict(P=0), dict(N=(1 << 31) - 255), dict(P=(1 << 20) + 1), dict(max_newton=0),
           dict(max_inner=0), dict(tol=-1.0), dict(tol=float('nan')), dict(reserved=1), dict(dim=6), dict(dim=0), dict(dim=1028),
           dict(x=_ptr(x, 4)), dict(w=_ptr(w, 4)), dict(N=1 << 30, dim=1024, P=1 << 20)]
    for kw in bad:
        assert _raw_fit(**dict(ok, **kw)) != 0, kw
        assert len(m._l.avae_last_error(m._h)) > 5, kw
    assert b'bytes' in m._l.avae_last_error(m._h)        # the workspace refusal names its size
    torch.cuda.synchronize(dev)
    for t in (w, st):
        assert (t == SENTINEL).all()                      # outputs untouched
    assert _raw_fit(**ok) == 0
