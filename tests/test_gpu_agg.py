"""aggregate-posterior diagnostics on the device (avae_agg_logq, avae_latent_moments, VAE.posterior_stats) against the float64
reference of tests/agg_ref.py.

Shapes: agg_ref.CASES x the two regimes of agg_ref (peaked, broad), whose inputs tests/test_agg.py checks on the CPU.  The
kernel has ONE tile form -- query tiles of 128 rows, bank tiles of 64 rows, dim chunks of 32 -- and the cases hold the
remainders 1, tile - 1 and tile + 1 on both axes (n 1, 127, 129; N 1 / 129 / 257 / 321, 63 / 127 / 191, 65), dim 4 .. 1024.

TOL.  Not chosen: the error of an entry is |device - float64| / max(1, |float64|), and MAX_ERR is the largest value over logq
and logqx of every case and regime, measured on MI355X: 9.117e-06 (logqx, peaked, n 65, N 300, dim 128, where |float64| is small; the other peaked cases 1.0e-07 .. 8.1e-06,
every broad case at most 1.5e-07).  TOL = 4 x MAX_ERR (the device sums in another order than
the reference, and another plan in yet another);
test_tol_is_four_times_the_measured_error prints the figures again and fails if a run measures more than MAX_ERR.
MOM_MAX_ERR is the same for avae_latent_moments, with the error of an entry taken RELATIVE, |device - float64| / |float64| (an entry
whose reference is 0, the variance at N = 1, must be exactly 0): 5.960e-08 = 2^-24 (N 2; every case 3.3e-08 .. 6.0e-08); the sums run in double on the device, so
this is the rounding of the result to fp32."""
import ctypes as C

import numpy as np
import pytest

import agg_ref as ar

pytestmark = pytest.mark.gpu

MAX_ERR = 9.2e-6            # measured: 9.117e-06 (logqx, peaked, n 65, N 300, dim 128)
TOL = 4 * MAX_ERR
MOM_MAX_ERR = 6.0e-8        # measured: 5.960e-08 (N 2)
MOM_TOL = 4 * MOM_MAX_ERR
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
        _STATE['m'], _STATE['ids'] = m, ids
    return _STATE['m']


def _padded(x, extra=3):
    """the rows of x on the device with `extra` NaN rows behind them: a read beyond the array shows in the result"""
    import torch
    x = np.asarray(x, np.float32)
    t = torch.full((x.shape[0] + extra, x.shape[1]), float('nan'), dtype=torch.float32, device=_model().device)
    t[:x.shape[0]] = torch.as_tensor(np.array(x, order='C')).to(t.device)
    return t


def _raw(z, n, mu, lv, N, dim, self_base, logq, logqx, reserved=(0, 0), null_cfg=False):
    """the C entry as it stands -> its return code"""
    from argsim_amd import lib
    m = _model()
    ac = lib.AvaeAggConfig(self_base, (C.c_int32 * 2)(*reserved))
    m._stream()
    return m._l.avae_agg_logq(m._h, z, n, mu, lv, N, dim, None if null_cfg else C.byref(ac), logq, logqx)


def _logq(z, mu, lv, self_base=-1):
    """avae_agg_logq on NaN-padded inputs and sentinel-padded outputs -> logq, or (logq, logqx) where self_base >= 0: numpy"""
    import torch
    m = _model()
    n, dim, N = z.shape[0], z.shape[1], mu.shape[0]
    dz, dm, dl = _padded(z), _padded(mu), _padded(lv)
    logq = torch.full((n + 4,), SENTINEL, dtype=torch.float32, device=m.device)
    logqx = torch.full((n + 4,), SENTINEL, dtype=torch.float32, device=m.device) if self_base >= 0 else None
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    m._ck(_raw(ptr(dz), n, ptr(dm), ptr(dl), N, dim, self_base, ptr(logq), ptr(logqx)))
    out = [logq.cpu().numpy()] + ([logqx.cpu().numpy()] if logqx is not None else [])
    for a in out:
        assert (a[n:] == SENTINEL).all(), a[n:]
    out = [a[:n] for a in out]
    return out[0] if self_base < 0 else tuple(out)


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _run(case, regime):
    """the default-plan run of a case (cached and shared: never modified)"""
    if (case, regime) not in _RUNS:
        out = _logq(*ar.case_inputs(case, regime), self_base=0)
        for a in out:
            a.setflags(write=False)
        _RUNS[case, regime] = out
    return _RUNS[case, regime]


def _case_err(case, regime):
    dev, ref = _run(case, regime), ar.case_ref(case, regime)
    return ar.rel_err(dev[0], ref[0]), ar.rel_err(dev[1], ref[1])


def test_tol_is_four_times_the_measured_error():
    worst = {}
    for case in ar.CASES:
        for regime in ar.REGIMES:
            eq, ex = _case_err(case, regime)
            worst[case, regime] = max(eq, ex)
            print("max |device - float64| / max(1, |float64|)  %-6s %-16s logq %.3e  logqx %.3e" % (regime, case, eq, ex))
    top = max(worst.values())
    print("MAX over all cases: %.3e  (MAX_ERR %.3e, TOL %.3e)" % (top, MAX_ERR, TOL))
    assert top <= MAX_ERR


@pytest.mark.parametrize('regime', ar.REGIMES)
@pytest.mark.parametrize('case', ar.CASES, ids=lambda c: 'n%d-N%d-d%d' % c)
def test_accuracy(case, regime):
    eq, ex = _case_err(case, regime)
    print("logq %.3e logqx %.3e" % (eq, ex))
    assert eq <= TOL and ex <= TOL, (eq, ex, TOL)
    # without self_base: the same logq bits
    z, mu, lv = ar.case_inputs(case, regime)
    if case[1] <= 777:
        assert _same_bits([_logq(z, mu, lv)], [_run(case, regime)[0]])


def _spike(N, dim, j, chunk):
    """one bank row j holds the query with lv = -8, every other row is 40 away in every dimension"""
    rng = np.random.default_rng(100 + j)
    z = rng.standard_normal((1, dim)).astype(np.float32)
    mu = (z + 40.0 + rng.standard_normal((N, dim))).astype(np.float32)
    lv = np.zeros((N, dim), np.float32)
    mu[j], lv[j] = z[0], -8.0
    m = _model()
    try:
        m.set_option('agg_chunk', chunk)
        return float(_logq(z, mu, lv)[0]), float(ar.logq64(z, mu, lv)[0])
    finally:
        m.set_option('agg_chunk', 0)


# N = 200: bank tiles [0, 64) [64, 128) [128, 192) and the remainder tile [192, 200); agg_chunk 70: parts [0, 70) [70, 140) [140, 200),
# whose tiles start at 0, 64 / 70, 134 / 140
@pytest.mark.parametrize('j,chunk', [(0, 0), (199, 0), (63, 0), (64, 0), (191, 0), (192, 0), (0, 1 << 20), (63, 1 << 20), (192, 1 << 20), (199, 1 << 20),
                                     (69, 70), (70, 70), (139, 70), (140, 70), (133, 70), (134, 70), (199, 70)])
def test_no_row_is_lost(j, chunk):
    N, dim = 200, 8
    dev, ref = _spike(N, dim, j, chunk)
    want = 4.0 * dim - np.log(N) - 0.5 * dim * np.log(2 * np.pi)      # t(i, j) = -1/2 (0 + 8 x -8) = 32; a dropped row costs thousands of nats
    assert abs(ref - want) < 1e-6 and abs(dev - want) < 0.5, (j, chunk, dev, ref, want)


@pytest.mark.parametrize('regime', ar.REGIMES)
def test_parts_agree_and_repeat_with_the_same_bits(regime):
    case = (130, 4099, 128)
    z, mu, lv = ar.case_inputs(case, regime)
    ref = ar.case_ref(case, regime)
    m = _model()
    runs = {}
    try:
        for chunk in (1 << 20, 1000, 1366, 70):          # 1, 5, 4 and 59 parts
            m.set_option('agg_chunk', chunk)
            a, b = _logq(z, mu, lv, self_base=0), _logq(z, mu, lv, self_base=0)
            assert _same_bits(a, b), chunk
            runs[chunk] = a
    finally:
        m.set_option('agg_chunk', 0)
    assert _same_bits(_logq(z, mu, lv, self_base=0), _run(case, regime))
    one = runs[1 << 20]
    for chunk, a in runs.items():
        assert ar.rel_err(a[0], ref[0]) <= TOL and ar.rel_err(a[1], ref[1]) <= TOL, chunk
        assert ar.rel_err(a[0], one[0]) <= TOL, chunk
        assert _same_bits([a[1]], [one[1]]), chunk       # the own pair does not depend on the plan


def test_edges():
    case = (33, 777, 20)
    z, mu, lv = (x.copy() for x in ar.case_inputs(case, 'broad'))
    clean = _run(case, 'broad')
    # a bank row with lv = +inf weighs nothing
    lv2 = lv.copy()
    lv2[100] = np.inf
    got, ref = _logq(z, mu, lv2), ar.logq64(z, mu, lv2)
    assert ar.rel_err(got, ref) <= TOL
    others = np.arange(777) != 100
    assert np.abs(ref - (ar.logq64(z, mu[others], lv[others]) + np.log(776.0 / 777.0))).max() <= 1e-9
    # a query of +inf has every term -inf: -inf, not NaN; the other queries keep their bits
    z2 = z.copy()
    z2[5] = np.inf
    got = _logq(z2, mu, lv)
    assert np.isneginf(got[5]) and np.isneginf(ar.logq64(z2, mu, lv)[5])
    keep = np.arange(33) != 5
    assert _same_bits([got[keep]], [clean[0][keep]])
    # every bank row at lv = +inf: every query -inf
    assert np.isneginf(_logq(z, mu, np.full_like(lv, np.inf))).all()
    # a NaN in one bank row reaches every query
    mu3 = mu.copy()
    mu3[700, 3] = np.nan
    assert np.isnan(_logq(z, mu3, lv)).all()
    lv3 = lv.copy()
    lv3[0, 19] = np.nan
    assert np.isnan(_logq(z, mu, lv3)).all()
    # a NaN in one query row reaches that row alone: the others keep their bits
    z4 = z.copy()
    z4[7, 0] = np.nan
    q4, x4 = _logq(z4, mu, lv, self_base=0)
    keep = np.arange(33) != 7
    assert np.isnan(q4[7]) and np.isnan(x4[7])
    assert _same_bits([q4[keep], x4[keep]], [clean[0][keep], clean[1][keep]])


def test_errors_have_text():
    import torch
    m = _model()
    dev = m.device
    z, mu, lv = (torch.zeros((8, 8), dtype=torch.float32, device=dev) for _ in range(3))
    out, outx = torch.zeros(8, dtype=torch.float32, device=dev), torch.zeros(8, dtype=torch.float32, device=dev)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    ok = dict(z=p(z), n=4, mu=p(mu), lv=p(lv), N=8, dim=8, self_base=-1, logq=p(out), logqx=None)
    assert _raw(**ok) == 0
    assert _raw(**dict(ok, self_base=4, logqx=p(outx))) == 0
    bad = [dict(z=None), dict(mu=None), dict(lv=None), dict(logq=None), dict(null_cfg=True), dict(n=0), dict(N=0), dict(N=(1 << 31) - 255),
           dict(dim=6), dict(dim=0), dict(dim=1028), dict(z=p(z, 4)), dict(mu=p(mu, 8)), dict(lv=p(lv, 4)), dict(self_base=-2),
           dict(self_base=5), dict(logqx=p(outx)), dict(reserved=(1, 0)), dict(reserved=(0, 1))]
    for kw in bad:
        assert _raw(**dict(ok, **kw)) != 0, kw
        assert len(m._l.avae_last_error(m._h)) > 5, kw
    mom = torch.zeros((4, 8), dtype=torch.float32, device=dev)
    call = lambda a, b, N, dim, o: m._l.avae_latent_moments(m._h, a, b, N, dim, o)
    assert call(p(mu), p(lv), 8, 8, p(mom)) == 0
    for args in ((None, p(lv), 8, 8, p(mom)), (p(mu), None, 8, 8, p(mom)), (p(mu), p(lv), 8, 8, None), (p(mu), p(lv), 0, 8, p(mom)),
                 (p(mu), p(lv), 8, 6, p(mom)), (p(mu), p(lv), 8, 1028, p(mom)), (p(mu, 4), p(lv), 4, 8, p(mom))):
        assert call(*args) != 0, args
        assert len(m._l.avae_last_error(m._h)) > 5, args
    torch.cuda.synchronize(dev)
    with pytest.raises(RuntimeError):
        m.set_option('agg_chunk', -1)


def _moments(N, dim):
    import torch
    m = _model()
    mu, lv = ar.moment_inputs(N, dim)
    dm, dl = _padded(mu), _padded(lv)
    out = torch.full((4 * dim + 4,), SENTINEL, dtype=torch.float32, device=m.device)
    m._stream()
    m._ck(m._l.avae_latent_moments(m._h, C.c_void_p(dm.data_ptr()), C.c_void_p(dl.data_ptr()), N, dim, C.c_void_p(out.data_ptr())))
    out = out.cpu().numpy()
    assert (out[4 * dim:] == SENTINEL).all()
    dev, ref = out[:4 * dim].reshape(4, dim).astype(np.float64), ar.moments64(mu, lv)
    assert np.isfinite(dev).all() and np.array_equal(dev[ref == 0], ref[ref == 0])
    nz = ref != 0
    return float((np.abs(dev[nz] - ref[nz]) / np.abs(ref[nz])).max()), dev, ref


def test_moments_tol_is_four_times_the_measured_error():
    worst = 0.0
    for N in ar.MOMENT_N:
        for dim in ar.MOMENT_DIM:
            err = _moments(N, dim)[0]
            print("max |device - float64| / |float64|  N %4d dim %4d  %.3e" % (N, dim, err))
            worst = max(worst, err)
    print("MAX over all cases: %.3e  (MOM_MAX_ERR %.3e, MOM_TOL %.3e)" % (worst, MOM_MAX_ERR, MOM_TOL))
    assert worst <= MOM_MAX_ERR


@pytest.mark.parametrize('dim', ar.MOMENT_DIM)
@pytest.mark.parametrize('N', ar.MOMENT_N)
def test_moments(N, dim):
    err, dev, ref = _moments(N, dim)
    assert err <= MOM_TOL, (err, MOM_TOL)
    if N == 1:
        assert (dev[1] == 0).all()
    else:
        assert int((dev[1] > ar.AU_THRESHOLD).sum()) == dim // 2
    # VAE.latent_moments returns the same numbers, and the same bits twice
    m = _model()
    mu, lv = ar.moment_inputs(N, dim)
    a, b = m.latent_moments(mu, lv), m.latent_moments(mu, lv)
    assert sorted(a) == ['kl_dim', 'mean', 'sigma2', 'var']
    for i, k in enumerate(('mean', 'var', 'sigma2', 'kl_dim')):
        assert np.array_equal(a[k].astype(np.float64), dev[i]) and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_log_q_method_matches_the_entry():
    import torch
    from argsim_amd.model import log_q
    m = _model()
    case = (33, 777, 20)
    z, mu, lv = ar.case_inputs(case, 'peaked')
    assert _same_bits(m.log_q(z, mu, lv, self_index=0), _run(case, 'peaked'))
    assert _same_bits([log_q(m, z, mu, lv)], [_run(case, 'peaked')[0]])
    dq = m.log_q(*(torch.as_tensor(np.array(x)).to(m.device) for x in (z, mu, lv)))
    assert dq.is_cuda and _same_bits([dq.cpu().numpy()], [_run(case, 'peaked')[0]])
    # queries that are samples of rows 100 .. 132
    z2 = (mu[100:133] + np.exp(0.5 * lv[100:133]) * np.random.default_rng(1).standard_normal((33, 20))).astype(np.float32)
    q, x = m.log_q(z2, mu, lv, self_index=100)
    rq, rx = ar.logq64(z2, mu, lv, self_base=100)
    assert ar.rel_err(q, rq) <= TOL and ar.rel_err(x, rx) <= TOL


def test_posterior_stats():
    m = _model()
    ids = _STATE['ids']
    N, R, S = ids.shape[0], 8, 3
    eps = np.random.default_rng(9).standard_normal((S, N, R)).astype(np.float32)
    got = m.posterior_stats(ids, samples=S, eps=eps, return_parts=True)
    mu, lv = m.encode(ids, return_lv=True)
    assert np.array_equal(got['mu'], mu) and np.array_equal(got['lv'], lv)
    ref = ar.posterior_stats64(mu, lv, eps)
    # z is formed in fp32 on the device (half an ulp of |z|, 6e-8 relative, against sigma: far below TOL for this model's sigma of
    # about 1); the per-sample values then carry the error of the entry, a mean of differences of two of them twice that
    assert np.abs(got['z'] - ref['z']).max() <= 1e-6 * max(1.0, np.abs(ref['z']).max())
    for k in ('logq', 'logqx', 'logp'):
        assert ar.rel_err(got[k], ref[k]) <= TOL, k
    scale = max(1.0, np.abs(ref['logq']).max(), np.abs(ref['logqx']).max(), np.abs(ref['logp']).max())
    assert abs(got['mi'] - ref['mi']) <= 2 * TOL * scale and abs(got['kl_marginal'] - ref['kl_marginal']) <= 2 * TOL * scale
    assert got['mi'] <= np.log(N) + TOL and got['n'] == N
    assert got['kl'] == float(got['kl_dim'].astype(np.float64).sum()) and abs(got['kl'] - ref['kl']) <= MOM_TOL * abs(ref['kl'])
    nz = ref['var_mu'] != 0
    assert (np.abs(got['var_mu'][nz] - ref['var_mu'][nz]) <= MOM_TOL * np.abs(ref['var_mu'][nz])).all()
    assert (np.abs(got['kl_dim'] - ref['kl_dim']) <= MOM_TOL * np.abs(ref['kl_dim'])).all()
    assert got['au'] == int((got['var_mu'] > 0.01).sum()) and 0 <= got['au'] <= R
    if not ((ref['var_mu'] > 0.005) & (ref['var_mu'] < 0.02)).any():
        assert got['au'] == ref['au']
    # a batch smaller than N gives the same numbers within the tolerance; the same seed the same result twice, another seed another
    small = m.posterior_stats(ids, samples=S, eps=eps, batch=3, return_parts=True)
    for k in ('logq', 'logqx'):          # (the encoder may take another kernel form at another batch size: not the same bits)
        assert ar.rel_err(small[k], ref[k]) <= TOL, k
    from argsim_amd.model import posterior_stats
    a, b, c = m.posterior_stats(ids, samples=2, seed=5), posterior_stats(m, ids, 2, 5), m.posterior_stats(ids, samples=2, seed=6)
    assert sorted(a) == ['au', 'kl', 'kl_dim', 'kl_marginal', 'mi', 'n', 'var_mu']
    assert a['mi'] == b['mi'] and a['kl_marginal'] == b['kl_marginal'] and a['kl'] == b['kl'] and a['mi'] != c['mi']
