"""Exact t-SNE on the device (avae_tsne, VAE.tsne) against the float64 restatement of tests/tsne_ref.py.

A fit is chaotic, so no test compares a fitted embedding or its KL with a reference fit by tolerance.  beta and one iteration are
compared in BITS wherever tsne_ref's derived margins allow it (tests/test_tsne.py asserts on the CPU that the chosen inputs leave no
row and no gradient entry without its margin); P is compared with the float64 P of the device's own beta; a chain and the stop rule
are checked link by link against the device's own previous state and trace; a run carries a certificate on its own outputs; the quality
case asserts a property that held in every plain and perturbed reference run.  Outputs are guarded by sentinels."""
import ctypes as C
import importlib.util

import numpy as np
import pytest

import tsne_ref as tr

pytestmark = pytest.mark.gpu

KEYS = ('dim_tgt', 'dim_emb', 'dim_rep', 'rnn_layers', 'accelerate', 'learn_rate', 'bos', 'eos')
SENT = 123.0
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


def _cfg(perplexity=30.0, ee=12.0, min_grad_norm=1e-7, lr=0.0, max_iter=0, it0=0, exag_iter=250, nic=50, nwp=300, init=0, warm=0, seed=0,
         reserved=(0, 0)):
    from argsim_amd import lib
    return lib.AvaeTsneConfig(perplexity=perplexity, early_exaggeration=ee, min_grad_norm=min_grad_norm, learning_rate=lr, max_iter=max_iter,
                              it0=it0, exaggeration_iter=exag_iter, n_iter_check=nic, n_iter_without_progress=nwp, init=init, warm=warm,
                              seed=seed, reserved=(C.c_int32 * 2)(*reserved))


def _ts(x=None, p_in=None, y=None, ug=None, prog=None, state=True, want_p=False, chunk=0, raw_status=False, **kw):
    """avae_tsne on NaN-padded rows and sentinel-guarded outputs -> dict of numpy arrays"""
    import torch
    m = _model()
    dev = m.device
    cfg = _cfg(**kw)
    N = x.shape[0] if x is not None else p_in.shape[0]
    dim = x.shape[1] if x is not None else 0
    dx = dp = None
    if x is not None:
        dx = torch.full((N + 3, dim), float('nan'), dtype=torch.float32, device=dev)
        dx[:N] = torch.as_tensor(np.ascontiguousarray(x, np.float32)).to(dev)
    if p_in is not None:
        dp = torch.as_tensor(np.ascontiguousarray(p_in, np.float64)).to(dev)
    T = max(cfg.max_iter, 1)

    def guarded(n, dt, init=None):
        t = torch.full((n + 8,), SENT, dtype=dt, device=dev)
        if init is not None:
            t[:n] = torch.as_tensor(np.ascontiguousarray(init).ravel()).to(dev).to(dt)
        return t
    bufs = dict(y=guarded(2 * N, torch.float32, y), kl=guarded(2, torch.float64), stat=guarded(4, torch.int32), trace=guarded(2 * T, torch.float64),
                grad=guarded(2 * N, torch.float32))
    if want_p:
        bufs['p'] = guarded(N * N, torch.float64)
    if x is not None:
        bufs['beta'] = guarded(N, torch.float64)
    if state or ug is not None:
        bufs['ug'] = guarded(4 * N, torch.float32, ug)
        bufs['prog'] = guarded(4, torch.float64, prog)
    m._ck(m._l.avae_set_option(m._h, b'tsne_chunk', chunk))
    m._stream()
    rc = m._l.avae_tsne(m._h, _ptr(dx), N, dim, C.byref(cfg), _ptr(dp), _ptr(bufs['y']), _ptr(bufs['kl']), _ptr(bufs['stat']), _ptr(bufs.get('p')),
                        _ptr(bufs.get('beta')), _ptr(bufs['trace']), _ptr(bufs['grad']), _ptr(bufs.get('ug')), _ptr(bufs.get('prog')))
    m._l.avae_set_option(m._h, b'tsne_chunk', 0)
    if raw_status:
        return rc
    m._ck(rc)
    sizes = dict(y=2 * N, kl=2, stat=4, trace=2 * cfg.max_iter, grad=2 * N, p=N * N, beta=N, ug=4 * N, prog=4)
    shapes = dict(y=(N, 2), trace=(2, cfg.max_iter), grad=(N, 2), p=(N, N), ug=(2, N, 2))
    out = {}
    for name, t in bufs.items():
        v = t.cpu().numpy()
        n = sizes[name]
        guard = v[max(n, 2 * T if name == 'trace' else n):]
        assert (guard == SENT).all(), name
        out[name] = v[:n].reshape(shapes.get(name, (n,)))
    return out


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view({4: np.uint32, 8: np.uint64}[v.dtype.itemsize])


def _same(p, q):
    return np.array_equal(_bits(p), _bits(q))


def _device_distances(x):
    """the distances as the device forms them: the negated similarities of avae_affinity's metric 0 (the same kernel)"""
    import torch
    from argsim_amd import lib
    m = _model()
    N, dim = x.shape
    dx = torch.as_tensor(np.ascontiguousarray(x, np.float32)).to(m.device)
    label = torch.zeros((N,), dtype=torch.int32, device=m.device)
    stat = torch.zeros((4,), dtype=torch.int32, device=m.device)
    s = torch.zeros((N, N), dtype=torch.float32, device=m.device)
    cfg = lib.AvaeAffinityConfig(metric=0, max_iter=1, convergence_iter=1, use_preference=1, noise=0, warm=0, damping=0.5, preference=0.0, seed=0)
    m._stream()
    m._ck(m._l.avae_affinity(m._h, _ptr(dx), N, dim, C.byref(cfg), _ptr(label), _ptr(stat), _ptr(s), None, None))
    D = -s.cpu().numpy().astype(np.float64)
    np.fill_diagonal(D, 0.0)
    return D


def _joint_of(case):
    """the reference's P of a case, computed once"""
    key = ('P',) + tuple(case)
    if key not in _STATE:
        N, dim, _, perp = case
        x, _ = tr.clusters(N, dim, 100 + N)
        _STATE[key] = tr.joint(tr.conditionals(tr.distances(x), perp)['C'])
    return _STATE[key]


@pytest.mark.parametrize('case', tr.CASES)
def test_beta_and_joint(case):
    N, dim, chunk, perp = case
    x, _ = tr.clusters(N, dim, 100 + N)
    D = _device_distances(x)
    ref_d = tr.distances(x)
    assert (np.abs(D - ref_d) <= np.spacing(ref_d.astype(np.float32)).astype(np.float64)).all()
    ref = tr.conditionals(D, perp)
    out = _ts(x, perplexity=perp, max_iter=0, want_p=True, chunk=chunk)
    sure = ref['margin'] > ref['eval_err']
    print("N %d: %d rows without margin, smallest margin %.3g, largest eval_err %.3g" % (N, (~sure).sum(), ref['margin'].min(), ref['eval_err'].max()))
    assert (~sure).sum() <= 0.02 * N
    assert _same(out['beta'][sure], ref['beta'][sure])
    Cd, h = tr.conditionals_at(D, out['beta'])
    assert ((np.abs(h - np.log(perp)) <= tr.TOL + 1e-9) | (ref['steps'] == 100)).all()
    P, want = out['p'], tr.joint(Cd)
    off = ~np.eye(N, dtype=bool)
    assert (np.abs(P - want)[off] <= 1e-12 * want[off]).all()
    assert _same(P, P.T.copy()) and (np.diag(P) == 0).all() and (P[off] >= tr.EPS).all()
    # the entries sum to 1 before the floor; the floor adds at most eps per entry it raises (most entries at dim 1024)
    assert -1e-12 <= P.sum() - 1.0 <= (P[off] == tr.EPS).sum() * tr.EPS + 1e-12
    assert out['stat'].tolist() == [-1, 0, -1, 0] and np.isnan(out['kl']).all()


def _check_step(P, y0, ug0, out, phase, lr, ee, what):
    """one iteration from (y0, ug0): grad against the reference in bits where it has its margin, else within one ulp; the state
    against the fp32 arithmetic applied to the device's own grad, in bits -> whether every entry had its margin"""
    ps = tr.pair_sums(ee * P if phase == 1 else P, y0)
    want = ps['g64'].astype(np.float32)
    sure = tr.round_margin(ps['g64']) > ps['bound']
    g = out['grad']
    assert np.array_equal(_bits(g)[sure], _bits(want)[sure]), what
    assert (np.abs(g.astype(np.float64) - want) <= np.spacing(np.abs(want))).all(), what
    assert (~sure).sum() <= 0.01 * sure.size, what
    y, upd, gains, gp = tr.update(y0, ug0[0], ug0[1], g, 0.5 if phase == 1 else 0.8, lr)
    return ps, (y, upd, gains, gp), bool(sure.all())


@pytest.mark.parametrize('phase', [1, 2])
@pytest.mark.parametrize('case', tr.CASES + [tr.STEP_ONLY])
def test_one_step(case, phase):
    N, dim, chunk, perp = case
    P = _joint_of(case)
    r = np.random.default_rng(7 * N + phase)
    y0 = tr.start(N, N + phase, 1e-4 if phase == 1 else 1.0)
    ug0 = np.stack([(1e-3 * r.standard_normal((N, 2))), r.uniform(0.2, 2.0, (N, 2))]).astype(np.float32)
    lr, ee = tr.auto_lr(N, 12.0), 12.0
    out = _ts(p_in=P, y=y0, ug=ug0, prog=[0.5, 3.0, float(phase), 0.0], warm=1, it0=7, max_iter=8, nic=4, exag_iter=1000 if phase == 1 else 0,
              chunk=chunk, lr=lr, ee=ee)
    ps, (y, upd, gains, gp), _ = _check_step(P, y0, ug0, out, phase, lr, ee, case)
    assert _same(out['y'], y) and _same(out['ug'][0], upd) and _same(out['ug'][1], gains)
    err = tr.error(ee * P if phase == 1 else P, ps['q'], ps['Z'])
    gn = float(np.sqrt((gp.astype(np.float64) ** 2).sum()))
    assert abs(out['trace'][0, 7] - err) <= 1e-10 * abs(err) and abs(out['trace'][1, 7] - gn) <= 1e-12 * gn
    assert np.isnan(out['trace'][:, :7]).all() or (out['trace'][:, :7] == SENT).all()      # a warm call leaves the earlier entries alone
    assert out['stat'].tolist() == [7, 0, 7 if phase == 1 else -1, 0]
    assert _bits(out['kl'])[0] == _bits(out['trace'])[0, 7]


def test_chain_of_warm_calls():
    """60 one-iteration warm calls against one 60-iteration call, every link a step from the device's previous state"""
    case = tr.CASES[4]
    N, chunk = case[0], case[2]
    P = _joint_of(case)
    kw = dict(exag_iter=20, nic=5, lr=tr.auto_lr(N, 12.0), ee=12.0)
    y0 = tr.start(N, 5)
    whole = _ts(p_in=P, y=y0, max_iter=60, chunk=chunk, **kw)
    plain = _ts(p_in=P, y=y0, max_iter=60, chunk=0, **kw)
    y, ug, prog, margins = y0, None, None, True
    for i in range(60):
        prev = (y, np.stack([np.zeros((N, 2), np.float32), np.ones((N, 2), np.float32)]) if ug is None else ug)
        out = _ts(p_in=P, y=y, ug=ug, prog=prog, warm=0 if i == 0 else 1, it0=i, max_iter=i + 1, chunk=chunk, **kw)
        phase = 1 if i < 20 else 2
        _, (wy, wu, wg, _), ok = _check_step(P, prev[0], prev[1], out, phase, kw['lr'], 12.0, i)
        margins = margins and ok
        if i == 19:                                           # phase 1's last iteration: the fresh state of phase 2
            wu, wg = np.zeros_like(wu), np.ones_like(wg)
        assert _same(out['y'], wy) and _same(out['ug'][0], wu) and _same(out['ug'][1], wg), i
        assert out['prog'][2] == (1 if i < 19 else 2)
        if (i + 1) % 5 == 0:
            assert _bits(out['trace'])[0, i] == _bits(whole['trace'])[0, i] and _bits(out['trace'])[1, i] == _bits(whole['trace'])[1, i]
        y, ug, prog = out['y'], out['ug'], out['prog']
    assert _same(y, whole['y']) and _same(ug, whole['ug']) and _same(prog, whole['prog'])
    assert whole['stat'].tolist() == plain['stat'].tolist() == [59, 0, 19, 0]
    print("every link had its margin: %s" % margins)
    if margins:                                               # no entry of any link was free to round either way: another part size, the same run
        assert _same(plain['y'], whole['y'])


STOPS = [dict(max_iter=40, exag_iter=10, nic=5, min_grad_norm=1e30),
         dict(max_iter=60, exag_iter=10, nic=5, nwp=0, lr=1e-30),
         dict(max_iter=40, exag_iter=10, nic=5),
         dict(max_iter=30, exag_iter=30, nic=7),
         dict(max_iter=23, exag_iter=50, nic=7)]


@pytest.mark.parametrize('k', range(len(STOPS)))
def test_stop_rule(k):
    """stat and kl against the stop rule replayed over the device's own trace, for every ending"""
    kw = STOPS[k]
    P = _joint_of(tr.CASES[1])
    out = _ts(p_in=P, y=tr.start(37, 3), **kw)
    last, how, p1_last, kl0, kl1 = tr.replay_stop(out['trace'], kw['max_iter'], kw['exag_iter'], kw['nic'], kw.get('nwp', 300), kw.get('min_grad_norm', 1e-7))
    assert out['stat'].tolist() == [last, how, p1_last, 0]
    assert _same(out['kl'], np.array([kl0, kl1]))
    want = [(9, 2, 4), (19, 1, 9), (39, 0, 9), (29, 0, 29), (22, 0, 22)][k]
    assert (last, how, p1_last) == want
    if k >= 3:
        assert _bits(out['kl'])[0] == _bits(out['kl'])[1]      # an empty phase 2
    ran = ~np.isnan(out['trace'][0])
    assert not ran[last + 1:].any()                              # nothing after the stop


def test_certificate():
    """the last error of a run to m is the float64 error of the y a run to m - 1 returns"""
    P = _joint_of(tr.CASES[4])
    kw = dict(p_in=P, y=tr.start(96, 11), exag_iter=10, nic=50)
    a, b = _ts(max_iter=29, **kw), _ts(max_iter=30, **kw)
    ps = tr.pair_sums(P, a['y'])
    err = tr.error(P, ps['q'], ps['Z'])
    assert abs(b['trace'][0, 29] - err) <= 1e-10 * abs(err)
    assert _bits(b['kl'])[0] == _bits(b['trace'])[0, 29]


def test_quality_four_clusters():
    x, lab = tr.clusters(96 * 16, 16, 4)
    out = _ts(x, perplexity=10.0, max_iter=120, exag_iter=60, nic=10, init=1, seed=3)
    assert tr.purity_1nn(out['y'], lab) == 1.0
    first2 = out['trace'][0, 60:][~np.isnan(out['trace'][0, 60:])][0]
    print("kl %.6f, first phase-2 error %.6f" % (out['kl'][0], first2))
    assert out['kl'][0] < first2 and out['stat'].tolist() == [119, 0, 59, 0]


def test_random_init_twice_and_not_finite():
    P = _joint_of(tr.CASES[1])
    out = _ts(p_in=P, max_iter=0, init=1, seed=77)
    want = tr.random_init(37, 77)
    # fp32 against float64: the cosine's argument errs by 2 pi 2^-24, the radius (< 6) by a few 2^-24: below 1e-4 * 6 * 1e-6
    assert (np.abs(out['y'] - want) <= 1e-9).all() and out['y'].std() > 5e-5
    assert not _same(out['y'], _ts(p_in=P, max_iter=0, init=1, seed=78)['y'])
    x, _ = tr.clusters(65, 8, 9)
    kw = dict(perplexity=12.0, max_iter=25, exag_iter=10, nic=5, init=1, seed=1, want_p=True, chunk=33)
    a, b = _ts(x, **kw), _ts(x, **kw)
    assert all(_same(a[n], b[n]) for n in a) and np.isfinite(a['y']).all() and np.isfinite(a['kl']).all()
    x[5, 3], x[9, 0] = np.nan, np.inf
    out = _ts(x, **kw)                                          # unspecified but complete: the call returns, the guards hold
    assert out['stat'][0] <= 24 and out['stat'][3] == 0


def test_every_error_has_text():
    import torch
    m = _model()
    P = _joint_of(tr.CASES[1])
    x, _ = tr.clusters(37, 8, 1)
    bad = [dict(max_iter=-1), dict(max_iter=32769), dict(max_iter=5, it0=6), dict(it0=-1), dict(nic=0), dict(ee=0.5), dict(reserved=(0, 1)),
           dict(warm=1, state=False), dict(exag_iter=-1), dict(nwp=-1), dict(init=2), dict(lr=float('nan'))]
    for kw in bad:
        assert _ts(p_in=P, raw_status=True, **kw) != 0, kw
        assert len(m._l.avae_last_error(m._h)) > 10, kw
    for kw in (dict(perplexity=0.0), dict(perplexity=37.0), dict(perplexity=float('nan'))):
        assert _ts(x, raw_status=True, **kw) != 0 and b'perplexity' in m._l.avae_last_error(m._h)
    assert _ts(x[:, :6], raw_status=True) != 0 and b'dim' in m._l.avae_last_error(m._h)
    assert _ts(x[:1], raw_status=True) != 0 and b'N must' in m._l.avae_last_error(m._h)
    cfg = _cfg()
    t = torch.zeros((64,), dtype=torch.float64, device=m.device)
    f = torch.zeros((37 * 8 + 8,), dtype=torch.float32, device=m.device)
    p = lambda v, o=0: C.c_void_p(v.data_ptr() + o)
    calls = [(None, None, p(f), p(t), p(t), None, None),                       # neither x nor p_in
             (p(f), None, None, p(t), p(t), None, None),                       # no y
             (p(f), None, p(f), None, p(t), None, None),                       # no kl
             (p(f), None, p(f), p(t), None, None, None),                       # no stat
             (p(f, 4), None, p(f), p(t), p(t), None, None),                    # x not aligned
             (p(f), None, p(f), p(t), p(t), p(f), None),                       # ug without prog
             (p(f), None, p(f), p(t), p(t), None, p(t))]                       # prog without ug
    for dx, dp, y, kl, stat, ug, prog in calls:
        assert m._l.avae_tsne(m._h, dx, 37, 8, C.byref(cfg), dp, y, kl, stat, None, None, None, None, ug, prog) != 0
        assert len(m._l.avae_last_error(m._h)) > 10
    assert m._l.avae_tsne(m._h, p(f), 37, 8, None, None, p(f), p(t), p(t), None, None, None, None, None, None) != 0
    assert m._l.avae_set_option(m._h, b'tsne_chunk', -1) != 0


def test_python_layer_end_to_end(tmp_path, capsys, monkeypatch):
    from argsim_amd import eval_cluster, eval_explore, model
    m = _model()
    x, lab = tr.clusters(120, 10, 21)                            # 10 columns: padded to 12
    res = m.tsne(x, perplexity=8.0, max_iter=60, exaggeration_iter=20, n_iter_check=10, return_p=True, return_trace=True)
    assert res['y'].shape == (120, 2) and res['y'].dtype == np.float32 and res['n_iter'] == 60 and res['stop'] == 'max_iter'
    assert res['kl'] == res['trace'][0, 59] and res['p'].shape == (120, 120) and res['beta'].shape == (120,)
    assert np.isfinite(res['y']).all() and res['y'].std() > 1e-3
    again = model.tsne(m, None, max_iter=60, exaggeration_iter=20, n_iter_check=10, init='random', seed=5, p=res['p'])
    assert again['y'].shape == (120, 2) and np.isfinite(again['kl'])
    names = np.array(['%s-p-1' % ('abortion', 'gun', 'obama', 'marijuana')[t] for t in lab])
    np.save(str(tmp_path / 'z.npy'), x)
    np.save(str(tmp_path / 'l.npy'), names)
    monkeypatch.setattr(eval_cluster, 'make_vae', lambda device: m)
    have_plt = importlib.util.find_spec('matplotlib') is not None
    eval_explore.main(['--inputs', str(tmp_path / 'z.npy'), '--labels', str(tmp_path / 'l.npy'), '--tsne', str(tmp_path / 't.npy'), '--perplexity', '8',
                       '--tsne-iter', '60', '--max-iter', '50'] + (['--tsne-plot', str(tmp_path / 't.png')] if have_plt else []))
    lines = capsys.readouterr().out.strip().split('\n')
    assert lines[0].startswith('t-SNE: KL ') and 'after 60 iterations (max_iter)' in lines[0]
    y = np.load(str(tmp_path / 't.npy'))
    assert y.shape == (120, 2) and np.isfinite(y).all() and (not have_plt or (tmp_path / 't.png').stat().st_size > 1000)
