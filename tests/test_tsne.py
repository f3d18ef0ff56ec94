"""The float64 restatement of avae_tsne's contract (tests/tsne_ref.py) against sklearn's own pure functions and its loop, the margins of
the cases that tests/test_gpu_tsne.py compares in bits, and the Python layer (argsim_amd/tsne.py, eval_explore --tsne) with a stub
in place of the device call.  No GPU."""
import numpy as np
import pytest

import tsne_ref as tr

_P = {}


def _case_p(case):
    if case not in _P:
        N, dim, _, perp = case
        x, _ = tr.clusters(N, dim, 100 + N)
        ref = tr.conditionals(tr.distances(x), perp)
        _P[case] = (ref, tr.joint(ref['C']))
    return _P[case]


def test_joint_against_sklearn():
    ts = pytest.importorskip('sklearn.manifold._t_sne')
    from scipy.spatial.distance import squareform
    for case in tr.CASES[1:5]:
        N, dim, _, perp = case
        x, _ = tr.clusters(N, dim, 100 + N)
        D = tr.distances(x)
        want = squareform(ts._joint_probabilities(D.astype(np.float32), perp, 0))
        got = _case_p(case)[1]
        off = ~np.eye(N, dtype=bool)
        assert (np.abs(got - want)[off] <= 1e-12 * want[off]).all(), case


def test_error_and_gradient_against_sklearn():
    ts = pytest.importorskip('sklearn.manifold._t_sne')
    from scipy.spatial.distance import squareform
    for case in tr.CASES[1:5]:
        N = case[0]
        P = _case_p(case)[1]
        y = tr.start(N, N, 1.0)
        kl, grad = ts._kl_divergence(y.ravel().copy(), squareform(P, checks=False), 1.0, N, 2)
        ps = tr.pair_sums(P, y)
        assert abs(tr.error(P, ps['q'], ps['Z']) - kl) <= 1e-12 * abs(kl)
        g = ps['g64'].ravel()
        assert (np.abs(g - grad) <= 1e-6 * np.abs(g).max()).all(), case


def test_loop_against_sklearn_bit_for_bit():
    """two phases of sklearn's _gradient_descent driven by the reference's objective: y, iteration and error in bits"""
    ts = pytest.importorskip('sklearn.manifold._t_sne')
    for case, iters, exag in ((tr.CASES[1], 60, 25), (tr.CASES[4], 45, 20)):
        N = case[0]
        P = _case_p(case)[1]
        lr, y0 = tr.auto_lr(N, 12.0), tr.start(N, 2)

        def objective(p, Pe, compute_error=True):
            ps = tr.pair_sums(Pe, p.reshape(N, 2))
            return (tr.error(Pe, ps['q'], ps['Z']) if compute_error else np.nan), ps['g64'].astype(np.float32).ravel()
        kw = dict(n_iter_check=5, learning_rate=lr, min_grad_norm=1e-7, verbose=0)
        p, err1, it = ts._gradient_descent(objective, y0.ravel(), it=0, max_iter=exag, momentum=0.5, n_iter_without_progress=exag, args=[12.0 * P], **kw)
        assert it == exag - 1
        p, err, it = ts._gradient_descent(objective, p, it=it + 1, max_iter=iters, momentum=0.8, n_iter_without_progress=300, args=[P], **kw)
        ref = tr.fit(P, y0, iters, lr, 12.0, exag, 5, 300, 1e-7)
        assert p.dtype == np.float32 and np.array_equal(p.view(np.uint32), ref['y'].ravel().view(np.uint32))
        assert it == ref['stat'][0] and err == ref['kl'][0] and err1 == ref['kl'][1] and ref['stat'].tolist() == [iters - 1, 0, exag - 1, 0]
        assert tr.replay_stop(ref['trace'], iters, exag, 5, 300, 1e-7)[:3] == (iters - 1, 0, exag - 1)


def test_warm_reference_continues_in_bits():
    case = tr.CASES[1]
    P = _case_p(case)[1]
    lr, y0 = tr.auto_lr(37, 12.0), tr.start(37, 2)
    whole = tr.fit(P, y0, 30, lr, exag_iter=10, n_iter_check=5)
    y, state = y0, None
    for i in range(30):
        out = tr.fit(P, y, i + 1, lr, exag_iter=10, n_iter_check=5, it0=i, state=state)
        y, state = out['y'], (out['ug'], out['prog'])
    assert np.array_equal(y, whole['y']) and np.array_equal(state[0], whole['ug']) and np.array_equal(state[1], whole['prog'])


@pytest.mark.parametrize('case', tr.CASES)
def test_bisection_margins(case):
    """the inputs of the device's beta test excuse no row"""
    ref = _case_p(case)[0]
    print("N %d: smallest margin %.3g, largest eval_err %.3g, steps up to %d" % (case[0], ref['margin'].min(), ref['eval_err'].max(), ref['steps'].max()))
    assert (ref['margin'] > ref['eval_err']).all()
    assert ref['steps'].max() < 100


@pytest.mark.parametrize('phase', [1, 2])
@pytest.mark.parametrize('case', tr.CASES + [tr.STEP_ONLY])
def test_step_margins(case, phase):
    """the states of the device's one-step test: no gradient entry falls under its bound"""
    N = case[0]
    P = _case_p(case)[1]
    ps = tr.pair_sums(12.0 * P if phase == 1 else P, tr.start(N, N + phase, 1e-4 if phase == 1 else 1.0))
    m = tr.round_margin(ps['g64'])
    print("N %d phase %d: smallest margin / bound %.3g" % (N, phase, (m / ps['bound']).min()))
    assert (m > ps['bound']).all()


def test_update_is_rounded_fp32():
    r = np.random.default_rng(0)
    y, u, g = (r.standard_normal((50, 2)).astype(np.float32) for _ in range(3))
    gains = r.uniform(0.005, 2, (50, 2)).astype(np.float32)
    ny, nu, ng, gp = tr.update(y, u, gains, g, 0.8, 200.0)
    for v in (ny, nu, ng, gp):
        assert v.dtype == np.float32
    inc = (u * g) < 0
    assert np.array_equal(ng, np.maximum(np.where(inc, gains + np.float32(0.2), gains * np.float32(0.8)), np.float32(0.01)))
    assert np.array_equal(nu, np.float32(0.8) * u - np.float32(200.0) * (g * ng)) and np.array_equal(ny, y + nu)
    assert tr.round_margin(np.array([1.0 + 2.0 ** -24 + 2.0 ** -40]))[0] == 2.0 ** -40


# ---------------------------------------------------------------- the Python layer, with a stub in place of the device call
class _FakeVAE:
    device = 'cpu'

    def raw(self, vae, x, cfg, p_in=None, y=None, want_p=False, want_beta=False, want_trace=False, **kw):
        self.seen = (x, cfg, p_in, y)
        N = x.shape[0] if x is not None else p_in.shape[0]
        if p_in is None:
            ref = tr.conditionals(tr.distances(x), cfg.perplexity)
            P, beta = tr.joint(ref['C']), ref['beta']
        else:
            P, beta = p_in, None
        y0 = tr.random_init(N, cfg.seed).astype(np.float32) if cfg.init == 1 else y
        lr = cfg.learning_rate if cfg.learning_rate > 0 else tr.auto_lr(N, cfg.early_exaggeration)
        out = tr.fit(P, y0, cfg.max_iter, lr, cfg.early_exaggeration, cfg.exaggeration_iter, cfg.n_iter_check, cfg.n_iter_without_progress,
                     cfg.min_grad_norm)
        if want_p:
            out['p'] = P
        if want_beta and beta is not None:
            out['beta'] = beta
        return out

    def tsne(self, z, **kw):
        from argsim_amd import tsne
        return tsne.tsne(self, z, raw=self.raw, **kw)


def test_pca_init():
    from argsim_amd import tsne
    x, _ = tr.clusters(40, 6, 3)
    y = tsne.pca_init(x)
    assert y.shape == (40, 2) and y.dtype == np.float32 and abs(y[:, 0].astype(np.float64).std() - 1e-4) < 1e-10
    xc = x.astype(np.float64) - x.astype(np.float64).mean(0)
    w, v = np.linalg.eigh(xc.T @ xc)
    for c in range(2):                                           # the principal directions, up to the fixed sign
        proj = xc @ v[:, -1 - c]
        corr = abs(np.corrcoef(proj, y[:, c])[0, 1])
        assert corr > 1 - 1e-6
        assert y[np.abs(y[:, c]).argmax(), c] > 0
    assert np.array_equal(tsne.pca_init(-x)[:, 0] != 0, y[:, 0] != 0)
    flat = tsne.pca_init(np.ones((5, 4), np.float32))
    assert flat.shape == (5, 2) and not flat.any()


def test_tsne_checks_its_arguments_and_builds_the_config():
    fake = _FakeVAE()
    x, lab = tr.clusters(48, 10, 5)
    res = fake.tsne(x, perplexity=8.0, max_iter=30, exaggeration_iter=10, n_iter_check=5, return_p=True, return_trace=True)
    xs, cfg, p_in, y = fake.seen
    assert xs.shape == (48, 12) and not xs[:, 10:].any() and p_in is None and y.shape == (48, 2) and y.dtype == np.float32
    assert (cfg.perplexity, cfg.max_iter, cfg.it0, cfg.exaggeration_iter, cfg.n_iter_check, cfg.n_iter_without_progress) == (8.0, 30, 0, 10, 5, 300)
    assert (cfg.init, cfg.warm, cfg.learning_rate, cfg.early_exaggeration, cfg.min_grad_norm) == (0, 0, 0.0, 12.0, 1e-7)
    assert res['n_iter'] == 30 and res['stop'] == 'max_iter' and res['kl'] == res['trace'][0, 29] and res['p'].shape == (48, 48) and res['beta'].shape == (48,)
    res2 = fake.tsne(None, max_iter=5, init='random', seed=9, learning_rate=120.0, p=res['p'])
    xs, cfg, p_in, y = fake.seen
    assert xs is None and p_in is res['p'] and y is None and (cfg.init, cfg.seed, cfg.learning_rate) == (1, 9, 120.0) and res2['y'].shape == (48, 2)
    fake.tsne(x, perplexity=8.0, max_iter=2, init=np.zeros((48, 2), np.float32))
    assert fake.seen[3].shape == (48, 2) and fake.seen[1].init == 0
    bad = [dict(z=x.astype(np.float64)), dict(z=[[1.0]]), dict(z=x[0]), dict(z=x[:1]), dict(z=np.zeros((3, 1028), np.float32)), dict(perplexity=0),
           dict(perplexity=48), dict(perplexity='a'), dict(max_iter=-1), dict(max_iter=32769), dict(max_iter=2.5), dict(init='spectral'),
           dict(init=np.zeros((47, 2), np.float32)), dict(seed=-1), dict(learning_rate=0), dict(learning_rate='fast'), dict(early_exaggeration=0.5),
           dict(exaggeration_iter=-1), dict(n_iter_check=0), dict(n_iter_without_progress=-1), dict(min_grad_norm=-1.0),
           dict(p=np.zeros((48, 47))), dict(p=np.zeros((48, 48), np.float32)), dict(z=None, p=res['p']), dict(p=np.zeros((47, 47)))]
    for kw in bad:
        args = dict(dict(z=x, perplexity=8.0), **kw)
        fake.seen = None
        with pytest.raises(ValueError):
            fake.tsne(args.pop('z'), **args)
        assert fake.seen is None                                 # refused before the library is touched


def test_eval_explore_tsne_plumbing(tmp_path, capsys, monkeypatch):
    from argsim_amd import eval_cluster, eval_explore, tsne
    x, lab = tr.clusters(40, 8, 2)
    names = np.array(['%s-p-1' % ('abortion', 'gun', 'obama', 'marijuana')[t] for t in lab])
    np.save(str(tmp_path / 'z.npy'), x)
    np.save(str(tmp_path / 'l.npy'), names)
    seen = {}

    class Stub:
        def tsne(self, z, **kw):
            seen.update(kw, n=z.shape[0])
            return dict(y=tr.start(z.shape[0], 1, 1.0), kl=0.75, n_iter=17, stop='grad_norm')

        def affinity(self, z, metric, **kw):
            seen['affinity'] = seen.get('affinity', 0) + 1
            return dict(labels=np.arange(z.shape[0]) % 4, converged=True, n_iter=3)
    monkeypatch.setattr(eval_cluster, 'make_vae', lambda device: Stub())
    base = ['--inputs', str(tmp_path / 'z.npy'), '--labels', str(tmp_path / 'l.npy')]
    eval_explore.main(base)
    assert 'n' not in seen and seen['affinity'] == 2 and not capsys.readouterr().out.startswith('t-SNE')
    eval_explore.main(base + ['--tsne', str(tmp_path / 't.npy'), '--seed', '4'])
    assert capsys.readouterr().out.split('\n')[0] == "t-SNE: KL 0.750000 after 17 iterations (grad_norm)"
    assert (seen['n'], seen['perplexity'], seen['max_iter'], seen['init'], seen['seed']) == (40, 40.0, 20000, 'random', 4)
    assert np.array_equal(np.load(str(tmp_path / 't.npy')), tr.start(40, 1, 1.0))
    with pytest.raises(ValueError):
        eval_explore.main(base + ['--tsne-plot', str(tmp_path / 't.png')])
    # without matplotlib: a clear error
    import builtins
    real = builtins.__import__

    def no_mpl(name, *a, **k):
        if name.startswith('matplotlib'):
            raise ImportError(name)
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, '__import__', no_mpl)
    with pytest.raises(RuntimeError, match='matplotlib'):
        tsne.plot(str(tmp_path / 'x.png'), tr.start(40, 1, 1.0), names)
    monkeypatch.setattr(builtins, '__import__', real)
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    eval_explore.main(base + ['--tsne', str(tmp_path / 't.npy'), '--tsne-plot', str(tmp_path / 't.png'), '--perplexity', '5', '--tsne-iter', '100'])
    assert (seen['perplexity'], seen['max_iter']) == (5.0, 100) and (tmp_path / 't.png').stat().st_size > 1000
