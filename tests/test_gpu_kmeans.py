"""K-means on the device (avae_kmeans, VAE.kmeans) against the float64 reference of tests/kmeans_ref.py.

No tolerance here is measured.  On the margin cases (kmeans_ref.CASES and the cases built here the same way; has_margins is asserted on
the reference alone) every decision of a run -- a row's nearest centre, a relocation, a seeding candidate, the shift against the
tolerance -- has a relative margin of 2^-30, far above the error of a double sum, so labels, iterations, stop codes and relocations must
equal the reference's exactly; centres and inertias must agree within the bounds kmeans_ref derives from operation counts (twice: the
reference errs as well).  Which restart is best is compared where the two smallest inertias have the margin too (has_margins; every
single-restart call, and the three-restart calls of the two Gaussian cases); where two restarts reach the same partition it has to be
the first minimum of the device's own inertias.  For ANY input the result carries a certificate that is evaluated in float64 from
the returned labels, centres, inertias and statistics.  Rows are padded with NaN rows and every output is guarded by a sentinel.  (The
refusal of a workspace the device cannot give is not provoked.)"""
import ctypes as C

import numpy as np
import pytest

import kmeans_ref as kr

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


def _cfg(k, n_init=1, max_iter=30, metric=0, init=1, reserved=0, tol=0.0, seed=0):
    from argsim_amd import lib
    return lib.AvaeKmeansConfig(k=k, n_init=n_init, max_iter=max_iter, metric=metric, init=init, reserved=reserved, tol=tol, seed=seed)


def _km(x, k, init=None, chunk=0, **kw):
    """avae_kmeans on NaN-padded rows and sentinel-guarded outputs -> dict of numpy arrays.  init: (n_init, k, dim) centres or None"""
    import torch
    m = _model()
    dev = m.device
    x = np.ascontiguousarray(x, np.float32)
    N, dim = x.shape
    if init is not None:
        init = np.ascontiguousarray(init, np.float32).reshape(-1, k, dim)
        kw['n_init'] = init.shape[0]
    R = kw.get('n_init', 1)
    dx = torch.full((N + 3, dim), float('nan'), dtype=torch.float32, device=dev)
    dx[:N] = torch.as_tensor(x).to(dev)
    dc = None if init is None else torch.as_tensor(init).to(dev)
    bufs = dict(label=(N, torch.int32), centers=(k * dim, torch.float32), stat=(4, torch.int32), inertia=(R, torch.float64),
                label_all=(R * N, torch.int32), centers_all=(R * k * dim, torch.float64), stat_all=(R * 4, torch.int32))
    t = {n: torch.full((s + 8,), SENT_I if dt == torch.int32 else SENT_F, dtype=dt, device=dev) for n, (s, dt) in bufs.items()}
    cfg = _cfg(k, init=0 if init is None else 1, **kw)
    assert m._l.avae_set_option(m._h, b'kmeans_chunk', chunk) == 0
    m._stream()
    try:
        m._ck(m._l.avae_kmeans(m._h, _ptr(dx), N, dim, C.byref(cfg), _ptr(dc), *[_ptr(t[n]) for n in bufs]))
    finally:
        m._l.avae_set_option(m._h, b'kmeans_chunk', 0)
    out = {}
    for n, (s, dt) in bufs.items():
        v = t[n].cpu().numpy()
        assert (v[s:] == (SENT_I if dt == torch.int32 else SENT_F)).all(), n
        out[n] = v[:s]
    out['centers'] = out['centers'].reshape(k, dim)
    out['label_all'] = out['label_all'].reshape(R, N)
    out['centers_all'] = out['centers_all'].reshape(R, k, dim)
    out['stat_all'] = out['stat_all'].reshape(R, 4)
    return out


NAMES = ('label', 'centers', 'stat', 'inertia', 'label_all', 'centers_all', 'stat_all')


def _same_bits(p, q, names=NAMES):
    return all(p[n].tobytes() == q[n].tobytes() for n in names)


def _consistent(out):
    """the best restart's outputs are copies of its row of the *_all outputs; stat[0] is the first minimum of inertia"""
    b = int(out['stat'][0])
    assert b == int(np.argmin(out['inertia']))
    assert out['stat'][1:].tolist() == out['stat_all'][b, :3].tolist() and (out['stat_all'][:, 3] == 0).all()
    assert np.array_equal(out['label'], out['label_all'][b])
    assert np.array_equal(out['centers'].view(np.uint32), out['centers_all'][b].astype(np.float32).view(np.uint32))


def _against(out, ref, metric):
    """the device's result against the reference's on a case with margins"""
    assert kr.restarts_have_margins(ref), ref['margin']
    X = ref['X']
    _consistent(out)
    for r, q in enumerate(ref['runs']):
        assert out['stat_all'][r].tolist() == [q['n_iter'], q['stop'], q['relocations'], 0], (r, out['stat_all'][r], q['n_iter'], q['stop'])
        assert np.array_equal(out['label_all'][r], q['labels']), r
        e = kr.centre_bound(X, q['labels'], q['centers'], metric)
        dc = np.abs(out['centers_all'][r] - q['centers'])
        bi = kr.inertia_bound(X, q['labels'], q['centers'], e)
        di = abs(out['inertia'][r] - q['inertia'])
        print("restart %d: centre error / bound %.3g, inertia error / bound %.3g" % (r, (dc / (2 * e + 1e-300)).max(), di / (2 * bi + 1e-300)))
        assert (dc <= 2 * e).all() and di <= 2 * bi
    if kr.has_margins(ref):
        assert out['stat'][0] == ref['best']


def _certificate(out, x, metric):
    """what any result must satisfy, from the returned outputs alone"""
    X = kr.rows_of(x, metric)
    N = X.shape[0]
    _consistent(out)
    for r in range(out['label_all'].shape[0]):
        lab, Cn = out['label_all'][r], out['centers_all'][r]
        k = Cn.shape[0]
        assert ((lab >= 0) & (lab < k)).all()
        D = kr.sqdist(X, Cn)
        B = kr.dist_bound(X, Cn)
        own = D[np.arange(N), lab]
        assert (own <= (D + B).min(1) + B[np.arange(N), lab]).all(), r                # every row's centre is its nearest
        cnt = np.bincount(lab, minlength=k)
        assert (cnt > 0).all(), r                                                      # no cluster is empty
        if out['stat_all'][r, 1] == 0:                                                 # converged: every centre is its members' mean
            S = np.zeros_like(Cn)
            np.add.at(S, lab, X)
            mean = S / cnt[:, None]
            mean = kr.project(mean) if metric else mean
            assert (np.abs(Cn - mean) <= 2 * kr.centre_bound(X, lab, mean, metric)).all(), r
        e = np.zeros_like(Cn)
        assert abs(out['inertia'][r] - own.sum()) <= 2 * kr.inertia_bound(X, lab, Cn, e), r
        assert 1 <= out['stat_all'][r, 0] and 0 <= out['stat_all'][r, 1] <= 2


# ---------------------------------------------------------------- Lloyd with given centres
@pytest.mark.parametrize('metric', [0, 1], ids=['euc', 'cos'])
@pytest.mark.parametrize('case', kr.CASES, ids=kr.CASE_IDS)
def test_margin_cases_and_the_plan_with_several_parts(case, metric):
    name, make, k = case
    x = make()
    for which, init in kr.case_inits(x, k).items():
        ref = kr.run(x, k, metric, n_init=init.shape[0], max_iter=30, init=init)
        out = _km(x, k, init, metric=metric)
        _against(out, ref, metric)
        _certificate(out, x, metric)
        chunk = max(2, (k + 3) // 4)                     # >= 3 centre parts, and with chunk rows per tile, slice and block >= 3 of each
        assert -(-k // chunk) >= 3 and -(-x.shape[0] // chunk) >= 3
        small = _km(x, k, init, chunk=chunk, metric=metric)
        _against(small, ref, metric)
        assert _same_bits(out, small, ('label', 'stat', 'label_all', 'stat_all')), which


def test_tol_and_max_iter_stops():
    x = kr.gaussian(200, 16, 3)
    init = kr.random_init(x, 8, 5, 2)
    full = kr.run(x, 8, 0, n_init=2, max_iter=60, init=init)
    assert min(q['n_iter'] for q in full['runs']) > 4
    ref = kr.run(x, 8, 0, n_init=2, max_iter=3, init=init)
    assert [q['stop'] for q in ref['runs']] == [2, 2]
    _against(_km(x, 8, init, max_iter=3), ref, 0)
    for metric in (0, 1):
        ref = kr.run(x, 8, metric, n_init=2, max_iter=60, tol=0.5, init=init)
        assert 1 in [q['stop'] for q in ref['runs']]
        _against(_km(x, 8, init, metric=metric, max_iter=60, tol=0.5), ref, metric)


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize('N', [1, 2, 63, 64, 65, 257])
def test_row_counts(N):
    for k in sorted({1, min(2, N), N}):
        x = kr.gaussian(N, 4, 100 + N)
        init = kr.random_init(x, k, N + k, 1)
        ref = kr.run(x, k, 0, max_iter=30, init=init)
        for chunk in (0, 5):
            out = _km(x, k, init, chunk=chunk)
            _certificate(out, x, 0)
            if kr.has_margins(ref):
                _against(out, ref, 0)


@pytest.mark.parametrize('k', [63, 64, 65, 130])
def test_centre_counts_across_a_wave_and_a_part(k):
    x = kr.pad4(kr.gaussian(300, 12, k))
    init = kr.random_init(x, k, k, 3)                     # different centres per restart
    unit = kr.project(init.reshape(-1, 12).astype(np.float64)).astype(np.float32).reshape(init.shape)
    for metric, init in ((0, init), (1, unit)):
        ref = kr.run(x, k, metric, n_init=3, max_iter=30, init=init)
        out = _km(x, k, init, metric=metric)
        _certificate(out, x, metric)
        _against(out, ref, metric)
        assert _same_bits(out, _km(x, k, init, metric=metric, chunk=48), ('label_all', 'stat_all'))
        one = _km(x, k, init[1:2], metric=metric)             # a restart alone is that restart
        assert np.array_equal(one['label'], out['label_all'][1]) and one['stat'][1:].tolist() == out['stat_all'][1, :3].tolist()


@pytest.mark.parametrize('dim', [128, 1024])
def test_wide_rows(dim):
    """dim 128, and 1024 where every thread of the centre kernel owns four columns"""
    x = kr.gaussian(150 if dim == 128 else 60, dim, 8)
    init = kr.random_init(x, 7, 3, 2)
    unit = kr.project(init.reshape(-1, dim).astype(np.float64)).astype(np.float32).reshape(init.shape)
    for metric, start in ((0, init), (1, unit)):
        ref = kr.run(x, 7, metric, n_init=2, max_iter=30, init=start)
        out = _km(x, 7, start, metric=metric)
        _certificate(out, x, metric)
        _against(out, ref, metric)


# ---------------------------------------------------------------- relocation, ties
@pytest.mark.parametrize('n_far', [1, 2])
def test_relocation(n_far):
    """one empty cluster, and two in the same iteration from duplicate far centres"""
    x = kr.planted(96, 8, 6, 1)
    init = kr.far_init(x, 6, 4, n_far)[None]
    ref = kr.run(x, 6, 0, max_iter=30, init=init)
    assert ref['relocations'] >= n_far
    for chunk in (0, 7):
        out = _km(x, 6, init, chunk=chunk)
        _against(out, ref, 0)
        _certificate(out, x, 0)
    one = kr.run(x, 6, 0, max_iter=1, init=init)            # the iteration that relocates, on its own
    assert one['relocations'] == n_far
    _against(_km(x, 6, init, max_iter=1), one, 0)


def test_repeated_points_and_duplicate_centres_take_the_first_minimum():
    pts = kr.gaussian(4, 8, 5)
    x = np.tile(pts, (6, 1))
    init = np.stack([pts[0], pts[0], pts[2]])[None]         # centres 0 and 1 are equal: every tie goes to 0, cluster 1 is empty
    out = _km(x, 3, init, max_iter=1)
    first = kr.sqdist(kr.rows_of(x, 0), init[0].astype(np.float64)).argmin(1)
    assert (first != 1).all()
    ref = kr.run(x, 3, 0, max_iter=1, init=init)
    assert out['stat_all'][0].tolist() == [1, 2, 1, 0] and ref['relocations'] == 1
    full = _km(x, 4, np.stack([pts[0], pts[1], pts[2], pts[3]])[None])
    assert np.array_equal(full['label'], np.tile(np.arange(4), 6)) and full['inertia'][0] == 0.0
    _certificate(full, x, 0)


# ---------------------------------------------------------------- seeding
@pytest.mark.parametrize('metric', [0, 1], ids=['euc', 'cos'])
@pytest.mark.parametrize('case', kr.CASES, ids=kr.CASE_IDS)
def test_seeding(case, metric):
    name, make, k = case
    x = make()
    one = kr.run(x, k, metric, n_init=3, max_iter=1, seed=5)            # the chosen rows, visible through the first update
    _against(_km(x, k, n_init=3, max_iter=1, seed=5, metric=metric), one, metric)
    ref = kr.run(x, k, metric, n_init=3, max_iter=30, seed=5)
    out = _km(x, k, n_init=3, max_iter=30, seed=5, metric=metric)
    _against(out, ref, metric)
    _certificate(out, x, metric)
    for R in (1, 5):                                                     # restart r does not depend on n_init
        other = _km(x, k, n_init=R, max_iter=30, seed=5, metric=metric, chunk=0 if R == 1 else 16)
        n = min(R, 3)
        assert np.array_equal(other['label_all'][:n], out['label_all'][:n]) and np.array_equal(other['stat_all'][:n], out['stat_all'][:n])
        if R == 1:
            assert _same_bits({k_: v[:1] for k_, v in out.items() if k_.endswith('_all')}, other, ('label_all', 'centers_all', 'stat_all'))


# ---------------------------------------------------------------- any input
@pytest.mark.parametrize('metric', [0, 1], ids=['euc', 'cos'])
def test_certificate_on_random_data(metric):
    x = kr.gaussian(300, 32, 21)
    for chunk in (0, 6):
        out = _km(x, 17, n_init=4, max_iter=60, seed=3, metric=metric, chunk=chunk)
        _certificate(out, x, metric)


def test_the_same_call_twice_gives_the_same_bits():
    x = kr.gaussian(300, 32, 21)
    for kw in (dict(metric=0, seed=9, n_init=3), dict(metric=1, seed=2, n_init=2, tol=1e-4)):
        assert _same_bits(_km(x, 17, **kw), _km(x, 17, **kw))


def test_errors_have_text():
    import torch
    m = _model()
    dev = m.device
    N, k, dim = 16, 3, 8
    x = torch.ones((N, dim), dtype=torch.float32, device=dev)
    cin = torch.ones((2 * k * dim + 4,), dtype=torch.float32, device=dev)
    label = torch.full((N,), SENT_I, dtype=torch.int32, device=dev)
    centers = torch.full((k * dim,), SENT_F, dtype=torch.float32, device=dev)
    stat = torch.full((4,), SENT_I, dtype=torch.int32, device=dev)
    inertia = torch.full((2,), SENT_F, dtype=torch.float64, device=dev)

    def call(x=x, N=N, dim=dim, cin=cin, label=label, centers=centers, stat=stat, inertia=inertia, off=0, coff=0, null_cfg=False, **kw):
        kw.setdefault('k', k)
        cfg = _cfg(**kw)
        return m._l.avae_kmeans(m._h, _ptr(x, off), N, dim, None if null_cfg else C.byref(cfg), _ptr(cin, coff), _ptr(label), _ptr(centers),
                                _ptr(stat), _ptr(inertia), None, None, None)

    bad = [dict(null_cfg=True), dict(x=None), dict(label=None), dict(centers=None), dict(stat=None), dict(inertia=None), dict(N=0),
           dict(N=(1 << 22) + 1), dict(dim=6), dict(dim=0), dict(dim=1028), dict(off=4), dict(coff=4), dict(k=0), dict(k=N + 1), dict(k=4097, N=8192),
           dict(n_init=0), dict(n_init=65), dict(max_iter=0), dict(max_iter=10001), dict(metric=2), dict(metric=-1), dict(init=2), dict(init=-1),
           dict(init=1, cin=None), dict(tol=-1e-9), dict(tol=float('nan')), dict(reserved=1)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert len(m._l.avae_last_error(m._h)) > 5, kw
    torch.cuda.synchronize(dev)
    assert (label == SENT_I).all() and (stat == SENT_I).all() and (centers == SENT_F).all() and (inertia == SENT_F).all()      # untouched
    assert call(n_init=2) == 0                              # the handle stays usable
    assert call(init=0, cin=None, n_init=2) == 0
    torch.cuda.synchronize(dev)
    assert (label != SENT_I).all() and (stat != SENT_I).all()


def test_python_layer():
    import torch
    from argsim_amd import model
    m = _model()
    z = kr.gaussian(37, 10, 2)                              # 10 columns: padded with zeros to 12
    x = kr.pad4(z)
    raw = _km(x, 5, n_init=3, max_iter=30, seed=4, metric=1, tol=1e-4 * 12 / 10)
    res = m.kmeans(z, 5, 'cosine', n_init=3, max_iter=30, seed=4, return_all=True)
    assert res['labels'].dtype == np.int64 and np.array_equal(res['labels'], raw['label'])
    assert res['centers'].shape == (5, 10) and np.array_equal(res['centers'], raw['centers'][:, :10])
    assert res['best'] == raw['stat'][0] and res['n_iter'] == raw['stat'][1] and res['stop'] == kr.STOPS[raw['stat'][2]]
    assert res['relocations'] == raw['stat'][3] and np.array_equal(res['inertias'], raw['inertia']) and res['inertia'] == raw['inertia'][res['best']]
    assert np.array_equal(res['labels_all'], raw['label_all']) and res['centers_all'].shape == (3, 5, 10) and len(res['stats_all']) == 3
    c0 = z[[0, 7, 14, 21, 28]]
    given = model.kmeans(m, z, 5, init=c0, max_iter=30, tol=0.0)                       # a (k, dim) start: one restart
    ref = kr.run(x, 5, 0, max_iter=30, init=kr.pad4(c0)[None])
    assert np.array_equal(given['labels'], ref['labels']) and given['n_iter'] == ref['n_iter'] and len(given['inertias']) == 1
    dev = m.kmeans(torch.as_tensor(x).to(m.device), 5, init=kr.pad4(c0), max_iter=30, tol=0.0)      # a device tensor is taken as it is
    assert np.array_equal(dev['labels'], given['labels']) and dev['centers'].shape == (5, 12)
