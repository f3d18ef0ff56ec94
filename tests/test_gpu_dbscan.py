"""Density clustering on the device (avae_dbscan, VAE.dbscan) against the float64 reference of tests/dbscan_ref.py.

No tolerance: label, count, stat[0:4] and stat[5] must EQUAL the reference on every case.  The random cases have the margin (every pair's
p is at least 1e-9 thr away from thr, asserted on the reference alone in test_dbscan.py); the others have integer coordinates, so p is exact
and pairs at exactly eps are inside.  stat[4], the rounds used, must equal the CPU model of the round rule wherever the test has the core
graph at hand, and stay within the planner's default everywhere.  Rows are padded with NaN rows and every output is guarded by a sentinel."""
import ctypes as C

import numpy as np
import pytest

import dbscan_ref as dr
from test_gpu_kmeans import _model, _ptr

pytestmark = pytest.mark.gpu

SENT = -77
_REF = {}


def _cfg(metric, eps, min_samples, max_rounds=0, reserved=0):
    from argsim_amd import lib
    return lib.AvaeDbscanConfig(metric=metric, min_samples=min_samples, max_rounds=max_rounds, reserved=reserved, eps=eps)


def _db(x, metric, eps, min_samples, max_rounds=0, chunk=0, want_count=True):
    """avae_dbscan on NaN-padded rows and sentinel-guarded outputs -> dict(label, count, stat)"""
    import torch
    m = _model()
    dev = m.device
    x = np.ascontiguousarray(x, np.float32)
    N, dim = x.shape
    dx = torch.full((N + 3, dim), float('nan'), dtype=torch.float32, device=dev)
    dx[:N] = torch.as_tensor(x).to(dev)
    bufs = dict(label=N, count=N, stat=8)
    t = {n: torch.full((s + 8,), SENT, dtype=torch.int32, device=dev) for n, s in bufs.items()}
    cfg = _cfg(metric, eps, min_samples, max_rounds)
    assert m._l.avae_set_option(m._h, b'dbscan_chunk', chunk) == 0
    m._stream()
    try:
        m._ck(m._l.avae_dbscan(m._h, _ptr(dx), N, dim, C.byref(cfg), _ptr(t['label']), _ptr(t['count']) if want_count else None, _ptr(t['stat'])))
    finally:
        m._l.avae_set_option(m._h, b'dbscan_chunk', 0)
    out = {}
    for n, s in bufs.items():
        v = t[n].cpu().numpy()
        assert (v[s:] == SENT).all(), n
        out[n] = v[:s]
    if not want_count:
        assert (out['count'] == SENT).all()
    return out


def _ref(key, x, metric, eps, min_samples):
    """the reference of a case, computed once"""
    if key not in _REF:
        _REF[key] = dr.dbscan(x, metric, eps, min_samples)
    return _REF[key]


def _equal(out, ref, N, what, count=True):
    print("%s: stat %s" % (what, out['stat'].tolist()))
    assert np.array_equal(out['label'], ref['label']), what
    if count:
        assert np.array_equal(out['count'], ref['count']), what
    assert out['stat'][:4].tolist() == ref['stat'].tolist() and out['stat'][5] == 0 and (out['stat'][6:] == 0).all(), what
    assert 1 <= out['stat'][4] <= dr.default_rounds(N), what


def _model_rounds(x, metric, eps, min_samples):
    """the rounds the CPU model of the rule takes on the case's core graph"""
    A = dr.pair_values(x, metric) <= dr.threshold(metric, eps)
    core = A.sum(1) >= min_samples
    src, dst = np.nonzero(A & core[:, None] & core[None, :])
    return dr.round_model(len(A), src, dst)[1]


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize('metric', [0, 1], ids=['euc', 'cos'])
@pytest.mark.parametrize('shape', dr.RANDOM_SHAPES, ids=['%dx%d' % s for s in dr.RANDOM_SHAPES])
def test_shapes_against_the_reference(shape, metric):
    """N in {1, 2, 63, 64, 65, 127, 128, 129, 257} x dim in {4, 36, 132}: the word and tile edges, more than one staging stage"""
    x, eps, ms = dr.random_case(shape[0], shape[1], metric)
    ref = _ref(('random', shape, metric), x, metric, eps, ms)
    out = _db(x, metric, eps, ms)
    _equal(out, ref, shape[0], 'random %s %d' % (shape, metric))
    assert out['stat'][4] == _model_rounds(x, metric, eps, ms)


@pytest.mark.parametrize('name', sorted(dr.EXACT))
def test_exact_cases(name):
    """integer grids: pairs at exactly eps are inside; min_samples 1 (every row core, singletons are clusters); min_samples > N (all
    noise); duplicate rows; a line over more than two words"""
    x, metric, eps, ms = dr.EXACT[name]
    ref = _ref(('exact', name), x, metric, eps, ms)
    out = _db(x, metric, eps, ms)
    _equal(out, ref, len(x), name)
    assert out['stat'][4] == _model_rounds(x, metric, eps, ms)
    again = _db(x, metric, eps, ms, want_count=False, chunk=8 | (1 << 8))             # count is optional
    _equal(again, ref, len(x), name + ' without count', count=False)


def test_the_bridge_and_the_numbering():
    x, eps, ms, labels, counts = dr.bridge()
    out = _db(x, 0, eps, ms)
    assert out['label'].tolist() == labels and out['count'].tolist() == counts and out['stat'][:4].tolist() == [2, 10, 1, 0] and out['stat'][5] == 0
    x, eps, ms, labels = dr.numbering()
    out = _db(x, 0, eps, ms)
    assert out['label'].tolist() == labels and out['count'].tolist() == [2, 2, 3, 2, 3, 3, 2] and out['stat'][:4].tolist() == [2, 3, 4, 0]


# ---------------------------------------------------------------- diameter
@pytest.mark.parametrize('order', ['ascending', 'descending', 'bitrev', 'random'])
def test_a_chain_of_4096_rows(order):
    """one cluster, the two ends border; the rounds are the model's and within the default.  With max_rounds = 1 the bit-reversed and
    the random chain have not settled: the verify flag is set and VAE.dbscan raises -- a refusal, not a fault.  (In ascending and in
    descending order row i's neighbours are rows i - 1 and i + 1: the first hook takes every row to its lower neighbour, the first jump
    to row 0 or 1, and one round is all there is to do.)"""
    n = 4096
    o = dr.orders(n)[order]
    x = dr.chain(n, o)
    out = _db(x, 0, 1.0, 3)
    ends = sorted([int(o[0]), int(o[n - 1])])
    assert (out['label'] == 0).all() and np.flatnonzero(out['count'] < 3).tolist() == ends and (np.delete(out['count'], ends) == 3).all()
    assert out['stat'][:4].tolist() == [1, n - 2, 2, 0] and out['stat'][5] == 0
    pos = np.empty(n, np.int64)
    pos[o] = np.arange(n)
    core = np.flatnonzero((pos > 0) & (pos < n - 1))
    at = np.full(n, -1)
    at[pos] = np.arange(n)                                          # the row at each position
    e = np.array([(i, at[pos[i] + 1]) for i in core if pos[i] + 1 < n - 1], np.int64)
    rounds = dr.round_model(n, *dr._both(e))[1]
    print("chain %s: rounds %d, model %d, default %d" % (order, out['stat'][4], rounds, dr.default_rounds(n)))
    assert out['stat'][4] == rounds <= dr.default_rounds(n) // 2
    one = _db(x, 0, 1.0, 3, max_rounds=1)
    assert one['stat'][4] == 1 and np.array_equal(one['count'], out['count'])
    m = _model()
    if order in ('ascending', 'descending'):
        assert rounds == 2 and one['stat'][5] == 0 and np.array_equal(one['label'], out['label'])
        assert m.dbscan(x, 1.0, 3, max_rounds=1)['n_clusters'] == 1
    else:
        assert one['stat'][5] == 1 and one['stat'][0] > 1
        with pytest.raises(RuntimeError, match='max_rounds'):
            m.dbscan(x, 1.0, 3, max_rounds=1)
    assert m.dbscan(x, 1.0, 3, max_rounds=rounds)['n_clusters'] == 1


def test_a_ring_of_4096_rows():
    n = 4096
    for order in ('bitrev', 'random'):
        out = _db(dr.ring(n, dr.orders(n)[order]), 0, 1.0, 3)
        assert (out['label'] == 0).all() and (out['count'] == 3).all() and out['stat'][:4].tolist() == [1, n, 0, 0] and out['stat'][5] == 0
        assert out['stat'][4] <= dr.default_rounds(n) // 2


# ---------------------------------------------------------------- cosine
def test_cosine_zero_rows_and_scaled_copies():
    x = dr.cosine_rows()
    out = _db(x, 1, 0.5, 2)
    assert out['label'].tolist() == [0, -1, 0, 0, -1] and out['count'].tolist() == [3, 1, 3, 3, 1]
    out = _db(x, 1, 0.999, 2)                                       # the zero row is at distance 1 from every other row: noise below 1
    assert out['label'].tolist() == [0, -1, 0, 0, 0] and out['count'].tolist() == [4, 1, 4, 4, 4]
    out = _db(x, 1, 1.0, 5)                                         # ... and a neighbour of every row at 1
    assert out['label'].tolist() == [0] * 5 and out['count'].tolist() == [5] * 5
    out = _db(x, 1, 1e-12, 3)                                       # scaled copies of a row have p = 0
    assert out['label'].tolist() == [0, -1, 0, 0, -1] and out['count'].tolist() == [3, 1, 3, 3, 1]
    two = np.zeros((3, 8), np.float32)                              # two zero rows: p = 2 between them, 0 on the diagonal
    two[2, 5] = 3.0
    out = _db(two, 1, 0.5, 1)
    assert out['label'].tolist() == [0, 1, 2] and out['count'].tolist() == [1, 1, 1]


# ---------------------------------------------------------------- the plan does not show
@pytest.mark.parametrize('metric', [0, 1], ids=['euc', 'cos'])
def test_plan_independence_and_repeatability(metric):
    """label, count and stat (the rounds among them: the rule is schedule-free) are the same bytes for every TI, for several part
    shapes, and across two calls"""
    x, eps, ms = dr.random_case(257, 36, metric)
    ref = _ref(('random', (257, 36), metric), x, metric, eps, ms)
    base = _db(x, metric, eps, ms)
    _equal(base, ref, 257, 'plan base')
    for chunk in (0, 4, 8 | (1 << 8), 16 | (2 << 8), 32 | (3 << 8), 64 | (1 << 8), 64 | (5 << 8), 2 << 8):
        out = _db(x, metric, eps, ms, chunk=chunk)
        assert all(out[n].tobytes() == base[n].tobytes() for n in ('label', 'count', 'stat')), chunk


def test_the_refusals():
    import torch
    m = _model()
    dx = torch.zeros((8, 8), dtype=torch.float32, device=m.device)
    lab = torch.zeros((8,), dtype=torch.int32, device=m.device)
    st = torch.zeros((8,), dtype=torch.int32, device=m.device)
    good = dict(x=_ptr(dx), N=8, dim=8, cfg=_cfg(0, 1.0, 2), label=_ptr(lab), stat=_ptr(st))
    bad = [(dict(x=None), 'x is null'), (dict(label=None), 'label is null'), (dict(stat=None), 'stat is null'), (dict(N=0), 'N must be in [1, 2^17]'),
           (dict(N=(1 << 17) + 1), 'N must be in [1, 2^17]'), (dict(dim=6), 'dim must be a multiple of 4 in [4, 1024]'), (dict(dim=1028), 'dim must be'),
           (dict(cfg=_cfg(2, 1.0, 2)), 'metric must be'), (dict(cfg=_cfg(0, 1.0, 0)), 'min_samples must be >= 1'),
           (dict(cfg=_cfg(0, 1.0, 2, max_rounds=-1)), 'max_rounds must be'), (dict(cfg=_cfg(0, 1.0, 2, max_rounds=4097)), 'max_rounds must be'),
           (dict(cfg=_cfg(0, 0.0, 2)), 'eps must be'), (dict(cfg=_cfg(0, float('nan'), 2)), 'eps must be'), (dict(cfg=_cfg(0, float('inf'), 2)), 'eps must be'),
           (dict(x=_ptr(dx, 4)), '16-byte aligned'), (dict(cfg=_cfg(0, 1.0, 2, reserved=1)), 'reserved')]
    for kw, text in bad:
        a = dict(good)
        a.update(kw)
        rc = m._l.avae_dbscan(m._h, a['x'], a['N'], a['dim'], C.byref(a['cfg']), a['label'], None, a['stat'])
        assert rc != 0 and text in m._l.avae_last_error(m._h).decode(), (kw, m._l.avae_last_error(m._h))
    assert m._l.avae_dbscan(m._h, good['x'], 8, 8, None, good['label'], None, good['stat']) != 0
    assert m._l.avae_set_option(m._h, b'dbscan_chunk', -1) != 0


# ---------------------------------------------------------------- through the Python layer
def test_vae_dbscan_on_host_and_device_rows():
    import torch
    m = _model()
    x, eps, ms = dr.random_case(129, 4, 0)
    z = np.ascontiguousarray(np.concatenate([x, x[:, :2] * 0.5], 1))              # 6 columns: no multiple of 4
    ref = dr.dbscan(z, 0, eps, ms)
    assert dr.margin(z, 0, eps) >= dr.MARGIN
    for arg in (z, torch.as_tensor(z), torch.as_tensor(z).to(m.device)):
        res = m.dbscan(arg, eps, ms)
        assert res['labels'].dtype == np.int64 and np.array_equal(res['labels'], ref['label']) and np.array_equal(res['counts'], ref['count'])
        assert np.array_equal(res['core_sample_indices'], np.flatnonzero(ref['core']))
        assert [res['n_clusters'], len(res['core_sample_indices']), res['n_border'], res['n_noise']] == ref['stat'].tolist()
    x8 = np.ascontiguousarray(np.concatenate([z, z[:, :2]], 1))                    # 8 columns on the device: taken as it is
    from argsim_amd.model import dbscan
    res = dbscan(m, torch.as_tensor(x8).to(m.device), eps, ms, 'cosine')
    assert np.array_equal(res['labels'], dr.dbscan(x8, 1, eps, ms)['label'])


def test_sweep_eps_against_silhouette_by_hand():
    m = _model()
    x, eps, ms = dr.random_case(257, 36, 0)
    grid = [1e-3, 0.8 * eps, eps, 1.2 * eps, 1000.0]
    t = m.sweep_eps(x, grid, ms)
    ok = [1, 2, 3]
    assert t['n_clusters'][0] == 0 and t['n_clusters'][4] == 1 and all(2 <= t['n_clusters'][i] for i in ok)
    for i, e in enumerate(grid):
        assert np.array_equal(t['labels'][i], m.dbscan(x, e, ms)['labels'])
    q = m.silhouette(x, t['labels'][ok], 'euclidean')
    for name in ('score', 'ch', 'db'):
        assert np.array_equal(t[name][ok], q[name]) and np.isnan(t[name][[0, 4]]).all(), name
    assert t['best'] == grid[ok[int(np.argmax(q['score']))]] and t['n_noise'][0] == 257 and t['n_noise'][4] == 0


def test_kdist_against_a_sort():
    """the tolerance tests/test_gpu_knn.py has for the scores of rows of norm about 1 (TOL, on the squared distance), on such rows"""
    from test_gpu_knn import TOL
    m = _model()
    x = dr.blobs(200, 36, 5)
    x = np.ascontiguousarray(x / np.sqrt((x.astype(np.float64) ** 2).sum(1)).mean(), np.float32)
    d2 = ((x[:, None].astype(np.float64) - x[None]) ** 2).sum(2)
    np.fill_diagonal(d2, np.inf)
    want = np.sort(np.sort(d2, 1)[:, 3])
    got = m.kdist(x, 4)
    print("kdist: largest error of the squared distance %.3g (TOL %.3g)" % (np.abs(got ** 2 - want).max(), TOL))
    assert got.shape == (200,) and (np.diff(got) >= 0).all()
    assert (np.abs(got ** 2 - want) <= TOL).all()
    u = x.astype(np.float64) / np.sqrt((x.astype(np.float64) ** 2).sum(1))[:, None]
    c = 1.0 - u @ u.T
    np.fill_diagonal(c, np.inf)
    assert (np.abs(m.kdist(x, 4, 'cosine') - np.sort(np.sort(c, 1)[:, 3])) <= TOL).all()
