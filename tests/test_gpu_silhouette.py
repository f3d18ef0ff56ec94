"""Cluster-quality scores on the device (avae_silhouette, VAE.silhouette) against the float64 reference of tests/sil_ref.py.

No tolerance here is measured: a, b, s, score, cluster_mean, CH and DB must agree within twice the bounds sil_ref derives from
operation counts (twice: the reference errs as well); count is exact, and so is nearest on the cases whose reference has the margin
(sil_ref.has_margins, asserted on the reference alone).  sil, ab and nearest must be the same BITS for every sil_chunk, that is for
every tile shape and every grouping of the labelings into passes.  Rows are padded with NaN rows, rows that no labeling labels hold
NaN, and every output is guarded by a sentinel.  (The refusal of a workspace the device cannot give is not provoked.)"""
import ctypes as C

import numpy as np
import pytest

import sil_ref as sr
from test_gpu_kmeans import _model, _ptr

pytestmark = pytest.mark.gpu

SENT_I, SENT_F = -77, 123.0
OUTS = ('score', 'sil', 'ab', 'nearest', 'count', 'cluster_mean', 'index')
_REF = {}


def _cfg(metric, L, reserved=0, reserved2=0):
    from argsim_amd import lib
    return lib.AvaeSilhouetteConfig(metric=metric, L=L, reserved=reserved, reserved2=reserved2)


def _sil(x, metric, labels, K, chunk=0, skip=()):
    """avae_silhouette on NaN-padded rows and sentinel-guarded outputs -> dict of numpy arrays; skip: optional outputs passed as null"""
    import torch
    m = _model()
    dev = m.device
    x = np.ascontiguousarray(x, np.float32)
    labels = np.ascontiguousarray(np.atleast_2d(labels), np.int32)
    K = np.ascontiguousarray(K, np.int32)
    (L, N), dim, kmax = labels.shape, x.shape[1], int(K.max())
    dx = torch.full((N + 3, dim), float('nan'), dtype=torch.float32, device=dev)
    dx[:N] = torch.as_tensor(x).to(dev)
    dl = torch.full((L * N + 8,), 1, dtype=torch.int32, device=dev)
    dl[:L * N] = torch.as_tensor(labels.reshape(-1)).to(dev)
    bufs = dict(score=(L, torch.float64), sil=(L * N, torch.float64), ab=(L * N * 2, torch.float64), nearest=(L * N, torch.int32),
                count=(L * kmax, torch.int32), cluster_mean=(L * kmax, torch.float64), index=(L * 2, torch.float64))
    t = {n: torch.full((s + 8,), SENT_I if dt == torch.int32 else SENT_F, dtype=dt, device=dev) for n, (s, dt) in bufs.items()}
    cfg = _cfg(metric, L)
    assert m._l.avae_set_option(m._h, b'sil_chunk', chunk) == 0
    m._stream()
    try:
        m._ck(m._l.avae_silhouette(m._h, _ptr(dx), N, dim, C.byref(cfg), _ptr(dl), K.ctypes.data_as(C.POINTER(C.c_int32)),
                                   *[None if n in skip else _ptr(t[n]) for n in OUTS]))
    finally:
        m._l.avae_set_option(m._h, b'sil_chunk', 0)
    out = {}
    for n, (s, dt) in bufs.items():
        v = t[n].cpu().numpy()
        sent = SENT_I if dt == torch.int32 else SENT_F
        assert (v[s:] == sent).all(), n
        if n in skip:
            assert (v == sent).all(), n
        out[n] = v[:s]
    for n, shape in (('sil', (L, N)), ('ab', (L, N, 2)), ('nearest', (L, N)), ('count', (L, kmax)), ('cluster_mean', (L, kmax)), ('index', (L, 2))):
        out[n] = out[n].reshape(shape)
    return out


def _refs(key, x, metric, labels, K):
    """the reference of a case, computed once"""
    if key not in _REF:
        _REF[key] = sr.run(x, metric, labels, K)
    return _REF[key]


def _close(got, want, bound, what):
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    err = np.where(both_nan, 0.0, np.abs(got - want))
    bound = np.where(both_nan, 0.0, bound)
    worst = np.max(err / (2 * bound + 1e-300)) if err.size else 0.0
    print("%s: error / (2 bound) %.3g" % (what, worst))
    assert (np.isnan(got) == np.isnan(want)).all(), what
    assert (err <= 2 * bound).all(), (what, float(err.max()), float(np.max(bound)))


def _against(out, x, metric, refs, K, exact_nearest=True):
    kmax = int(np.max(K))
    for l, ref in enumerate(refs):
        bd = sr.bounds(x, metric, ref)
        k = int(K[l])
        assert np.array_equal(out['count'][l, :k], ref['count']) and (out['count'][l, k:] == 0).all(), l
        if exact_nearest:
            assert sr.has_margins(ref), l
            assert np.array_equal(out['nearest'][l], ref['nearest']), l
        off = ref['label'] < 0
        assert (out['sil'][l][off] == 0).all() and (out['ab'][l][off] == 0).all() and (out['nearest'][l][off] == -1).all(), l
        _close(out['ab'][l, :, 0], ref['a'], bd['a'], 'a[%d]' % l)
        _close(out['ab'][l, :, 1], ref['b'], bd['b'], 'b[%d]' % l)
        _close(out['sil'][l], ref['sil'], bd['s'], 's[%d]' % l)
        _close(out['score'][l], ref['score'], bd['score'], 'score[%d]' % l)
        _close(out['cluster_mean'][l, :k], ref['cluster_mean'], bd['cluster_mean'], 'cluster_mean[%d]' % l)
        assert (out['cluster_mean'][l, k:] == 0).all() and kmax >= k
        _close(out['index'][l, 0], ref['ch'], bd['ch'], 'CH[%d]' % l)
        _close(out['index'][l, 1], ref['db'], bd['db'], 'DB[%d]' % l)


def _same_bits(p, q, names=OUTS):
    return all(p[n].tobytes() == q[n].tobytes() for n in names)


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize('metric', [0, 1, 2], ids=['euc', 'cos', 'sqeuc'])
@pytest.mark.parametrize('case', sr.CASES, ids=sr.CASE_IDS)
def test_shapes_against_the_reference(case, metric):
    """N in {2, 3, 65, 130, 257}, dim in {4, 12, 128}, L in {1, 3, 5}, K in {2, 3, 7, 70}, cluster ids without members"""
    x, labels, K = sr.case_labels(case)
    refs = _refs((case[0], metric), x, metric, labels, K)
    _against(_sil(x, metric, labels, K), x, metric, refs, K)


# ---------------------------------------------------------------- the plan does not show
@pytest.mark.parametrize('metric', [0, 1], ids=['euc', 'cos'])
def test_plan_independence_and_repeatability(metric):
    """sum K = 159 over five labelings: with sil_chunk 24 three passes, with 4 one labeling per pass and TI = 4, 8 and 40 the other row
    tiles; sil, ab and nearest are the same bits whatever the tile shape and the passes, a repeated call repeats every output"""
    x, labels, K = sr.case_labels(sr.CASES[3])
    assert K.tolist() == [3, 7, 70, 2, 7]
    refs = _refs((sr.CASES[3][0], metric), x, metric, labels, K)
    base = _sil(x, metric, labels, K)
    _against(base, x, metric, refs, K)
    assert _same_bits(base, _sil(x, metric, labels, K))
    for chunk in (4, 24, 8, 40, 64):
        other = _sil(x, metric, labels, K, chunk=chunk)
        assert _same_bits(base, other, ('sil', 'ab', 'nearest', 'count')), chunk
        _against(other, x, metric, refs, K)


def test_k_4096_runs_the_smallest_row_tile():
    """N = 260 with labels spread over [0, 4096): the bins of four rows fill the LDS"""
    N = 260
    x = sr.pad4(sr.gaussian(N, 12, 9))
    r = np.random.default_rng(3)
    labels = np.sort(r.choice(4096, 130, replace=False))[np.arange(N) % 130].astype(np.int32)[None]      # 130 clusters of two rows
    labels[0, 0], labels[0, 130] = 0, 4095                                                              # the first and the last bin
    K = np.array([4096], np.int32)
    plan = np.zeros(8, np.int32)
    m = _model()
    assert m._l.avae_debug_sil_plan(N, 12, 1, K.ctypes.data_as(C.POINTER(C.c_int32)), 0, 256, plan.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    assert plan[0] == 4 and plan[2] == 1
    for metric in (0, 1):
        refs = sr.run(x, metric, labels, K)
        _against(_sil(x, metric, labels, K), x, metric, refs, K)


# ---------------------------------------------------------------- unlabelled rows
@pytest.mark.parametrize('metric', [0, 1, 2], ids=['euc', 'cos', 'sqeuc'])
def test_unlabelled_rows_enter_nothing(metric):
    """labels -1 and >= K, different per labeling; rows unlabelled in EVERY labeling hold NaN; the outputs are those of the labelled
    subset on its own"""
    x, labels, K = sr.case_labels(sr.CASES[2])
    N = x.shape[0]
    labels = labels.copy()
    labels[0, 5::7] = -1
    labels[1, 3::5] = K[1]
    labels[2, 1::4] = -5
    labels[2, 2::9] = 4096
    dead = np.arange(4, N, 11)
    labels[:, dead] = -1
    xn = x.copy()
    xn[dead] = np.nan
    out = _sil(xn, metric, labels, K, chunk=24)
    for n in OUTS:
        assert np.isfinite(out[n]).all(), n
    refs = sr.run(xn, metric, labels, K)
    _against(out, np.where(np.isnan(xn), 0, xn).astype(np.float32), metric, refs, K)
    for l in range(3):                                       # ... and the subset as a call of its own: the same bits row by row
        on = (labels[l] >= 0) & (labels[l] < K[l])
        sub = _sil(x[on], metric, labels[l][on], K[l:l + 1])
        assert np.array_equal(sub['sil'][0], out['sil'][l][on]) and np.array_equal(sub['ab'][0], out['ab'][l][on])
        assert np.array_equal(sub['nearest'][0], out['nearest'][l][on]) and np.array_equal(sub['count'][0], out['count'][l, :K[l]])
        _against(sub, x[on], metric, sr.run(x[on], metric, labels[l][on][None], K[l:l + 1]), K[l:l + 1])


# ---------------------------------------------------------------- degenerate cases
def test_degenerate_cases():
    x = sr.gaussian(12, 8, 4)
    one = _sil(x, 0, np.zeros(12, np.int32), [1])                                     # K = 1: no other cluster
    assert (one['sil'] == 0).all() and one['score'][0] == 0 and (one['nearest'] == -1).all() and (one['ab'][0, :, 1] == 0).all()
    assert np.isnan(one['index']).all() and one['count'][0, 0] == 12 and (one['ab'][0, :, 0] > 0).all()
    _against(one, x, 0, sr.run(x, 0, np.zeros((1, 12), np.int32), [1]), [1])
    each = _sil(x, 0, np.arange(12, dtype=np.int32), [12])                            # every row its own cluster
    assert (each['sil'] == 0).all() and (each['ab'][0, :, 0] == 0).all() and (each['ab'][0, :, 1] > 0).all() and (each['count'] == 1).all()
    assert np.isnan(each['index'][0, 0]) and each['index'][0, 1] == 0
    _against(each, x, 0, sr.run(x, 0, np.arange(12, dtype=np.int32)[None], [12]), [12])
    two = _sil(x[:2], 2, np.array([0, 1], np.int32), [2])                             # N = 2
    assert (two['sil'] == 0).all() and two['nearest'].tolist() == [[1, 0]] and two['ab'][0, 0, 1] == two['ab'][0, 1, 0 + 1] > 0


@pytest.mark.parametrize('metric', [0, 2], ids=['euc', 'sqeuc'])
def test_duplicate_rows_give_exact_zeros(metric):
    """cluster 0 is six copies of one row: a = 0 exactly there; all clusters made of copies: trW = 0 and CH = 1.0"""
    pts = sr.gaussian(3, 8, 6)
    x = np.concatenate([np.tile(pts[0], (6, 1)), sr.gaussian(9, 8, 7)])
    labels = np.array([0] * 6 + [1] * 5 + [2] * 4, np.int32)
    out = _sil(x, metric, labels, [3])
    assert (out['ab'][0, :6, 0] == 0).all() and (out['sil'][0, :6] == 1).all() and (out['ab'][0, 6:, 0] > 0).all()
    _against(out, x, metric, sr.run(x, metric, labels[None], [3]), [3])
    x = np.repeat(pts, 4, axis=0)
    labels = np.repeat(np.arange(3), 4).astype(np.int32)
    out = _sil(x, metric, labels, [3])
    assert (out['ab'][0, :, 0] == 0).all() and (out['sil'] == 1).all() and out['score'][0] == 1 and out['index'][0, 0] == 1.0 and out['index'][0, 1] == 0
    # coincident centroids: clusters 0 and 1 hold the same two points, R_01 = 0; cluster 2 is apart
    p = sr.gaussian(4, 8, 8)
    x = np.stack([p[0], p[1], p[0], p[1], p[2], p[3]])
    labels = np.array([0, 0, 1, 1, 2, 2], np.int32)
    ref = sr.run(x, metric, labels[None], [3])
    assert ref[0]['R'][0, 1] == 0 and ref[0]['R'][0, 2] > 0
    out = _sil(x, metric, labels, [3])
    _against(out, x, metric, ref, [3], exact_nearest=False)      # rows 4 and 5 are equally far from clusters 0 and 1, bit for bit:
    assert out['nearest'][0].tolist() == ref[0]['nearest'].tolist() and out['nearest'][0, 4:].tolist() == [0, 0]      # the first of them


def test_a_zero_row_under_the_cosine():
    x, labels, K = sr.case_labels(sr.CASES[2])
    x = x.copy()
    x[7] = 0
    refs = sr.run(x, 1, labels, K)
    out = _sil(x, 1, labels, K)
    assert (out['ab'][:, 7] == 1).all()                      # 1 - 0 to every other row
    _against(out, x, 1, refs, K, exact_nearest=False)


# ---------------------------------------------------------------- optional outputs, errors
def test_optional_outputs():
    x, labels, K = sr.case_labels(sr.CASES[2])
    full = _sil(x, 1, labels, K)
    for n in OUTS[1:]:
        part = _sil(x, 1, labels, K, skip=(n,))
        assert _same_bits(full, part, [q for q in OUTS if q != n]), n
    bare = _sil(x, 1, labels, K, skip=OUTS[1:])
    assert np.array_equal(bare['score'], full['score'])


def test_errors_have_text():
    import torch
    m = _model()
    dev = m.device
    N, dim, L = 16, 8, 2
    x = torch.ones((N + 1, dim), dtype=torch.float32, device=dev)
    label = torch.zeros((L * N,), dtype=torch.int32, device=dev)
    score = torch.full((L,), SENT_F, dtype=torch.float64, device=dev)
    sil = torch.full((L * N,), SENT_F, dtype=torch.float64, device=dev)
    Ks = np.array([2, 3], np.int32)

    def call(x=x, N=N, dim=dim, label=label, K=Ks, score=score, off=0, null_cfg=False, metric=0, L=L, **kw):
        cfg = _cfg(metric, L, **kw)
        kp = None if K is None else np.ascontiguousarray(K, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
        return m._l.avae_silhouette(m._h, _ptr(x, off), N, dim, None if null_cfg else C.byref(cfg), _ptr(label), kp, _ptr(score), _ptr(sil), None,
                                    None, None, None, None)

    bad = [dict(null_cfg=True), dict(x=None), dict(label=None), dict(K=None), dict(score=None), dict(N=1), dict(N=(1 << 18) + 1), dict(dim=6),
           dict(dim=0), dict(dim=1028), dict(L=0), dict(L=65, K=[2] * 65), dict(K=[2, 0]), dict(K=[4097, 2]), dict(metric=3), dict(metric=-1),
           dict(off=4), dict(reserved=1), dict(reserved2=1)]
    texts = set()
    for kw in bad:
        assert call(**kw) != 0, kw
        text = m._l.avae_last_error(m._h)
        assert len(text) > 5, kw
        texts.add(text)
    assert len(texts) >= 13                                  # null sc, x, label, K, score; N, dim, L, K[l], metric; alignment; reserved
    torch.cuda.synchronize(dev)
    assert (score == SENT_F).all() and (sil == SENT_F).all()                           # untouched
    assert call() == 0                                       # the handle stays usable
    torch.cuda.synchronize(dev)
    assert (score != SENT_F).all() and (sil != SENT_F).all()


# ---------------------------------------------------------------- the public path
def test_python_layer():
    import torch
    from argsim_amd import model
    m = _model()
    z = sr.gaussian(65, 10, 3)                              # 10 columns: padded with zeros to 12
    x = sr.pad4(z)
    labels = np.stack([sr.labels_of(65, 3, 1), sr.labels_of(65, 7, 2)]).astype(np.int64) * 5 + 2      # values 2, 7, 12 ..
    labels[1, ::6] = -3
    for metric, code in (('euclidean', 0), ('cosine', 1)):
        res = m.silhouette(z, labels, metric, return_samples=True)
        comp = np.where(labels >= 0, (labels - 2) // 5, -1)
        refs = sr.run(x, code, comp, [3, 7])
        for l, ref in enumerate(refs):
            bd = sr.bounds(x, code, ref)
            assert res['clusters'][l].tolist() == (np.arange(res['n_clusters'][l]) * 5 + 2).tolist()
            assert np.array_equal(res['counts'][l], ref['count'])
            _close(res['samples'][l], ref['sil'], bd['s'], 'samples')
            _close(res['a'][l], ref['a'], bd['a'], 'a')
            _close(res['b'][l], ref['b'], bd['b'], 'b')
            _close(res['score'][l], ref['score'], bd['score'], 'score')
            _close(res['ch'][l], ref['ch'], bd['ch'], 'ch')
            _close(res['db'][l], ref['db'], bd['db'], 'db')
            assert sr.has_margins(ref) and np.array_equal(res['nearest'][l], np.where(ref['nearest'] >= 0, ref['nearest'] * 5 + 2, -1))
    one = model.silhouette(m, torch.as_tensor(x).to(m.device), labels[0])             # (N,) labels; a device tensor is taken as it is
    assert one['score'].shape == () and one['score'] == m.silhouette(z, labels)['score'][0]
    with pytest.raises(ValueError):
        m.silhouette(z, np.zeros(65, np.int64))
    metrics = pytest.importorskip('sklearn.metrics')
    # sklearn forms Euclidean distances by the dot trick: d^2 = |x|^2 + |y|^2 - 2 xy is a sum of 3 dim terms, good to (3 dim + 4) EPS
    # (|x|^2 + |y|^2) absolute, and |sqrt(d^2 + t) - d| <= |t| / d.  A mean of distances errs by at most the largest of them, E_i, and
    # s_i then by (ea + eb) (1 + |s|) / max(a, b) <= 4 E_i / max(a_i, b_i); the device's own bound comes on top (twice: the reference's)
    X64 = x.astype(np.float64)
    lab = labels[0]
    ref = sr.run(x, 0, (lab - 2) // 5, [3])[0]
    D = sr.distances(x, 0)
    n2 = (X64 * X64).sum(1)
    with np.errstate(divide='ignore', invalid='ignore'):
        E = np.where(D > 0, (3 * 12 + 4) * sr.EPS * (n2[:, None] + n2[None, :]) / D, 0.0).max(1)
    loose = (4 * E / np.maximum(ref['a'], ref['b'])).mean() + 2 * sr.bounds(x, 0, ref)['score']
    got = m.silhouette(z, lab)['score']
    want = metrics.silhouette_score(X64, lab)
    print("sklearn: |difference| %.3g, bound %.3g" % (abs(got - want), loose))
    assert abs(got - want) <= loose
