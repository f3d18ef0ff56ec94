"""The kernel two-sample test on the device (avae_mmd, avae_mmd_relabel, VAE.mmd) against the float64 reference of tests/mmd_ref.py.

No tolerance here is measured: the U sums, the statistic and the witness must agree within twice the bounds mmd_ref derives from
operation counts (twice: the reference errs as well); the counts are exact, the generated masks equal the reference's bit for bit, and
the p-value is exactly equal on the cases whose reference has the margin (mmd_ref.has_margins, asserted on the reference alone for
every case).  Every output must be the same BITS for every mmd_chunk, that is for every tile shape and every grouping of the
relabelings into passes.  Rows are padded with NaN rows, rows that no comparison takes hold NaN, and every output and the mask words
behind the call's own are guarded by a sentinel."""
import ctypes as C

import numpy as np
import pytest

import mmd_ref as mr
from test_gpu_kmeans import _model, _ptr

pytestmark = pytest.mark.gpu

SENT_I, SENT_F, SENT_W = -77, 123.0, 0x5A5A5A5A5A5A5A5A
OUTS = ('stat', 'pvalue', 'counts', 'sums', 'ull', 'witness', 'stat_out')
_REF = {}


def _cfg(kernel, metric, G, P, gamma=(), nbw=None, reserved=0):
    from argsim_amd import lib
    cfg = lib.AvaeMmdConfig(kernel=kernel, metric=metric, G=G, P=P, nbw=len(gamma) if nbw is None else nbw, reserved=reserved)
    for b, v in enumerate(gamma):
        cfg.gamma[b] = v
    return cfg


def _words(w, extra=4):
    """uint64 words -> an int64 tensor on the device with `extra` sentinel words behind them"""
    import torch
    flat = np.concatenate([np.ascontiguousarray(w, '<u8').reshape(-1), np.full(extra, SENT_W, '<u8')])
    return torch.from_numpy(flat.view(np.int64)).to(_model().device)


def _host_words(t, shape):
    v = t.cpu().numpy().view('<u8')
    n = int(np.prod(shape))
    assert (v[n:] == SENT_W).all(), "mask words behind the call's own were written"
    return v[:n].reshape(shape)


def _relabel(N, valid, a0, P, seed):
    """avae_mmd_relabel -> the device tensor of (G, 1 + P, W) words (+ sentinels) and its host copy"""
    m = _model()
    G, W = len(valid), (N + 63) // 64
    inA = np.full((G, 1 + P, W), SENT_W, '<u8')
    inA[:, 0] = mr.pack(a0)
    din, dv = _words(inA), _words(mr.pack(valid))
    m._stream()
    m._ck(m._l.avae_mmd_relabel(m._h, N, G, P, _ptr(dv), _ptr(din), C.c_uint64(seed)))
    _host_words(dv, (G, W))
    return din, _host_words(din, (G, 1 + P, W))


def _mmd(x, cfg, valid, din, chunk=0, skip=(), N=None, expect_fail=False):
    """avae_mmd on NaN-padded rows and sentinel-guarded outputs -> dict of numpy arrays; skip: optional outputs passed as null"""
    import torch
    m = _model()
    dev = m.device
    x = np.ascontiguousarray(x, np.float32)
    n_rows, dim = x.shape
    N = n_rows if N is None else N
    G, P1 = (max(cfg.G, 1), 1 + max(cfg.P, 0)) if cfg is not None else (1, 1)
    dx = torch.full((n_rows + 3, dim), float('nan'), dtype=torch.float32, device=dev)
    dx[:n_rows] = torch.as_tensor(x).to(dev)
    dv = _words(mr.pack(valid))
    bufs = dict(stat=(G * P1, torch.float64), pvalue=(G, torch.float64), counts=(2 * G, torch.int32), sums=(2 * G * P1, torch.float64),
                ull=(G, torch.float64), witness=(G * n_rows, torch.float64), stat_out=(1, torch.int32))
    t = {n: torch.full((s + 8,), SENT_I if dt == torch.int32 else SENT_F, dtype=dt, device=dev) for n, (s, dt) in bufs.items()}
    assert m._l.avae_set_option(m._h, b'mmd_chunk', chunk) == 0
    m._stream()
    try:
        rc = m._l.avae_mmd(m._h, _ptr(dx), N, dim, C.byref(cfg) if cfg is not None else None, _ptr(dv), _ptr(din),
                           *[None if n in skip else _ptr(t[n]) for n in OUTS])
    finally:
        m._l.avae_set_option(m._h, b'mmd_chunk', 0)
    torch.cuda.synchronize()
    out = {}
    for n, (s, dt) in bufs.items():
        v = t[n].cpu().numpy()
        sent = SENT_I if dt == torch.int32 else SENT_F
        assert (v[s:] == sent).all(), n
        if n in skip or expect_fail:
            assert (v == sent).all(), n
        out[n] = v[:s]
    if expect_fail:
        assert rc != 0
        return m._l.avae_last_error(m._h).decode()
    assert rc == 0, m._l.avae_last_error(m._h)
    for n, shape in (('stat', (G, P1)), ('counts', (G, 2)), ('sums', (G, P1, 2)), ('witness', (G, n_rows))):
        out[n] = out[n].reshape(shape)
    return out


def _close(got, want, bound, what):
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    err = np.abs(got - want)
    worst = np.max(err / (2 * bound + 1e-300)) if err.size else 0.0
    print("%s: error / (2 bound) %.3g" % (what, worst))
    assert np.isfinite(got).all(), what
    assert (err <= 2 * bound).all(), (what, float(err.max()), float(np.max(bound)))


# ---------------------------------------------------------------- the cases
# id -> N, dim, G, P, left-out rows, the last comparison in word 0 only, (m, n) of comparison 0, duplicate rows
CASES = {
    'n4': (4, 4, 1, 0, False, False, (2, 2), False),
    'n63': (63, 36, 1, 1, True, False, None, False),
    'n64': (64, 4, 3, 62, True, True, None, True),
    'n65': (65, 128, 1, 63, False, False, (20, 45), True),
    'n130': (130, 36, 3, 64, True, True, None, False),
    'n200': (200, 36, 3, 199, True, True, (70, 63), True),
}
KERNELS = {'rbf1': (0, (0.02,)), 'rbf3': (0, (0.005, 0.03, 0.2)), 'energy': (1, ())}


def _case(name, metric):
    """-> x (N, dim) with NaN in the rows nobody takes, valid, a0 (G, N) bool, P, the seed of the relabelings"""
    N, dim, G, P, left, oneword, sizes, dup = CASES[name]
    seed = sum(name.encode())
    x = mr.rows(N, dim, seed, shift=0.4)
    valid, a0 = mr.split(N, G, seed + 1, left, oneword, sizes)
    on = np.flatnonzero(valid.any(0))
    if dup and len(on) > 6:
        x[on[5]] = x[on[1]]
        x[on[-1]] = x[on[1]]
    if metric == 1 and len(on) > 4:
        x[on[3]] = 0.0                                   # a zero row stays zero under the cosine
    x[~valid.any(0)] = np.nan
    return x, valid, a0, P, seed + 2


def _reference(name, kname, metric):
    key = (name, kname, metric)
    if key not in _REF:
        x, valid, a0, P, seed = _case(name, metric)
        kernel, gamma = KERNELS[kname]
        masks = mr.relabel(valid, a0, P, seed)
        ref = mr.run(x, kernel, metric, gamma, valid, masks)
        bd = mr.bounds(x, kernel, metric, gamma, valid, masks, ref)
        _REF[key] = (masks, ref, bd)
    return _REF[key]


def _against(out, ref, bd, valid):
    assert out['stat_out'][0] == 0
    assert np.array_equal(out['counts'], ref['counts'])
    _close(out['sums'], ref['sums'], bd['sums'], 'U_AA, U_BB')
    _close(out['ull'], ref['ull'], bd['ull'], 'U_LL')
    _close(out['stat'], ref['stat'], bd['stat'], 'stat')
    _close(out['witness'], ref['witness'], bd['witness'], 'witness')
    assert (out['witness'][~valid] == 0).all()
    assert mr.has_margins(ref, bd)
    assert np.array_equal(out['pvalue'], ref['pvalue'])


@pytest.mark.parametrize('metric', [0, 1], ids=['euc', 'cos'])
@pytest.mark.parametrize('kname', list(KERNELS))
@pytest.mark.parametrize('name', list(CASES))
def test_shapes_against_the_reference(name, kname, metric):
    """N in {4, 63, 64, 65, 130, 200}, dim in {4, 36, 128}, G in {1, 3}, P in {0, 1, 62, 63, 64, 199}, m = n = 2 and m != n, left-out rows,
    a comparison inside one word, duplicate rows, a zero row under the cosine; the masks come from avae_mmd_relabel"""
    x, valid, a0, P, seed = _case(name, metric)
    kernel, gamma = KERNELS[kname]
    masks, ref, bd = _reference(name, kname, metric)
    din, got = _relabel(len(x), valid, a0, P, seed)
    # (relabeling 0 is the caller's own a0, whose bits outside valid are ignored; the generated ones hold no such bit)
    assert np.array_equal(got[:, 1:], mr.pack(masks)[:, 1:]) and np.array_equal(got[:, 0] & mr.pack(valid), mr.pack(masks)[:, 0])
    out = _mmd(x, _cfg(kernel, metric, len(valid), P, gamma), valid, din)
    _against(out, ref, bd, valid)


def test_relabel_one_row_short_of_a_word():
    """N = 200: every row valid and m = 63, then 127 valid rows of which m = 64; bits beyond N in valid and inA are ignored"""
    N, P = 200, 9
    for nvalid, m in ((200, 63), (127, 64), (200, 199), (129, 1)):
        valid = np.zeros((2, N), bool)
        valid[:, np.random.default_rng(nvalid).permutation(N)[:nvalid]] = True
        a0 = np.zeros((2, N), bool)
        for g in range(2):
            a0[g, np.flatnonzero(valid[g])[g:g + m]] = True
        _, got = _relabel(N, valid, a0, P, 77)
        assert np.array_equal(got[:, 1:], mr.pack(mr.relabel(valid, a0, P, 77))[:, 1:]), (nvalid, m)
    # garbage beyond N and outside valid changes nothing
    m_ = _model()
    vw, aw = mr.pack(valid), mr.pack(a0)
    vw[:, -1] |= np.uint64(0xFF) << np.uint64(56)
    aw2 = aw | ~vw
    inA = np.full((2, 1 + P, vw.shape[1]), SENT_W, '<u8')
    inA[:, 0] = aw2
    din, dv = _words(inA), _words(vw)
    m_._ck(m_._l.avae_mmd_relabel(m_._h, N, 2, P, _ptr(dv), _ptr(din), C.c_uint64(77)))
    assert np.array_equal(_host_words(din, inA.shape)[:, 1:], got[:, 1:])


# ---------------------------------------------------------------- the plan does not show
@pytest.mark.parametrize('kname,metric', [('rbf3', 0), ('energy', 1)])
def test_plan_independence(kname, metric):
    """G (1 + P) = 600 relabelings over 200 rows: with mmd_chunk 1 a pass per relabeling at TI = 8, 5 and 16 ragged passes that straddle
    the comparisons at TI = 8 and 16, 40 and 64 the two larger row tiles; 0 is the planner's own"""
    x, valid, a0, P, seed = _case('n200', metric)
    kernel, gamma = KERNELS[kname]
    masks, ref, bd = _reference('n200', kname, metric)
    din = _words(mr.pack(masks))
    cfg = _cfg(kernel, metric, len(valid), P, gamma)
    base = _mmd(x, cfg, valid, din)
    _against(base, ref, bd, valid)
    for chunk in (1, 5, 16, 40, 64, 0):
        out = _mmd(x, cfg, valid, din, chunk=chunk)
        for n in OUTS:
            assert out[n].tobytes() == base[n].tobytes(), (chunk, n)


def test_optional_outputs_as_null():
    x, valid, a0, P, seed = _case('n130', 0)
    masks, ref, bd = _reference('n130', 'rbf1', 0)
    din = _words(mr.pack(masks))
    cfg = _cfg(0, 0, 3, P, KERNELS['rbf1'][1])
    full = _mmd(x, cfg, valid, din)
    out = _mmd(x, cfg, valid, din, skip=('sums', 'ull', 'witness'))
    for n in ('stat', 'pvalue', 'counts', 'stat_out'):
        assert out[n].tobytes() == full[n].tobytes(), n


def test_a_relabeling_of_the_wrong_size_is_reported():
    x, valid, a0, P, seed = _case('n130', 0)
    masks, ref, bd = _reference('n130', 'energy', 0)
    bad = masks.copy()
    g, p = 1, 7
    i = np.flatnonzero(valid[g] & ~bad[g, p])[0]
    bad[g, p, i] = True
    bad[2, 3, np.flatnonzero(valid[2] & bad[2, 3])[0]] = False
    out = _mmd(x, _cfg(1, 0, 3, P), valid, _words(mr.pack(bad)))
    assert out['stat_out'][0] == 1 + g * (1 + P) + p
    keep = np.ones((3, 1 + P), bool)
    keep[g, p] = keep[2, 3] = False
    _close(out['stat'][keep], ref['stat'][keep], bd['stat'][keep], 'the other statistics')


def test_refusals_leave_the_outputs_alone():
    x, valid, a0, P, seed = _case('n65', 0)
    masks, _, _ = _reference('n65', 'rbf1', 0)
    din = _words(mr.pack(masks))
    g1 = (0.02,)
    texts = [_mmd(x, None, valid, din, expect_fail=True)]
    for N in (1, (1 << 17) + 1):
        texts.append(_mmd(x, _cfg(0, 0, 1, P, g1), valid, din, N=N, expect_fail=True))
    texts.append(_mmd(x[:, :6], _cfg(0, 0, 1, P, g1), valid, din, expect_fail=True))
    texts.append(_mmd(np.zeros((65, 1028), np.float32), _cfg(0, 0, 1, P, g1), valid, din, expect_fail=True))
    for G in (0, 65):
        texts.append(_mmd(x, _cfg(0, 0, G, 0, g1), valid, din, expect_fail=True))
    for G, Pb in ((1, -1), (1, 16384), (64, 256)):
        texts.append(_mmd(x, _cfg(0, 0, G, Pb, g1), valid, din, expect_fail=True))
    for nbw in (0, 9):
        texts.append(_mmd(x, _cfg(0, 0, 1, P, g1, nbw=nbw), valid, din, expect_fail=True))
    for gam in ((0.0,), (-1.0,), (float('inf'),), (float('nan'),), (0.5, 0.0)):
        texts.append(_mmd(x, _cfg(0, 0, 1, P, gam), valid, din, expect_fail=True))
    for kernel, metric, reserved in ((2, 0, 0), (0, 2, 0), (0, 0, 1)):
        texts.append(_mmd(x, _cfg(kernel, metric, 1, P, g1, reserved=reserved), valid, din, expect_fail=True))
    # a sample of fewer than 2 rows: found on the device, refused before anything is written
    for keep_a, keep_b in ((1, 5), (5, 1), (0, 9)):
        a1 = np.zeros_like(a0)
        v1 = np.zeros_like(valid)
        v1[0, :keep_a + keep_b] = True
        a1[0, :keep_a] = True
        t = _mmd(x, _cfg(1, 0, 1, 0), v1, _words(mr.pack(a1)[:, None, :]), expect_fail=True)
        assert 'at least 2' in t
        texts.append(t)
    assert all(t.startswith('mmd') for t in texts) and len(set(texts)) >= 12, texts
    m = _model()
    dv = _words(mr.pack(valid))
    for args in ((1, 1, 0), (65, 0, 0), (65, 1, -1), (65, 64, 256)):
        assert m._l.avae_mmd_relabel(m._h, *args, _ptr(dv), _ptr(din), C.c_uint64(0)) != 0
    assert m._l.avae_mmd_relabel(m._h, 65, 1, 0, None, _ptr(din), C.c_uint64(0)) != 0
    assert m._l.avae_set_option(m._h, b'mmd_chunk', -1) != 0


# ---------------------------------------------------------------- the Python layer, end to end
def _groups(valid, a0):
    return np.where(valid, np.where(a0, 0, 1), -1).astype(np.int64)


def test_vae_mmd_end_to_end():
    x, valid, a0, P, _ = _case('n130', 0)
    x = np.nan_to_num(x[:, :34])                          # 34 columns: the wrapper pads to 36
    gamma = (0.01, 0.05)
    masks = mr.relabel(valid, a0, 19, 5)
    ref = mr.run(x, 0, 0, gamma, valid, masks)
    bd = mr.bounds(x, 0, 0, gamma, valid, masks, ref)
    assert mr.has_margins(ref, bd)
    m = _model()
    out = m.mmd(x, _groups(valid, a0), 'rbf', gamma, 'euclidean', 19, 5, return_null=True, return_witness=True)
    _close(out['stat'], ref['stat'][:, 0], bd['stat'][:, 0], 'stat')
    _close(out['null'], ref['stat'][:, 1:], bd['stat'][:, 1:], 'null')
    _close(out['witness'], ref['witness'], bd['witness'], 'witness')
    assert np.array_equal(out['pvalue'], ref['pvalue']) and np.array_equal(out['m'], ref['counts'][:, 0]) and np.array_equal(out['n'], ref['counts'][:, 1])
    one = m.mmd(x, _groups(valid, a0)[1], 'rbf', gamma, 'euclidean', 19, 5)
    assert one['stat'].shape == () and one['m'] == ref['counts'][1, 0]
    # comparison 1 alone is comparison 0 of its own call: other relabelings, the same observed statistic
    _close(one['stat'], ref['stat'][1, 0], bd['stat'][1, 0], 'stat of a single comparison')


def test_vae_mmd_numpy_and_device_rows_give_the_same_bits():
    import torch
    x, valid, a0, P, _ = _case('n65', 1)
    x = np.nan_to_num(x)
    m = _model()
    a = m.mmd(x, _groups(valid, a0), 'energy', 'median', 'cosine', 29, 1, True, True)
    b = m.mmd(torch.as_tensor(x).to(m.device), _groups(valid, a0), 'energy', 'median', 'cosine', 29, 1, True, True)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_vae_mmd2_and_prior_match_end_to_end():
    m = _model()
    xa, xb = mr.rows(40, 8, 1), mr.rows(50, 8, 2) * np.float32(1.5)
    ref = mr.mmd2(xa, xb, 1, 0, (), 39, 3)
    x = np.concatenate([xa, xb])
    valid = np.ones((1, 90), bool)
    bd = mr.bounds(x, 1, 0, (), valid, mr.relabel(valid, np.arange(90)[None, :] < 40, 39, 3), ref)
    out = m.mmd2(xa, xb, 'energy', n_perm=39, seed=3, return_null=True)
    _close(out['stat'], ref['stat'][0, 0], bd['stat'][0, 0], 'mmd2 stat')
    _close(out['null'], ref['stat'][0, 1:], bd['stat'][0, 1:], 'mmd2 null')
    assert mr.has_margins(ref, bd) and out['pvalue'] == ref['pvalue'][0] and (out['m'], out['n']) == (40, 50)
    # prior_match: z against N(0, I) rows of default_rng(seed), the rbf kernel at the median bandwidth
    z = mr.rows(60, 8, 4) * np.float32(0.5)
    prior = np.random.default_rng(6).standard_normal((60, 8)).astype(np.float32)
    gamma = (mr.median_gamma(np.concatenate([z, prior])),)
    ref = mr.mmd2(z, prior, 0, 0, gamma, 49, 6)
    valid = np.ones((1, 120), bool)
    bd = mr.bounds(np.concatenate([z, prior]), 0, 0, gamma, valid, mr.relabel(valid, np.arange(120)[None, :] < 60, 49, 6), ref)
    out = m.prior_match(z, 49, 6)
    _close(out['stat'], ref['stat'][0, 0], bd['stat'][0, 0], 'prior_match stat')
    assert mr.has_margins(ref, bd) and out['pvalue'] == ref['pvalue'][0] and out['pvalue'] <= 0.05
