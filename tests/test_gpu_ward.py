"""Ward clustering on the device (avae_ward, avae_ward_cut, VAE.ward / ward_cut / cluster_eval) against the float64 reference of
tests/ward_ref.py.

No tolerance here is measured.  A stored pair value is ONE rounding to fp32 of a double result, so (a) where every merge of the
reference is decided by a relative gap >= 2^-20 (ward_ref.CASES; asserted on the CPU by tests/test_ward.py) the device's merge list
is the reference's exactly and its values are within one fp32 ulp (the double summation order may differ from numpy's); (b) for ANY
input the device's own merge list carries a certificate that ward_ref.follow evaluates in float64: the chosen pair's value is within
(1 + 2^-21) of the minimum over all alive pairs (two roundings of 2^-24 and the double error leave 2^-23), the returned delta is
within 2^-22 of the float64 value, and the heights do not decrease beyond the same factor (Ward's distance is reducible).  Both
kernel forms run every case and must agree bit for bit.  Operands are padded with NaN rows and outputs guarded by a sentinel."""
import ctypes as C

import numpy as np
import pytest

import ward_ref as wr

pytestmark = pytest.mark.gpu

KEYS = ('dim_tgt', 'dim_emb', 'dim_rep', 'rnn_layers', 'accelerate', 'learn_rate', 'bos', 'eos')
SENT_I, SENT_F = -77, 123.0
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


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else None


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _carr(a):
    return (C.c_int32 * len(a))(*[int(v) for v in a])


def _raw(x, dim, off, G, pair, delta, size, reserved=(0, 0), null_cfg=False):
    """the C entry as it stands -> its return code"""
    from argsim_amd import lib
    m = _model()
    wc = lib.AvaeWardConfig((C.c_int32 * 2)(*reserved))
    m._stream()
    return m._l.avae_ward(m._h, x, dim, off, G, None if null_cfg else C.byref(wc), pair, delta, size)


def _ward(x, sizes, form=0):
    """avae_ward on NaN-padded rows and sentinel-guarded outputs -> per group (pair, delta, size) numpy, and the raw outputs"""
    import torch
    m = _model()
    x = np.ascontiguousarray(x, np.float32)
    off, G, N = _off(sizes), len(sizes), x.shape[0]
    assert off[-1] == N
    dx = torch.full((N + 3, x.shape[1]), float('nan'), dtype=torch.float32, device=m.device)
    dx[:N] = torch.as_tensor(x).to(m.device)
    M = N - G
    pair = torch.full((2 * M + 4,), SENT_I, dtype=torch.int32, device=m.device)
    delta = torch.full((M + 4,), SENT_F, dtype=torch.float32, device=m.device)
    size = torch.full((M + 4,), SENT_I, dtype=torch.int32, device=m.device)
    try:
        m.set_option('ward_form', form)
        m._ck(_raw(_ptr(dx), x.shape[1], _carr(off), G, _ptr(pair), _ptr(delta), _ptr(size)))
    finally:
        m.set_option('ward_form', 0)
    pair, delta, size = pair.cpu().numpy(), delta.cpu().numpy(), size.cpu().numpy()
    assert (pair[2 * M:] == SENT_I).all() and (delta[M:] == SENT_F).all() and (size[M:] == SENT_I).all()
    pair = pair[:2 * M].reshape(M, 2)
    out = []
    for g in range(G):
        lo, hi = off[g] - g, off[g + 1] - g - 1
        out.append((pair[lo:hi], delta[lo:hi], size[lo:hi]))
    return out, (pair, delta[:M], size[:M])


def _same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)) for x, y in zip(a, b))


def _run(case, form):
    """one group alone in the given form (cached and shared: never modified)"""
    if (case, form) not in _RUNS:
        x = wr.case_inputs(case)
        out = _ward(x, [x.shape[0]], form)[0][0]
        for a in out:
            a.setflags(write=False)
        _RUNS[case, form] = out
    return _RUNS[case, form]


def _ref(case):
    if ('ref', case) not in _RUNS:
        _RUNS['ref', case] = wr.ward(wr.case_inputs(case))
    return _RUNS['ref', case]


def _complete(pair, size, n):
    """n - 1 merges of slots a < b, every slot but 0 retired exactly once, sizes that add up"""
    assert pair.shape == (n - 1, 2)
    assert (pair[:, 0] >= 0).all() and (pair[:, 0] < pair[:, 1]).all() and (pair[:, 1] < n).all()
    assert sorted(pair[:, 1].tolist()) == list(range(1, n))
    cnt = np.ones(n, np.int64)
    for t, (a, b) in enumerate(pair):
        assert cnt[a] > 0 and cnt[b] > 0, t
        cnt[a] += cnt[b]
        cnt[b] = 0
        assert size[t] == cnt[a], t


def _check_certificate(x, pair, delta, size):
    n = x.shape[0]
    _complete(pair, size, n)
    chosen, least = wr.follow(x, pair)
    print("worst chosen / least - 1 = %.3g, worst |delta - chosen| / chosen = %.3g" % (
        float(np.max(chosen / np.where(least > 0, least, 1) - 1)), float(np.max(np.abs(delta - chosen) / np.where(chosen > 0, chosen, 1)))))
    assert (chosen <= (1 + 2.0 ** -21) * least).all()
    assert (np.abs(delta.astype(np.float64) - chosen) <= 2.0 ** -22 * chosen).all()
    assert (chosen[:-1] <= (1 + 2.0 ** -21) * chosen[1:]).all()
    assert (delta[:-1].astype(np.float64) <= (1 + 2.0 ** -21) * delta[1:].astype(np.float64)).all()


@pytest.mark.parametrize('form', [1, 2])
@pytest.mark.parametrize('case', wr.CASES, ids=wr.CASE_IDS)
def test_exact_cases(case, form):
    pair, delta, size = _run(case, form)
    ref = _ref(case)
    assert np.array_equal(pair, ref['pair']) and np.array_equal(size, ref['size'])
    ulp = np.spacing(ref['delta'])
    assert (np.abs(delta.astype(np.float64) - ref['delta'].astype(np.float64)) <= ulp).all()


@pytest.mark.parametrize('case', wr.CASES + [wr.NEAR_TIES], ids=wr.CASE_IDS + ['lattice'])
def test_certificate(case):
    for form in (1, 2):
        _check_certificate(wr.case_inputs(case), *_run(case, form))


def test_certificate_beyond_the_one_workgroup_threshold():
    """1100 rows: the planner's own choice is the launch-per-merge form; the one-workgroup form gives the same bits"""
    x = wr.case_inputs(wr.BIG)
    own = _ward(x, [x.shape[0]], 0)[0][0]
    _check_certificate(x, *own)
    assert _same_bits(own, _ward(x, [x.shape[0]], 2)[0][0])
    assert _same_bits(own, _ward(x, [x.shape[0]], 1)[0][0])
    small = wr.case_inputs(wr.CASES[0])
    assert _same_bits(_ward(small, [small.shape[0]], 0)[0][0], _run(wr.CASES[0], 1))


def test_tie_rule():
    m = 9
    x = wr.tie_inputs(m)
    ref = wr.ward(x)
    assert not ref['delta'][:3 * m].any() and ref['delta'][3 * m] > 0
    for form in (1, 2):
        pair, delta, size = _ward(x, [x.shape[0]], form)[0][0]
        assert np.array_equal(pair[:3 * m], ref['pair'][:3 * m])
        assert np.array_equal(delta[:3 * m].view(np.uint32), np.zeros(3 * m, np.uint32))          # +0
        assert np.array_equal(size[:3 * m], ref['size'][:3 * m])
        _check_certificate(x, pair, delta, size)


@pytest.mark.parametrize('case', wr.CASES + [wr.NEAR_TIES], ids=wr.CASE_IDS + ['lattice'])
def test_forms_give_the_same_bits(case):
    assert _same_bits(_run(case, 1), _run(case, 2))
    x = wr.case_inputs(case)
    assert _same_bits(_ward(x, [x.shape[0]], 1)[0][0], _run(case, 1))          # and the same call again


def test_a_group_does_not_depend_on_its_companions():
    sizes = wr.GROUP_SIZES
    r = np.random.default_rng(17)
    xs = [wr.planted(n, 36, 100 + n) for n in sizes]
    alone = [_ward(x, [n])[0][0] for x, n in zip(xs, sizes)]
    for form in (1, 2):
        for order in (list(range(len(sizes))), list(r.permutation(len(sizes)))):
            got, raw = _ward(np.concatenate([xs[i] for i in order]), [sizes[i] for i in order], form)
            for slot, i in enumerate(order):
                assert _same_bits(got[slot], alone[i]), (form, order, i)
                assert got[slot][0].shape == (sizes[i] - 1, 2)
    # a call of single rows is legal and writes nothing
    got, raw = _ward(np.concatenate([xs[0], xs[0], xs[0]]), [1, 1, 1])
    assert all(a.size == 0 for a in raw)


def test_cut():
    import torch
    m = _model()
    sizes = [1, 65, 200, 2]
    xs = [wr.planted(n, 36, 200 + n) for n in sizes]
    got, (pair, _, _) = _ward(np.concatenate(xs), sizes)
    off, G, N = _off(sizes), len(sizes), sum(sizes)
    dp = torch.as_tensor(pair).to(m.device)
    for ks in ([1, 1, 1, 1], [1, 65, 200, 2], [1, 7, 5, 1]):
        label = torch.full((N + 4,), SENT_I, dtype=torch.int32, device=m.device)
        m._stream()
        m._ck(m._l.avae_ward_cut(m._h, _ptr(dp), _carr(off), G, _carr(ks), _ptr(label)))
        label = label.cpu().numpy()
        assert (label[N:] == SENT_I).all()
        for g in range(G):
            assert np.array_equal(label[off[g]:off[g + 1]], wr.cut(got[g][0], sizes[g], ks[g])), (ks, g)
            assert len(set(label[off[g]:off[g + 1]].tolist())) == ks[g]


def test_cluster_eval_finds_planted_clusters():
    from argsim_amd import cluster
    m = _model()
    r = np.random.default_rng(3)
    gold = r.integers(0, 4, 300)
    gold[:4] = np.arange(4)
    groups = np.array(['a'] * 120 + ['b'] * 180)[r.permutation(300)]
    z = (40.0 * r.standard_normal((4, 36))[gold] + r.standard_normal((300, 36))).astype(np.float32)
    res = m.cluster_eval(z, gold, groups)
    assert set(res) == {'a', 'b'} and all(v == (1.0, 1.0) for v in res.values()), res
    assert m.cluster_eval(z[:, :35], gold) == {0: (1.0, 1.0)}                                    # 35 columns: padded with a zero column
    tree = m.ward(z, groups)
    for key in tree['keys']:
        g = tree['groups'][key]
        assert np.array_equal(groups[g['rows']], np.repeat(key, len(g['rows']))) and g['Z'].shape == (len(g['rows']) - 1, 4)
        _check_certificate(z[g['rows']], g['pair'], g['delta'], g['size'])
    labels = m.ward_cut(tree, 4)
    assert all(cluster.adjusted_rand(gold[tree['groups'][k]['rows']], labels[k]) == 1.0 for k in tree['keys'])


def test_eval_cluster_prints_the_reference_format(tmp_path, capsys):
    from argsim_amd import eval_cluster
    r = np.random.default_rng(9)
    names = np.array(['%s-%s-%d' % (t, s, q) for t in ('abortion', 'gun') for s in ('p', 'c') for q in (1, 2) for _ in range(12)])
    _, ids = np.unique(names, return_inverse=True)
    z = (30.0 * r.standard_normal((8, 16))[ids] + r.standard_normal((len(names), 16))).astype(np.float32)
    np.save(str(tmp_path / 'z.npy'), z)
    np.save(str(tmp_path / 'l.npy'), names)
    args = ['--inputs', str(tmp_path / 'z.npy'), '--labels', str(tmp_path / 'l.npy')]
    eval_cluster.main(args + ['--by', 'topic'])
    lines = capsys.readouterr().out.strip().split('\n')
    assert lines == ["{:<20s}\tARS: {:.4F}\tV_MSR: {:.4f}".format(t, 1.0, 1.0) for t in ('abortion', 'gun')]
    eval_cluster.main(args + ['--by', 'all'])
    lines = capsys.readouterr().out.strip().split('\n')
    assert len(lines) == 4 and lines[0].startswith("TOPIC:  ARS: ") and "\tV_MSR: " in lines[0]       # 2 clusters of 8 centres: any score
    assert lines[1] == "REASON: ARS: 1.0000\tV_MSR: 1.0000"
    assert lines[2:] == ["{:<20s}: ARS: 1.0000\tV_MSR: 1.0000".format(t) for t in ('abortion', 'gun')]


def test_a_row_that_is_not_finite_gives_a_complete_tree():
    x = wr.case_inputs(wr.CASES[1]).copy()
    x[17, 5] = np.nan
    n = x.shape[0]
    for form in (1, 2):
        pair, delta, size = _ward(x, [n], form)[0][0]
        _complete(pair, size, n)
    x[40, 0] = np.inf
    x[3] = np.nan
    other = wr.planted(65, 36, 165)
    got, _ = _ward(np.concatenate([x, other]), [n, 65])
    _complete(got[0][0], got[0][2], n)
    assert _same_bits(got[1], _ward(other, [65])[0][0])          # the companion group is untouched by it


def test_errors_have_text():
    import torch
    m = _model()
    dev = m.device
    x = torch.ones((8, 8), dtype=torch.float32, device=dev)
    pair = torch.full((16,), SENT_I, dtype=torch.int32, device=dev)
    delta = torch.full((8,), SENT_F, dtype=torch.float32, device=dev)
    size = torch.full((8,), SENT_I, dtype=torch.int32, device=dev)
    label = torch.full((8,), SENT_I, dtype=torch.int32, device=dev)
    ok = dict(x=_ptr(x), dim=8, off=_carr([0, 3, 8]), G=2, pair=_ptr(pair), delta=_ptr(delta), size=_ptr(size))
    huge = _carr(np.arange(129) * (1 << 15))                  # 128 groups of 2^15 rows: 512 GiB of pair values
    bad = [dict(x=None), dict(off=None), dict(pair=None), dict(delta=None), dict(null_cfg=True), dict(G=0), dict(G=(1 << 16) + 1),
           dict(off=_carr([1, 3, 8])), dict(off=_carr([0, 3, 3])), dict(off=_carr([0, 5, 4])), dict(off=_carr([0, (1 << 15) + 1]), G=1),
           dict(dim=6), dict(dim=0), dict(dim=1028), dict(x=_ptr(x, 4)), dict(reserved=(1, 0)), dict(reserved=(0, 1)),
           dict(off=huge, G=128, dim=1024)]
    for kw in bad:
        assert _raw(**dict(ok, **kw)) != 0, kw
        assert len(m._l.avae_last_error(m._h)) > 5, kw
    assert b'bytes' in m._l.avae_last_error(m._h)        # the workspace refusal names its size
    cut = lambda *a: m._l.avae_ward_cut(m._h, *a)
    off, k = _carr([0, 3, 8]), _carr([1, 2])
    for args in ((None, off, 2, k, _ptr(label)), (_ptr(pair), None, 2, k, _ptr(label)), (_ptr(pair), off, 2, None, _ptr(label)),
                 (_ptr(pair), off, 2, k, None), (_ptr(pair), off, 0, k, _ptr(label)), (_ptr(pair), _carr([0, 3, 3]), 2, k, _ptr(label)),
                 (_ptr(pair), off, 2, _carr([0, 2]), _ptr(label)), (_ptr(pair), off, 2, _carr([1, 6]), _ptr(label))):
        assert cut(*args) != 0, args
        assert len(m._l.avae_last_error(m._h)) > 5, args
    torch.cuda.synchronize(dev)
    assert (pair == SENT_I).all() and (delta == SENT_F).all() and (size == SENT_I).all() and (label == SENT_I).all()      # outputs untouched
    assert _raw(**ok) == 0                                # the handle stays usable
    assert _raw(**dict(ok, size=None)) == 0               # size is optional
    torch.cuda.synchronize(dev)
    assert (pair[:12] != SENT_I).all() and (pair[12:] == SENT_I).all()
    with pytest.raises(RuntimeError):
        m.set_option('ward_form', 3)
