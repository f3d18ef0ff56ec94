"""The float64 reference of the kernel two-sample test (tests/mmd_ref.py) against a brute-force restatement and the textbook identities,
the generated relabelings, the calibration and the power of the permutation test on the reference, the launch planner
(avae_debug_mmd_plan, host arithmetic), and the parts of the Python layer that need no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mmd_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the reference against itself
def _brute(x, kernel, metric, gamma, v, a):
    """U_AA, U_BB, U_LL by two Python loops, one pair at a time, the kernel value from the two rows alone"""
    X = mr.rows_of(x, metric)
    uaa = ubb = ull = 0.0
    for i in range(len(X)):
        for j in range(i + 1, len(X)):
            if not (v[i] and v[j]):
                continue
            d2 = 0.0
            for e in range(X.shape[1]):
                d2 += (X[i, e] - X[j, e]) ** 2
            k = -np.sqrt(d2) if kernel == 1 else sum(np.exp(-(g * d2)) for g in gamma)
            ull += k
            if a[i] and a[j]:
                uaa += k
            if not a[i] and not a[j]:
                ubb += k
    return uaa, ubb, ull


@pytest.mark.parametrize('kernel,metric', [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_reference_against_brute_force(kernel, metric):
    x = mr.rows(21, 4, 3)
    x[5] = x[9]
    x[20] = np.nan
    gamma = (0.3, 1.1)
    valid, a0 = mr.split(21, 2, 4)
    valid[:, 20] = False
    inA = mr.relabel(valid, a0, 3, 9)
    ref = mr.run(x, kernel, metric, gamma, valid, inA)
    for g in range(2):
        for p in range(4):
            uaa, ubb, ull = _brute(x, kernel, metric, gamma, valid[g], inA[g, p])
            assert np.allclose([uaa, ubb], ref['sums'][g, p], rtol=1e-12, atol=1e-13) and np.isclose(ull, ref['ull'][g], rtol=1e-12)
    assert np.isfinite(ref['stat']).all() and (ref['witness'][:, 20] == 0).all()


def test_biased_and_unbiased_identities():
    """the unbiased statistic from the full Gram sums: U = (sum of the block - its diagonal) / 2, and the biased V-statistic
    differs from it by the diagonal terms alone"""
    x = mr.rows(30, 6, 1, shift=0.5)
    v = np.ones((1, 30), bool)
    a = (np.arange(30) < 13)[None, :]
    ref = mr.run(x, 0, 0, (0.25,), v, a[:, None, :])
    K = ref['K']
    A, B = a[0], ~a[0]
    m, n = 13, 17
    kaa, kbb, kab = K[np.ix_(A, A)], K[np.ix_(B, B)], K[np.ix_(A, B)]
    unb = (kaa.sum() - np.trace(kaa)) / (m * (m - 1)) + (kbb.sum() - np.trace(kbb)) / (n * (n - 1)) - 2 * kab.mean()
    assert np.isclose(ref['stat'][0, 0], unb, rtol=1e-12)
    biased = kaa.mean() + kbb.mean() - 2 * kab.mean()
    # k(i, i) = 1: the biased form adds (1 - mean off-diagonal) / m per sample
    fix = (1 - (kaa.sum() - m) / (m * (m - 1))) / m + (1 - (kbb.sum() - n) / (n * (n - 1))) / n
    assert np.isclose(biased, unb + fix, rtol=1e-12)
    # the witness: mean to A minus mean to B without the row itself
    i = 4
    w = K[i, A & (np.arange(30) != i)].mean() - K[i, B].mean()
    assert np.isclose(ref['witness'][0, i], w, rtol=1e-12)


def test_energy_kernel_is_the_energy_distance():
    """m = n: 2 E|X - Y| - E|X - X'| - E|Y - Y'| with the unbiased within-sample means"""
    xa, xb = mr.rows(12, 4, 5), mr.rows(12, 4, 6) + np.float32(0.7)
    ref = mr.mmd2(xa, xb, 1, 0, (), 0, 0)
    d = lambda p, q: np.sqrt(((p[:, None, :].astype(np.float64) - q[None, :, :]) ** 2).sum(-1))
    e = 2 * d(xa, xb).mean() - d(xa, xa).sum() / (12 * 11) - d(xb, xb).sum() / (12 * 11)
    assert np.isclose(ref['stat'][0, 0], e, rtol=1e-12) and ref['pvalue'][0] == 1.0 and ref['counts'].tolist() == [[12, 12]]


def test_p_value_counts_ties_and_the_observed_split():
    s = np.array([[0.5, 0.5, 0.6, 0.1]])
    assert (1 + int((s[0, 1:] >= s[0, 0]).sum())) / 4 == 0.75


# ---------------------------------------------------------------- the masks
def test_pack_and_unpack():
    r = np.random.default_rng(0)
    for N in (4, 63, 64, 65, 200):
        b = r.random((2, 3, N)) < 0.5
        w = mr.pack(b)
        assert w.shape == (2, 3, (N + 63) // 64) and w.dtype == np.uint64 and np.array_equal(mr.unpack(w, N), b)
        assert int(w[0, 0, 0]) & 1 == int(b[0, 0, 0]) and (int(w[1, 2, -1]) >> ((N - 1) % 64)) & 1 == int(b[1, 2, N - 1])


def test_mix64_is_the_library_mixer():
    # splitmix64 from state 0: its first outputs are published with the algorithm
    assert int(mr.mix64(0)) == 0xE220A8397B1DCDAF and int(mr.mix64(0x9E3779B97F4A7C15)) == 0x6E789E6AA1B965F4


def test_generated_relabelings():
    N, P = 200, 20
    valid, a0 = mr.split(N, 3, 7)
    valid[1] = valid[0]
    a0[1] = a0[0]
    masks = mr.relabel(valid, a0, P, 11)
    for g in range(3):
        m = int((valid[g] & a0[g]).sum())
        assert (masks[g].sum(1) == m).all() and not (masks[g] & ~valid[g]).any()
        assert np.array_equal(masks[g, 0], valid[g] & a0[g])
        assert len({masks[g, p].tobytes() for p in range(1, 1 + P)}) == P
    # a function of (seed, g, p): fewer relabelings or fewer comparisons give the same masks where they overlap
    assert np.array_equal(mr.relabel(valid[:2], a0[:2], 5, 11), masks[:2, :6])
    assert np.array_equal(mr.relabel(valid, a0, P, 11), masks)
    other = mr.relabel(valid, a0, P, 12)
    assert not any(np.array_equal(other[0, p], masks[0, p]) for p in range(1, 1 + P))
    # two comparisons with the same valid rows and the same observed split still get different relabelings
    assert not any(np.array_equal(masks[0, p], masks[1, p]) for p in range(1, 1 + P))
    # a mask depends on the observed split only through m
    b0 = np.zeros_like(a0)
    for g in range(3):
        b0[g, np.flatnonzero(valid[g])[-int((valid[g] & a0[g]).sum()):]] = True
    assert np.array_equal(mr.relabel(valid, b0, P, 11)[:, 1:], masks[:, 1:])


# ---------------------------------------------------------------- calibration and power, on the reference
def _draw_test(kernel, seed, shift, P=199):
    x = mr.rows(40, 4, seed, shift)
    gamma = (mr.median_gamma(x),) if kernel == 0 else ()
    valid = np.ones((1, 40), bool)
    a0 = (np.arange(40) < 20)[None, :]
    K = mr.kernel_values(x, kernel, 0, gamma)
    inA = mr.relabel(valid, a0, P, seed)
    uaa, ubb, ull = mr.u_sums(K, valid[0], inA[0])
    s = mr.statistic(uaa, ubb, ull, 20, 20)
    return (1 + int((s[1:] >= s[0]).sum())) / (1 + P)


@pytest.mark.parametrize('kernel', [0, 1], ids=['rbf', 'energy'])
def test_calibration_under_the_null(kernel):
    """200 draws of two samples of 20 from the same N(0, I_4), P = 199: the share with p <= 0.05 is binomial(200, 0.05) / 200, mean 0.05 and
    sd 0.0154; [0.01, 0.10] is about 3 sd either side"""
    share = np.mean([_draw_test(kernel, 1000 + s, 0.0) <= 0.05 for s in range(200)])
    print("kernel %d: share of p <= 0.05 under the null %.3f" % (kernel, share))
    assert 0.01 <= share <= 0.10


@pytest.mark.parametrize('kernel', [0, 1], ids=['rbf', 'energy'])
def test_power_against_a_mean_shift(kernel):
    """a shift of 1 in every dimension: no relabeling reaches the observed statistic"""
    assert _draw_test(kernel, 5, 1.0) == 1 / 200


# ---------------------------------------------------------------- bounds and margins
def test_bounds_are_small_and_margins_hold_on_a_plain_case():
    x = mr.rows(65, 36, 2, shift=0.3)
    valid, a0 = mr.split(65, 1, 3)
    inA = mr.relabel(valid, a0, 5, 1)
    for kernel, gamma in ((0, (0.02, 0.1, 0.5)), (1, ())):
        ref = mr.run(x, kernel, 0, gamma, valid, inA)
        bd = mr.bounds(x, kernel, 0, gamma, valid, inA, ref)
        scale = np.abs(ref['sums']).max()
        assert 0 < bd['sums'].max() < 1e-9 * scale and 0 < bd['stat'].max() < 1e-9 and bd['witness'].max() < 1e-9
        assert mr.has_margins(ref, bd)
    same = dict(stat=np.array([[1.0, 1.0, 0.5]]))
    assert not mr.has_margins(same, dict(stat=np.full((1, 3), 1e-15)))


# ---------------------------------------------------------------- the Python layer
class _NoDevice:
    device = 'cpu'


def test_argument_errors():
    from argsim_amd import mmd as M
    z = mr.rows(20, 4, 0)
    g = (np.arange(20) % 2).astype(np.int64)
    v = _NoDevice()
    bad = [
        dict(z=z.astype(np.float64)), dict(z=z[0]), dict(z=z[:1], groups=g[:1]), dict(z=[[0.0] * 4] * 20),
        dict(groups=g.astype(np.float32)), dict(groups=g[:19]), dict(groups=np.zeros((65, 20), np.int64)), dict(groups=g + 1),
        dict(groups=np.where(np.arange(20) < 1, 0, 1)), dict(groups=np.where(np.arange(20) < 19, 0, 1)),
        dict(groups=np.where(np.arange(20) < 2, 0, -1)),
        dict(kernel='linear'), dict(metric='manhattan'),
        dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=float('nan')), dict(gamma=[1.0] * 9), dict(gamma=[]), dict(gamma='mean'),
        dict(n_perm=-1), dict(n_perm=16384), dict(n_perm=1.5), dict(n_perm=True),
    ]
    for kw in bad:
        args = dict(z=z, groups=g, kernel='rbf', gamma=1.0, metric='euclidean', n_perm=9)
        args.update(kw)
        with pytest.raises(ValueError):
            M.mmd(v, **args)
    with pytest.raises(ValueError):
        M.mmd(v, z, np.stack([g] * 2), n_perm=8192, gamma=1.0)
    with pytest.raises(ValueError):
        M.mmd2(v, z, mr.rows(20, 8, 0), gamma=1.0)
    with pytest.raises(ValueError):
        M.mmd2(v, z, z.astype(np.float64), gamma=1.0)
    with pytest.raises(ValueError):
        M.mmd2(v, z[:1], z, gamma=1.0)


def test_wrapper_builds_the_call():
    """the masks, the config and the shape of the result, with the two device calls replaced"""
    from argsim_amd import mmd as M
    z = mr.rows(70, 6, 0)
    groups = np.stack([np.arange(70) % 3 - 1, (np.arange(70) >= 30).astype(np.int64)])
    seen = {}

    def relabel(vae, N, valid, a0, P, seed):
        seen.update(N=N, valid=valid, a0=a0, P=P, seed=seed)
        return 'masks'

    def raw(vae, x, cfg, valid, inA, want):
        seen.update(x=x, cfg=cfg, inA=inA, want=want)
        G, P1 = cfg.G, 1 + cfg.P
        return dict(stat=np.arange(G * P1, dtype=np.float64).reshape(G, P1), pvalue=np.full(G, 0.5), counts=np.array([[23, 23], [30, 40]], np.int32),
                    stat_out=0, witness=np.ones((G, 70)))
    out = M.mmd(_NoDevice(), z, groups, 'rbf', [0.5, 2.0], 'cosine', 4, 7, True, True, raw=raw, relabel=relabel)
    assert seen['x'].shape == (70, 8) and seen['x'].dtype == np.float32 and (seen['x'][:, 6:] == 0).all()
    assert np.array_equal(seen['valid'], mr.pack(groups >= 0)) and np.array_equal(seen['a0'], mr.pack(groups == 0))
    cfg = seen['cfg']
    assert (cfg.kernel, cfg.metric, cfg.G, cfg.P, cfg.nbw, cfg.reserved) == (0, 1, 2, 4, 2, 0) and list(cfg.gamma)[:2] == [0.5, 2.0]
    assert seen['inA'] == 'masks' and seen['want'] == ('witness',) and (seen['N'], seen['P'], seen['seed']) == (70, 4, 7)
    assert out['stat'].tolist() == [0.0, 5.0] and out['null'].shape == (2, 4) and out['witness'].shape == (2, 70)
    assert out['m'].tolist() == [23, 30] and out['n'].tolist() == [23, 40]
    one = M.mmd(_NoDevice(), z, groups[1], 'energy', 'median', 'euclidean', 4, 7, raw=raw, relabel=relabel)
    assert one['stat'] == 0.0 and one['pvalue'] == 0.5 and set(one) == {'stat', 'pvalue', 'm', 'n'} and seen['cfg'].nbw == 0


def test_median_gamma_is_the_reference_s():
    from argsim_amd import mmd as M
    z = mr.rows(300, 5, 4)
    assert M.median_gamma(None, z, 64) == mr.median_gamma(z, 64) and M.median_gamma(None, z) == mr.median_gamma(z)
    with pytest.raises(ValueError):
        M.median_gamma(None, np.zeros((10, 4), np.float32))


def test_the_declarations_match_the_header():
    from argsim_amd import lib
    res, args = lib.SIGNATURES['avae_mmd']
    assert res is C.c_int and len(args) == 14 and args[4] == C.POINTER(lib.AvaeMmdConfig)
    res, args = lib.SIGNATURES['avae_mmd_relabel']
    assert res is C.c_int and len(args) == 7 and args[6] is C.c_uint64
    with open(os.path.join(ROOT, 'include', 'argsim_vae.h')) as f:
        text = f.read()
    body = re.search(r'typedef struct avae_mmd_config \{(.*?)\} avae_mmd_config;', text, re.S).group(1)
    fields = re.findall(r'^\s*(int32_t|double)\s+(\w+)(\[8\])?;', body, re.M)
    want = [(n, (C.c_double * 8) if arr else C.c_int32) for t, n, arr in fields]
    assert want == list(lib.AvaeMmdConfig._fields_) and C.sizeof(lib.AvaeMmdConfig) == 88
    for name, count in (('avae_mmd', 14), ('avae_mmd_relabel', 7)):
        decl = re.search(r'int\s+%s\((.*?)\);' % name, text, re.S).group(1)
        assert len(re.sub(r'/\*.*?\*/', '', decl, flags=re.S).split(',')) == count
    assert hasattr(lib.load(), 'avae_debug_mmd_plan')


# ---------------------------------------------------------------- eval_explore
class _Vae:
    """affinity by a fixed rule, the two-sample test by the reference"""
    def __init__(self):
        self.calls = []

    def affinity(self, x, metric, max_iter, seed):
        return dict(labels=np.arange(len(x)) % 2, converged=True, n_iter=3)

    def mmd(self, x, groups, n_perm=999, seed=0):
        self.calls.append(groups.copy())
        valid, a0 = groups >= 0, groups == 0
        gamma = (mr.median_gamma(x),)
        ref = mr.run(x, 0, 0, gamma, valid, mr.relabel(valid, a0, n_perm, seed))
        return dict(stat=ref['stat'][:, 0], pvalue=ref['pvalue'], m=ref['counts'][:, 0], n=ref['counts'][:, 1])


def test_eval_explore_flag():
    from argsim_amd import eval_explore as ee
    ap = ee.build_parser()
    base = ['--inputs', 'a.npy', '--labels', 'b.npy']
    A = ap.parse_args(base)
    assert A.mmd is None and A.mmd_perm == 999
    A = ap.parse_args(base + ['--mmd', 'stance', '--mmd-perm', '49'])
    assert A.mmd == 'stance' and A.mmd_perm == 49
    for bad in (['--mmd', 'topic'], ['--mmd-perm', '0']):
        with pytest.raises(SystemExit):
            ap.parse_args(base + bad)
    z = mr.rows(26, 4, 1)
    labels = np.array(['t%d-%s-x' % (i % 3, 'pro' if i % 2 else 'con') for i in range(24)] + ['t3-pro-x', 't3-con-y'])
    v = _Vae()
    cols0, lines0 = ee.evaluate(v, z, None, labels)
    assert not v.calls and not any('mmd' in line for line in lines0)                                     # without the flag: as before
    cols, lines = ee.evaluate(v, z, None, labels, mmd='stance', mmd_perm=19, seed=2)
    assert list(cols) == list(cols0) and lines[:len(lines0)] == lines0
    tail = lines[len(lines0):]
    assert tail[:2] == ['mmd stance z', 'topic m n mmd2 p'] and len(tail) == 6 and len(v.calls) == 1 and v.calls[0].shape == (3, 26)
    assert tail[2] == 't3 1 1 n/a'                                                                    # too few rows of either stance
    g = v.calls[0]
    for t in range(3):
        on = np.arange(26) % 3 == t
        on[24:] = False
        first = 'con' if t % 2 == 0 else 'pro'                # the stance of the topic's first row is sample A
        want = np.where(on, np.where(np.array([('pro' if i % 2 else 'con') == first for i in range(26)]), 0, 1), -1)
        assert np.array_equal(g[t], want)
        name, m, n, s, p = tail[3 + t].split()
        assert (name, int(m), int(n)) == ('t%d' % t, 4, 4) and 0 < float(p) <= 1 and float(s) == float('%.6f' % float(s))


# ---------------------------------------------------------------- the planner
def _plan(N, dim, G, P, chunk, cus, cap=64):
    from argsim_amd import lib
    out = np.full(7 + 2 * cap, -1, np.int32)
    assert lib.load().avae_debug_mmd_plan(N, dim, G, P, chunk, cus, out.ctypes.data_as(C.POINTER(C.c_int32)), cap) == 0
    return out


@pytest.mark.parametrize('N,dim,G,P,chunk,cus', [
    (4, 4, 1, 0, 0, 256), (200, 36, 3, 199, 0, 256), (200, 36, 3, 199, 1, 256), (200, 36, 3, 63, 5, 256), (130, 128, 3, 64, 16, 256),
    (3000, 128, 1, 999, 0, 256), (65536, 128, 1, 999, 0, 256), (65536, 128, 8, 999, 0, 256), (131072, 1024, 64, 255, 0, 256),
    (131072, 4, 1, 16383, 0, 304), (131072, 4, 64, 0, 64, 8), (5000, 64, 64, 255, 40, 64)])
def test_plan(N, dim, G, P, chunk, cus):
    cap = 64
    o = _plan(N, dim, G, P, chunk, cus, cap)
    TI, nq, npass, limit, tiles, slots, wit = (int(v) for v in o[:7])
    Q = G * (1 + P)
    assert TI in (8, 16, 32, 64) and limit == 160 * 1024 and tiles == -(-N // TI) and wit <= limit
    assert 1 <= nq <= Q and npass == -(-Q // nq)
    if chunk > 0:
        assert nq <= chunk and TI == max(8, min(64, 1 << (chunk.bit_length() - 1)))
    else:
        assert TI == 32 or (TI < 32 and -(-N // (2 * TI)) < cus)
    # every relabeling in exactly one pass: pass q begins at q nq, the last one ends at Q; the LDS of every pass within the limit
    seen = 0
    for q in range(min(npass, cap)):
        q0, lds = int(o[7 + 2 * q]), int(o[8 + 2 * q])
        assert q0 == seen and 0 < lds <= limit
        n = min(nq, Q - q0)
        comparisons = (q0 + n - 1) // (1 + P) - q0 // (1 + P) + 1
        assert n + comparisons <= slots
        seen += n
    if npass <= cap:
        assert seen == Q and (o[7 + 2 * npass:] == -1).all()
    else:
        assert (npass - 1) * nq < Q <= npass * nq


def test_plan_hook_refuses_bad_arguments():
    from argsim_amd import lib
    out = np.zeros(16, np.int32)
    p = out.ctypes.data_as(C.POINTER(C.c_int32))
    l = lib.load()
    for a in ((1, 4, 1, 0, 0, 256), (131073, 4, 1, 0, 0, 256), (10, 4, 0, 0, 0, 256), (10, 4, 65, 0, 0, 256), (10, 4, 1, -1, 0, 256),
              (10, 4, 2, 8192, 0, 256), (10, 4, 1, 0, -1, 256), (10, 4, 1, 0, 0, 0)):
        assert l.avae_debug_mmd_plan(*a, p, 4) == 1
    assert l.avae_debug_mmd_plan(10, 4, 1, 0, 0, 256, None, 4) == 1
