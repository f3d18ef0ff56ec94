"""nucleus sampling on the device (avae_decode_sample_p, avae_debug_sample_rows_p) against the float64 reference of tests/nucleus_ref.py.

Crafted rows go through the per-token kernel alone: geometric decays whose nucleus boundary and Gumbel winner are decidable (both
margins >= 1e-3; tests/test_nucleus.py checks that on the reference alone), so nkept and the token must EQUAL the reference's.  At
top_p = 1 - 2^-24 no boundary can be further than 2^-24 from top_p.  Where cum_j is exactly 1 in float64, the mass behind group j is 0
in the device's 2^-40 fixed point too and need <= W holds by the clamp: only the other side, top_p - cum_(j-1), can move, and that is
the last kept token's share, > 1e-3.  With top_k 8 the decays keep all 8 (the +inf row: 1; the dominant row is left out of that one
configuration: its seven other tokens hold 4.5e-5 each).  With top_k 0 the 'cliff' row is judged: six tokens one apart, every other
token 100 below them -- weight 0 on the device -- so need, a few 10^4 below W, must stop after exactly those six of V.

Model level: the reference REPLAYS the device's tokens and is told the device's nkept, so every position is judged on the device's
own history and on the device's own set (geometries and parameters as tests/test_gpu_sampling.py builds them).

TOL_MASS, TOL_LOGP.  Not chosen in advance: 4 x the largest violation of the device's set and 4 x the largest |device logp - float64
logp over the device's set| over every live position of ALL below (two competing quantities each carry the fp32 logit error).
Measured on MI355X over the 44 cases (12 928 live positions): largest violation 1.077e-08 -- ONE position's set differs from the
reference's at all, production geometry, b = 32 / 40, (T 1.0, top_k 0, top_p 0.9), on both paths, where the boundary
itself is 1.08e-8 from top_p; every other violation is 0 -- and largest |dlogp| 6.200e-06 (production, b = 32 and 40, per-token
path, T 0.7, top_k 40, top_p 0.9).  So MAX_VIOL = 1.1e-8, TOL_MASS = 4.4e-8, MAX_DLOGP = 6.3e-6, TOL_LOGP = 2.52e-5; no token of
any case is undecidable at that TOL_LOGP.  test_tolerances_are_four_times_the_measured_errors prints both figures again and fails
if a run measures more than a quarter of a constant, or if TOL_MASS > 1e-4 or TOL_LOGP > 1e-3.  The crafted rows: |dlogp| <= 2.6e-7."""
import ctypes as C

import numpy as np
import pytest

import nucleus_ref as nr
import sampling_ref as sr
from helpers import make_case
from oracle import vae_numpy as vn
from test_gpu_sampling import _first_logits

pytestmark = pytest.mark.gpu

MAX_VIOL = 1.1e-8           # measured: 1.077e-08 (see the docstring)
MAX_DLOGP = 6.3e-6          # measured: 6.200e-06
TOL_MASS = 4 * MAX_VIOL
TOL_LOGP = 4 * MAX_DLOGP
KEYS = ('dim_tgt', 'dim_emb', 'dim_rep', 'rnn_layers', 'accelerate', 'learn_rate', 'bos', 'eos')
CONFIGS = [(1.0, 0, 0.9), (0.7, 0, 0.5), (0.7, 40, 0.9), (1.3, 8, 0.95)]
GEOMS = [('tiny', 4, 1), ('tiny', 4, 0), ('mid', 8, 1), ('mid', 8, 0),
         ('prod', 1, 1), ('prod', 5, 1), ('prod', 32, 1), ('prod', 1, 0), ('prod', 5, 0), ('prod', 32, 0), ('prod', 40, 0)]
STEPS = {'tiny': 40, 'mid': 40, 'prod': 20}
ALL = [(g, c) for g in GEOMS for c in CONFIGS]
_PARAMS, _MODELS, _RUNS = {}, {}, {}


def f32(p):
    """top_p as the device gets it"""
    return float(np.float32(p))


def params(name):
    """(cfg, P, z (40, R)) of a geometry as test_gpu_sampling._model makes them: the `out` affine scaled to max |logit| = 8 at step 0"""
    if name not in _PARAMS:
        if name == 'prod':
            cfg = vn.make_cfg(dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3)
            P = {k: v.astype(np.float32).astype(np.float64) for k, v in vn.init_params(cfg, 4, bias_scale=0.1).items()}
        else:
            cfg, P = make_case(name)[:2]
            P = dict(P)
        z = np.random.default_rng(11).standard_normal((40, cfg['dim_rep'])).astype(np.float32)
        f = 8.0 / float(np.abs(_first_logits(P, cfg, z)).max())
        for k in ('decode/out/kernel', 'decode/out/bias'):
            P[k] = (P[k] * f).astype(np.float32).astype(np.float64)
        _PARAMS[name] = (cfg, P, z)
    return _PARAMS[name]


def _model(name):
    if name not in _MODELS:
        from argsim_amd.model import VAE
        cfg, P, z = params(name)
        m = VAE('infer', init=False, **{k: cfg[k] for k in KEYS})
        m.set_params(P)
        _MODELS[name] = m
    return (_MODELS[name],) + params(name)


# ---------------------------------------------------------------- crafted rows
CRAFT_V = [32, 1000, 8192, 8200]       # below one pass of the workgroup, no multiple of 256, the register form's limit, the streaming form
CRAFT_CFG = [(1.0, 0, 0.9), (0.7, 8, 0.9), (1.3, 0, 0.5), (1.0, 8, 1.0 - 2.0 ** -24), (1.0, 0, 1.0 - 2.0 ** -24)]
LIVE = (0, 1, 2, 3, 4, 5, 6, 8)
CRAFT_ROWS = {(8, 1.0 - 2.0 ** -24): (0, 1, 2, 3, 4, 5, 8), (0, 1.0 - 2.0 ** -24): (8,)}      # (top_k, top_p) -> the rows judged there (default: LIVE)
CRAFT_T0, CRAFT_SEED = 9, 21
ROW_NAMES = ('decay', 'slow decay', 'tie group on the boundary', '-inf and NaN', '+inf', 'all -inf', 'dominant', 'finished', 'cliff')


def crafted(V):
    """(x (9, V) float32, lead (9,) int32 with eos = 1 in row 7): see ROW_NAMES.  Ranks are dealt to ids by a permutation, so
    the kept ids lie all over the row (and over the threads of the workgroup)."""
    rng = np.random.default_rng(V)
    rank = lambda: rng.permutation(V).astype(np.float64)
    x = np.zeros((9, V))
    x[0] = 3.0 - 0.5 * rank()
    x[1] = -1.0 - 0.125 * rank()
    r = rank()
    x[2] = 2.0 - 0.5 * np.where((r >= 2) & (r <= 5), 2.0, r)          # ranks 2..5 share one value: the boundary of 0.9 falls inside them
    r = rank()
    x[3] = 1.0 - 0.25 * r
    x[3, r == 0] = np.nan                                              # the would-be maximum is absent
    x[3, (r >= 3) & (r % 3 == 0)] = -np.inf
    x[3, (r >= 4) & (r % 5 == 0)] = np.nan
    x[4] = -0.25 * rank()
    x[4, rng.integers(V)] = np.inf
    x[5] = -np.inf
    r = rank()
    x[6] = np.where(r == 0, 6.0, -4.0 - 0.001 * r)                      # p_max > top_p wherever V <= 8200: one token kept
    x[7] = 1.0 - 0.5 * rank()
    r = rank()
    x[8] = np.where(r < 6, 2.0 - r, -100.0 - 0.001 * r)                 # the last of the six holds 4.3e-3, everything behind them nothing
    lead = np.full(9, 3, np.int32)
    lead[7] = 1
    return x.astype(np.float32), lead


def crafted_ref(V, T, k, p):
    """the reference's positions of crafted(V)'s LIVE rows at (T, k, p), by row"""
    x, _ = crafted(V)
    return {r: nr.position(x[r].astype(np.float64), T, k, f32(p), CRAFT_SEED, r, CRAFT_T0) for r in LIVE}


def crafted_margin(p):
    """boundary margin of a crafted position: where cum_j is exactly 1 only the lower side can move (see the docstring of the file)"""
    nu = p['nucleus']
    return p['top_p'] - nu['cum_jm1'] if nu['cum_j'] == 1.0 else nu['bmargin']


def _rows_p(m, x, t0, T, k, p, seed, lead=None, reserved=0, null_sc=False):
    import torch
    xd = torch.as_tensor(x, dtype=torch.float32).to(m.device).contiguous()
    n, V = xd.shape
    pred = torch.full((n,), -7, dtype=torch.int32, device=m.device)
    logp = torch.full((n,), 7.0, dtype=torch.float32, device=m.device)
    nk = torch.full((n,), -7, dtype=torch.int32, device=m.device)
    ld = torch.as_tensor(lead, dtype=torch.int32).to(m.device) if lead is not None else None
    sc = m._l.avae_debug_sample_rows_p.argtypes[5]._type_(float(T), int(k), int(seed), float(p), int(reserved))
    rc = m._l.avae_debug_sample_rows_p(m._h, C.c_void_p(xd.data_ptr()), n, V, t0, None if null_sc else C.byref(sc), C.c_void_p(pred.data_ptr()),
                                       C.c_void_p(logp.data_ptr()), C.c_void_p(nk.data_ptr()), C.c_void_p(ld.data_ptr()) if ld is not None else None)
    torch.cuda.synchronize()
    return rc, pred.cpu().numpy(), logp.cpu().numpy(), nk.cpu().numpy()


@pytest.mark.parametrize("V", CRAFT_V)
def test_row_kernel_on_crafted_rows_equals_the_reference_exactly(V):
    m = _model('tiny')[0]
    x, lead = crafted(V)
    worst = 0.0
    for T, k, p in CRAFT_CFG:
        rc, pred, logp, nk = _rows_p(m, x, CRAFT_T0, T, k, p, CRAFT_SEED, lead)
        assert rc == 0, m._l.avae_last_error(m._h)
        ref = crafted_ref(V, T, k, p)
        rows = CRAFT_ROWS.get((k, p), LIVE)
        for r in rows:
            q = ref[r]
            assert nk[r] == q['nkept'], (V, T, k, p, ROW_NAMES[r], nk[r], q['nkept'])
            assert pred[r] == q['token'], (V, T, k, p, ROW_NAMES[r], pred[r], q['token'])
            if r == 5:
                assert pred[r] == 0 and np.isnan(logp[r]) and nk[r] == V
                continue
            d = abs(float(logp[r]) - q['logp'][q['token']])
            worst = max(worst, d)
            assert d <= TOL_LOGP, (V, T, k, p, ROW_NAMES[r], logp[r], q['logp'][q['token']])
        assert nk[4] == 1 and logp[4] == 0.0 and np.isinf(x[4, pred[4]])
        assert 6 not in rows or (nk[6] == 1 and pred[6] == int(x[6].argmax()))
        assert pred[7] == 1 and logp[7] == 0.0 and nk[7] == 0                  # finished through lead
        assert not np.isnan(x[3, pred[3]])
        assert 8 not in rows or p < 0.99 or (nk[8] == 6 and x[8, pred[8]] >= -3.0)
    print("V %d: max |dlogp| %.3e" % (V, worst))
    # without lead nobody is finished; nucleus off: avae_debug_sample_rows' results, nkept -1
    rc, pred, logp, nk = _rows_p(m, x[7:], CRAFT_T0, 1.0, 0, 0.9, CRAFT_SEED)
    assert rc == 0 and nk[0] > 0 and logp[0] < 0.0
    for T, k, p in ((1.0, 0, 0.0), (1.0, 0, 1.0), (0.0, 0, 0.5), (0.7, 1, 0.5)):
        rc, pred, logp, nk = _rows_p(m, x[:3], CRAFT_T0, T, k, p, CRAFT_SEED)
        q = [sr.position(x[r].astype(np.float64), T, k, CRAFT_SEED, r, CRAFT_T0) for r in range(3)]
        assert rc == 0 and (nk == -1).all() and [int(v) for v in pred] == [v['token'] for v in q]


# ---------------------------------------------------------------- model level
def _run(name, b, persistent, T, k, p, seed=1):
    """device run + replay of one case -> dict (cached: the tolerance test and the per-case test share the runs)"""
    key = (name, b, persistent, T, k, p, seed)
    if key not in _RUNS:
        m, cfg, P, z = _model(name)
        m.set_option('persistent', persistent)
        ids, logp, nk = m.sample(z[:b], steps=STEPS[name], temperature=T, top_k=k, seed=seed, return_logp=True, top_p=p, return_nkept=True)
        m.set_option('persistent', 1)
        ref = nr.sample(P, cfg, z[:b], STEPS[name], T, k, f32(p), seed, replay=ids, nkept=nk)
        assert logp.shape == ref['live'].shape == nk.shape and ref['n_steps'] == ids.shape[1], (logp.shape, nk.shape, ref['live'].shape, ref['n_steps'], ids.shape)
        live = ref['live']
        _RUNS[key] = dict(ids=ids, logp=logp, nk=nk, ref=ref, cfg=cfg, viol=float(ref['viol'][live].max()),
                          dlogp=float(np.abs(logp - ref['logp_set'])[live].max()))
    return _RUNS[key]


def test_tolerances_are_four_times_the_measured_errors():
    """over all cases and every live position, against the float64 reference alone: the largest violation of the device's set and the
    largest |device logp - float64 logp over the device's set|"""
    viol = {(g, c): _run(*g, *c)['viol'] for g, c in ALL}
    dlogp = {(g, c): _run(*g, *c)['dlogp'] for g, c in ALL}
    tv = sorted(viol.items(), key=lambda kv: -kv[1])[:5]
    tl = sorted(dlogp.items(), key=lambda kv: -kv[1])[:5]
    print("max violation over %d cases: %.3e (TOL_MASS / 4 = %.3e); worst: %s" % (len(viol), tv[0][1], TOL_MASS / 4, tv))
    print("max |dlogp| over %d cases: %.3e (TOL_LOGP / 4 = %.3e); worst: %s" % (len(dlogp), tl[0][1], TOL_LOGP / 4, tl))
    assert TOL_MASS <= 1e-4 and TOL_LOGP <= 1e-3
    assert tv[0][1] <= TOL_MASS / 4, tv
    assert tl[0][1] <= TOL_LOGP / 4, tl


@pytest.mark.parametrize("g,c", ALL, ids=lambda v: str(v).replace(' ', ''))
def test_device_sets_tokens_and_logp_against_the_float64_reference(g, c):
    """per live position: the device's set is a prefix of whole tie groups with violation <= TOL_MASS, and the reference's own set
    where the boundary margin exceeds TOL_MASS; logp within TOL_LOGP of the float64 logp over THAT set; the token is the Gumbel
    winner over that set where the top-2 margin exceeds TOL_LOGP, elsewhere (at most 2 % of the live positions) it scores within
    TOL_LOGP of the best.  Finished rows: eos, logp 0, nkept 0."""
    r = _run(*g, *c)
    ref, ids, logp, nk, eos = r['ref'], r['ids'], r['logp'], r['nk'], r['cfg']['eos']
    live = ref['live']
    dec = live & (ref['margin_set'] > TOL_LOGP)
    und = live & ~dec
    print("%s %s: %d live, %d undecidable tokens, max violation %.2e, max dlogp %.2e, min boundary margin %.2e, %d sets differ from the reference's" %
          (g, c, live.sum(), und.sum(), r['viol'], r['dlogp'], ref['bmargin'][live].min(), (live & (ref['same'] == 0)).sum()))
    assert live.sum() >= ids.shape[0]
    assert (ref['viol'][live] <= TOL_MASS).all(), np.argwhere(live & ~(ref['viol'] <= TOL_MASS))[:5]
    assert (np.abs(logp - ref['logp_set'])[live] <= TOL_LOGP).all()
    assert np.array_equal(ref['dev'][dec], ref['win'][dec].astype(np.int32)), np.argwhere(dec & (ref['dev'] != ref['win']))[:5]
    assert und.sum() <= 0.02 * live.sum(), (und.sum(), live.sum())
    assert (ref['deficit_set'][und] <= TOL_LOGP).all()
    clear = live & (ref['bmargin'] > TOL_MASS)
    assert (ref['same'][clear] == 1).all() and np.array_equal(nk[clear], ref['nkept_ref'][clear].astype(np.int32))
    assert (nk[live] >= 1).all()
    assert (logp[~live] == 0.0).all() and (nk[~live] == 0).all() and (ref['dev'][~live] == eos).all()
    padded = np.full(live.shape, eos, np.int32)
    padded[:, :ids.shape[1]] = ids
    assert (padded[~live] == eos).all()


@pytest.mark.parametrize("name,b", [('mid', 8), ('prod', 5)])
@pytest.mark.parametrize("persistent", [1, 0])
def test_nucleus_off_is_avae_decode_sample_bit_for_bit(name, b, persistent):
    m, cfg, P, z = _model(name)
    m.set_option('persistent', persistent)
    for T, k in ((1.0, 0), (0.7, 40)):
        ids, logp = m.sample(z[:b], steps=24, temperature=T, top_k=k, seed=3, return_logp=True)
        for p in (0.0, 1.0):
            i2, l2, nk = m.sample(z[:b], steps=24, temperature=T, top_k=k, seed=3, return_logp=True, top_p=p, return_nkept=True)
            assert np.array_equal(ids, i2) and np.array_equal(logp.view(np.int32), l2.view(np.int32)) and (nk == -1).all(), (T, k, p)
    want = m.decode(z[:b], steps=24)
    got, nk = m.sample(z[:b], steps=24, temperature=0.0, top_p=0.5, seed=3, return_nkept=True)
    n = min(want.shape[1], got.shape[1])
    for r in range(b):                                   # (beyond a row's eos the greedy loop goes on feeding it, the sampled one does not)
        e = np.flatnonzero(got[r, :n] == cfg['eos'])
        stop = e[0] + 1 if len(e) else n
        assert np.array_equal(got[r, :stop], want[r, :stop]), r
    assert (nk == -1).all()
    m.set_option('persistent', 1)


@pytest.mark.parametrize("persistent", [1, 0])
def test_same_call_same_bits_and_the_step_cap_cuts_a_prefix(persistent):
    m, cfg, P, z = _model('prod')
    m.set_option('persistent', persistent)
    kw = dict(temperature=0.9, top_k=40, top_p=0.9, seed=7, return_logp=True, return_nkept=True)
    a, la, na = m.sample(z[:8], steps=20, **kw)
    b_, lb, nb = m.sample(z[:8], steps=20, **kw)
    assert np.array_equal(a, b_) and np.array_equal(la.view(np.int32), lb.view(np.int32)) and np.array_equal(na, nb)
    s10, l10, n10 = m.sample(z[:8], steps=10, **kw)
    assert np.array_equal(s10, a[:, :10]) and np.array_equal(l10.view(np.int32), la[:, :10].view(np.int32)) and np.array_equal(n10, na[:, :10])
    assert (na[:, 0] >= 1).all() and (na <= 40).all()
    m.set_option('persistent', 1)


@pytest.mark.parametrize("top_p", [0.0, 0.8])
@pytest.mark.parametrize("top_k", [0, 4])
@pytest.mark.parametrize("persistent", [1, 0])
def test_optional_outputs_do_not_change_the_others(persistent, top_k, top_p):
    """logp_out and nkept_out are optional buffers of both loops' scratch: every combination of given / null returns the bits of the
    call that asks for both (which the cases above hold against the float64 reference).  Nucleus off: nkept is -1 throughout."""
    m, cfg, P, z = _model('tiny')
    m.set_option('persistent', persistent)
    kw = dict(steps=5, temperature=0.9, top_k=top_k, seed=5, top_p=top_p)
    ids, logp, nk = m.sample(z[:3], return_logp=True, return_nkept=True, **kw)
    i1, l1 = m.sample(z[:3], return_logp=True, **kw)
    i2, n2 = m.sample(z[:3], return_nkept=True, **kw)
    i3 = m.sample(z[:3], **kw)
    m.set_option('persistent', 1)
    assert np.array_equal(ids, i1) and np.array_equal(ids, i2) and np.array_equal(ids, i3)
    assert np.array_equal(logp.view(np.int32), l1.view(np.int32)) and np.array_equal(nk, n2)
    assert (nk >= 1).any() if top_p else (nk == -1).all()


def test_bad_arguments_are_errors_and_the_handle_works_afterwards():
    import torch
    m, cfg, P, z = _model('mid')
    zd = torch.as_tensor(z[:4]).to(m.device)
    out = torch.full((4, 8), -5, dtype=torch.int32, device=m.device)
    n = C.c_int32(-9)
    mk = m._l.avae_decode_sample_p.argtypes[4]._type_
    for T, k, p, res in ((1.0, 0, -0.1, 0), (1.0, 0, float('nan'), 0), (1.0, 0, 0.9, 1), (-1.0, 0, 0.9, 0), (1.0, -2, 0.9, 0)):
        sc = mk(T, k, 0, p, res)
        rc = m._l.avae_decode_sample_p(m._h, C.c_void_p(zd.data_ptr()), 4, 8, C.byref(sc), C.c_void_p(out.data_ptr()), None, None, C.byref(n))
        assert rc != 0 and len(m._l.avae_last_error(m._h)) > 0, (T, k, p, res)
        torch.cuda.synchronize()
        assert bool((out == -5).all()) and n.value == -9
    assert m._l.avae_decode_sample_p(m._h, C.c_void_p(zd.data_ptr()), 4, 8, None, C.c_void_p(out.data_ptr()), None, None, C.byref(n)) != 0
    x = np.zeros((2, 8), np.float32)
    for kw in (dict(p=-0.5), dict(p=float('nan')), dict(p=0.9, reserved=1), dict(p=0.9, null_sc=True)):
        rc, pred, logp, nk = _rows_p(m, x, 0, 1.0, 0, kw.pop('p'), 0, **kw)
        assert rc != 0 and (pred == -7).all() and (nk == -7).all()
    with pytest.raises(ValueError):
        m.sample(z[:4], top_p=-0.1)
    ids = m.generate(3, steps=12, temperature=0.9, top_k=8, seed=5, top_p=0.8)
    assert ids.shape[0] == 3 and ids.shape[1] <= 12 and np.array_equal(ids, m.generate(3, steps=12, temperature=0.9, top_k=8, seed=5, top_p=0.8))
    from argsim_amd import model
    assert np.array_equal(model.sample(m, z[:3], steps=12, seed=5, top_p=0.8), m.sample(z[:3], steps=12, seed=5, top_p=0.8))
