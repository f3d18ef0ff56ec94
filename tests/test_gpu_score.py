"""importance-weighted sentence likelihood on the device (avae_score, avae_score_z) against the float64 reference of tests/score_ref.py.

Models: make_case('tiny' / 'mid' / 'tab' / 'd128') at their own batch and the production geometry (V 8192, D 512, R 128, L 3) with
B = 8, S = 64 ragged, k = 4; decode/out/* scaled so that the first step's max |logit| is 8 (as tests/test_gpu_sampling.py does: random
initialisation gives an almost flat distribution).  'prodlv' is the production model with latent/lv/bias = -4: narrow posteriors, a
large spread of logw.

Tolerances.  None was chosen in advance; each is 4 x the largest value measured on MI355X over every case and every row, printed
again by the test_tol_* tests, which fail if a run measures more than a quarter of the constant or if the constant exceeds its cap.
  TOL_TOK   |device logpx - reference logpx| / ntok, eps injected.  Measured: 1.376e-06 ('tab'; 1.353e-06 at the production geometry,
            1.344e-06 there in f32s), so MEASURED_TOK = 1.4e-6 and TOL_TOK = 5.6e-6 (cap 1e-4, the per-token CE bound the project
            holds at this geometry).  bf16 at the production geometry measures 3.1e-03 against its bound of 6e-2.
  TOL_LAT   |device (logw - logpx) - float64 latent term of the device's own eps, mu, lv| / R.  Measured: 2.650e-07 ('tiny'),
            so MEASURED_LAT = 2.7e-7 and TOL_LAT = 1.08e-6 (cap 1e-5).
  bound     against float64 logsumexp - log k of the device's own logw: 1e-6 |bound| + 1e-6 (fixed by the formats: one fp32 rounding
            of a sum of at most k terms in [0, 1] and of the result).
  generator Box-Muller in fp32 against float64 on the exact uniforms: 1e-5 absolute (2 pi u is rounded by at most 2.4e-7, |eps| <= 5.9).
"""
import ctypes as C
import os

import numpy as np
import pytest

import score_ref
from helpers import make_case
from oracle import vae_numpy as vn
from test_gpu_sampling import MAX_DLOGP

pytestmark = pytest.mark.gpu

MEASURED_TOK = 1.4e-6        # measured on MI355X: 1.376e-06 ('tab'; production geometry 1.353e-06)
TOL_TOK = 4 * MEASURED_TOK
MEASURED_LAT = 2.7e-7        # measured on MI355X: 2.650e-07 ('tiny', R = 8; production geometry 1.711e-07)
TOL_LAT = 4 * MEASURED_LAT
TOL_BF16 = 6e-2              # the project's bf16 per-token bound
KEYS = ('dim_tgt', 'dim_emb', 'dim_rep', 'rnn_layers', 'accelerate', 'learn_rate', 'bos', 'eos')
CASES = ['tiny', 'mid', 'tab', 'd128', 'prod', 'prodlv']
K = 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MODELS, _RUNS = {}, {}


def _first_logits(P, cfg, z):
    D, L = cfg['dim_emb'], cfg['rnn_layers']
    E = P['embed/embedding']
    h0 = np.asarray(z, np.float64) @ P['latent/ex/kernel'] + P['latent/ex/bias']
    hd, _ = vn.decoder_rnn(P, cfg, E[np.full((1, len(z)), cfg['bos'], np.int32)], np.stack([h0] * L))
    hd = hd.reshape(-1, D) @ P['decode/out/kernel'] + P['decode/out/bias']
    return hd @ ((D ** -0.5) * E.T)


def _ragged(cfg, B, S, seed=23):
    rng = np.random.default_rng(seed)
    lens = rng.integers(2, S + 1, B)
    lens[0] = S
    if B > 1:
        lens[1] = 1
    ids = np.full((B, S + 2), cfg['eos'], np.int32)
    for b, n in enumerate(lens):
        ids[b, :n] = rng.integers(3, cfg['dim_tgt'], n)
    return ids


def _params(name, eos_lean=0.0):
    if name.startswith('prod'):
        cfg = vn.make_cfg(dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3)
        P = {k: v.astype(np.float32).astype(np.float64) for k, v in vn.init_params(cfg, 4, bias_scale=0.1).items()}
        ids = _ragged(cfg, 8, 64)
    else:
        cfg, P, ids = make_case(name)[:3]
    z = np.random.default_rng(11).standard_normal((40, cfg['dim_rep'])).astype(np.float32)
    f = 8.0 / float(np.abs(_first_logits(P, cfg, z)).max())
    for k in ('decode/out/kernel', 'decode/out/bias'):
        P[k] = (P[k] * f).astype(np.float32).astype(np.float64)
    if name == 'prodlv':
        P['latent/lv/bias'] = np.full_like(P['latent/lv/bias'], -4.0)
    if eos_lean:
        e = P['embed/embedding'][cfg['eos']]
        P['decode/out/bias'] = (P['decode/out/bias'] + eos_lean * np.sqrt(cfg['dim_emb']) * e / (e @ e)).astype(np.float32).astype(np.float64)
    return cfg, P, ids, z


def _model(name, dtype='f32', eos_lean=0.0):
    key = (name, dtype, eos_lean)
    if key not in _MODELS:
        from argsim_amd.model import VAE
        cfg, P, ids, z = _params(name, eos_lean)
        m = VAE('infer', init=False, dtype=dtype, **{k: cfg[k] for k in KEYS})
        m.set_params(P)
        _MODELS[key] = (m, cfg, P, ids, z)
    return _MODELS[key]


def _run(name, dtype='f32'):
    """device score with injected eps + the float64 reference on the same eps (cached)"""
    key = (name, dtype)
    if key not in _RUNS:
        m, cfg, P, ids, _ = _model(name, dtype)
        eps = np.random.default_rng(5).standard_normal((K, len(ids), cfg['dim_rep'])).astype(np.float32)
        dev = m.score(ids, None, K, eps=eps, return_parts=True)
        ref = score_ref.score(P, cfg, ids, ids, eps)
        _RUNS[key] = dict(dev=dev, ref=ref, eps=eps, R=cfg['dim_rep'])
    return _RUNS[key]


def _per_token(r):
    return float((np.abs(r['dev']['logpx'] - r['ref']['logpx']) / r['ref']['ntok'][None]).max())


def _latent_replay(name):
    """device (logw - logpx) against the float64 latent term of the device's own eps_out, mu, lv -> largest |difference| / R"""
    m, cfg, P, ids, _ = _model(name)
    d = m.score(ids, None, K, seed=9, return_parts=True)
    mu, lv = m.encode(ids, return_lv=True)
    lat = score_ref.latent_term(mu.astype(np.float64), lv.astype(np.float64), d['eps'].astype(np.float64))
    got = d['logw'].astype(np.float64) - d['logpx'].astype(np.float64)
    return d, float(np.abs(got + lat).max()) / cfg['dim_rep']


# ------------------------------------------------------------------------------------------ 1. end to end
def test_tol_per_token_is_four_times_the_measured_error():
    """max |device logpx - reference logpx| / ntok over every case, draw and row, eps injected.  MEASURED_TOK x 4 = TOL_TOK must
    cover it and stay <= 1e-4."""
    worst = {n: _per_token(_run(n)) for n in CASES}
    mx = max(worst.values())
    print("max |dlogpx| / ntok over %d cases: %.3e (TOL_TOK / 4 = %.3e); per case: %s" % (len(worst), mx, TOL_TOK / 4, worst))
    assert TOL_TOK <= 1e-4
    assert mx <= TOL_TOK / 4, worst


@pytest.mark.parametrize("name", CASES)
def test_score_equals_the_float64_reference(name):
    r = _run(name)
    dev, ref, R = r['dev'], r['ref'], r['R']
    assert np.array_equal(dev['ntok'], ref['ntok'])
    assert np.array_equal(dev['eps'], r['eps'])
    per = np.abs(dev['logpx'] - ref['logpx']) / ref['ntok'][None]
    print("%s: max per-token |dlogpx| %.3e, logw in [%.1f, %.1f]" % (name, per.max(), ref['logw'].min(), ref['logw'].max()))
    assert (per <= TOL_TOK).all()
    tol_w = TOL_TOK * ref['ntok'][None] + TOL_LAT * R
    assert (np.abs(dev['logw'] - ref['logw']) <= tol_w).all()
    # log-mean-exp moves by at most the largest move of its arguments
    assert (np.abs(dev['bound'] - ref['bound']) <= tol_w.max(0) + 1e-6 * np.abs(ref['bound']) + 1e-6).all()
    assert (dev['bound'] >= dev['logw'].mean(0) - 1e-4).all()


# ------------------------------------------------------------------------------------------ 2. latent term and bound, replayed
def test_tol_latent_term_is_four_times_the_measured_error():
    worst = {n: _latent_replay(n)[1] for n in CASES}
    mx = max(worst.values())
    print("max |d latent term| / R over %d cases: %.3e (TOL_LAT / 4 = %.3e); per case: %s" % (len(worst), mx, TOL_LAT / 4, worst))
    assert TOL_LAT <= 1e-5
    assert mx <= TOL_LAT / 4, worst


@pytest.mark.parametrize("name", CASES)
def test_latent_term_and_bound_replayed_from_the_device_draws(name):
    d, per_r = _latent_replay(name)
    assert per_r <= TOL_LAT
    want = score_ref.log_mean_exp(d['logw'].astype(np.float64))
    assert (np.abs(d['bound'] - want) <= 1e-6 * np.abs(want) + 1e-6).all(), np.abs(d['bound'] - want).max()
    assert np.isfinite(d['bound']).all()
    if name == 'prodlv':        # exp(logw) is 0 in fp32: only the subtracted maximum keeps the bound finite
        assert (np.exp(d['logw'].astype(np.float32)) == 0).all() and (d['logw'].max(0) - d['logw'].min(0)).max() > 1.0


# ------------------------------------------------------------------------------------------ 3. generator
@pytest.mark.parametrize("name", ['tiny', 'prod'])
def test_generator_is_stream_four_and_holds_neither_k_nor_the_batch(name):
    m, cfg, P, ids, _ = _model(name)
    B, R = len(ids), cfg['dim_rep']
    e8 = m.score(ids, None, 8, seed=12, return_parts=True)['eps']
    e4 = m.score(ids, None, 4, seed=12, return_parts=True)['eps']
    want = score_ref.eps_all(12, 8, B, R)
    assert e8.shape == (8, B, R)
    assert np.abs(e8 - want).max() <= 1e-5
    assert np.array_equal(e4, e8[:4])
    b5 = min(5, B)
    e5 = m.score(ids[:b5], None, 4, seed=12, return_parts=True)['eps']
    assert np.array_equal(e5[:, b5 - 2], e4[:, b5 - 2])          # (row 3 of a B = 8 and of a B = 5 call)
    assert not np.array_equal(m.score(ids, None, 4, seed=13, return_parts=True)['eps'], e4)


# ------------------------------------------------------------------------------------------ 4. consistency with what exists
def _row_sums(m, cfg, ids, lgen):
    """per-row sums of eval's compacted per-token CE (time-major boolean_mask order)"""
    t = m.trim(ids)
    msk = np.concatenate([np.ones((1, len(t)), bool), (t != cfg['eos']).T], 0)
    ce = np.zeros(msk.shape)
    ce[msk] = lgen
    return ce.sum(0), msk.sum(0)


@pytest.mark.parametrize("name", CASES)
def test_score_z_at_mu_is_the_row_sum_of_eval(name):
    m, cfg, P, ids, _ = _model(name)
    _, lgen, _ = m.eval(ids, ids)
    want, n = _row_sums(m, cfg, ids, lgen)
    mu = m.encode(ids)
    logpx, ntok = m.score_z(mu, ids)
    assert np.array_equal(ntok, n)
    assert (np.abs(logpx + want) <= TOL_TOK * n).all(), (np.abs(logpx + want) / n).max()
    one = m.score(ids, None, 1, eps=np.zeros((1,) + mu.shape, np.float32), return_parts=True)
    assert (np.abs(one['logpx'][0] - logpx) <= TOL_TOK * n).all()
    assert np.array_equal(one['ntok'], n)


@pytest.mark.parametrize("name,b", [('tiny', 4), ('mid', 8), ('prod', 32), ('prod', 40)])
def test_score_z_inverts_sample(name, b):
    """the log-probability sample() reports for the sentences it drew is what score_z gives for them.  The out bias leans towards eos
    (10 logit units) so that every row closes well inside the step cap: a row cut at the cap has no closing eos in logp, while
    score_z always scores one."""
    m, cfg, P, ids, z = _model(name, eos_lean=10.0)
    steps = 64
    out, logp = m.sample(z[:b], steps=steps, temperature=1.0, top_k=0, seed=3, return_logp=True)
    length = np.array([int(np.argmax(np.append(r, cfg['eos']) == cfg['eos'])) for r in out])
    assert (length < steps).all(), "a row reached the step cap: its logp has no closing eos"
    if out.shape[1] == 0:
        out = np.full((b, 1), cfg['eos'], np.int32)
    logpx, ntok = m.score_z(z[:b], out)
    assert np.array_equal(ntok, length + 1)
    tol = ntok * (TOL_TOK + 4 * MAX_DLOGP)
    assert (np.abs(logp.sum(1) - logpx) <= tol).all(), (np.abs(logp.sum(1) - logpx) / ntok).max()


# ------------------------------------------------------------------------------------------ 5. determinism and shapes
def test_same_arguments_same_bytes_and_another_seed_moves_the_draws():
    m, cfg, P, ids, _ = _model('prod')
    m.score(ids, None, K, seed=1)
    a = m.score(ids, None, K, seed=1, return_parts=True)
    b = m.score(ids, None, K, seed=1, return_parts=True)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    assert m.score(ids, None, K, seed=1).tobytes() == a['bound'].tobytes()
    c = m.score(ids, None, K, seed=2, return_parts=True)
    for key in ('eps', 'logw', 'bound'):
        assert not np.array_equal(a[key], c[key]), key
    assert np.array_equal(a['ntok'], c['ntok'])


def test_rows_beyond_the_decoder_batch_size_equal_small_calls():
    """production geometry, B = 8, k = 40: 320 (k, r) pairs, above the decoder batch size of 252 rows (2^27 floats of logits / (65 x 8192)) -- batches of 6 rows x 40 draws = 240
    and 2 x 40 = 80 rows.  The same pairs in five calls of k = 8 (64 rows each, one batch) with the same eps."""
    m, cfg, P, ids, _ = _model('prod')
    big = m.score(ids, None, 40, seed=4, return_parts=True)
    assert _plan(m) == [252, 6, 40, 0]          # (65 x 240 tokens >= V: table-fed batches, their projection is per id)
    n = big['ntok'][None]
    for j in range(5):
        sl = slice(8 * j, 8 * j + 8)
        small = m.score(ids, None, 8, eps=big['eps'][sl], return_parts=True)
        assert np.array_equal(small['ntok'], big['ntok'])
        assert (np.abs(small['logpx'] - big['logpx'][sl]) <= TOL_TOK * n).all()
        assert (np.abs(small['logw'] - big['logw'][sl]) <= TOL_TOK * n + TOL_LAT * cfg['dim_rep']).all()
    want = score_ref.log_mean_exp(big['logw'].astype(np.float64))
    assert (np.abs(big['bound'] - want) <= 1e-6 * np.abs(want) + 1e-6).all()


def _plan(m):
    """decoder batches of the model's last score call: [N, rc, kc, batches that shared one first-layer projection through a row index]"""
    out = (C.c_int32 * 4)()
    assert m._l.avae_debug_score_plan(m._h, out) == 0
    return list(out)


def test_draws_of_a_row_share_one_first_layer_projection():
    """production geometry, B = 8, k = 4: one decoder batch of 32 rows, 65 x 32 = 2080 tokens < V, so it is not table-fed; 32 rows have a
    team-kernel geometry, so the first layer projects the 65 x 8 distinct lead rows once and the team kernel reads them through a row
    index (lead_rows + GruJob::gi_rows).  The same pairs one draw at a time (k = 1: nothing to share, every row projected) agree within
    the case-1 tolerance."""
    m, cfg, P, ids, _ = _model('prod')
    eps = _run('prod')['eps']
    shared = m.score(ids, None, K, eps=eps, return_parts=True)
    assert _plan(m) == [32, 8, 4, 1]
    n = shared['ntok']
    for j in range(K):
        plain = m.score(ids, None, 1, eps=eps[j:j + 1], return_parts=True)
        assert _plan(m) == [8, 8, 1, 0]
        assert np.array_equal(plain['ntok'], n)
        assert (np.abs(plain['logpx'][0] - shared['logpx'][j]) <= TOL_TOK * n).all(), (np.abs(plain['logpx'][0] - shared['logpx'][j]) / n).max()
        assert (np.abs(plain['logw'][0] - shared['logw'][j]) <= TOL_TOK * n + TOL_LAT * cfg['dim_rep']).all()


def test_phantom_row_batch_one_row_and_all_eos_rows():
    m, cfg, P, ids8, _ = _model('prod')
    ids = _ragged(cfg, 100, 12, seed=31)
    d = m.score(ids, None, 2, seed=6, return_parts=True)          # 200 decoder rows: the 256-slot geometry with phantom rows
    assert d['bound'].shape == (100,) and np.isfinite(d['bound']).all() and np.isfinite(d['logw']).all()
    assert np.array_equal(d['ntok'], (ids != cfg['eos']).sum(1) + 1)
    one = m.score(ids[:1], None, 2, eps=d['eps'][:, :1], return_parts=True)
    assert one['bound'].shape == (1,) and one['ntok'][0] == d['ntok'][0]
    assert (np.abs(one['logpx'][:, 0] - d['logpx'][:, 0]) <= TOL_TOK * d['ntok'][0]).all()
    tgt = ids8.copy()
    tgt[2] = cfg['eos']
    src = ids8.copy()
    src[5] = cfg['eos']
    e = m.score(src, tgt, K, seed=6, return_parts=True)
    assert e['ntok'][2] == 1 and all(np.isfinite(e[k]).all() for k in ('bound', 'logw', 'logpx'))


def test_bad_arguments_are_errors_with_a_message():
    import torch
    from argsim_amd import lib
    m, cfg, P, ids, _ = _model('mid')
    B, R = len(ids), cfg['dim_rep']
    t = m._ids(m.trim(ids))
    bound = torch.empty(B, dtype=torch.float32, device=m.device)
    p = lambda x: C.c_void_p(x.data_ptr())
    m._stream()

    def call(sc, b=B, bound_=bound, eps=None):
        return m._l.avae_score(m._h, p(t), p(t), b, t.shape[1], t.shape[1], C.byref(sc) if sc is not None else None,
                               p(eps) if eps is not None else None, None, None, None, p(bound_) if bound_ is not None else None, None)
    good = lib.AvaeScoreConfig(2, 0)
    assert call(good) == 0
    for kw, word in ((dict(sc=lib.AvaeScoreConfig(0, 0)), b'k must'), (dict(sc=None), b'null'), (dict(sc=good, b=0), b'empty'),
                     (dict(sc=good, bound_=None), b'bound')):
        rc = call(**kw)
        assert rc != 0 and word in m._l.avae_last_error(m._h), (rc, word, m._l.avae_last_error(m._h))
    eps = torch.zeros((2, B, R), dtype=torch.float32, device=m.device)
    eps[1, 2, 3] = float('nan')
    assert call(good, eps=eps) != 0 and b'finite' in m._l.avae_last_error(m._h)
    eps[1, 2, 3] = 0.0
    assert call(good, eps=eps) == 0                     # the flag does not stick
    with pytest.raises(ValueError):
        m.score(ids, None, 0)
    with pytest.raises(ValueError):
        m.score(ids, None, 2, eps=np.zeros((3, B, R), np.float32))


# ------------------------------------------------------------------------------------------ 6. other dtypes
@pytest.mark.parametrize("name", CASES)
def test_split_bf16_fp32_passes_at_the_fp32_tolerance(name):
    r = _run(name, 'f32s')
    dev, ref = r['dev'], r['ref']
    per = _per_token(r)
    print("%s f32s: max per-token |dlogpx| %.3e" % (name, per))
    assert np.array_equal(dev['ntok'], ref['ntok'])
    assert per <= TOL_TOK
    tol_w = TOL_TOK * ref['ntok'][None] + TOL_LAT * r['R']
    assert (np.abs(dev['logw'] - ref['logw']) <= tol_w).all()
    assert (np.abs(dev['bound'] - ref['bound']) <= tol_w.max(0) + 1e-6 * np.abs(ref['bound']) + 1e-6).all()


def test_bf16_runs_the_production_case():
    r = _run('prod', 'bf16')
    per = _per_token(r)
    print("prod bf16: max per-token |dlogpx| %.3e" % per)
    assert np.array_equal(r['dev']['ntok'], r['ref']['ntok'])
    assert per <= TOL_BF16 and np.isfinite(r['dev']['bound']).all()


# ------------------------------------------------------------------------------------------ 7. driver
def test_summ_iw_on_real_text_is_the_sums_of_score():
    from argsim_amd.train import summ_iw
    m, cfg, P, _, _ = _model('prod')
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'configs0_ids.npz'), allow_pickle=False) as f:
        valid = f['ids'][:64].astype(np.int32)
    nll, ppl = summ_iw(m, valid, 20, 4, 7)
    parts = [m.score(valid[i:i + 20], None, 4, 7, return_parts=True) for i in range(0, 64, 20)]
    b = sum(float(p['bound'].sum(dtype=np.float64)) for p in parts)
    n = sum(int(p['ntok'].sum()) for p in parts)
    assert n == int((valid != cfg['eos']).sum()) + 64
    assert nll == pytest.approx(-b / 64, rel=1e-12) and ppl == pytest.approx(np.exp(-b / n), rel=1e-12)
    assert np.isfinite(nll) and ppl > 1.0
