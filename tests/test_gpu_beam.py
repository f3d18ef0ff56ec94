"""beam-search decoding on the device (avae_decode_beam, avae_debug_beam_select) against the float64 reference of tests/beam_ref.py.

The reference REPLAYS the device's lattice: at every step the hypotheses are the device's, each selection is judged on the device's own
history.  Models and shapes: beam_ref.CASES (tiny, mid, production geometry; widths 1 .. 32; b = 1, 5, 40; one case of 1280 hypotheses
that runs as two groups), whose inputs tests/test_beam.py checks on the CPU.

TOL_TOK.  Not chosen: MAX_DCUM is the largest |device lat_cum - float64 cum along the device's path| / (t + 1) over every case,
measured on MI355X: 5.788e-06 (production geometry, b = 5, width 8, at t = 0: the error of the first step's fp32 logits, |logit| up to 8
over D = 512 products; the production cases measure 2.3e-06 .. 5.8e-06, mid 1.1e-06 .. 2.5e-06, tiny 4.7e-07 .. 8.6e-07, and the figure
per token falls with t).  MAX_DCUM = 5.8e-6 and TOL_TOK = 4 x MAX_DCUM = 2.32e-5 (two competing scores each carry the error);
test_tol_is_four_times_the_measured_cum_error prints the figure again and fails if a run measures more than TOL_TOK / 4 or if
TOL_TOK > 1e-4.  (The sampler's figure on the same logits is 7.0e-6, tests/test_gpu_sampling.py; avae_score's per-token figure on the
same logits path is 1.4e-6.)"""
import ctypes as C

import numpy as np
import pytest

import beam_ref as br

pytestmark = pytest.mark.gpu

MAX_DCUM = 5.8e-6           # measured: 5.788e-06 (production geometry, b = 5, width 8, step 0)
TOL_TOK = 4 * MAX_DCUM
# the select kernel alone on synthetic logits: scores up to 32 in magnitude (fp32 ulp 1.9e-6) formed by three roundings and the logf of
# a sum of up to 8192 terms -- under 5 ulp
SYN_TOL = 1e-5
KEYS = ('dim_tgt', 'dim_emb', 'dim_rep', 'rnn_layers', 'accelerate', 'learn_rate', 'bos', 'eos')
_MODELS, _RUNS = {}, {}
_ID = lambda c: '%s-b%d-w%d-lean%g' % c


def _model(name, lean=0.0):
    key = (name, lean)
    if key not in _MODELS:
        from argsim_amd.model import VAE
        cfg, P, z = br.params(name, lean)
        m = VAE('infer', init=False, **{k: cfg[k] for k in KEYS})
        m.set_params(P)
        _MODELS[key] = (m, cfg, P, z)
    return _MODELS[key]


def _run(case):
    """device run + replay of one case (cached: the tolerance test and the selection test share the runs)"""
    if case not in _RUNS:
        name, b, W, lean = case
        m, cfg, P, z = _model(name, lean)
        out = m.beam(z[:b], steps=br.STEPS[name], width=W, return_all=True)
        ref = br.search(P, cfg, z[:b], br.STEPS[name], W, replay=(out['lat_parent'], out['lat_token']))
        assert ref['n'] == out['n'] and out['lat_cum'].shape == ref['cum'].shape == (out['n'], b, W)
        assert np.isfinite(ref['cum']).all(), "the device took something that is no candidate"
        per_tok = np.abs(out['lat_cum'].astype(np.float64) - ref['cum']) / (np.arange(out['n']) + 1)[:, None, None]
        _RUNS[case] = dict(out=out, ref=ref, dcum=float(per_tok.max()), at=np.unravel_index(per_tok.argmax(), per_tok.shape), cfg=cfg)
    return _RUNS[case]


def test_tol_is_four_times_the_measured_cum_error():
    worst = {c: _run(c)['dcum'] for c in br.CASES}
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    mx = top[0][1]
    print("max |dcum| / (t + 1) over %d cases: %.3e (TOL_TOK / 4 = %.3e); worst cases: %s" % (len(worst), mx, TOL_TOK / 4, top))
    for c in br.CASES:
        print("  %s: %.3e at (t, r, slot) = %s" % (_ID(c), worst[c], tuple(int(i) for i in _RUNS[c]['at'])))
    assert TOL_TOK <= 1e-4
    assert mx <= TOL_TOK / 4, top


@pytest.mark.parametrize("case", br.CASES, ids=_ID)
def test_device_selections_equal_the_float64_reference(case):
    """decidable step (gap > TOL_TOK (t + 1)): the device's chosen set IS the reference's, and neighbours of the reference's order whose
    margin exceeds the tolerance come in that order.  Elsewhere every device choice scores within the tolerance of the reference's
    width-th.  At most 2 % of the (sentence, step) selections of a case may be undecidable."""
    r = _run(case)
    out, ref = r['out'], r['ref']
    n, b, W = out['lat_parent'].shape
    und = 0
    for t in range(n):
        tol = TOL_TOK * (t + 1)
        for s in range(b):
            dev = list(zip(out['lat_parent'][t, s].tolist(), out['lat_token'][t, s].tolist()))
            want = list(zip(ref['ref_parent'][s, t].tolist(), ref['ref_token'][s, t].tolist()))
            assert len(set(dev)) == W, (t, s, dev)
            if ref['gap'][s, t] > tol:
                assert set(dev) == set(want), (t, s, dev, want)
                for i in range(W - 1):
                    if ref['margin'][s, t, i] > tol:
                        assert dev.index(want[i]) < dev.index(want[i + 1]), (t, s, i, dev, want)
            else:
                und += 1
                assert (ref['cum'][t, s] >= ref['kth'][s, t] - tol).all(), (t, s)
    print("%s: %d steps, %d selections, %d undecidable, min gap %.2e, max |dcum| / (t + 1) %.2e" % (_ID(case), n, n * b, und, ref['gap'].min(), r['dcum']))
    assert und <= 0.02 * n * b, (und, n * b)
    # the frozen rule on the device's own lattice: a finished parent is followed by (itself, eos) with its cum
    eos = r['cfg']['eos']
    for t in range(1, n):
        pf = np.take_along_axis(out['lat_token'][t - 1] == eos, out['lat_parent'][t], 1)
        assert (out['lat_token'][t][pf] == eos).all()
        assert np.array_equal(out['lat_cum'][t][pf], np.take_along_axis(out['lat_cum'][t - 1], out['lat_parent'][t], 1)[pf])


@pytest.mark.parametrize("case", [c for c in br.CASES if c[3] > 0 or c[0] == 'prod'], ids=_ID)
@pytest.mark.parametrize("alpha", [0.0, 0.7])
def test_outputs_equal_a_host_backtrack_of_the_returned_lattice_exactly(case, alpha):
    name, b, W, lean = case
    m, cfg, P, z = _model(name, lean)
    out = m.beam(z[:b], steps=br.STEPS[name], width=W, length_alpha=alpha, return_all=True)
    ids, score, cum, ln = br.backtrack(out['lat_parent'], out['lat_token'], out['lat_cum'], cfg['eos'], alpha)
    assert np.array_equal(out['ids'], ids)
    assert np.array_equal(out['len'], ln)
    assert np.array_equal(out['cum'].view(np.int32), cum.view(np.int32))
    assert np.array_equal(out['score'].view(np.int32), score.astype(np.float32).view(np.int32))
    sc = out['score'].astype(np.float64)
    assert (sc[:, :-1] >= sc[:, 1:]).all()                                  # best first
    if alpha == 0.0:
        assert np.array_equal(out['score'], out['cum'])
    # the lattice does not depend on alpha
    base = _run(case)['out']
    for k in ('lat_parent', 'lat_token', 'lat_cum'):
        assert np.array_equal(out[k], base[k]), k


def _raw(m, z, steps, W, alpha=0.0, lattice=True):
    """avae_decode_beam itself, every buffer whole (prefilled with -5) -> (rc, dict)"""
    import torch
    zd = torch.as_tensor(np.ascontiguousarray(z, np.float32)).to(m.device)
    b = zd.shape[0]
    i32, f32 = dict(dtype=torch.int32, device=m.device), dict(dtype=torch.float32, device=m.device)
    t = dict(ids=torch.full((b, W, steps), -5, **i32), score=torch.full((b, W), -5.0, **f32), cum=torch.full((b, W), -5.0, **f32),
             len=torch.full((b, W), -5, **i32))
    if lattice:
        t.update(lat_parent=torch.full((steps, b, W), -5, **i32), lat_token=torch.full((steps, b, W), -5, **i32), lat_cum=torch.full((steps, b, W), -5.0, **f32))
    ptr = lambda k: C.c_void_p(t[k].data_ptr()) if k in t else None
    n = C.c_int32(-9)
    bc = m._l.avae_decode_beam.argtypes[4]._type_(W, alpha)
    m._stream()
    rc = m._l.avae_decode_beam(m._h, C.c_void_p(zd.data_ptr()), b, steps, C.byref(bc), ptr('ids'), ptr('score'), ptr('cum'), ptr('len'),
                               ptr('lat_parent'), ptr('lat_token'), ptr('lat_cum'), C.byref(n))
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in t.items()}
    res['n'] = n.value
    return rc, res


@pytest.mark.parametrize("case", [('mid', 5, 4, 4.0), ('mid', 40, 32, 4.0), ('prod', 5, 8, 3.0)], ids=_ID)
def test_eos_padding_and_the_lattice_beyond_the_steps_run(case):
    """steps above what the search needs: out_ids is eos beyond *n_steps, the lattice beyond it (parent = slot, eos, cum unchanged);
    the optional outputs may be left out; two identical calls give identical bits"""
    name, b, W, lean = case
    m, cfg, P, z = _model(name, lean)
    steps = br.STEPS[name] + 21
    rc, a = _raw(m, z[:b], steps, W)
    assert rc == 0
    n, eos = a['n'], cfg['eos']
    assert 1 <= n <= steps
    if lean >= 4.0:
        assert n < steps                                                    # every hypothesis finished: the loop ended early
        assert (a['lat_token'][n - 1] == eos).all()
        assert n == 1 or (a['lat_token'][n - 2] != eos).any()
    assert (a['ids'][:, :, n:] == eos).all() and (a['ids'] >= 0).all()
    assert (a['lat_token'][n:] == eos).all()
    assert (a['lat_parent'][n:] == np.arange(W)[None, None, :]).all()
    assert np.array_equal(a['lat_cum'][n:].view(np.int32), np.broadcast_to(a['lat_cum'][n - 1], a['lat_cum'][n:].shape).view(np.int32))
    fin = (a['ids'] == eos).any(-1)
    assert (a['len'][~fin] == n).all() and (a['len'][fin] <= n).all() and (a['len'] >= 1).all()
    rc, c = _raw(m, z[:b], steps, W)
    assert rc == 0 and c['n'] == n
    for k in a:
        if k != 'n':
            assert np.array_equal(a[k].view(np.int32), c[k].view(np.int32)), k
    rc, d = _raw(m, z[:b], steps, W, lattice=False)
    assert rc == 0 and d['n'] == n and np.array_equal(d['ids'], a['ids']) and np.array_equal(d['cum'], a['cum'])
    # the same sentences through the default call and the module-level function
    from argsim_amd import model
    best = m.beam(z[:b], steps=steps, width=W)
    assert best.shape[0] == b and np.array_equal(best, model.beam(m, z[:b], steps=steps, width=W))
    keep = best.shape[1]
    assert np.array_equal(best, a['ids'][:, 0, :keep]) and (a['ids'][:, 0, keep:] == eos).all()


def _upto_first_eos(a, eos, steps):
    p = np.full((a.shape[0], steps + 1), eos, np.int32)
    p[:, :a.shape[1]] = a
    return p, (p == eos).argmax(1) + 1


@pytest.mark.parametrize("name,b", [('mid', 8), ('prod', 5), ('prod', 40)])
@pytest.mark.parametrize("persistent", [1, 0])
def test_width_1_is_the_greedy_ids(name, b, persistent):
    """bit-equal to VAE.decode on every row up to and including its first eos (the greedy loop goes on feeding a finished row, the beam
    does not: beyond a row's eos they differ on purpose)"""
    for lean in (0.0, 6.0):
        m, cfg, P, z = _model(name, lean)
        m.set_option('persistent', persistent)
        want, nw = _upto_first_eos(m.decode(z[:b], steps=24), cfg['eos'], 24)
        m.set_option('persistent', 1)
        out = m.beam(z[:b], steps=24, width=1, return_all=True)
        got, ng = _upto_first_eos(out['ids'][:, 0], cfg['eos'], 24)
        assert np.array_equal(ng, nw), lean
        for r in range(b):
            assert np.array_equal(got[r, :ng[r]], want[r, :ng[r]]), (lean, r)
            assert (got[r, ng[r]:] == cfg['eos']).all()
        assert (out['lat_parent'] == 0).all() and (out['cum'] < 0).all()


@pytest.mark.parametrize("case", [c for c in br.CASES if c[3] > 0], ids=_ID)
def test_finished_hypotheses_score_what_avae_score_z_scores(case):
    """every finished hypothesis: the teacher-forced log p(tokens + closing eos | z) of avae_score_z is within TOL_TOK len of its cum"""
    name, b, W, lean = case
    m, cfg, P, z = _model(name, lean)
    out = _run(case)['out']
    eos, n = cfg['eos'], out['n']
    fin = (out['ids'] == eos).any(-1)
    assert fin.any()
    rows, slots = np.nonzero(fin)
    tgt = out['ids'][rows, slots]                                           # (hyps, n), eos from the closing eos on
    logpx, ntok = m.score_z(z[:b][rows], tgt)
    ln = out['len'][rows, slots]
    assert np.array_equal(ntok, ln)
    err = np.abs(logpx.astype(np.float64) - out['cum'][rows, slots]) / ln
    print("%s: %d finished hypotheses, max |score_z - cum| / len %.3e" % (_ID(case), len(rows), err.max()))
    assert (err <= TOL_TOK).all(), float(err.max())


def _select(m, logits, cum, fin, n, W):
    import torch
    x = torch.as_tensor(np.ascontiguousarray(logits, np.float32)).to(m.device)
    c = torch.as_tensor(np.ascontiguousarray(cum, np.float32)).to(m.device)
    f = torch.as_tensor(np.ascontiguousarray(fin, np.int32)).to(m.device)
    rows, V = x.shape
    assert rows == n * W
    i32, f32 = dict(dtype=torch.int32, device=m.device), dict(dtype=torch.float32, device=m.device)
    par, tok, co, fo = torch.full((rows,), -7, **i32), torch.full((rows,), -7, **i32), torch.full((rows,), 7.0, **f32), torch.full((rows,), -7, **i32)
    m._stream()
    rc = m._l.avae_debug_beam_select(m._h, C.c_void_p(x.data_ptr()), n, W, V, C.c_void_p(c.data_ptr()), C.c_void_p(f.data_ptr()),
                                     C.c_void_p(par.data_ptr()), C.c_void_p(tok.data_ptr()), C.c_void_p(co.data_ptr()), C.c_void_p(fo.data_ptr()))
    torch.cuda.synchronize()
    return rc, par.cpu().numpy().reshape(n, W), tok.cpu().numpy().reshape(n, W), co.cpu().numpy().reshape(n, W), fo.cpu().numpy().reshape(n, W)


def _ref_select(logits, cum, fin, n, W, eos):
    """float64 selection of the same inputs (a NaN logit is no candidate and no term of the normaliser)"""
    V = logits.shape[1]
    cum = np.asarray(cum, np.float32).astype(np.float64)                    # (what the device is given)
    l = np.asarray(logits, np.float64).reshape(n, W, V)
    nan = np.isnan(l)
    lc = np.where(nan, -np.inf, l)
    mx = lc.max(-1, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
        logp = (lc - mx) - np.log(np.exp(lc - mx).sum(-1, keepdims=True))
        scores = np.asarray(cum, np.float64).reshape(n, W, 1) + logp
    valid = ~nan
    f = np.asarray(fin, bool).reshape(n, W)
    for r, w in zip(*np.nonzero(f)):
        valid[r, w] = False; valid[r, w, eos] = True; scores[r, w, eos] = np.float64(np.asarray(cum).reshape(n, W)[r, w])
    return [br.select(scores[r], valid[r], W, by=lc[r] if W == 1 else None) for r in range(n)], f


def _check_select(m, logits, cum, fin, n, W, eos, exact=False):
    rc, par, tok, co, fo = _select(m, logits, cum, fin, n, W)
    assert rc == 0
    ref, f = _ref_select(logits, cum, fin, n, W, eos)
    for r in range(n):
        p, k, sc, gap = ref[r]
        dev, want = list(zip(par[r].tolist(), tok[r].tolist())), list(zip(p.tolist(), k.tolist()))
        if exact:
            assert dev == want, (r, dev, want)
        elif gap > SYN_TOL:
            assert set(dev) == set(want), (r, dev, want)
            for i in range(W - 1):
                if sc[i] - sc[i + 1] > SYN_TOL:
                    assert dev.index(want[i]) < dev.index(want[i + 1]), (r, i)
        if exact or gap > SYN_TOL:
            order = [want.index(d) for d in dev]
            with np.errstate(invalid='ignore'):
                d = np.abs(co[r].astype(np.float64) - sc[order])
            same_inf = np.isinf(sc[order]) & (co[r] == sc[order])
            assert ((d <= SYN_TOL) | same_inf).all(), (r, co[r], sc[order])
        assert np.array_equal(fo[r] != 0, f[r][par[r]] | (tok[r] == eos)), r
    return par, tok, co, fo


def test_select_kernel_alone():
    """avae_debug_beam_select on synthetic logits: exact ties at the threshold resolve by (slot, token); a -inf slot; a NaN logit;
    all but one hypothesis finished; width 32 at V = 8192"""
    m, cfg = _model('tiny')[:2]
    eos = cfg['eos']
    rng = np.random.default_rng(0)
    # identical rows and equal cums: 3 tokens of value 3 in each of 4 rows -> 12 candidates tie bit for bit for 4 slots
    n, W, V = 2, 4, 64
    x = np.full((n * W, V), 1.0, np.float32)
    x[:, [5, 9, 40]] = 3.0
    par, tok, co, fo = _check_select(m, x, np.zeros(n * W), np.zeros(n * W), n, W, eos, exact=True)
    assert par.tolist() == [[0, 0, 0, 1]] * 2 and tok.tolist() == [[5, 9, 40, 5]] * 2
    # everything ties (flat rows): slot 0's first tokens; and with the cums apart, the best slot's
    par, tok, _, _ = _check_select(m, np.zeros((n * W, V), np.float32), np.zeros(n * W), np.zeros(n * W), n, W, eos, exact=True)
    assert par.tolist() == [[0] * 4] * 2 and tok.tolist() == [[0, 1, 2, 3]] * 2
    par, tok, _, _ = _check_select(m, np.zeros((n * W, V), np.float32), np.array([-3.0, -1.0, -2.0, -1.0] * 2), np.zeros(n * W), n, W, eos, exact=True)
    assert par.tolist() == [[1] * 4] * 2 and tok.tolist() == [[0, 1, 2, 3]] * 2
    # a tie at the threshold of ONE row that the tokens decide, behind larger candidates of another row
    x = rng.standard_normal((n * W, V)).astype(np.float32)
    x[1] = x[0]                                                             # slots 0 and 1 of sentence 0: the same row, the same cum
    _check_select(m, x, np.array([0.0, 0.0, -9.0, -9.0, -1.0, -2.0, -3.0, -4.0]), np.zeros(n * W), n, W, eos, exact=True)
    # a -inf slot (never before a number), -inf logits, and a sentence whose slots are all -inf but one
    x = (2.0 * rng.standard_normal((n * W, V))).astype(np.float32)
    x[2, ::2] = -np.inf
    cum = np.array([-1.0, -np.inf, -0.5, -2.0, -np.inf, -np.inf, -1.0, -np.inf])
    par, tok, co, fo = _check_select(m, x, cum, np.zeros(n * W), n, W, eos)
    assert not np.isin(par[0], [1]).any() and (par[1] == 2).all() and np.isfinite(co).all()
    # NaN logits: no candidate before a number, not in the normaliser
    x = (2.0 * rng.standard_normal((n * W, V))).astype(np.float32)
    x[0, ::3] = np.nan
    x[5, :] = np.nan
    x[5, 7] = 0.5                                                           # one number: logp 0
    par, tok, co, fo = _check_select(m, x, np.array([-1.0, -1.5, -0.5, -2.0, -3.0, -0.25, -1.0, -2.0]), np.zeros(n * W), n, W, eos)
    assert not np.isnan(x[par[0], tok[0]]).any() and (par[1, 0], tok[1, 0]) == (1, 7) and co[1, 0] == np.float32(-0.25)
    assert not np.isnan(co).any()
    # all but one hypothesis finished: the finished offer (cum, eos) alone
    x = (2.0 * rng.standard_normal((n * W, V))).astype(np.float32)
    fin = np.array([1, 1, 0, 1, 1, 0, 1, 1])
    cum = np.array([-4.0, -2.0, -1.0, -3.0, -0.5, -6.0, -0.7, -0.6])
    par, tok, co, fo = _check_select(m, x, cum, fin, n, W, eos)
    for r in range(n):
        for j in range(W):
            if fin[r * W + par[r, j]]:
                assert tok[r, j] == eos and co[r, j] == np.float32(cum[r * W + par[r, j]]) and fo[r, j]
    assert par[1, :3].tolist() == [0, 3, 2]                                 # sentence 1: its three finished ones lead (-0.5, -0.6, -0.7)
    # every hypothesis finished: the beam stays as it is
    par, tok, co, fo = _check_select(m, x, np.array([-1.0, -2.0, -3.0, -4.0] * 2), np.ones(n * W), n, W, eos, exact=True)
    assert par.tolist() == [[0, 1, 2, 3]] * 2 and (tok == eos).all() and fo.all()
    # width 32 at V = 8192, and width 1 (the first maximum of the logits)
    n, W, V = 3, 32, 8192
    x = (3.0 * rng.standard_normal((n * W, V))).astype(np.float32)
    fin = (rng.random(n * W) < 0.2).astype(np.int32)
    _check_select(m, x, -5.0 * rng.random(n * W), fin, n, W, eos)
    x = np.round(2.0 * rng.standard_normal((6, V))).astype(np.float32)       # many equal maxima
    par, tok, _, _ = _check_select(m, x, -rng.random(6), np.zeros(6), 6, 1, eos, exact=True)
    assert np.array_equal(tok[:, 0], x.argmax(1))


def test_bad_arguments_are_errors_with_a_message_and_launch_nothing():
    import torch
    m, cfg, P, z = _model('mid')
    zd = torch.as_tensor(z[:4]).to(m.device)
    out = torch.full((4, 32, 8), -5, dtype=torch.int32, device=m.device)
    n = C.c_int32(-9)
    mk = m._l.avae_decode_beam.argtypes[4]._type_
    zp, op = C.c_void_p(zd.data_ptr()), C.c_void_p(out.data_ptr())
    none = [None] * 6

    def refused(rc, what):
        assert rc != 0 and len(m._l.avae_last_error(m._h)) > 0, what
        torch.cuda.synchronize()
        assert bool((out == -5).all()) and n.value == -9, what

    for W, a, b, steps in ((0, 0.0, 4, 8), (-1, 0.0, 4, 8), (33, 0.0, 4, 8), (4, -0.5, 4, 8), (4, float('nan'), 4, 8), (4, float('inf'), 4, 8),
                           (4, 0.0, 0, 8), (4, 0.0, -2, 8), (4, 0.0, 4, 0), (4, 0.0, 4, -3), (4, 0.0, 4, (1 << 20) + 1)):
        bc = mk(W, a)
        refused(m._l.avae_decode_beam(m._h, zp, b, steps, C.byref(bc), op, *none, C.byref(n)), (W, a, b, steps))
    bc = mk(4, 0.0)
    refused(m._l.avae_decode_beam(m._h, zp, 4, 8, None, op, *none, C.byref(n)), 'null bc')
    refused(m._l.avae_decode_beam(m._h, None, 4, 8, C.byref(bc), op, *none, C.byref(n)), 'null z')
    refused(m._l.avae_decode_beam(m._h, zp, 4, 8, C.byref(bc), None, *none, C.byref(n)), 'null out_ids')
    # width above dim_tgt: a vocabulary of 8
    from argsim_amd.model import VAE
    small = VAE('infer', seed=1, dim_tgt=8, dim_emb=16, dim_rep=8, rnn_layers=1)
    zs = torch.zeros((4, 8), dtype=torch.float32, device=small.device)
    bc = mk(9, 0.0)
    rc = small._l.avae_decode_beam(small._h, C.c_void_p(zs.data_ptr()), 4, 8, C.byref(bc), op, *none, C.byref(n))
    assert rc != 0 and b'dim_tgt' in small._l.avae_last_error(small._h)
    torch.cuda.synchronize()
    assert bool((out == -5).all()) and n.value == -9
    with pytest.raises(ValueError):
        small.beam(np.zeros((4, 8), np.float32), width=9)
    assert small.beam(np.zeros((4, 8), np.float32), steps=6, width=8, return_all=True)['ids'].shape[:2] == (4, 8)
    small.close()
    rc = _select(m, np.zeros((4, 8), np.float32), np.zeros(4), np.zeros(4), 1, 4)[0]
    assert rc == 0
    rc, par = _select(m, np.zeros((33, 64), np.float32), np.zeros(33), np.zeros(33), 1, 33)[:2]
    assert rc != 0 and (par == -7).all()
    rc, par = _select(m, np.zeros((9, 8), np.float32), np.zeros(9), np.zeros(9), 1, 9)[:2]
    assert rc != 0 and (par == -7).all()
    with pytest.raises(ValueError):
        m.beam(z[:4], length_alpha=-1.0)
    with pytest.raises(ValueError):
        m.beam(z[:4, :5])
    # and the public call works on the same handle afterwards
    ids = m.beam(z[:3], steps=12, width=4)
    assert ids.shape[0] == 3 and ids.shape[1] <= 12
