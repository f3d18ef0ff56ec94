"""One-launch decoding (csrc/decode.hip) at every branch of its launch geometry, against the float64 references of tests/sampling_ref.py and
tests/nucleus_ref.py: the cases of tests/decode_geom.py (embedding block in LDS or read from global memory, the same model caching it in one mode
and not in another, ragged and empty vocabulary blocks, D = 32 .. 512, L = 1 .. 8, refused geometries, b = 17), each in five modes (greedy, sampled,
top-k, nucleus, top-k then nucleus), on the one-launch path and on the launch-per-token loop.

Which code a case runs is asked of the library itself for the device at hand (avae_debug_decode_plan with G = 0) and held against the case's claimed
reach; tests/test_decode_plan.py proves the same table without a GPU.  The calls go through the C entry points on buffers with guard words
behind b * steps.  The references REPLAY the device's tokens (and are told its nkept), so every position is judged on the device's own history;
the rules are those of tests/test_gpu_sampling.py and tests/test_gpu_nucleus.py.

TOL.  Not chosen in advance: 4 x the largest |device logp - float64 logp| at the device's own tokens over every run below, on positions whose
top-k boundary gap exceeds 1e-3 (two competing scores each carry the error).  Measured on MI355X over the 110 runs, per geometry, one launch /
launch per token (where a geometry is refused both options run the per-token loop):
    nocache        1.974e-06 (sampled, b 32)          8.067e-06 (sampled, b 32)
    cache-by-mode  1.985e-06 (sampled)                6.790e-06 (top-k then nucleus)
    deep           1.997e-06 (sampled)                7.100e-06 (sampled)
    refused        --                                 8.163e-06 (sampled)
    bigv           1.745e-06 (sampled)                5.665e-06 (top-k)
    d256           1.685e-06 (nucleus)                3.521e-06 (sampled)
    d256-ragged    1.505e-06 (sampled)                6.035e-06 (sampled)
    d128           1.130e-06 (sampled)                2.981e-06 (top-k then nucleus)
    d32            2.233e-06 (sampled)                2.283e-06 (sampled)
The largest is 8.163e-06 (refused: D 512, L 7, V 512, sampled at T 0.7, b 17, the per-token loop), so MAX_DLOGP = 8.2e-6 and TOL = 3.28e-5;
test_tol_is_four_times_the_measured_logp_error prints the figures again and fails if a run measures more than TOL / 4 or if TOL > 1e-3.  With
this TOL the most undecidable case has 4 of 1810 emitted positions (cache-by-mode: 0.2 %; the cap is 2 %).
TOL_MASS, the bound on the violation of a nucleus (nucleus_ref.judge), is derived, not measured: a share of the mass is exp(logp), so an error
eps <= TOL / 4 in the logits moves the mass at or above a boundary, c, by at most 2 eps c (1 - c) <= eps / 2, and the device's 2^-40 fixed-point
weights truncate at most V 2^-40 <= 8192 x 2^-40 of it: TOL_MASS = TOL / 8 + 2^-27.  Largest violation measured: 0 in every run.
One thing the float64 reference cannot decide: the nucleus keeps whole tie groups, and two logits less than an fp32 rounding apart are ONE group on
the device and two in float64 -- the device then keeps the second with the first although the first alone holds top_p (seen once: d128, top-k then
nucleus, per-token loop, row 13, step 1: the 34th and 35th logit 7.5e-7 apart in float64, bit-equal on the device, which keeps 35 where the reference
keeps 34).  Where the device's last value lies within TOL under the reference's last (nucleus_ref.judge: tie), its size is not held against the
reference's; the position counts as undecidable, and logp and the token are still judged over the device's own set.

Safety: the kernel's spins are bounded (2 s, error word); the first unexpected non-zero return or failed synchronise sets a module latch, and every
later case fails at once without launching."""
import ctypes as C

import numpy as np
import pytest

import decode_geom as dg
import nucleus_ref as nr
import sampling_ref as sr

pytestmark = pytest.mark.gpu

MAX_DLOGP = 8.2e-6          # measured: 8.163e-06 (see the docstring)
TOL = 4 * MAX_DLOGP
TOL_MASS = TOL / 8 + 2.0 ** -27
GUARD = 64                                 # words behind b * steps of every output
SENT = -0x5A5A5A5B                         # their content (bits a5a5a5a5; as float32 -2.9e-16: no value a call writes)
KEYS = ('dim_tgt', 'dim_emb', 'dim_rep', 'rnn_layers', 'accelerate', 'learn_rate', 'bos', 'eos')
RUNS = [(c, mode, b) for c in dg.CASES for mode in dg.MODE_NAMES for b in c.batches]
_LATCH, _MODELS, _DEV, _REF = [], {}, {}, {}


def _id(v):
    return v.name if isinstance(v, dg.Case) else str(v)


def guard():
    if _LATCH:
        pytest.fail('not run after an earlier GPU failure: %s' % _LATCH[0])


def trip(what):
    _LATCH.append(what)
    pytest.fail(what)


def f32(p):
    return float(np.float32(p))


def model(c):
    """the case's VAE: only what decoding reads is set (the encoder's tensors stay zero)"""
    if c.name not in _MODELS:
        guard()
        from argsim_amd.model import VAE
        cfg, P, z = dg.params(c)
        m = VAE('infer', init=False, **{k: cfg[k] for k in KEYS})
        for k in P:
            m.set_tensor(k, P[k])
        _MODELS[c.name] = m
    return _MODELS[c.name]


def device_plan(c, mode, b, persistent):
    from argsim_amd import lib
    return dg.ask(lib.load(), dg.hook_ints(c, mode, b, persistent, G=0, lds_max=0))


def device_run(c, mode, b, persistent):
    """one call of the C entry point on guarded buffers -> dict: n (n_steps), out (b, STEPS) i32, logp (b, STEPS) f32 / nk (b, STEPS) i32 or None
    (the whole buffers, as the call left them), err (avae_last_error afterwards)"""
    key = (c.name, mode, b, persistent)
    if key in _DEV:
        return _DEV[key]
    guard()
    import torch
    from argsim_amd import lib
    m, md = model(c), dg.MODES[mode]
    cfg, P, z = dg.params(c)
    what = '%s %s b %d persistent %d' % key
    n_el = b * dg.STEPS
    zd = torch.as_tensor(z[:b]).to(m.device).contiguous()
    out = torch.full((n_el + GUARD,), SENT, dtype=torch.int32, device=m.device)
    logp = nk = None
    if md['sampled']:
        logp = torch.full((n_el + GUARD,), SENT, dtype=torch.int32, device=m.device).view(torch.float32)
    if md['p'] > 0.0:
        nk = torch.full((n_el + GUARD,), SENT, dtype=torch.int32, device=m.device)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    n = C.c_int32(-9)
    m.set_option('persistent', persistent)
    m._stream()
    if not md['sampled']:
        rc = m._l.avae_decode_greedy(m._h, ptr(zd), b, dg.STEPS, ptr(out), C.byref(n))
    elif nk is None:
        sc = lib.AvaeSampleConfig(md['T'], md['k'], c.seed)
        rc = m._l.avae_decode_sample(m._h, ptr(zd), b, dg.STEPS, C.byref(sc), ptr(out), ptr(logp), C.byref(n))
    else:
        sc = lib.AvaeSamplePConfig(md['T'], md['k'], c.seed, md['p'], 0)
        rc = m._l.avae_decode_sample_p(m._h, ptr(zd), b, dg.STEPS, C.byref(sc), ptr(out), ptr(logp), ptr(nk), C.byref(n))
    err = (m._l.avae_last_error(m._h) or b'').decode()
    if rc != 0:
        trip('%s: return %d: %s' % (what, rc, err))
    try:
        torch.cuda.synchronize()
    except Exception as e:          # noqa: BLE001 -- whatever the runtime raises: nothing more is launched
        trip('%s: synchronise failed: %s' % (what, e))
    m.set_option('persistent', 1)
    res = dict(n=n.value, err=err)
    for name, t in (('out', out), ('logp', logp), ('nk', nk)):
        if t is None:
            res[name] = None
            continue
        a = t.view(torch.int32).cpu().numpy()
        assert (a[n_el:] == SENT).all(), '%s: %s written behind b * steps' % (what, name)
        assert (a[:n_el] != SENT).all(), '%s: %s not written everywhere' % (what, name)
        res[name] = a[:n_el].view(np.float32 if name == 'logp' else np.int32).reshape(b, dg.STEPS).copy()
    assert 0 <= res['n'] <= dg.STEPS, (what, res['n'])
    _DEV[key] = res
    return res


def upto_first_eos(a, eos):
    """(b, n) ids with everything behind a row's first eos set to eos"""
    a = a.copy()
    seen = np.cumsum(a == eos, axis=1) > 0
    a[seen] = eos
    return a


def judged(c, mode, b, persistent):
    """the device run and the float64 replay of it -> dict (cached: the tolerance test and the per-run test share it)"""
    key = (c.name, mode, b, persistent)
    if key in _REF:
        return _REF[key]
    d, md = device_run(c, mode, b, persistent), dg.MODES[mode]
    cfg, P, z = dg.params(c)
    eos, n = cfg['eos'], d['n']
    ids = d['out'][:, :n]
    w = min(n + 1, dg.STEPS)
    r = dict(d=d, ids=ids, family='greedy', dlogp=0.0, viol=0.0)
    if not md['sampled']:
        # the greedy loop goes on feeding a finished row: a row is compared up to and including its first eos
        r['ref'] = ref = sr.sample(P, cfg, z[:b], dg.STEPS, 0.0, 0, c.seed, replay=upto_first_eos(ids, eos))
        assert ref['live'].shape[1] <= w
    elif md['p'] == 0.0:
        r['family'] = 'sampled'
        r['ref'] = ref = sr.sample(P, cfg, z[:b], dg.STEPS, md['T'], md['k'], c.seed, replay=ids)
        assert ref['live'].shape == (b, w) and ref['n_steps'] == n, (ref['live'].shape, ref['n_steps'], n)
        same_set = ref['live'] & (ref['gap'] > 1e-3)          # (the ceiling of TOL: the measurement must not depend on TOL)
        r['dlogp'] = float(np.abs(d['logp'][:, :w] - ref['logp_dev'])[same_set].max())
    else:
        r['family'] = 'nucleus'
        r['ref'] = ref = nr.sample(P, cfg, z[:b], dg.STEPS, md['T'], md['k'], f32(md['p']), c.seed, replay=ids, nkept=d['nk'][:, :w])
        assert ref['live'].shape == (b, w) and ref['n_steps'] == n, (ref['live'].shape, ref['n_steps'], n)
        same_k0 = ref['live'] & (ref['gap'] > 1e-3)
        r['viol'] = float(ref['viol'][same_k0 & (ref['tie'] > 1e-3)].max())
        r['dlogp'] = float(np.abs(d['logp'][:, :w] - ref['logp_set'])[same_k0 & np.isfinite(ref['viol'])].max())
    live = r['ref']['live']
    if r['family'] == 'nucleus':
        r['und'] = live & ~((r['ref']['margin_set'] > TOL) & (r['ref']['gap'] > TOL) & (r['ref']['tie'] > TOL))
    else:
        r['und'] = live & ~((r['ref']['margin'] > TOL) & (r['ref']['gap'] > TOL))
    _REF[key] = r
    return r


@pytest.mark.parametrize("c", dg.CASES, ids=_id)
def test_every_case_reaches_its_claimed_form_on_this_device(c):
    for mode in dg.MODE_NAMES:
        for b in c.batches:
            p = device_plan(c, mode, b, 1)
            where = 'this device has %d CUs and %d bytes of LDS per workgroup, the table is for %d and %d' % (p['G'], p['lds_max'], dg.G_REF, dg.LDS_REF)
            assert (p['route'], p['nu'], p['vp'], p['cache_e']) == c.reach[mode], (c.name, mode, b, p, where)
            assert p['kmode'] == dg.kmode(c, mode), (c.name, mode, p, where)
            assert device_plan(c, mode, b, 0)['route'] == 1
        assert device_plan(c, mode, 33, 1)['route'] == 1


@pytest.mark.parametrize("persistent", [1, 0])
@pytest.mark.parametrize("c,mode,b", RUNS, ids=_id)
def test_tokens_logp_and_nkept_against_the_float64_reference(c, mode, b, persistent):
    """decidable position (top-2 score margin > TOL and, with top-k, boundary gap > TOL): the device token IS the reference's; elsewhere it scores
    within TOL of the best.  logp within TOL where the kept sets must agree.  Nucleus: the device's set is a prefix of whole tie groups with violation
    <= TOL_MASS, the reference's own where the boundary margin exceeds TOL_MASS -- unless it ends within TOL under the reference's last value (see the
    docstring of the file).  Finished rows: eos, logp 0, nkept 0; 0 / eos behind n_steps."""
    r = judged(c, mode, b, persistent)
    d, ref, md = r['d'], r['ref'], dg.MODES[mode]
    eos = dg.params(c)[0]['eos']
    live, und, n = ref['live'], r['und'], d['n']
    w = live.shape[1]
    dec = live & ~und
    print("%s %s b %d persistent %d: n_steps %d, %d live, %d undecidable, max dlogp %.3e, max violation %.3e" %
          (c.name, mode, b, persistent, n, live.sum(), und.sum(), r['dlogp'], r['viol']))
    assert live.sum() >= b and (d['out'][:, n:] == eos).all()
    if r['family'] == 'nucleus':
        logp, nk = d['logp'][:, :w], d['nk'][:, :w]
        k0 = live & (ref['gap'] > TOL)                       # the top-k sets agree: the nucleus is judged
        # ... and its size, unless the device's last value lies within TOL under the reference's last: one tie group in fp32, kept whole
        sized = k0 & (ref['tie'] > TOL)
        assert (ref['viol'][sized] <= TOL_MASS).all(), np.argwhere(sized & ~(ref['viol'] <= TOL_MASS))[:5]
        assert np.isfinite(ref['viol'][k0]).all()
        assert (np.abs(logp - ref['logp_set'])[k0] <= TOL).all()
        assert np.array_equal(ref['dev'][dec], ref['win'][dec].astype(np.int32)), np.argwhere(dec & (ref['dev'] != ref['win']))[:5]
        assert (ref['deficit_set'][und & k0] <= TOL).all()
        clear = sized & (ref['bmargin'] > TOL_MASS)
        assert (ref['same'][clear] == 1).all() and np.array_equal(nk[clear], ref['nkept_ref'][clear].astype(np.int32))
        assert (nk[live] >= 1).all() and (nk[live] <= c.V).all()
        assert (logp[~live] == 0.0).all() and (nk[~live] == 0).all() and (ref['dev'][~live] == eos).all()
        assert (d['logp'][:, w:] == 0.0).all() and (d['nk'][:, w:] == 0).all()
    else:
        assert np.array_equal(ref['dev'][dec], ref['token'][dec]), np.argwhere(dec & (ref['dev'] != ref['token']))[:5]
        assert (ref['deficit'][und] <= TOL).all()
        assert (ref['dev'][~live] == eos).all()
        if r['family'] == 'sampled':
            logp = d['logp'][:, :w]
            assert (ref['below'][und] <= TOL * md['T']).all()
            chk = live & (ref['gap'] > TOL)
            assert np.abs(logp - ref['logp_dev'])[chk].max() <= TOL
            assert (logp[~live] == 0.0).all() and (d['logp'][:, w:] == 0.0).all()


@pytest.mark.parametrize("c", dg.CASES, ids=_id)
def test_greedy_ids_are_bit_equal_on_both_paths(c):
    """one launch against the launch-per-token loop (another summation order: equal unless two logits tie to rounding, which the seeds avoid);
    a refused geometry runs the per-token loop either way"""
    for b in c.batches:
        one, per = device_run(c, 'greedy', b, 1), device_run(c, 'greedy', b, 0)
        assert one['n'] == per['n'] and np.array_equal(one['out'], per['out']), (c.name, b, one['n'], per['n'])


@pytest.mark.parametrize("c,mode", [(c, m) for c in dg.CASES for m in dg.MODE_NAMES if c.reach[m][0] == 2], ids=_id)
def test_a_refused_geometry_runs_the_per_token_loop_without_an_error(c, mode):
    for b in c.batches:
        assert device_plan(c, mode, b, 1)['route'] == 2
        one, per = device_run(c, mode, b, 1), device_run(c, mode, b, 0)
        assert one['err'] == '' and per['err'] == ''
        assert one['n'] == per['n']
        for k in ('out', 'logp', 'nk'):
            assert (one[k] is None) == (per[k] is None)
            assert one[k] is None or one[k].tobytes() == per[k].tobytes(), (c.name, mode, b, k)


def test_the_lean_case_ends_rows_early():
    (c,) = [c for c in dg.CASES if c.eos_lean]
    for mode in dg.MODE_NAMES[1:]:
        live = judged(c, mode, 17, 1)['ref']['live']
        ends = live.sum(1)
        assert (~live).any() and len(set(ends.tolist())) > 1, (mode, ends)


@pytest.mark.parametrize("c", dg.CASES, ids=_id)
def test_at_most_2_percent_of_a_case_is_undecidable(c):
    und = tot = 0
    for cc, mode, b in RUNS:
        if cc is c:
            for persistent in (1, 0):
                r = judged(c, mode, b, persistent)
                und, tot = und + int(r['und'].sum()), tot + int(r['ref']['live'].sum())
    print("%s: %d of %d emitted positions undecidable" % (c.name, und, tot))
    assert und <= 0.02 * tot, (c.name, und, tot)


def test_tol_is_four_times_the_measured_logp_error():
    """max |device logp - float64 logp| at the device's own tokens over all runs (positions whose top-k boundary is further than 1e-3 from a tie),
    per geometry; TOL = 4 x MAX_DLOGP must cover it and be <= 1e-3.  The largest violation of a nucleus is printed beside it."""
    worst, viol = {}, {}
    for c, mode, b in RUNS:
        for persistent in (1, 0):
            r = judged(c, mode, b, persistent)
            worst[(c.name, mode, b, persistent)] = r['dlogp']
            viol[(c.name, mode, b, persistent)] = r['viol']
    for c in dg.CASES:
        k = max((k for k in worst if k[0] == c.name), key=lambda k: worst[k])
        print("%-14s max |dlogp| %.3e at %s" % (c.name, worst[k], k[1:]))
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    tv = sorted(viol.items(), key=lambda kv: -kv[1])[:3]
    print("max |dlogp| over %d runs: %.3e (TOL / 4 = %.3e); worst runs: %s" % (len(worst), top[0][1], TOL / 4, top))
    print("max violation: %.3e (TOL_MASS = %.3e); worst runs: %s" % (tv[0][1], TOL_MASS, tv))
    assert TOL <= 1e-3
    assert top[0][1] <= TOL / 4, top
