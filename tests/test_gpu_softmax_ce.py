"""The loss head kernel by kernel: every form of softmax_ce (ops.hip) and argmax_rows against the float64 reference of
model.py:170-181 (tests/helpers.softmax_ce_reference) on the same input values, through the test hooks avae_debug_softmax_ce /
avae_debug_argmax_rows.  Each case asserts the form it meant to reach (softmax_ce_form: 0 register, 1 fp16 panel, 2 streaming).

Tolerances (from the fp32 arithmetic of the kernels; scale = inv_n, or 1 / n rows when inv_n <= 0):
    loss              |got - ref| <= 2^-20 (1 + |max logit| + |label logit|)      largest seen on MI355X: 0.38 of it
    fp32 gradient     |got - ref| <= 2^-22 scale, elementwise                      0.50 of it (derived 2^-20; tightened to 4x the largest seen)
    bf16 gradient     |got - ref| <= 2^-8 |ref| + 2^-20 scale, elementwise         0.99 of it (bf16 keeps 8 significant bits: nearest even
                                                                                   is 2^-8 relative, the bound is that plus the fp32 error)
    pred, errt        exact (pred = the FIRST maximum)
Rows at or beyond the device-side row count keep their sentinels bit for bit.

Then the fp16 logits panel of the phased GEMM at values beyond the fp16 range (saturated, NaN kept), and the whole model at
trained-like logit scale (|logit| ~ 40) against the live oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import ce_scale, make_case, rel_l2, softmax_ce_reference

pytestmark = pytest.mark.gpu

REG, H16, STREAM = 0, 1, 2
FORM_NAME = {REG: 'reg', H16: 'h16', STREAM: 'stream'}
ULP20 = 2.0 ** -20
ULP22 = 2.0 ** -22
BF16_REL = 2.0 ** -8
SENT_F = -1234.5           # loss / errt sentinel
SENT_I = -7                # pred sentinel
SENT_PANEL = 0x7777        # bf16 gradient panel sentinel
KINDS = ('rand', 'peaked', 'equal', 'span80', 'f16max')


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture(scope='module')
def vae():
    from argsim_amd.model import VAE
    m = VAE('train', dtype='bf16', dim_tgt=64, dim_emb=16, dim_rep=8, rnn_layers=1)
    yield m
    m.close()


def expected_form(V, mode):
    if V > 8192:
        return STREAM
    return H16 if mode == 'panel' and V % 8 == 0 else REG


def make_logits(n, V, seed, kinds=KINDS):
    """(n, V) float64 on the device; row r is of kind kinds[(r // 5) % len(kinds)]:
    rand    sigma 1 (random initialisation)
    peaked  sigma 20 and one column 60 above the rest (a trained model)
    equal   every column the same value
    span80  uniform over [-80, 80] (exp underflows in the exp2 path)
    f16max  the fp16 range's edge: columns at 65504, 65472, 65440 and -65504 over sigma-2000 noise"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn((n, V), device='cuda', dtype=torch.float64, generator=g)
    kind = torch.tensor([KINDS.index(kinds[(r // 5) % len(kinds)]) for r in range(n)], device='cuda')
    pk = kind == KINDS.index('peaked')
    x[pk] *= 20.0
    col = torch.randint(0, V, (n,), device='cuda', generator=g)
    rows = torch.arange(n, device='cuda')
    x[rows[pk], col[pk]] = x[pk].max(-1).values + 60.0
    x[kind == KINDS.index('equal')] = 3.25
    sp = kind == KINDS.index('span80')
    x[sp] = torch.rand((int(sp.sum()), V), device='cuda', dtype=torch.float64, generator=g) * 160.0 - 80.0
    fm = kind == KINDS.index('f16max')
    if bool(fm.any()):
        xf = x[fm].clamp(-6, 6) * 2000.0
        k = xf.shape[0]
        for v in (65504.0, 65472.0, 65440.0, -65504.0):
            xf[torch.arange(k, device='cuda'), torch.randint(0, V, (k,), device='cuda', generator=g)] = v
        x[fm] = xf
    return x


def pick_labels(xs, seed):
    """row r % 5: column 0, column V - 1, the row's (first) argmax, its argmin, a random column"""
    n, V = xs.shape
    x = xs.double()
    g = torch.Generator(device='cuda').manual_seed(seed + 1)
    choice = torch.stack([torch.zeros(n, dtype=torch.long, device='cuda'), torch.full((n,), V - 1, dtype=torch.long, device='cuda'),
                          x.argmax(-1), x.argmin(-1), torch.randint(0, V, (n,), device='cuda', generator=g)])
    return choice[torch.arange(n, device='cuda') % 5, torch.arange(n, device='cuda')]


def stored(x, mode):
    return x.half() if mode == 'panel' else x.float()


def run_ce(m, xs, labels, mode, n_dev, inv_n, seed=0):
    """softmax_ce on xs (n_max x V: fp32 logits, or the fp16 panel for mode 'panel') through the hook, labels through a
    non-identity cidx permutation into a larger gold array.  -> dict of the buffers after the call and the form"""
    n_max, V = xs.shape
    G = n_max + 3
    g = torch.Generator().manual_seed(seed * 7919 + n_max * 31 + V)
    perm = torch.randperm(G, generator=g)[:n_max]
    gold = torch.randint(0, V, (G,), generator=g, dtype=torch.int32)
    gold[perm] = labels.to('cpu', torch.int32)
    gold, cidx = gold.cuda(), perm.to(torch.int32).cuda()
    ndev = torch.tensor([n_dev], dtype=torch.int32, device='cuda')
    o = dict(loss=torch.full((n_max,), SENT_F, device='cuda'), errt=torch.full((n_max,), SENT_F, device='cuda'),
             pred=torch.full((n_max,), SENT_I, dtype=torch.int32, device='cuda'), logits=None, panel=None)
    if mode == 'panel':
        o['panel'] = xs.clone().view(torch.int16)
    else:
        o['logits'] = xs.clone()
        if mode == 'f32_bf16':
            o['panel'] = torch.full((n_max, V), SENT_PANEL, dtype=torch.int16, device='cuda')
    form = C.c_int(-9)
    m._stream()
    rc = m._l.avae_debug_softmax_ce(m._h, _p(o['logits']), _p(o['panel']), int(mode == 'panel'), _p(gold), _p(cidx), _p(ndev), n_max, V,
                                    int(mode != 'eval'), float(inv_n), _p(o['loss']), _p(o['errt']), _p(o['pred']), C.byref(form))
    assert rc == 0, m._l.avae_last_error(m._h)
    torch.cuda.synchronize()
    o['form'] = form.value
    return o


def check_ce(o, xs, labels, mode, n_dev, inv_n, record=None):
    """every output against the float64 reference; rows >= n keep their sentinels; -> (loss ratio, grad ratio) to the bounds"""
    n_max, V = xs.shape
    n = max(0, min(n_max, n_dev))
    scale = ce_scale(inv_n, n_dev, n_max)
    assert bool((o['loss'][n:] == SENT_F).all()) and bool((o['errt'][n:] == SENT_F).all()) and bool((o['pred'][n:] == SENT_I).all())
    if mode == 'panel':
        assert torch.equal(o['panel'][n:], xs[n:].view(torch.int16))
    else:
        assert torch.equal(o['logits'][n:], xs[n:])
        if mode != 'f32':
            assert torch.equal(o['logits'], xs)            # the logits stay where the gradient goes elsewhere (or nowhere)
        if mode == 'f32_bf16':
            assert bool((o['panel'][n:] == SENT_PANEL).all())
    if n == 0:
        return 0.0, 0.0
    x = xs[:n].double()
    lab = labels[:n].long()
    rl, rp, re, rg = softmax_ce_reference(x, lab, scale)
    got_pred = o['pred'][:n].long()
    bad = torch.nonzero(got_pred != rp)[:5, 0].tolist()
    assert not bad, [(r, int(got_pred[r]), int(rp[r])) for r in bad]
    assert torch.equal(o['errt'][:n].double(), re)
    lb = ULP20 * (1.0 + x.max(-1).values.abs() + x.gather(1, lab[:, None])[:, 0].abs())
    lr = float(((o['loss'][:n].double() - rl).abs() / lb).max())
    gr = 0.0
    if mode == 'f32':
        gr = float((o['logits'][:n].double() - rg).abs().max()) / (ULP22 * scale)
    elif mode in ('f32_bf16', 'panel'):
        got = o['panel'][:n].view(torch.bfloat16).double()
        gr = float(((got - rg).abs() / (BF16_REL * rg.abs() + ULP20 * scale)).max())
    if record is not None:
        record('loss_ratio', lr)
        record('grad_ratio', gr)
    assert lr <= 1.0, ('loss', lr)
    assert gr <= 1.0, ('grad', gr)
    return lr, gr


# ------------------------------------------------------------------------------------------ every form x every in / out combination x V edges
MODES = ('f32', 'f32_bf16', 'panel', 'eval')
VS = (4, 8, 1020, 1024, 1028, 8184, 8188, 8192, 8196, 12800, 50000)
MATRIX = [(V, mode) for V in VS for mode in MODES]


@pytest.mark.parametrize("V,mode", MATRIX, ids=['%s-V%d-%s' % (FORM_NAME[expected_form(V, md)], V, md) for V, md in MATRIX])
def test_softmax_ce_form_against_float64(vae, V, mode, record_property):
    """37 rows, 33 of them real (device-side count): every logit range and every label position (column 0, V - 1, the row's argmax and
    argmin, random) on every form and every input / output combination the dispatch admits -- fp32 logits with the fp32 gradient over
    them, with the bf16 gradient beside them, the fp16 panel turned into the bf16 gradient in place, no gradient (eval) -- device-count scale"""
    x = make_logits(37, V, seed=V)
    xs = stored(x, mode)
    lab = pick_labels(xs, seed=V)
    o = run_ce(vae, xs, lab, mode, 33, 0.0)
    assert o['form'] == expected_form(V, mode)
    check_ce(o, xs, lab, mode, 33, 0.0, record_property)


# ------------------------------------------------------------------------------------------ row counts, grid stride, prefetch, both scales
ROWS = [(1, 1, 1e-3), (1, 1, 0.0), (37, 30, 0.0), (37, 30, 5e-4), (8192 + 300, 8192 + 300, 0.0), (2 * 8192 + 7, 2 * 8192 + 7 - 40, -1.0),
        (2 * 8192 + 7, 2 * 8192 + 7, 3e-5), (64, 0, 0.0), (40, 1000, 0.0)]
ROW_FORMS = [(1024, 'f32'), (1024, 'panel'), (1020, 'panel'), (8196, 'f32_bf16'), (8200, 'panel')]
ROW_CASES = [(V, mode, n_max, n_dev, inv_n) for V, mode in ROW_FORMS for n_max, n_dev, inv_n in ROWS]


@pytest.mark.parametrize("V,mode,n_max,n_dev,inv_n", ROW_CASES,
                         ids=['%s-V%d-%s-n%d-dev%d-inv%g' % ((FORM_NAME[expected_form(c[0], c[1])],) + c) for c in ROW_CASES])
def test_softmax_ce_row_counts_and_scales(vae, V, mode, n_max, n_dev, inv_n, record_property):
    """one row; a few; more than the 8192 workgroups (grid stride, and the fp16-panel form's next-row prefetch, which runs only there);
    a device-side count below n_max, of 0, and above n_max (clamped); the scale given (inv_n > 0) and counted on the device (<= 0)"""
    x = make_logits(n_max, V, seed=n_max + V, kinds=('rand', 'peaked', 'span80'))
    xs = stored(x, mode)
    lab = pick_labels(xs, seed=n_max)
    o = run_ce(vae, xs, lab, mode, n_dev, inv_n, seed=1)
    assert o['form'] == expected_form(V, mode)
    check_ce(o, xs, lab, mode, n_dev, inv_n, record_property)


# ------------------------------------------------------------------------------------------ ties for the first maximum
# duplicated maxima: within one thread's float4 / 8-half group, across threads, across waves (also with the first index in the later
# wave), across the register form's 1024-column and the panel form's 2048-column chunks, across the streaming form's 1024-column strides,
# a three-way tie, at the last columns
TIE_PAIRS = [(16, 17), (16, 23), (3, 4), (7, 8), (100, 300), (100, 600), (200, 261), (1020, 1026), (600, 1030), (5, 1029), (5, 2053),
             (2050, 4100), (4000, 8000), (1, 7000), (8191, 8192 + 1024), (9000, 10024), (12000, 13024), (3, 1027, 2051)]
TIE_CASES = [(8, 'panel'), (1024, 'f32'), (1024, 'panel'), (4096, 'f32_bf16'), (4096, 'panel'), (8188, 'panel'), (8192, 'eval'),
             (12800, 'f32'), (12800, 'panel'), (50000, 'eval')]


@pytest.mark.parametrize("V,mode", TIE_CASES, ids=['%s-V%d-%s' % (FORM_NAME[expected_form(V, md)], V, md) for V, md in TIE_CASES])
def test_softmax_ce_ties_give_the_first_maximum(vae, V, mode, record_property):
    sets = [t for t in TIE_PAIRS if max(t) < V] + [(V - 2, V - 1), (0, V - 1)]
    g = torch.Generator(device='cuda').manual_seed(V)
    n = 4 * len(sets) + 1
    x = torch.randn((n, V), device='cuda', dtype=torch.float64, generator=g).clamp(-6, 6)
    lab = torch.randint(0, V, (n,), device='cuda', generator=g)
    for i, t in enumerate(sets):
        for k in range(4):          # label elsewhere, at the first, at the second tied column, at column 0
            r = 4 * i + k
            x[r, list(t)] = 8.0
            lab[r] = (lab[r], t[0], t[1], 0)[k]
    x[n - 1] = 2.5                  # every column tied
    xs = stored(x, mode)
    o = run_ce(vae, xs, lab, mode, n, 0.0)
    assert o['form'] == expected_form(V, mode)
    check_ce(o, xs, lab, mode, n, 0.0, record_property)
    assert o['pred'][:n - 1].view(-1, 4)[:, 0].tolist() == [t[0] for t in sets] and int(o['pred'][n - 1]) == 0


def test_softmax_ce_refuses_what_it_cannot_run(vae):
    """V not a multiple of 4, and the fp16 panel without its in-place gradient: an error, no launch (form -1)"""
    form = C.c_int(-9)
    z = torch.zeros(64, dtype=torch.int32, device='cuda')
    f = torch.zeros(64 * 64, device='cuda')
    h = torch.zeros(64 * 64, dtype=torch.int16, device='cuda')
    ndev = torch.tensor([4], dtype=torch.int32, device='cuda')
    vae._stream()
    for args in [(f, None, 0, 6, 1), (None, h, 1, 64, 0), (f, None, 1, 64, 1)]:
        rc = vae._l.avae_debug_softmax_ce(vae._h, _p(args[0]), _p(args[1]), args[2], _p(z), _p(z), _p(ndev), 4, args[3], args[4], 0.0,
                                          _p(f), None, None, C.byref(form))
        assert rc != 0 and form.value == -1, args
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ argmax_rows (the stepwise decode)
ARGMAX_CASES = [(V, 37) for V in (1, 3, 4, 7, 100, 255, 256, 257, 1023, 1030, 8193, 50000)] + [(300, 4100)]


@pytest.mark.parametrize("V,n", ARGMAX_CASES)
def test_argmax_rows_first_maximum(vae, V, n):
    """first maximum per row over V columns (any V, not a multiple of 4 included), more rows than the 4096 workgroups; rows >= n untouched"""
    pairs = [(0, 1), (3, 4), (63, 64), (255, 256), (100, 356), (200, 261), (1, 1000), (700, 1030), (0, V - 1), (V - 2, V - 1)]
    pairs = [t for t in pairs if 0 <= t[0] < t[1] < V]
    g = torch.Generator(device='cuda').manual_seed(V + n)
    x = (torch.randn((n, V), device='cuda', generator=g) * 20.0).clamp(-70, 70)
    for r, t in enumerate(pairs):
        x[r, list(t)] = 80.0
    x[len(pairs)] = -3.0                    # every column tied
    x[len(pairs) + 1] = torch.rand(V, device='cuda', generator=g) * 160 - 80
    pred = torch.full((n + 3,), SENT_I, dtype=torch.int32, device='cuda')
    vae._stream()
    assert vae._l.avae_debug_argmax_rows(vae._h, _p(x), _p(pred), n, V) == 0, vae._l.avae_last_error(vae._h)
    torch.cuda.synchronize()
    _, want, _, _ = softmax_ce_reference(x.double(), torch.zeros(n, dtype=torch.long, device='cuda'), 1.0)
    assert torch.equal(pred[:n].long(), want)
    assert pred[n:].tolist() == [SENT_I] * 3
    assert [int(pred[r]) for r in range(len(pairs))] == [t[0] for t in pairs] and int(pred[len(pairs)]) == 0


# ------------------------------------------------------------------------------------------ the fp16 logits panel saturates
def test_fp16_panel_saturates_beyond_the_range_and_keeps_nan():
    """GemmArgs::c16 (gemm_bf16_p8.hip): products beyond +-65504 leave the epilogue as +-65504, not +-inf -- bit for bit the fp32 output
    clamped, then rounded; a NaN in A stays NaN in its row of the panel (a diverged step still shows in the loss)"""
    from argsim_amd.model import VAE
    M, N, K = 8200, 8192, 512
    m = VAE('train', dtype='bf16', dim_tgt=64, dim_emb=16, dim_rep=8, rnn_layers=1)
    g = torch.Generator(device='cuda').manual_seed(11)
    A = torch.randn((M, K), device='cuda', generator=g) * 1e4           # |C| ~ 1e5: about half the outputs beyond the fp16 range
    B = torch.randn((N, K), device='cuda', generator=g) * 0.5
    A[:64] *= 1e-4                                                       # and rows well inside it
    A[77, 5] = float('nan')
    m._stream()
    C32 = torch.zeros((M, N), device='cuda')
    rc = m._l.avae_debug_gemm(m._h, 0, 0, _p(A), _p(B), _p(C32), None, M, N, K, K, K, N, 1.0, 0, 1)
    assert rc == 0, m._l.avae_last_error(m._h)
    C16 = torch.full((M, N), 7.0, dtype=torch.float16, device='cuda')
    rc = m._l.avae_debug_gemm_c16(m._h, _p(A), _p(B), _p(C16), M, N, K, 1.0, None)
    assert rc == 0, m._l.avae_last_error(m._h)
    torch.cuda.synchronize()
    want = C32.clamp(-65504.0, 65504.0).half()
    nan = torch.isnan(want)
    assert bool(nan[77].all()) and int(nan.sum()) == N
    assert torch.equal(torch.isnan(C16), nan)
    assert torch.equal(C16[~nan], want[~nan])
    assert bool(torch.isfinite(C16[~nan]).all())
    assert bool((C32.abs() > 65504.0).float().mean() > 0.3) and bool((C16.abs() == 65504.0).any())
    m.close()


def test_bf16_step_with_logits_beyond_the_fp16_range_stays_finite():
    """bf16 mode, D 512 / V 8192, ~2 100 target rows: the training forward's logits go through the fp16 panel.  One word's logit is pushed
    to ~1e5 in every row (decode/out/bias along its embedding): the panel saturates it at 65504, so loss and gradients stay finite, the
    per-token CE is computed from the saturated value, and the gradient ((onehot(argmax) - onehot(label)) / N per row, softmax saturated
    either way) is the one the fp32-logits path (logits16 = 0) gives.  Before the saturation the panel held inf and every row turned NaN."""
    from argsim_amd import synth
    from argsim_amd.model import VAE
    ids = synth.batch(64, 64, 8192, ragged=True, seed=5)
    m = VAE('train', seed=0, dtype='bf16', dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3)
    m.step = 20000
    E = m.get_tensor('embed/embedding').astype(np.float64)
    w = int(np.setdiff1d(np.arange(8192), ids)[-1])          # a word no token has as its label
    bias = m.get_tensor('decode/out/bias').astype(np.float64)
    m.set_tensor('decode/out/bias', (bias + 1e5 * np.sqrt(512.0) * E[w] / (E[w] @ E[w])).astype(np.float32))
    out = {}
    for v in (1, 0):
        m.set_option('logits16', v)
        m.forward_backward(ids, ids, seed=3)
        out[v] = (m.losses(), m.train_ce().copy(), m.grads.clone())
        assert all(np.isfinite(out[v][0])), (v, out[v][0])
        assert bool(np.isfinite(out[v][1]).all()), v
        assert bool(torch.isfinite(out[v][2]).all()), v
    ce1, ce0 = out[1][1].astype(np.float64), out[0][1].astype(np.float64)
    assert ce1.size >= 1600
    assert ce0.min() > 70000.0                    # the true logit is beyond the fp16 range ...
    assert ce1.max() <= 2 * 65504.0 and ce1.min() > 40000.0      # ... and the panel held the saturated one
    assert float((out[1][2] - out[0][2]).norm() / out[0][2].norm()) <= 1e-2
    m.close()


# ------------------------------------------------------------------------------------------ whole model at trained-like logit scale
KEYS = ('dim_tgt', 'dim_emb', 'dim_rep', 'rnn_layers', 'accelerate', 'learn_rate', 'bos', 'eos')
_ORACLE = {}


def _peaked_case(name, target=45.0):
    """make_case(name) with decode/out/kernel and decode/out/bias scaled so that max |logit| of the training forward is `target`
    (trained-like; random initialisation gives a few units), and the live oracle of its training step"""
    if name not in _ORACLE:
        from oracle import vae_numpy as vn
        from oracle import vae_torch as vt
        cfg, P, ids, keep, eps = make_case(name)
        f = target / float(np.abs(vn.forward(P, cfg, ids, ids, 'train', 20000, keep, eps)['logits']).max())
        for k in ('decode/out/kernel', 'decode/out/bias'):
            P[k] = (P[k] * f).astype(np.float32).astype(np.float64)
        outs, grads = vt.loss_and_grads(P, cfg, ids, ids, 20000, keep, eps)
        assert 30.0 <= float(np.abs(outs['logits']).max()) <= 60.0
        _ORACLE[name] = (cfg, P, ids, keep, eps, outs, grads)
    return _ORACLE[name]


@pytest.mark.parametrize("dtype", ['f32', 'f32s', 'bf16'])
@pytest.mark.parametrize("name", ['mid', 'tab', 'full2', 'bigv'])
def test_whole_model_at_trained_logit_scale(name, dtype):
    """the training step with logits reaching +-30..60 against the float64 oracle at the EXISTING tolerances: fp32 and f32s per-token
    CE <= 1e-4 abs, losses <= 2e-5 rel, gradients <= 2e-4 relative L2 per variable; bf16 losses <= 1e-2 rel, gradients <= 5e-2"""
    from argsim_amd.model import VAE
    cfg, P, ids, keep, eps, outs, grads = _peaked_case(name)
    m = VAE('train', init=False, dtype=dtype, **{k: cfg[k] for k in KEYS})
    m.set_params(P)
    m.step = 20000
    m.forward_backward(ids, ids, keep_mask=keep, eps=eps)
    lg, lk, lo = m.losses()
    got = m.get_grads()
    if dtype == 'bf16':
        assert abs(lo - outs['loss']) <= 1e-2 * abs(outs['loss'])
        bad = {k: rel_l2(got[k], grads[k]) for k in grads if rel_l2(got[k], grads[k]) > 5e-2}
    else:
        ce = m.train_ce().astype(np.float64)
        assert ce.shape == outs['loss_gen_samp'].shape
        assert np.abs(ce - outs['loss_gen_samp']).max() <= 1e-4, float(np.abs(ce - outs['loss_gen_samp']).max())
        assert abs(lg - outs['loss_gen']) <= 2e-5 * abs(outs['loss_gen'])
        assert abs(lk - outs['loss_kld']) <= 2e-5 * abs(outs['loss_kld'])
        assert abs(lo - outs['loss']) <= 2e-5 * abs(outs['loss'])
        bad = {k: rel_l2(got[k], grads[k]) for k in grads if rel_l2(got[k], grads[k]) > 2e-4}
    assert not bad, bad
    m.close()


def test_fp16_logits_panel_at_trained_logit_scale():
    """the fp16 panel (D 512, V 8192, ~2 100 target rows) on a peaked batch (|logit| up to ~45) against logits16 = 0, at the bounds of
    test_fp16_logits_panel_changes_the_training_step_by_less_than_the_bf16_gradient_rounding -- except the mean per-token CE change:
    that test's 2e-3 holds for |logit| <~ 10; fp16 rounds each logit by up to 2^-11 of its size, so a token's CE moves by up to
    2^-11 (max |logit| + |label logit|) of ITS row (0.04 at 45), bounded here per token from the oracle's logits (10 % margin for
    the bf16 operands)"""
    from oracle import vae_numpy as vn
    from argsim_amd.model import VAE
    cfg, P, ids, keep, eps = make_case('prod64')
    o = vn.forward(P, cfg, ids, ids, 'train', 20000, keep, eps)
    f = 45.0 / float(np.abs(o['logits']).max())
    x = f * np.abs(o['logits'])
    ce_bound = 1.1 * 2.0 ** -11 * (x.max(-1) + x[np.arange(x.shape[0]), o['labels']]) + 1e-4
    for k in ('decode/out/kernel', 'decode/out/bias'):
        P[k] = P[k] * f
    m = VAE('train', init=False, dtype='bf16', **{k: cfg[k] for k in KEYS})
    m.set_params(P)
    m.step = 20000
    out = {}
    for v in (1, 0):
        m.set_option('logits16', v)
        m.forward_backward(ids, ids, keep_mask=keep, eps=eps)
        out[v] = (m.losses(), m.train_ce().copy(), m.grads.clone(), m.encode(ids))
    assert out[1][1].size >= 1600
    assert np.array_equal(out[1][3], out[0][3])
    assert abs(out[1][0][0] - out[0][0][0]) <= 2e-4 * abs(out[0][0][0]), (out[1][0], out[0][0])
    dce = np.abs(out[1][1].astype(np.float64) - out[0][1])
    assert dce.shape == ce_bound.shape
    assert float(dce.max()) <= 2e-2, float(dce.max())
    assert float((dce / ce_bound).max()) <= 1.0, (float((dce / ce_bound).max()), float(dce.mean()))
    d = float((out[1][2] - out[0][2]).norm() / out[0][2].norm())
    assert d <= 1e-2, d
    m.close()
