"""Whole training steps at dim_emb = 512 against the float64 oracle, variable by variable and block by block, on every route model.cpp can
take at that width (tests/step_routes.py: the case table and what each batch reaches).

Each case forces its options, runs one forward_backward (AUTO: two) and asserts that VAE.step_route() -- what the step itself noted where it
decided -- equals its table entry BEFORE it compares a number.  Then, against vt.loss_and_grads in float64 (once per batch: options do not
change the truth), with the project's own tolerances:

    quantity                                      fp32 and f32s     bf16
    loss_gen, loss_kld, loss (relative)           2e-5              1e-2
    mu and log sigma^2 (encode, absolute)         2e-5              3e-2
    per-token train CE, token by token            1e-4              6e-2
    every gradient, relative L2 per variable      2e-4              5e-2
    every gradient through helpers.grads_bad      the same          the same (see below)

and the oracle's exact zeros (the dead direction's R of a one-step top encoder layer) are exact zeros in every dtype.  helpers.grad_blocks is
the per-block criterion: 16 leading rows (one hidden tile of one gate) at the variable's tolerance, relative to the block's own norm or its
fair share of the variable's norm; the embedding also row by row (one token id each).  Every variable prints a RATIO line -- its worst block
error over its bound, and the float32 run of the oracle beside it --, every case a ROUTE line with the worst of them; DESIGN.md section 2 holds the
figures seen on MI355X.

Safety, as tests/test_gpu_gru.py: one module latch -- the first unexpected non-zero return, failed synchronise or non-finite loss fails every
later case without launching; the kernels' spins are bounded and a time-out comes back as a non-zero return from losses()."""
import numpy as np
import pytest

import step_routes as SR
from oracle import vae_torch as vt

pytestmark = pytest.mark.gpu

KEYS = ('dim_tgt', 'dim_emb', 'dim_rep', 'rnn_layers', 'accelerate', 'learn_rate', 'bos', 'eos')
TOLS = SR.TOLS      # losses rel, mu / lv abs, CE abs, gradients
_LATCH = []
_TRUTH = {}         # batch -> the batch, the float64 oracle, the float32 oracle's ratios
_MODELS = {}        # (batch, dtype) -> VAE; the models of one batch at a time


def guard():
    if _LATCH:
        pytest.fail('not run after an earlier GPU failure: %s' % _LATCH[0])


def trip(what):
    _LATCH.append(what)
    pytest.fail(what)


block_ratios = SR.block_ratios


def truth(name):
    if name not in _TRUTH:
        import torch
        cfg, P, src, tgt, keep, eps = SR.make(name)
        outs, grads = vt.loss_and_grads(P, cfg, src, tgt, SR.STEP, keep, eps)
        g32 = vt.loss_and_grads(P, cfg, src, tgt, SR.STEP, keep, eps, dtype=torch.float32)[1]
        _TRUTH[name] = dict(cfg=cfg, P=P, src=src, tgt=tgt, keep=keep, eps=eps, outs=outs, grads=grads,
                            f32={tol: block_ratios(g32, grads, tol) for tol in (2e-4, 5e-2)})
    return _TRUTH[name]


def model(name, dtype):
    from argsim_amd.model import VAE
    for key in [k for k in _MODELS if k[0] != name]:        # (the cases come batch by batch: one batch's workspaces on the device at a time)
        _MODELS.pop(key).close()
    if (name, dtype) not in _MODELS:
        t = truth(name)
        m = VAE('train', init=False, dtype=dtype, **{k: t['cfg'][k] for k in KEYS})
        m.set_params(t['P'])
        m.step = SR.STEP
        _MODELS[(name, dtype)] = m
    return _MODELS[(name, dtype)]


@pytest.fixture(scope='module', autouse=True)
def _close_models():
    yield
    while _MODELS:
        _MODELS.popitem()[1].close()
    _TRUTH.clear()


@pytest.mark.parametrize('c', SR.CASES, ids=lambda c: c.id)
def test_step_route(c):
    import torch
    guard()
    t = truth(c.batch)
    m = model(c.batch, c.dtype)
    for k, v in c.options:
        m.set_option(k, v)
    try:
        for _ in range(c.calls):
            m.forward_backward(t['src'], t['tgt'], keep_mask=t['keep'], eps=t['eps'])
            losses = m.losses()                   # (synchronises and reads the GRU error word; AUTO: the first call's fill hint has arrived)
        route = m.step_route()
        torch.cuda.synchronize()
    except Exception as e:          # noqa: BLE001 -- a non-zero return or whatever the runtime raises: nothing more is launched
        trip('%s: %s' % (c.id, e))
    if not all(np.isfinite(losses)):
        trip('%s: non-finite losses %s' % (c.id, (losses,)))
    assert route == c.want(), (c.id, route)

    try:
        ce, got = m.train_ce().astype(np.float64), m.get_grads()
        mu, lv = m.encode(t['src'], return_lv=True)
        torch.cuda.synchronize()
    except Exception as e:          # noqa: BLE001
        trip('%s: %s' % (c.id, e))
    SR.check_step(c.id, c.dtype, t, losses, ce, got, mu, lv)
