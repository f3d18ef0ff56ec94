"""Training steps on the automatic path -- compact, bwd_rs and gru_spec at the library's defaults -- on ONE handle that has seen other batches,
against the float64 oracle (tests/step_history.py: the batches, the sequences, and the route every checked step must take, derived there from
the fill of the call before it).

A sequence runs on a fresh VAE; after every call the stream is synchronised, so the call's fill hint has arrived before the next call starts.
Every forward_backward on a probe batch is a checked step, in this order:

  1. VAE.step_route() equals the table's entry, and VAE.row_expect() -- the row counts the host expects behind the compact layout, the stale fill
     scaled to this batch -- what the table derives, before a number is compared;
  2. step_routes.check_step: the criteria and tolerances of tests/test_gpu_step_routes.py, unchanged -- losses, per-token train CE, every
     gradient per variable and per block, the oracle's exact zeros, mu and log sigma^2 of an encode after the step;
  3. "shapes launches only, never a value": losses() and train_ce() are bit for bit those of an ANCHOR, a fresh handle that runs the batch
     once with compact and bwd_rs forced to what the route shows and gru_spec = 0 (it has no hint and no row expectation).  The forward has no
     atomics, so the route is all that may move its bits.

The flat gradient is bound state that DataParallel and adam_step read later: after every step it is cloned, and after every call that is not
a step (eval, encode, decode, score, knn -- the encode of 2. included) it must be the same bits.

Each checked step prints a HISTORY line: sequence, step, the fill of the call before it, the route, the worst block ratio and the float32
oracle's ratio of that variable; DESIGN.md section 2 holds the figures seen on MI355X.

Safety, as tests/test_gpu_step_routes.py: one module latch -- the first unexpected non-zero return, failed synchronise or non-finite loss fails
every later case without launching."""
import numpy as np
import pytest

import step_history as SH
import step_routes as SR
from oracle import vae_torch as vt

pytestmark = pytest.mark.gpu

KEYS = ('dim_tgt', 'dim_emb', 'dim_rep', 'rnn_layers', 'accelerate', 'learn_rate', 'bos', 'eos')
_LATCH = []
_TRUTH = {}         # probe -> the float64 oracle, the float32 oracle's ratios
_ANCHOR = {}        # (probe, dtype, compact, bwd_rs) -> (losses, train CE) as bytes


def guard():
    if _LATCH:
        pytest.fail('not run after an earlier GPU failure: %s' % _LATCH[0])


def trip(what):
    _LATCH.append(what)
    pytest.fail(what)


def truth(name):
    if name not in _TRUTH:
        import torch
        cfg, P, src, tgt, keep, eps = SH.make(name)
        outs, grads = vt.loss_and_grads(P, cfg, src, tgt, SR.STEP, keep, eps)
        g32 = vt.loss_and_grads(P, cfg, src, tgt, SR.STEP, keep, eps, dtype=torch.float32)[1]
        _TRUTH[name] = dict(cfg=cfg, outs=outs, grads=grads, f32={tol: SR.block_ratios(g32, grads, tol) for tol in (2e-4, 5e-2)})
    return _TRUTH[name]


def fresh(dtype):
    from argsim_amd.model import VAE
    cfg, P = SH.make('b64')[:2]
    m = VAE('train', init=False, dtype=dtype, **{k: cfg[k] for k in KEYS})
    m.set_params(P)
    m.step = SR.STEP
    return m


def step(m, batch, tag):
    """one forward_backward -> losses, route, row expectations; synchronised: its hint has arrived"""
    import torch
    _, _, src, tgt, keep, eps = SH.make(batch)
    try:
        m.forward_backward(src, tgt, keep_mask=keep, eps=eps)
        losses = m.losses()
        route, rows = m.step_route(), m.row_expect()
        torch.cuda.synchronize()
    except Exception as e:          # noqa: BLE001 -- a non-zero return or whatever the runtime raises: nothing more is launched
        trip('%s: %s' % (tag, e))
    if not all(np.isfinite(losses)):
        trip('%s: non-finite losses %s' % (tag, (losses,)))
    return losses, route, rows


def anchor(batch, dtype, compact, rs):
    key = (batch, dtype, compact, rs)
    if key not in _ANCHOR:
        tag = 'anchor %s %s compact=%d bwd_rs=%d' % key
        m = fresh(dtype)
        try:
            for k, v in (('compact', compact), ('bwd_rs', rs), ('gru_spec', 0)):
                m.set_option(k, v)
            losses, route, rows = step(m, batch, tag)
            assert route['compact'] == (compact, compact) and route['bwd_rs'] == rs and rows == (0, 0, 0), (tag, route, rows)
            try:
                ce = m.train_ce()
            except Exception as e:          # noqa: BLE001
                trip('%s: %s' % (tag, e))
            _ANCHOR[key] = (np.asarray(losses, np.float32).tobytes(), ce.tobytes())
        finally:
            m.close()
    return _ANCHOR[key]


@pytest.fixture(scope='module', autouse=True)
def _forget():
    yield
    _TRUTH.clear()
    _ANCHOR.clear()


@pytest.mark.parametrize('name', list(SH.SEQUENCES))
def test_step_history(name):
    import torch
    guard()
    dtype = SH.SEQUENCES[name][0]
    m = fresh(dtype)
    kept = z = None         # the flat gradient after the last step; the rows of the last encode
    n = 0
    try:
        for kind, batch, prev, want, want_rows in SH.steps(name):
            tag = '%s %s %s' % (name, kind, batch)
            _, _, src, tgt, keep, eps = SH.make(batch)
            if kind == 'fb':
                losses, route, rows = step(m, batch, tag)
                if want is None:                                # a primer: its hint and its workspace are all it leaves
                    kept = m.grads.clone()
                    continue
                n += 1
                assert route == want, (tag, n, prev, route)
                assert rows == want_rows, (tag, n, prev, rows, want_rows)
                t = truth(batch)
                try:
                    ce, got = m.train_ce(), m.get_grads()
                    kept = m.grads.clone()
                    mu, lv = m.encode(src, return_lv=True)
                    torch.cuda.synchronize()
                    same = torch.equal(m.grads, kept)
                except Exception as e:          # noqa: BLE001
                    trip('%s: %s' % (tag, e))
                assert same, (tag, n, 'encode moved the flat gradient')
                head = 'HISTORY %s step %d %s %s prev fill %s compact %d bwd_rs %d Bx %d' % (
                    name, n, batch, dtype, 'none' if prev is None else '%.3f' % prev, route['compact'][0], route['bwd_rs'], route['Bx'])
                SR.check_step('%s#%d' % (name, n), dtype, t, losses, ce.astype(np.float64), got, mu, lv, head=head)
                a_losses, a_ce = anchor(batch, dtype, route['compact'][0], route['bwd_rs'])
                assert np.asarray(losses, np.float32).tobytes() == a_losses, (tag, n, 'losses differ from the anchor', losses)
                assert ce.tobytes() == a_ce, (tag, n, 'the per-token train CE differs from the anchor')
                continue
            try:
                if kind == 'eval':
                    m.eval(src, tgt)
                elif kind == 'encode':
                    z = m.encode(src)
                elif kind == 'score':
                    m.score(src, k=2, seed=1)
                elif kind == 'decode':
                    m.decode(z, steps=6)
                elif kind == 'knn':
                    m.neighbors(z, z, k=3, exclude_self=True)
                else:
                    raise AssertionError(kind)
                torch.cuda.synchronize()
                same = kept is None or torch.equal(m.grads, kept)
            except Exception as e:          # noqa: BLE001
                trip('%s: %s' % (tag, e))
            assert same, (tag, 'the call moved the flat gradient')
    finally:
        m.close()
