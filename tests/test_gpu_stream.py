"""The library on a stalled side stream, and training steps whose fill hint is late (the harness, the case table and why: tests/stream_stall.py).

A. Every entry of the C ABI that enqueues device work, three runs each on fresh handles:
     reference   the true inputs on the default stream; the host time of the call's enqueue sets the stall (stream_stall.stall_ms)
     decoy       the decoy inputs (and, for a model call, the decoy parameters) the same way: its outputs must DIFFER from the reference's,
                 else the comparison below could not see work that escaped the stream
     stalled     on a torch.cuda.Stream() that is busy: every input buffer holds the decoy and receives the true values through a copy
                 enqueued behind the stall, the outputs hold a sentinel.  A call that does not synchronise inside must return while the stall
                 still holds ("stall too short" otherwise: a failure).  Its outputs are the reference's BITS, no sentinel survives.
   The flat gradient of a step carries float atomics: it goes through step_routes.check_step against the float64 oracle, tolerances
   unchanged, while losses, the per-token CE and the present-id counts are the reference's bits.  train_step (its handle warmed like the step's, so the whole call sits
   behind the stall) runs its Adam update on a gradient that differs from the reference's in the last bits: its parameters are held to the reference's within 7 x the step's learning rate (at step 20000 the bias corrections are 1, the first
   update from m = v = 0 moves a parameter by lr 0.1 |g| / (sqrt(0.001) |g| + 1e-8) <= 3.17 lr, so two such updates differ by less than 7 lr;
   the decoy parameters are a quarter of each value away), adam_step itself bit for bit on the reference step's gradient copied in.
B. One handle, two streams: steps, eval and encode on stream A, then the same calls stalled on stream B -- the workspace, the exchange
   rings armed by the launch before, the error words and counters, and with option timing the events all carry over.
C. Steps whose hint is late (tests/step_history.py LATE_SEQUENCES): the route and the row expectations are read from host memory before
   anything synchronises, the last step of a run of unsynchronised calls is held to the oracle and to its anchor's bits exactly as
   tests/test_gpu_step_history.py holds its steps.

Each case prints a STALL line (the enqueue times and the stall used) and part C HISTORY lines; DESIGN.md section 2 holds those seen on MI355X."""
import time

import numpy as np
import pytest

import helpers
import step_history as SH
import step_routes as SR
import stream_stall as SS
from oracle import vae_torch as vt

pytestmark = pytest.mark.gpu

KEYS = ('dim_tgt', 'dim_emb', 'dim_rep', 'rnn_layers', 'accelerate', 'learn_rate', 'bos', 'eos')
_TRUTH, _ANCHOR, _AUX, _SIDE = {}, {}, {}, {}


@pytest.fixture(scope='module', autouse=True)
def _forget():
    yield
    for d in (_TRUTH, _ANCHOR, _AUX, _SIDE):
        d.clear()


def truth(name):
    if name not in _TRUTH:
        import torch
        cfg, P, src, tgt, keep, eps = SH.make(name)
        outs, grads = vt.loss_and_grads(P, cfg, src, tgt, SR.STEP, keep, eps)
        g32 = vt.loss_and_grads(P, cfg, src, tgt, SR.STEP, keep, eps, dtype=torch.float32)[1]
        _TRUTH[name] = dict(cfg=cfg, outs=outs, grads=grads, f32={tol: SR.block_ratios(g32, grads, tol) for tol in (2e-4, 5e-2)})
    return _TRUTH[name]


def side(name='side'):
    import torch
    if name not in _SIDE:
        _SIDE[name] = torch.cuda.Stream()
    return _SIDE[name]


def model(dtype='f32'):
    from argsim_amd.model import VAE
    cfg, P = SH.make('b64')[:2]
    m = VAE('train', init=False, dtype=dtype, **{k: cfg[k] for k in KEYS})
    m.set_params(P)
    m.step = SR.STEP
    return m


def handle(case):
    from argsim_amd.model import VAE
    m = model() if case.model else VAE('infer', init=False, **SS.ROWS_KW)
    for k, v in case.options:
        m.set_option(k, v)
    return m


def _tensor(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _warm(m, I):
    """the handle's first forward_backward, which synchronises once by itself, on the decoy batch (default stream)"""
    import torch
    t = {k: _tensor(v, m.device) for k, v in I.items()}
    ctx = SS.Ctx(m, t, I)
    m._stream()
    SS._fb(ctx)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ the harness's own teeth
def test_the_harness_has_teeth():
    """an elementwise op on the DEFAULT stream against a staged input, issued while the side stream is stalled, reads the decoy, and the
    comparison of bits flags it; the same op on the side stream reads the true values.  (Were the null stream ordered against torch's pool
    streams, the first half would read the true values and nothing below could catch work that leaves the handle's stream.)"""
    import torch
    SS.guard()
    try:
        dev = torch.device('cuda', 0)
        true, decoy = np.arange(4096, dtype=np.float32), -np.arange(4096, dtype=np.float32) - 1.0
        s = SS.staged(true, decoy, dev)
        torch.cuda.synchronize()
        st = side()
        ev = SS.stall(st, 100.0)
        with torch.cuda.stream(st):
            buf = s.arm()
            on_side = buf * 2.0
        with torch.cuda.stream(torch.cuda.default_stream()):
            escaped = buf * 2.0
        torch.cuda.default_stream().synchronize()
        alive = not ev.query()
        escaped = escaped.cpu().numpy()
        st.synchronize()
        on_side = on_side.cpu().numpy()
    except Exception as e:          # noqa: BLE001
        SS.trip('teeth: %s' % e)
    assert alive, 'stall too short: the default stream finished behind a 100 ms stall (%.0f cycles per ms)' % SS.cycles_per_ms()
    assert escaped.tobytes() == (decoy * 2.0).tobytes(), 'work on the default stream saw the true input: the null stream is ordered against the side stream'
    assert escaped.tobytes() != (true * 2.0).tobytes()
    assert on_side.tobytes() == (true * 2.0).tobytes()


# ------------------------------------------------------------------------------------------ A. every entry under the stall
def run(case, which, st=None, ms=None, post=None):
    """one run of a case on a fresh handle -> (results {name: numpy}, host seconds of the enqueue, the stall still held on return or None,
    what post(m) returned).  st None: the default stream, the inputs `which` in place.  st a stream: stalled for ms, every input staged."""
    import torch
    m = handle(case)
    try:
        dev = m.device
        aux = _AUX
        I = case.inputs(which, aux)
        Idec = case.inputs('decoy', aux) if st is not None else I
        if case.warm:
            _warm(m, SS.model_batch('decoy'))
        bufs, state = {}, {}
        for k in I:
            if k in case.state_in:
                continue
            bufs[k] = SS.staged(I[k], Idec[k], dev)
        if case.model:
            true_flat = m.params.clone()
            own = true_flat if which == 'true' else 0.75 * true_flat
            state['params'] = (own, 0.75 * true_flat if st is not None else own)
        for k in case.state_in:
            state[k] = (_tensor(I[k], dev), _tensor(Idec[k], dev))
        for k, (_, dec) in state.items():
            getattr(m, k).copy_(dec)
        spec = case.outputs(I)
        out = {k: torch.zeros(tuple(s), dtype=_tensor(np.zeros(1, dt), 'cpu').dtype, device=dev) for k, (s, dt) in spec.items()}
        torch.cuda.synchronize()
        stream = st if st is not None else torch.cuda.default_stream()
        with torch.cuda.stream(stream):
            ev = SS.stall(stream, ms) if st is not None else None
            # the sentinels go in BEHIND the stall too: a fill, a copy or a kernel of the call that left the stream has run by then, and
            # the sentinel lands over what it wrote and survives
            for k, (_, dt) in spec.items():
                out[k].fill_(SS.sentinel(dt).item())
            for k in case.state_out:
                if k not in state:
                    getattr(m, k).fill_(float(SS.sentinel(np.float32)))
            t = {k: b.arm() for k, b in bufs.items()}
            for k, (true, _) in state.items():
                getattr(m, k).copy_(true, non_blocking=True)
            t.update(out)
            ctx = SS.Ctx(m, t, I)
            m._stream()
            t0 = time.perf_counter()
            case.call(ctx)
            t1 = time.perf_counter()
            alive = None if ev is None else not ev.query()
            if case.after:
                case.after(ctx)
            stream.synchronize()
        torch.cuda.synchronize()
        o = {k: v.cpu().numpy() for k, v in out.items()}
        o.update({k: getattr(m, k).clone().cpu().numpy() for k in case.state_out})
        o.update({k: t[k].cpu().numpy() for k in SS.INOUT.get(case.id, ())})
        res = case.view(ctx.host, o) if case.view else o
        extra = post(m) if post else None
        torch.cuda.synchronize()
    except Exception as e:          # noqa: BLE001 -- a non-zero return or whatever the runtime raises: nothing more is launched
        SS.trip('%s (%s%s): %s' % (case.id, which, ', stalled' if st is not None else '', e))
    finally:
        m.close()
    if 'losses' in res and not np.isfinite(res['losses']).all():
        SS.trip('%s: non-finite losses %s' % (case.id, res['losses']))
    return res, t1 - t0, alive, extra


def ref_grads():
    """the flat gradient of the reference step (b64 on a fresh handle, default stream): what adam_step's cases run on"""
    if 'ref_grads' not in _AUX:
        import torch
        m = model()
        try:
            _warm(m, SS.model_batch('true'))
            _AUX['ref_grads'] = m.grads.clone().cpu().numpy()
        except Exception as e:          # noqa: BLE001
            SS.trip('reference step: %s' % e)
        finally:
            m.close()
    return _AUX['ref_grads']


def _step_post(m):
    """the step's gradient in the natural layout, and mu and log sigma^2 of an encode behind it (what check_step takes)"""
    src = SH.make('b64')[2]
    mu, lv = m.encode(src, return_lv=True)
    return dict(grads=m.get_grads(), mu=mu, lv=lv, lr=m.schedule()[2])


@pytest.mark.parametrize('case', SS.CASES, ids=[c.id for c in SS.CASES])
def test_entry_on_a_stalled_stream(case):
    SS.guard()
    if case.aux == 'ref_grads':
        ref_grads()
    post = (lambda m: dict(grads=m.get_grads())) if case.id == 'train_step' else (_step_post if case.id == 'step' else None)
    ref, t_ref, _, _ = run(case, 'true')
    dec, _, _, _ = run(case, 'decoy')
    differ = [k for k in ref if ref[k].tobytes() != dec[k].tobytes()]
    print('DECOY %s differs in %s, the same in %s' % (case.id, differ, [k for k in ref if k not in differ]))
    assert differ, 'the decoy run gives the reference\'s outputs: the comparison has nothing to catch'
    for k, v in ref.items():
        assert not (v == SS.sentinel(v.dtype)).any(), ('the reference run left a sentinel', case.id, k)
    ms = SS.stall_ms(t_ref)
    got, t_enq, alive, extra = run(case, 'true', side(), ms, post)
    print('STALL %s enqueue %.2f ms (reference run %.2f ms) stall %.0f ms %s' % (
        case.id, 1e3 * t_enq, 1e3 * t_ref, ms, 'synchronises inside' if case.sync else ('held' if alive else 'OVER on return')))
    if not case.sync:
        assert alive, 'stall too short: %.0f ms were over when the call returned after %.2f ms of enqueue' % (ms, 1e3 * t_enq)
    for k, v in got.items():
        assert not (v == SS.sentinel(v.dtype)).any(), ('a sentinel survived', case.id, k)
        if k not in case.loose:
            assert v.shape == ref[k].shape and v.tobytes() == ref[k].tobytes(), (
                case.id, k, 'the decoy\'s answer' if v.tobytes() == dec[k].tobytes() else 'differs from the reference run')
    if case.id == 'step':
        t = truth('b64')
        SR.check_step('stalled', 'f32', t, tuple(float(x) for x in got['losses']), got['ce'].astype(np.float64), extra['grads'], extra['mu'], extra['lv'],
                      head='STREAM step b64 f32')
    if case.id == 'train_step':
        t = truth('b64')
        bad = helpers.grads_bad(extra['grads'], t['grads'], SR.TOLS['f32'][3])
        assert not bad, bad
        cfg = SH.make('b64')[0]
        lr = float(cfg['learn_rate']) / (float(np.sqrt(cfg['accelerate'] * SR.STEP)) + 1.0)       # rate_update at the step (model.py:80)
        d = float(np.abs(got['params'].astype(np.float64) - ref['params']).max())
        print('STREAM train_step: params differ from the reference run by at most %.3g (bound %.3g)' % (d, 7 * lr))
        assert d <= 7 * lr, d


# ------------------------------------------------------------------------------------------ B. one handle, two streams
@pytest.mark.parametrize('timing', [0, 1])
def test_one_handle_two_streams(timing):
    """steps, eval and encode on stream A, then each of them stalled on stream B of the SAME handle: the bits of stream A.  Two steps run on A:
    the second has the first one's hint, as the step on B has, so the three take one route (a route may move the forward's bits)."""
    import torch
    SS.guard()
    step = next(c for c in SS.CASES if c.id == 'step')
    m = model()
    A, B = side('A'), side('B')
    try:
        dev = m.device
        if timing:
            m.set_option('timing', 1)
        I, Idec = SS.model_batch('true'), SS.model_batch('decoy')
        true_flat = m.params.clone()
        rt = SS._rt(I)
        f32 = torch.float32

        def outs():
            s = float(SS.sentinel(np.float32))
            return dict(ce=torch.full((rt,), s, dtype=f32, device=dev), errt=torch.full((rt,), s, dtype=f32, device=dev),
                        lgen=torch.full((rt,), s, dtype=f32, device=dev), lkld=torch.full((64, SR.R), s, dtype=f32, device=dev),
                        z=torch.full((64, SR.R), s, dtype=f32, device=dev), lv=torch.full((64, SR.R), s, dtype=f32, device=dev))

        def flow(stream, stalled, times):
            """step, eval, encode on `stream` -> their results and the routes; stalled: each call behind a stall with staged inputs, as long
            as stall_ms gives for the host time times[name] the call's enqueue took in the flow before; the times of this flow go there"""
            res, alive = {}, []
            for name, call, after, view in (('step', SS._fb, SS._after_step, SS._step_view), ('eval', SS._eval, None, SS._eval_view),
                                            ('encode', SS._encode, None, None)):
                bufs = {k: SS.staged(I[k], Idec[k] if stalled else I[k], dev) for k in I}
                o = {k: torch.zeros_like(v) for k, v in outs().items()}
                if stalled:
                    m.params.copy_(0.75 * true_flat)
                kept = m.grads.clone()
                torch.cuda.synchronize()
                with torch.cuda.stream(stream):
                    ev = SS.stall(stream, SS.stall_ms(times[name])) if stalled else None
                    for v in o.values():
                        v.fill_(float(SS.sentinel(np.float32)))
                    t = {k: b.arm() for k, b in bufs.items()}
                    m.params.copy_(true_flat, non_blocking=True)
                    t.update(o)
                    ctx = SS.Ctx(m, t, I)
                    m._stream()
                    t0 = time.perf_counter()
                    call(ctx)
                    times[name] = time.perf_counter() - t0
                    if stalled and name == 'step':
                        alive.append(not ev.query())
                        res['route'] = m.step_route()
                    if after:
                        after(ctx)
                    stream.synchronize()
                torch.cuda.synchronize()
                host = {k: v.cpu().numpy() for k, v in o.items()}
                host['grads'] = m.grads.clone().cpu().numpy()
                r = view(ctx.host, host) if view else dict(z=host['z'], lv=host['lv'])
                if name != 'step':
                    assert torch.equal(m.grads, kept), (name, 'moved the flat gradient')
                r.pop('grads', None)
                res[name] = r
            return res, alive

        _warm_on(m, A, I)
        times = {}
        on_a, _ = flow(A, False, times)
        route_a = m.step_route()
        torch.cuda.synchronize()
        ref_times = dict(times)
        on_b, alive = flow(B, True, times)
        print('STALL two streams (timing %d): enqueue on A %s, stalls on B %s' % (
            timing, {k: '%.2f ms' % (1e3 * v) for k, v in ref_times.items()}, {k: '%.0f ms' % SS.stall_ms(v) for k, v in ref_times.items()}))
        tc = m.timing_collect() if timing else None
    except Exception as e:          # noqa: BLE001
        SS.trip('two streams (timing %d): %s' % (timing, e))
    finally:
        m.close()
    assert alive == [True], 'stall too short: the step on stream B returned behind the stall'
    assert on_b['route'] == route_a, (on_b['route'], route_a)
    for name in ('step', 'eval', 'encode'):
        for k, v in on_b[name].items():
            assert not (v == SS.sentinel(v.dtype)).any(), ('a sentinel survived', name, k)
            assert v.tobytes() == on_a[name][k].tobytes(), (name, k, 'stream B differs from stream A')
    if timing:
        print('STREAM timing over both streams: %s' % (tc,))
        assert all(np.isfinite(ms) and ms >= 0 and n > 0 for ms, n, _ in tc.values()), tc


def _warm_on(m, stream, I):
    """the handle's first step (it synchronises by itself) on `stream`, the true batch: its hint is there for the steps that follow"""
    import torch
    t = {k: _tensor(v, m.device) for k, v in I.items()}
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        m._stream()
        SS._fb(SS.Ctx(m, t, I))
        stream.synchronize()


# ------------------------------------------------------------------------------------------ C. steps whose hint is late
def _fb_host(m, batch):
    """forward_backward on device copies of the batch made BEFORE the stall (VAE.forward_backward would upload behind it) -> the tensors, kept
    alive by the caller"""
    _, _, src, tgt, keep, eps = SH.make(batch)
    B, S = SH.shape(batch)
    I = dict(src=np.ascontiguousarray(src[:, :S], np.int32), tgt=np.ascontiguousarray(tgt[:, :S], np.int32), keep=np.ascontiguousarray(keep, np.uint8),
             eps=np.ascontiguousarray(eps, np.float32))
    return I, {k: _tensor(v, m.device) for k, v in I.items()}


def anchor(batch, dtype, compact, rs):
    """losses and train CE of a fresh handle that runs the batch once with the route forced (tests/test_gpu_step_history.py's anchor)"""
    import torch
    key = (batch, dtype, compact, rs)
    if key not in _ANCHOR:
        tag = 'anchor %s %s compact=%d bwd_rs=%d' % key
        m = model(dtype)
        try:
            for k, v in (('compact', compact), ('bwd_rs', rs), ('gru_spec', 0)):
                m.set_option(k, v)
            _, _, src, tgt, keep, eps = SH.make(batch)
            m.forward_backward(src, tgt, keep_mask=keep, eps=eps)
            losses = m.losses()
            route, rows = m.step_route(), m.row_expect()
            ce = m.train_ce()
            torch.cuda.synchronize()
        except Exception as e:          # noqa: BLE001
            SS.trip('%s: %s' % (tag, e))
        finally:
            m.close()
        assert route['compact'] == (compact, compact) and route['bwd_rs'] == rs and rows == (0, 0, 0), (tag, route, rows)
        _ANCHOR[key] = (np.asarray(losses, np.float32).tobytes(), ce.tobytes())
    return _ANCHOR[key]


def _late_run(name, dtype, st, stall_ms_of):
    """one pass over a late sequence on a fresh handle.  st None: every call synchronised, on the default stream -- the pass that measures the
    enqueue time of every run of late calls (and gives nothing else).  -> [(index, route, rows, alive, losses, ce, grads, mu, lv)] of the
    checked steps, {first index of a run: host seconds of its enqueue}"""
    import torch
    m = model(dtype)
    checked, times = [], {}
    calls = SH.late_steps(name)
    try:
        stream = st if st is not None else torch.cuda.default_stream()
        i = 0
        while i < len(calls):
            j = i
            while calls[j][2] == 'late' and j + 1 < len(calls) and calls[j + 1][2] == 'late':
                j += 1
            run_ = calls[i:j + 1]
            data = [_fb_host(m, b) for _, b, *_ in run_]
            late = run_[0][2] == 'late'
            if run_[0][2] == 'nohint':
                m.set_option('compact', 1)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                ev = SS.stall(stream, stall_ms_of(i)) if late and st is not None else None
                m._stream()
                t0 = time.perf_counter()
                seen = []
                for (I, t), (kind, batch, when, prev, want, want_rows, chk) in zip(data, run_):
                    SS._fb(SS.Ctx(m, t, I))
                    seen.append((m.step_route(), m.row_expect()))
                times[i] = time.perf_counter() - t0
                alive = None if ev is None else not ev.query()
                stream.synchronize()
            torch.cuda.synchronize()
            if run_[0][2] == 'nohint':
                m.set_option('compact', 2)
            if run_[-1][6]:
                batch = run_[-1][1]
                losses = m.losses()
                if not all(np.isfinite(losses)):
                    SS.trip('%s: non-finite losses %s' % (name, (losses,)))
                # nothing here feeds a hint (get_losses, the train-CE hook and get_tensor sort no source rows): what the NEXT call plans from
                # is what the calls above left in the pinned pair.  mu and lv are taken when the sequence is over -- the parameters never move
                ce, got = m.train_ce(), m.get_grads()
                torch.cuda.synchronize()
                checked.append([j, seen, alive, losses, ce, got, batch, None])
            i = j + 1
        kept = m.grads.clone()
        for c in checked:
            mu, lv = m.encode(SH.make(c[6])[2], return_lv=True)
            c[6:] = [mu, lv]
        torch.cuda.synchronize()
        assert torch.equal(m.grads, kept), (name, 'encode moved the flat gradient')
    except AssertionError:
        raise
    except Exception as e:          # noqa: BLE001
        SS.trip('%s: %s' % (name, e))
    finally:
        m.close()
    return checked, times


@pytest.mark.parametrize('name', list(SH.LATE_SEQUENCES))
def test_steps_with_a_late_hint(name):
    SS.guard()
    dtype = SH.LATE_SEQUENCES[name][0]
    calls = SH.late_steps(name)
    _, times = _late_run(name, dtype, None, None)
    checked, t_enq = _late_run(name, dtype, side(), lambda i: SS.stall_ms(times[i]))
    assert [c[0] for c in checked] == [i for i, c in enumerate(calls) if c[6]]
    n = 0
    for j, seen, alive, losses, ce, got, mu, lv in checked:
        kind, batch, when, prev, want, want_rows, _ = calls[j]
        first = j - len(seen) + 1
        if when == 'late':
            print('STALL %s calls %d..%d enqueue %.2f ms (reference run %.2f ms) stall %.0f ms %s' % (
                name, first, j, 1e3 * t_enq[first], 1e3 * times[first], SS.stall_ms(times[first]), 'held' if alive else 'OVER on return'))
            assert alive, 'stall too short: over when the last step of the run had been enqueued'
        for (route, rows), (_, b, _, p, w, wr, _) in zip(seen, calls[first:j + 1]):
            if w is not None:
                assert route == w, (name, b, p, route)
                assert rows == wr, (name, b, p, rows, wr)
        n += 1
        route = seen[-1][0]
        head = 'HISTORY %s step %d %s %s %s fill %s compact %d bwd_rs %d Bx %d' % (
            name, n, batch, dtype, 'late, arrived' if when == 'late' else 'prev', 'none' if prev is None else '%.3f' % prev, route['compact'][0],
            route['bwd_rs'], route['Bx'])
        SR.check_step('%s#%d' % (name, n), dtype, truth(batch), losses, ce.astype(np.float64), got, mu, lv, head=head)
        a_losses, a_ce = anchor(batch, dtype, route['compact'][0], route['bwd_rs'])
        assert np.asarray(losses, np.float32).tobytes() == a_losses, (name, n, 'losses differ from the anchor', losses)
        assert ce.tobytes() == a_ce, (name, n, 'the per-token train CE differs from the anchor')
