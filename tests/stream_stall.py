"""The library on a STALLED side stream (tests/test_gpu_stream.py): the harness and the case table.  No GPU work at import.

Every other GPU test runs the library on the null stream of an idle device and synchronises between calls.  There a launcher that drops its
stream argument, a hipMemset / hipMemcpy without a stream, or an upload from a host array that dies when the function returns all give the
right answer: the null stream orders everything, and an idle device finishes each piece before the next is enqueued.  Here the stream the
handle is given is BUSY while the call is enqueued, and what the call reads is not there yet:

  stall(stream, ms)       torch.cuda._sleep on `stream` (cycles per millisecond calibrated once, two events around one fixed sleep) -> an event
                          recorded right behind it.  A call that returns without synchronising must find `not event.query()` on return, else
                          the case is no measurement and FAILS as "stall too short" (never passes, never retried).  The length is
                          stall_ms(t): 4 x the host time t the same call's enqueue took in the reference run, within [20, 250] ms.
  staged(true, decoy)     a device buffer that holds `decoy` before the stall and receives `true` through a copy_ enqueued on the stalled
                          stream behind it.  Every device input of a call goes through one, the bound flat parameters of a model call too.
                          The decoy is always a VALID input of the same shape and dtype -- another batch with ids in range and the same
                          lengths, other finite rows, another labelling with the same label range, other finite parameters -- so work that
                          escapes the stream gives a wrong ANSWER, never an out-of-bounds access.  Outputs are pre-filled with a sentinel.
  side stream             torch.cuda.Stream(): torch creates its pool streams non-blocking, so the null stream is not ordered against
                          them; test_the_harness_has_teeth proves that before any case runs (an elementwise op on
                          torch.cuda.default_stream() against a staged input reads the decoy while the side stream is stalled).
  latch                   one per process, as tests/test_gpu_step_routes.py: after the first non-zero return, failed synchronise,
                          non-finite value or exception from the runtime every later case fails without launching.  Nothing is tried twice.

CASES is data: one entry of the C ABI (sometimes a flow of several) per case -- its inputs (true and decoy), its outputs, the options that
give the call at least two parts, and whether the call synchronises INSIDE (the host then waits the stall out and nothing is asserted on
the event).  tests/test_stream_table.py holds the table against argsim_amd/lib.py's signature table without a GPU: every avae_* entry that
is not a debug hook has a case or stands in EXEMPT with a reason.

What "synchronises inside" is read from the sources: every call that ends in check_gru_err (encode, eval, decode_step, the decoders, score,
score_z, get_losses), the probe fits (one synchronise per Newton iteration), avae_mmd (its p-values' bad-relabeling check), and the FIRST
forward_backward of a handle (model.cpp first_step_checked) -- so the step cases (step, train_step, timing) spend that check on the decoy
batch first, in all three runs alike, and the stalled step is the handle's second."""
import ctypes as C
import dataclasses
import time

import numpy as np

# ------------------------------------------------------------------------------------------ the harness
_LATCH = []
_CAL = {}
STALL_MIN_MS, STALL_MAX_MS, STALL_FACTOR = 20.0, 250.0, 4.0


def guard():
    import pytest
    if _LATCH:
        pytest.fail('not run after an earlier GPU failure: %s' % _LATCH[0])


def trip(what):
    import pytest
    _LATCH.append(what)
    pytest.fail(what)


def sentinel(dtype):
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        return dt.type(-7.0e33)
    if dt == np.int64:
        return np.int64(-0x5A5A5A5A5A5A5A5A)
    if dt == np.uint8:
        return np.uint8(0xA5)
    return np.int32(-0x5A5A5A5B)


def cycles_per_ms():
    """torch.cuda._sleep cycles per millisecond on this device: two events around one fixed sleep, once per process"""
    if 'c' not in _CAL:
        import torch
        n = 20_000_000
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(n)
        b.record()
        b.synchronize()
        _CAL['c'] = n / max(a.elapsed_time(b), 1e-3)
    return _CAL['c']


def stall_ms(enqueue_seconds):
    """the stall of a call whose enqueue took `enqueue_seconds` of host time in the reference run"""
    return min(STALL_MAX_MS, max(STALL_MIN_MS, STALL_FACTOR * 1e3 * enqueue_seconds))


def stall(stream, ms):
    """busy `stream` for ms milliseconds -> the event recorded right behind the sleep"""
    import torch
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * cycles_per_ms()))
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


class Staged:
    """buf holds the decoy now; arm() enqueues buf.copy_(true) on the current stream (the stalled one, behind the stall)"""
    def __init__(self, true, decoy, device):
        import torch
        t, d = np.ascontiguousarray(true), np.ascontiguousarray(decoy)
        assert t.shape == d.shape and t.dtype == d.dtype, (t.shape, d.shape, t.dtype, d.dtype)
        self.src = torch.from_numpy(t).to(device)
        self.buf = torch.from_numpy(d).to(device)

    def arm(self):
        self.buf.copy_(self.src, non_blocking=True)
        return self.buf


def staged(true, decoy, device):
    return Staged(true, decoy, device)


# ------------------------------------------------------------------------------------------ inputs
N_ROWS, DIM = 300, 32
STEPS, BEAM_W, SCORE_K = 6, 3, 2
ROWS_KW = dict(dim_tgt=32, dim_emb=16, dim_rep=8, rnn_layers=1)     # the handle of the latent-row calls: they take any width


def _seed(which):
    return {'true': 1, 'decoy': 2}[which]


def rows(which, n=N_ROWS, dim=DIM):
    """n finite rows around 4 centres (the decoy: other centres, other rows)"""
    rng = np.random.default_rng(100 + _seed(which))
    c = rng.standard_normal((4, dim)) * 2.0
    return np.ascontiguousarray(c[rng.integers(0, 4, n)] + 0.3 * rng.standard_normal((n, dim)), np.float32)


def labels(which, n=N_ROWS, k=3, L=None):
    rng = np.random.default_rng(200 + _seed(which))
    lab = rng.integers(0, k, (L or 1, n)).astype(np.int32)
    lab[:, :k] = np.arange(k)            # every label present in every labelling
    return lab if L else lab[0]


def model_batch(which):
    """the b64 batch of tests/step_history.py, trimmed as VAE.trim trims it; the decoy: other ids in [3, V) at the same positions (the same
    lengths), the complementary keep mask, other draws"""
    import step_history as SH
    cfg, _, src, tgt, keep, eps = SH.make('b64')
    B, S = SH.shape('b64')
    src, tgt = np.ascontiguousarray(src[:, :S]), np.ascontiguousarray(tgt[:, :S])
    if which == 'decoy':
        V, eos = cfg['dim_tgt'], cfg['eos']
        other = lambda a: np.where(a != eos, 3 + (a - 3 + 7) % (V - 3), a).astype(np.int32)
        src, tgt = other(src), other(tgt)
        keep, eps = (1 - keep).astype(np.uint8), np.ascontiguousarray(-eps[::-1])
    return dict(src=src.astype(np.int32), tgt=tgt.astype(np.int32), keep=np.ascontiguousarray(keep, np.uint8), eps=np.ascontiguousarray(eps, np.float32))


def latents(which, b):
    import step_routes as SR
    rng = np.random.default_rng(300 + _seed(which))
    return rng.standard_normal((b, SR.R)).astype(np.float32)


# ------------------------------------------------------------------------------------------ a call's context
class Ctx:
    """what a case's call sees: the library, the handle, the device tensors by name (inputs and outputs), the host inputs, and `host` for the
    scalars the call returns through host pointers"""
    def __init__(self, m, t, I):
        self.m, self.l, self.h, self.t, self.I, self.host = m, m._l, m._h, t, I, {}

    def p(self, name):
        v = self.t.get(name)
        return None if v is None else C.c_void_p(v.data_ptr())

    def ck(self, rc):
        if rc:
            raise RuntimeError(self.l.avae_last_error(self.h).decode())

    def state(self, name):
        return getattr(self.m, name)


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    entries: tuple                  # the C entries the case runs on the stalled stream
    inputs: object                  # f(which, aux) -> {name: numpy array}: 'true' or 'decoy'
    outputs: object                 # f(I) -> {name: (shape, numpy dtype)}
    call: object                    # f(ctx): the part of the flow that is enqueued behind the stall; returns without synchronising unless sync
    sync: bool                      # the call synchronises the stream inside
    model: bool = False             # a model call: the D = 512 model of tests/step_history.py, its flat parameters staged
    warm: bool = False              # a step flow: the handle's first forward_backward (which synchronises once) is spent on the decoy batch first
    after: object = None            # f(ctx): entries that synchronise, run behind `call` (behind the event check)
    options: tuple = ()             # (key, value) of avae_set_option
    state_in: tuple = ()            # bound state staged besides the parameters: 'grads', 'adam_m', 'adam_v' (inputs of these names)
    state_out: tuple = ()           # bound state that is a result
    view: object = None             # f(host, {name: array}) -> the part of the outputs that the call defines (default: all of them)
    loose: tuple = ()               # results NOT compared bit for bit here (the test file says how instead)
    aux: str = ''                   # 'ref_grads': inputs() wants the flat gradient of the reference step


def _i32(*v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


# ---- model calls ------------------------------------------------------------------------------------------------------------------
def _fb(ctx):
    I = ctx.I
    B, Ss = I['src'].shape
    ctx.ck(ctx.l.avae_forward_backward(ctx.h, ctx.p('src'), ctx.p('tgt'), B, Ss, I['tgt'].shape[1], C.c_uint64(7), ctx.p('keep'), ctx.p('eps'), 0.0, 0.0))


def _after_step(ctx):
    out = (C.c_float * 3)()
    ctx.ck(ctx.l.avae_get_losses(ctx.h, out))
    ctx.host['losses'] = np.array(list(out), np.float32)
    n = C.c_int32()
    ctx.ck(ctx.l.avae_debug_train_ce(ctx.h, ctx.p('ce'), ctx.t['ce'].numel(), C.byref(n)))
    ctx.host['n_ce'] = n.value
    ids = (C.c_int32 * 2)()
    ctx.ck(ctx.l.avae_debug_present_ids(ctx.h, ids))
    ctx.host['present'] = np.array(list(ids), np.int32)


def _after_timing(ctx):
    """the step's losses and CE, then the stamps of the warm step and of the stalled one: the count read of a dyn-count GEMM goes to the device"""
    _after_step(ctx)
    out = (C.c_double * 9)()
    ctx.ck(ctx.l.avae_timing_collect(ctx.h, out))
    ctx.host['timing'] = np.array(list(out), np.float64).reshape(3, 3)


def _timing_view(host, o):
    """per class (gemm, gru_fwd, gru_bwd): launches and FLOPs (exact: counts, and static FLOPs scaled by device-side row counts) are results; the
    milliseconds are whatever the device took"""
    t = host['timing']
    assert np.isfinite(t).all() and (t[:, 0] >= 0).all() and (t[:, 1] > 0).all(), t
    return dict(losses=host['losses'], ce=o['ce'][:host['n_ce']], launches=t[:, 1].copy(), flops=t[:, 2].copy())


def _train_step(ctx):
    I = ctx.I
    B, Ss = I['src'].shape
    ctx.ck(ctx.l.avae_train_step(ctx.h, ctx.p('src'), ctx.p('tgt'), B, Ss, I['tgt'].shape[1], C.c_uint64(7), ctx.p('keep'), ctx.p('eps')))


def _step_view(host, o):
    return dict(losses=host['losses'], ce=o['ce'][:host['n_ce']], present=host['present'], grads=o['grads'])


def _adam_inputs(which, aux):
    g = np.ascontiguousarray(aux['ref_grads'], np.float32)
    n = g.shape[0]
    rng = np.random.default_rng(400 + _seed(which))
    m0, v0 = (1e-3 * rng.standard_normal(n)).astype(np.float32), (1e-6 * rng.random(n)).astype(np.float32)
    return dict(grads=g if which == 'true' else np.ascontiguousarray(0.5 * g[::-1]), adam_m=m0, adam_v=v0)


SET_NAMES = ('decode/rnn/l1/W', 'latent/ex/kernel')          # a variable stored permuted (g16_permute) and one stored as it is (a copy)


def _tensor_inputs(which, aux):
    import step_history as SH
    P = SH.make('b64')[1]
    # neither is what the handle's parameters hold (P, or 0.75 P in the decoy run): the result has values that only a set_tensor which ran
    # in order, behind the staged parameters, can have put there
    f = 1.5 if which == 'true' else -0.5
    return {'buf%d' % i: np.ascontiguousarray(f * P[k] + (0.0 if which == 'true' else 0.01), np.float32) for i, k in enumerate(SET_NAMES)}


def _set_tensor(ctx):
    for i, k in enumerate(SET_NAMES):
        ctx.ck(ctx.l.avae_set_tensor(ctx.h, k.encode(), 0, ctx.p('buf%d' % i)))


def _get_tensor(ctx):
    for i, k in enumerate(SET_NAMES):
        ctx.ck(ctx.l.avae_get_tensor(ctx.h, k.encode(), 0, ctx.p('out%d' % i)))


def _get_outputs(I):
    import step_history as SH
    P = SH.make('b64')[1]
    return {'out%d' % i: (P[k].shape, np.float32) for i, k in enumerate(SET_NAMES)}


def _eval(ctx):
    B, Ss = ctx.I['src'].shape
    n = C.c_int32()
    ctx.ck(ctx.l.avae_eval(ctx.h, ctx.p('src'), ctx.p('tgt'), B, Ss, ctx.I['tgt'].shape[1], ctx.p('errt'), ctx.p('lgen'), ctx.p('lkld'), C.byref(n)))
    ctx.host['n'] = n.value


def _encode(ctx):
    B, Ss = ctx.I['src'].shape
    ctx.ck(ctx.l.avae_encode(ctx.h, ctx.p('src'), B, Ss, ctx.p('z'), ctx.p('lv')))


def _rt(I):
    return I['src'].shape[0] * (I['tgt'].shape[1] + 1)


def _dims():
    import step_history as SH
    import step_routes as SR
    return SH.KW['dim_tgt'], SR.D, SR.R, SH.KW['rnn_layers']


def _decode_init(ctx):
    ctx.ck(ctx.l.avae_decode_init(ctx.h, ctx.p('z'), ctx.I['z'].shape[0], ctx.p('state')))


def _decode_step_inputs(which, aux):
    V, D, R, L = _dims()
    rng = np.random.default_rng(500 + _seed(which))
    b = 64
    return dict(lead=rng.integers(3, V, b).astype(np.int32), state_in=(0.1 * rng.standard_normal((L, b, D))).astype(np.float32))


def _decode_step(ctx):
    ctx.ck(ctx.l.avae_decode_step(ctx.h, ctx.p('lead'), ctx.p('state_in'), ctx.I['lead'].shape[0], ctx.p('pred'), ctx.p('state')))


def _greedy(ctx):
    n = C.c_int32()
    ctx.ck(ctx.l.avae_decode_greedy(ctx.h, ctx.p('z'), ctx.I['z'].shape[0], STEPS, ctx.p('ids'), C.byref(n)))
    ctx.host['n'] = n.value


def _sample(ctx):
    from argsim_amd import lib
    n, sc = C.c_int32(), lib.AvaeSampleConfig(0.9, 5, 11)
    ctx.ck(ctx.l.avae_decode_sample(ctx.h, ctx.p('z'), ctx.I['z'].shape[0], STEPS, C.byref(sc), ctx.p('ids'), ctx.p('logp'), C.byref(n)))
    ctx.host['n'] = n.value


def _sample_p(ctx):
    from argsim_amd import lib
    n, sc = C.c_int32(), lib.AvaeSamplePConfig(0.9, 0, 11, 0.8, 0)
    ctx.ck(ctx.l.avae_decode_sample_p(ctx.h, ctx.p('z'), ctx.I['z'].shape[0], STEPS, C.byref(sc), ctx.p('ids'), ctx.p('logp'), ctx.p('nkept'), C.byref(n)))
    ctx.host['n'] = n.value


def _beam(ctx):
    from argsim_amd import lib
    n, bc = C.c_int32(), lib.AvaeBeamConfig(BEAM_W, 0.6)
    ctx.ck(ctx.l.avae_decode_beam(ctx.h, ctx.p('z'), ctx.I['z'].shape[0], STEPS, C.byref(bc), ctx.p('ids'), ctx.p('score'), ctx.p('cum'), ctx.p('len'),
                                  ctx.p('lat_parent'), ctx.p('lat_token'), ctx.p('lat_cum'), C.byref(n)))
    ctx.host['n'] = n.value


def _decode_outputs(extra):
    def f(I):
        b = I['z'].shape[0]
        o = dict(ids=((b, STEPS), np.int32))
        if 'logp' in extra:
            o['logp'] = ((b, STEPS), np.float32)
        if 'nkept' in extra:
            o['nkept'] = ((b, STEPS), np.int32)
        return o
    return f


def _beam_outputs(I):
    b, W = I['z'].shape[0], BEAM_W
    return dict(ids=((b, W, STEPS), np.int32), score=((b, W), np.float32), cum=((b, W), np.float32), len=((b, W), np.int32),
                lat_parent=((STEPS, b, W), np.int32), lat_token=((STEPS, b, W), np.int32), lat_cum=((STEPS, b, W), np.float32))


def _z_inputs(b):
    return lambda which, aux: dict(z=latents(which, b))


def _score_inputs(which, aux):
    I = model_batch(which)
    rng = np.random.default_rng(600 + _seed(which))
    B, R = I['eps'].shape
    return dict(src=I['src'], tgt=I['tgt'], eps=rng.standard_normal((SCORE_K, B, R)).astype(np.float32))


def _score(ctx):
    from argsim_amd import lib
    B, Ss = ctx.I['src'].shape
    sc = lib.AvaeScoreConfig(SCORE_K, 3)
    ctx.ck(ctx.l.avae_score(ctx.h, ctx.p('src'), ctx.p('tgt'), B, Ss, ctx.I['tgt'].shape[1], C.byref(sc), ctx.p('eps'), ctx.p('eps_out'), ctx.p('logpx'),
                            ctx.p('logw'), ctx.p('bound'), ctx.p('ntok')))


def _score_outputs(I):
    k, B, R = I['eps'].shape
    return dict(eps_out=((k, B, R), np.float32), logpx=((k, B), np.float32), logw=((k, B), np.float32), bound=((B,), np.float32), ntok=((B,), np.int32))


def _score_z(ctx):
    b, St = ctx.I['tgt'].shape
    ctx.ck(ctx.l.avae_score_z(ctx.h, ctx.p('z'), ctx.p('tgt'), b, St, ctx.p('logpx'), ctx.p('ntok')))


def _batch(*names):
    return lambda which, aux: {k: v for k, v in model_batch(which).items() if k in names}


def _eval_view(host, o):
    return dict(errt=o['errt'][:host['n']], lgen=o['lgen'][:host['n']], lkld=o['lkld'], n=np.array([host['n']]))


def _n_view(host, o):
    return dict(o, n=np.array([host['n']]))


# ---- latent-row calls -------------------------------------------------------------------------------------------------------------
def _knn(ctx):
    from argsim_amd import lib
    kc = lib.AvaeKnnConfig(5, 1, 0, 0, 0, 0)
    ctx.ck(ctx.l.avae_knn(ctx.h, ctx.p('q'), N_ROWS, ctx.p('bank'), N_ROWS, DIM, C.byref(kc), ctx.p('idx'), ctx.p('score')))


def _agg_inputs(which, aux):
    rng = np.random.default_rng(700 + _seed(which))
    mu, lv = rows(which), (0.3 * rng.standard_normal((N_ROWS, DIM))).astype(np.float32)
    z = (mu + np.exp(0.5 * lv) * rng.standard_normal((N_ROWS, DIM))).astype(np.float32)
    return dict(z=z, mu=mu, lv=lv)


def _agg(ctx):
    from argsim_amd import lib
    ac = lib.AvaeAggConfig(0, (C.c_int32 * 2)(0, 0))
    ctx.ck(ctx.l.avae_agg_logq(ctx.h, ctx.p('z'), N_ROWS, ctx.p('mu'), ctx.p('lv'), N_ROWS, DIM, C.byref(ac), ctx.p('logq'), ctx.p('logqx')))


def _moments(ctx):
    ctx.ck(ctx.l.avae_latent_moments(ctx.h, ctx.p('mu'), ctx.p('lv'), N_ROWS, DIM, ctx.p('out')))


def _probe_inputs(C_, cw):
    def f(which, aux):
        from argsim_amd import probe
        _, costs = probe.probe_costs(labels(which), None, C_, cw)
        return dict(x=rows(which), s=np.ascontiguousarray(costs, np.float32))
    return f


def _probe_fit(ctx):
    from argsim_amd import lib, probe
    pc = lib.AvaeProbeConfig(probe.DEFAULT_MAX_NEWTON, probe.DEFAULT_MAX_CG, probe.DEFAULT_TOL, 0)
    ctx.ck(ctx.l.avae_probe_fit(ctx.h, ctx.p('x'), N_ROWS, DIM, ctx.p('s'), ctx.I['s'].shape[0], C.byref(pc), ctx.p('w'), ctx.p('stats')))


def _probe_fit_l1(ctx):
    from argsim_amd import lib, probe
    pc = lib.AvaeProbeL1Config(probe.DEFAULT_MAX_NEWTON, probe.DEFAULT_MAX_INNER, probe.DEFAULT_TOL, 0)
    ctx.ck(ctx.l.avae_probe_fit_l1(ctx.h, ctx.p('x'), N_ROWS, DIM, ctx.p('s'), ctx.I['s'].shape[0], C.byref(pc), ctx.p('w'), ctx.p('stats')))


def _probe_outputs(I):
    P = I['s'].shape[0]
    return dict(w=((P, DIM + 1), np.float32), stats=((P, 4), np.float32))


def _decision_inputs(which, aux):
    rng = np.random.default_rng(800 + _seed(which))
    return dict(x=rows(which), w=(0.2 * rng.standard_normal((3, DIM + 1))).astype(np.float32))


def _decision(ctx):
    ctx.ck(ctx.l.avae_probe_decision(ctx.h, ctx.p('x'), N_ROWS, DIM, ctx.p('w'), 3, ctx.p('out')))


GROUP_OFF, CUT_K = (0, 100, 200, 300), (3, 5, 7)


def _ward(ctx):
    from argsim_amd import lib
    wc = lib.AvaeWardConfig()
    ctx.ck(ctx.l.avae_ward(ctx.h, ctx.p('x'), DIM, _i32(*GROUP_OFF), 3, C.byref(wc), ctx.p('pair'), ctx.p('delta'), ctx.p('size')))


def _cut_inputs(which, aux):
    """a valid merge list per group without running the clustering: the true one chains every row into slot 0, (0, 1), (0, 2), ..; the
    decoy merges from the top, (n - 2, n - 1), (n - 3, n - 2), ..  In both a < b, b is alive and is merged away exactly once"""
    out = []
    for g in range(3):
        n = GROUP_OFF[g + 1] - GROUP_OFF[g]
        out.append([(0, t + 1) if which == 'true' else (n - 2 - t, n - 1 - t) for t in range(n - 1)])
    return dict(pair=np.array(sum(out, []), np.int32).reshape(-1, 2))


def _ward_cut(ctx):
    ctx.ck(ctx.l.avae_ward_cut(ctx.h, ctx.p('pair'), _i32(*GROUP_OFF), 3, _i32(*CUT_K), ctx.p('label')))


def _affinity(ctx):
    from argsim_amd import lib
    ac = lib.AvaeAffinityConfig(metric=0, max_iter=30, convergence_iter=5, use_preference=0, noise=1, warm=0, damping=0.7, preference=0.0, seed=1)
    ctx.ck(ctx.l.avae_affinity(ctx.h, ctx.p('x'), N_ROWS, DIM, C.byref(ac), ctx.p('label'), ctx.p('stat'), ctx.p('s'), ctx.p('a'), ctx.p('r')))


TSNE_N, TSNE_ITER = 150, 25


def _tsne(ctx):
    from argsim_amd import lib
    tc = lib.AvaeTsneConfig(perplexity=12.0, early_exaggeration=12.0, min_grad_norm=1e-7, learning_rate=0.0, max_iter=TSNE_ITER, it0=0,
                            exaggeration_iter=10, n_iter_check=5, n_iter_without_progress=300, init=1, warm=0, seed=1)
    ctx.ck(ctx.l.avae_tsne(ctx.h, ctx.p('x'), TSNE_N, DIM, C.byref(tc), None, ctx.p('y'), ctx.p('kl'), ctx.p('stat'), ctx.p('p'), ctx.p('beta'), None, None,
                           ctx.p('ug'), ctx.p('prog')))


KM_K, KM_R = 5, 2


def _kmeans(ctx):
    from argsim_amd import lib
    kc = lib.AvaeKmeansConfig(k=KM_K, n_init=KM_R, max_iter=20, metric=0, init=0, reserved=0, tol=1e-4, seed=3)
    ctx.ck(ctx.l.avae_kmeans(ctx.h, ctx.p('x'), N_ROWS, DIM, C.byref(kc), None, ctx.p('label'), ctx.p('centers'), ctx.p('stat'), ctx.p('inertia'),
                             ctx.p('label_all'), ctx.p('centers_all'), ctx.p('stat_all')))


GM_K = 4


def _gmm_fit(ctx):
    from argsim_amd import lib
    gc = lib.AvaeGmmConfig(k=GM_K, n_init=1, max_iter=8, covariance=0, init=0, reserved=0, tol=1e-3, reg_covar=1e-6)
    outs = ('weights', 'means', 'covars', 'label', 'stat', 'lower', 'logp', 'resp')
    ctx.ck(ctx.l.avae_gmm_fit(ctx.h, ctx.p('x'), N_ROWS, DIM, C.byref(gc), ctx.p('label_in'), None, None, None, *[ctx.p(n) for n in outs],
                              None, None, None, None, None))


def _gmm_score_inputs(which, aux):
    rng = np.random.default_rng(900 + _seed(which))
    w = rng.random(GM_K) + 0.5
    return dict(x=rows(which), weights=w / w.sum(), means=rng.standard_normal((GM_K, DIM)) * 2.0, covars=0.5 + rng.random((GM_K, DIM)))


def _gmm_score(ctx):
    ctx.ck(ctx.l.avae_gmm_score(ctx.h, ctx.p('x'), N_ROWS, DIM, GM_K, ctx.p('weights'), ctx.p('means'), ctx.p('covars'), ctx.p('logp'), ctx.p('label'),
                                ctx.p('resp')))


SIL_L, SIL_K = 3, 4


def _sil_inputs(which, aux):
    lab = labels(which, k=SIL_K, L=SIL_L)
    lab[1, 10:20] = -1              # rows left out of one labelling
    return dict(x=rows(which), label=lab)


def _silhouette(ctx):
    from argsim_amd import lib
    sc = lib.AvaeSilhouetteConfig(0, SIL_L, 0, 0)
    ctx.ck(ctx.l.avae_silhouette(ctx.h, ctx.p('x'), N_ROWS, DIM, C.byref(sc), ctx.p('label'), _i32(*([SIL_K] * SIL_L)), ctx.p('score'), ctx.p('sil'),
                                 ctx.p('ab'), ctx.p('nearest'), ctx.p('count'), ctx.p('cluster_mean'), ctx.p('index')))


def _dbscan(ctx):
    from argsim_amd import lib
    dc = lib.AvaeDbscanConfig(metric=0, min_samples=4, max_rounds=0, reserved=0, eps=2.6)
    ctx.ck(ctx.l.avae_dbscan(ctx.h, ctx.p('x'), N_ROWS, DIM, C.byref(dc), ctx.p('label'), ctx.p('count'), ctx.p('stat')))


def _pca_fit(ctx):
    from argsim_amd import lib
    pc = lib.AvaePcaConfig(0, 0, 0, 0)
    ctx.ck(ctx.l.avae_pca_fit(ctx.h, ctx.p('x'), N_ROWS, DIM, C.byref(pc), ctx.p('mean'), ctx.p('var'), ctx.p('comp'), ctx.p('stat')))


PCA_K = 5


def _pca_t_inputs(which, aux):
    rng = np.random.default_rng(1000 + _seed(which))
    return dict(x=rows(which), mean=rng.standard_normal(DIM), comp=rng.standard_normal((PCA_K, DIM)), scale=0.5 + rng.random(PCA_K))


def _pca_transform(ctx):
    ctx.ck(ctx.l.avae_pca_transform(ctx.h, ctx.p('x'), N_ROWS, DIM, ctx.p('mean'), ctx.p('comp'), ctx.p('scale'), PCA_K, ctx.p('y')))


MMD_G, MMD_P = 2, 7
MMD_W = (N_ROWS + 63) // 64


def _pack(bits):
    from argsim_amd import mmd
    return np.ascontiguousarray(mmd.pack_bits(bits)).view(np.int64)


def _mmd_groups(which):
    """(G, N) group ids: 0 (sample A), 1 (sample B), -1 left out; every comparison has both samples"""
    rng = np.random.default_rng(1100 + _seed(which))
    g = rng.integers(-1, 2, (MMD_G, N_ROWS))
    g[:, 0], g[:, 1] = 0, 1
    return g


def _mmd_inputs(which, aux):
    """relabelings 1 .. P built on the host: permutations of the observed assignment among the valid rows (the sizes stay m and n)"""
    g = _mmd_groups(which)
    rng = np.random.default_rng(1200 + _seed(which))
    inA = np.zeros((MMD_G, 1 + MMD_P, N_ROWS), bool)
    for i in range(MMD_G):
        v = np.flatnonzero(g[i] >= 0)
        inA[i, 0] = g[i] == 0
        for p in range(1, 1 + MMD_P):
            inA[i, p, v] = inA[i, 0, rng.permutation(v)]
    return dict(x=rows(which), valid=_pack(g >= 0), inA=_pack(inA))


def _mmd(ctx):
    from argsim_amd import lib
    mc = lib.AvaeMmdConfig(kernel=0, metric=0, G=MMD_G, P=MMD_P, nbw=1, reserved=0)
    mc.gamma[0] = 0.02
    ctx.ck(ctx.l.avae_mmd(ctx.h, ctx.p('x'), N_ROWS, DIM, C.byref(mc), ctx.p('valid'), ctx.p('inA'), ctx.p('stat'), ctx.p('pvalue'), ctx.p('counts'),
                          ctx.p('sums'), ctx.p('ull'), ctx.p('witness'), ctx.p('stat_out')))


def _relabel_inputs(which, aux):
    """the mask words are in AND out: relabeling 0 comes from the host, 1 .. P are written on the device over the sentinel"""
    g = _mmd_groups(which)
    words = np.full((MMD_G, 1 + MMD_P, MMD_W), sentinel(np.int64), np.int64)
    words[:, 0] = _pack(g == 0)
    return dict(valid=_pack(g >= 0), inA=words)


def _mmd_relabel(ctx):
    ctx.ck(ctx.l.avae_mmd_relabel(ctx.h, N_ROWS, MMD_G, MMD_P, ctx.p('valid'), ctx.p('inA'), C.c_uint64(5)))


def _x(which, aux):
    return dict(x=rows(which))


def _cases():
    f32, f64, i32, i64 = np.float32, np.float64, np.int32, np.int64
    N, D = N_ROWS, DIM
    V_, D_, R_, L_ = 256, 512, 32, 2          # tests/step_history.py KW (asserted in test_stream_table.py)
    B_, S_ = 64, 6
    c = []
    add = lambda *a, **k: c.append(Case(*a, **k))
    # ---- state and training
    add('set_tensor', ('avae_set_tensor',), _tensor_inputs, lambda I: {}, _set_tensor, False, model=True, state_out=('params',))
    add('get_tensor', ('avae_get_tensor',), lambda w, a: {}, _get_outputs, _get_tensor, False, model=True)
    add('step', ('avae_forward_backward', 'avae_get_losses', 'avae_debug_train_ce', 'avae_debug_present_ids'), _batch('src', 'tgt', 'keep', 'eps'),
        lambda I: dict(ce=((_rt(I),), f32)), _fb, False, model=True, warm=True, after=_after_step, state_out=('grads',), view=_step_view, loose=('grads',))
    add('adam_step', ('avae_adam_step',), _adam_inputs, lambda I: {}, lambda ctx: ctx.ck(ctx.l.avae_adam_step(ctx.h)), False, model=True,
        state_in=('grads', 'adam_m', 'adam_v'), state_out=('params', 'adam_m', 'adam_v'), aux='ref_grads')
    add('train_step', ('avae_train_step',), _batch('src', 'tgt', 'keep', 'eps'), lambda I: dict(ce=((_rt(I),), f32)), _train_step, False, model=True,
        warm=True, after=_after_step, state_out=('grads', 'params'), view=lambda h, o: dict(_step_view(h, o), params=o['params']), loose=('grads', 'params'))
    add('timing', ('avae_timing_collect',), _batch('src', 'tgt', 'keep', 'eps'), lambda I: dict(ce=((_rt(I),), f32)), _fb, False, model=True, warm=True,
        after=_after_timing, view=_timing_view, options=(('timing', 1),))
    add('eval', ('avae_eval',), _batch('src', 'tgt'), lambda I: dict(errt=((_rt(I),), f32), lgen=((_rt(I),), f32), lkld=((B_, R_), f32)), _eval, True,
        model=True, view=_eval_view)
    add('encode', ('avae_encode',), _batch('src'), lambda I: dict(z=((B_, R_), f32), lv=((B_, R_), f32)), _encode, True, model=True)
    # ---- decoding and scoring: 64 rows take the launch-per-token loop, 20 rows the one persistent launch
    add('decode_init', ('avae_decode_init',), _z_inputs(64), lambda I: dict(state=((L_, 64, D_), f32)), _decode_init, False, model=True)
    add('decode_step', ('avae_decode_step',), _decode_step_inputs, lambda I: dict(pred=((64,), i32), state=((L_, 64, D_), f32)), _decode_step, True, model=True)
    for b in (64, 20):
        add('decode_greedy-b%d' % b, ('avae_decode_greedy',), _z_inputs(b), _decode_outputs(()), _greedy, True, model=True, view=_n_view)
        add('decode_sample-b%d' % b, ('avae_decode_sample',), _z_inputs(b), _decode_outputs(('logp',)), _sample, True, model=True, view=_n_view)
        add('decode_sample_p-b%d' % b, ('avae_decode_sample_p',), _z_inputs(b), _decode_outputs(('logp', 'nkept')), _sample_p, True, model=True, view=_n_view)
    add('decode_beam', ('avae_decode_beam',), _z_inputs(20), _beam_outputs, _beam, True, model=True,
        view=lambda h, o: dict({k: (v[:h['n']] if k[:3] == 'lat' else v) for k, v in o.items()}, n=np.array([h['n']])))
    add('score', ('avae_score',), _score_inputs, _score_outputs, _score, True, model=True)
    add('score_z', ('avae_score_z',), lambda w, a: dict(z=latents(w, B_), tgt=model_batch(w)['tgt']), lambda I: dict(logpx=((B_,), f32), ntok=((B_,), i32)),
        _score_z, True, model=True)
    # ---- nearest neighbours and posterior diagnostics
    add('knn', ('avae_knn',), lambda w, a: dict(q=rows(w), bank=rows(w)), lambda I: dict(idx=((N, 5), i64), score=((N, 5), f32)), _knn, False,
        options=(('knn_chunk', 128),))
    add('agg_logq', ('avae_agg_logq',), _agg_inputs, lambda I: dict(logq=((N,), f32), logqx=((N,), f32)), _agg, False, options=(('agg_chunk', 70),))
    add('latent_moments', ('avae_latent_moments',), lambda w, a: {k: v for k, v in _agg_inputs(w, a).items() if k != 'z'}, lambda I: dict(out=((4, D), f32)),
        _moments, False)
    # ---- probes
    add('probe_fit', ('avae_probe_fit',), _probe_inputs(0.001, 'balanced'), _probe_outputs, _probe_fit, True, options=(('probe_chunk', 50),))
    add('probe_fit_l1', ('avae_probe_fit_l1',), _probe_inputs(0.1, None), _probe_outputs, _probe_fit_l1, True, options=(('probe_chunk', 50),))
    add('probe_decision', ('avae_probe_decision',), _decision_inputs, lambda I: dict(out=((N, 3), f32)), _decision, False, options=(('probe_chunk', 50),))
    # ---- clustering
    for form in (1, 2):
        add('ward-form%d' % form, ('avae_ward',), _x, lambda I: dict(pair=((N - 3, 2), i32), delta=((N - 3,), f32), size=((N - 3,), i32)), _ward, False,
            options=(('ward_form', form),))
    add('ward_cut', ('avae_ward_cut',), _cut_inputs, lambda I: dict(label=((N,), i32)), _ward_cut, False)
    add('affinity', ('avae_affinity',), _x, lambda I: dict(label=((N,), i32), stat=((4,), i32), s=((N, N), f32), a=((N, N), f32), r=((N, N), f32)),
        _affinity, False)
    add('tsne', ('avae_tsne',), lambda w, a: dict(x=rows(w, TSNE_N)),
        lambda I: dict(y=((TSNE_N, 2), f32), kl=((2,), f64), stat=((4,), i32), p=((TSNE_N, TSNE_N), f64), beta=((TSNE_N,), f64), ug=((2, TSNE_N, 2), f32),
                       prog=((4,), f64)), _tsne, False, options=(('tsne_chunk', 33),))
    add('kmeans', ('avae_kmeans',), _x,
        lambda I: dict(label=((N,), i32), centers=((KM_K, D), f32), stat=((4,), i32), inertia=((KM_R,), f64), label_all=((KM_R, N), i32),
                       centers_all=((KM_R, KM_K, D), f64), stat_all=((KM_R, 4), i32)), _kmeans, False, options=(('kmeans_chunk', 2),))
    add('gmm_fit', ('avae_gmm_fit',), lambda w, a: dict(x=rows(w), label_in=labels(w, k=GM_K, L=1)),
        lambda I: dict(weights=((GM_K,), f64), means=((GM_K, D), f64), covars=((GM_K, D), f64), label=((N,), i32), stat=((4,), i32), lower=((1,), f64),
                       logp=((N,), f64), resp=((N, GM_K), f64)), _gmm_fit, False, options=(('gmm_chunk', 1),))
    add('gmm_score', ('avae_gmm_score',), _gmm_score_inputs, lambda I: dict(logp=((N,), f64), label=((N,), i32), resp=((N, GM_K), f64)), _gmm_score, False,
        options=(('gmm_chunk', 2),))
    add('silhouette', ('avae_silhouette',), _sil_inputs,
        lambda I: dict(score=((SIL_L,), f64), sil=((SIL_L, N), f64), ab=((SIL_L, N, 2), f64), nearest=((SIL_L, N), i32), count=((SIL_L, SIL_K), i32),
                       cluster_mean=((SIL_L, SIL_K), f64), index=((SIL_L, 2), f64)), _silhouette, False, options=(('sil_chunk', 4),))
    add('dbscan', ('avae_dbscan',), _x, lambda I: dict(label=((N,), i32), count=((N,), i32), stat=((8,), i32)), _dbscan, False,
        options=(('dbscan_chunk', 8 | (1 << 8)),))
    # ---- PCA and MMD
    for form in (1, 2):
        add('pca_fit-form%d' % form, ('avae_pca_fit',), _x, lambda I: dict(mean=((D,), f64), var=((D,), f64), comp=((D, D), f64), stat=((8,), i32)), _pca_fit,
            False, options=(('pca_chunk', 7), ('pca_form', form)))
    add('pca_transform', ('avae_pca_transform',), _pca_t_inputs, lambda I: dict(y=((N, PCA_K), f32)), _pca_transform, False, options=(('pca_chunk', 4),))
    add('mmd', ('avae_mmd',), _mmd_inputs,
        lambda I: dict(stat=((MMD_G, 1 + MMD_P), f64), pvalue=((MMD_G,), f64), counts=((MMD_G, 2), i32), sums=((MMD_G, 1 + MMD_P, 2), f64), ull=((MMD_G,), f64),
                       witness=((MMD_G, N), f64), stat_out=((1,), i32)), _mmd, True, options=(('mmd_chunk', 5),))
    add('mmd_relabel', ('avae_mmd_relabel',), _relabel_inputs, lambda I: {}, _mmd_relabel, False, view=lambda h, o: dict(inA=o['inA']))
    return c


CASES = _cases()
# in and out at once: the buffer is an input of that name and is read back as a result
INOUT = {'mmd_relabel': ('inA',)}

# host-only entries: nothing is enqueued, so there is nothing a stream could order
EXEMPT = {
    'avae_create': 'allocates and clears the small device state with synchronous calls before a stream exists',
    'avae_destroy': 'synchronises the stream and frees',
    'avae_last_error': 'reads a host string',
    'avae_set_stream': 'stores the stream; every case calls it',
    'avae_get_dims': 'reads the host configuration',
    'avae_state_numel': 'reads the host parameter table',
    'avae_bind_state': 'stores four pointers',
    'avae_param_count': 'reads the host parameter table',
    'avae_param_name': 'reads the host parameter table',
    'avae_param_info': 'reads the host parameter table',
    'avae_get_step': 'reads a host counter',
    'avae_set_step': 'writes a host counter',
    'avae_get_schedule': 'computes three host floats from the step',
    'avae_set_grad_hook': 'stores a host callback',
    'avae_set_option': 'writes host options',
    'avae_bucket_count': 'reads the host bucket table',
    'avae_bucket_info': 'reads the host bucket table',
}
# the debug hooks the issue names get a case all the same (both in the 'step' flow)
DEBUG_WITH_CASE = ('avae_debug_train_ce', 'avae_debug_present_ids')
