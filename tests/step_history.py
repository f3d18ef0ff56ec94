"""The table of tests/test_gpu_step_history.py: training steps on the AUTOMATIC path -- compact, bwd_rs and gru_spec left at the library's
default of 2 -- on one handle that has seen other batches before.  tests/step_routes.py pins every route with the three options forced, on a
handle that has seen one shape; the product runs neither way: every batch of a training loop has another width and another fill, and
validation, encoding and decoding calls sit between the steps.

What outlives a call in model.cpp and shapes the next one is the fill hint (build_row_orders: real and padded source positions of the last
call that sorted source rows -- forward_backward, eval, encode, score alike), read once where a call starts (latch_hint).  It decides whether
the step takes the compact layout (build_compact: fill < 0.92; a batch with phantom rows takes it whatever the hint), which BPTT team kernel
it runs (rs_pick: < 0.40), the exchange protocol (spec_pick: < 0.60) and the row counts gemm_plan expects behind the compact layout
(expect_val, then dyn_expect and the K split of the narrow backward GEMMs).  The workspace arena and the 16-bit panels are freed and
reallocated where a larger shape arrives.  The code says of all of it "shapes launches only, never a value"; the sequences below are where
that is held against float64 with a WRONG hint -- that of another batch.

One model configuration (KW), so that one handle runs every batch.  PROBES are compared with the float64 oracle; PRIMERS only leave their
hint and their workspace behind.  A sequence is a list of calls (kind, batch); every 'fb' on a probe is a checked step.  The route a checked
step must take (expected_route) is derived HERE from the fill of the call before it and the three thresholds -- nothing is read back from the
library; tests/test_step_history.py holds the table against the planners without a GPU.

LATE_SEQUENCES (below SEQUENCES) are the steps of a loop that does NOT synchronise, for tests/test_gpu_stream.py: what a step plans from when
the hint of the call in front of it has not arrived."""
import numpy as np

import helpers
import step_routes as SR

KW = dict(dim_tgt=256, dim_emb=SR.D, dim_rep=SR.R, rnn_layers=2)
COMPACT_BELOW, RS_BELOW, SPEC_BELOW = 0.92, 0.40, 0.60      # build_compact, rs_pick, spec_pick (model.cpp)
MARGIN = 0.03                                               # no fill of the table lies this close to a threshold

# ---- probe batches: (B, S, lens) of helpers.make_batch
#   b64      the batch of step_routes: ragged, both first layers table-fed, own team geometry
#   b64full  every row full: 384 source tokens >= V, so it is table-fed and CAN take the compact layout a stale hint asks for
#   b20      32 slots, 12 phantom rows: the compact layout whatever the hint
#   b100v    128 slots; lengths 2..9 in a fixed pattern, rows 0 and 50 full, row 1 of length 1 (the 'ragged' draw of 100 x 11 has a fill of
#            0.576, inside the margin of 0.60)
_L100 = [2 + (7 * i) % 8 for i in range(100)]
_L100[0] = _L100[50] = 11
_L100[1] = 1
PROBES = {
    'b64':     (64, 6, 'ragged'),
    'b64full': (64, 6, None),
    'b20':     (20, 14, 'ragged'),
    'b100v':   (100, 11, _L100),
}
# ---- primer batches: explicit lengths, no oracle
#   low   one full row, the rest of length 2 or 3; 64 x 14 is larger than every 64-row probe: the workspace grows on the way in
#   mid   between the BPTT and the exchange thresholds
#   full  a FULL batch of another shape than b64full
PRIMERS = {
    'low':  (64, 14, [14] + [2 + i % 2 for i in range(63)]),
    'mid':  (64, 8, [8] + [3 + i % 3 for i in range(63)]),
    'full': (64, 3, None),
}
FILL = {'b64': 0.648, 'b64full': 1.0, 'b20': 0.496, 'b100v': 0.507, 'low': 0.191, 'mid': 0.508, 'full': 1.0}
# rows of the team kernels' launch geometry (gru_team_batch) and the (T, C) of the two-direction and the one-job launches there
TEAMS = {64: (64, (4, 2), (2, 2)), 20: (32, (2, 2), (2, 1)), 100: (128, (2, 8), (2, 4))}

_BATCH = {}


def make(name):
    """-> cfg, P, src, tgt, keep, eps of helpers.make_batch; P depends on KW alone, so every batch carries the same parameters"""
    if name not in _BATCH:
        B, S, lens = PROBES.get(name) or PRIMERS[name]
        cfg, P, ids, keep, eps = helpers.make_batch(KW, B, S, lens if lens is None or isinstance(lens, str) else list(lens))
        _BATCH[name] = (cfg, P, ids.copy(), ids.copy(), keep, eps)
    return _BATCH[name]


def shape(name):
    """(B, Ss) as the library sees the batch: trailing all-eos columns trimmed"""
    cfg, _, src, _, _, _ = make(name)
    lens = (src != cfg['eos']).sum(1)
    return len(lens), int(lens.max())


def fill(name):
    """real source positions / padded source positions: what the fill hint holds once a call on the batch has completed"""
    cfg, _, src, _, _, _ = make(name)
    lens = (src != cfg['eos']).sum(1)
    return float(lens.sum()) / float(lens.max() * len(lens))


# ------------------------------------------------------------------------------------------ sequences
# kinds of call:  fb forward_backward   eval   encode   score (k = 2)   decode (greedy) and knn (the rows among themselves): of the rows the
# last encode of the sequence returned -- its batch is named again.  FEEDS: the kinds whose encoder pass sorts the source rows and so leaves
# a hint (build_row_orders, which[0] == 0).
FEEDS = ('fb', 'eval', 'encode', 'score')
SEQUENCES = {
    # nothing arrived: no layout, gather BPTT; then its own fill
    'fresh':        ('f32', [('fb', 'b64'), ('fb', 'b64')]),
    # a long-tailed batch in front of a FULL one: compact layout, reduce-scatter BPTT and a 5-times-too-small dyn_expect on full rows; then
    # its own hint of 1.0: no layout
    'low-full':     ('f32', [('fb', 'low'), ('fb', 'b64full'), ('fb', 'b64full')]),
    # a FULL batch in front of a ragged one, by encode: no compact layout on a ragged batch
    'full-ragged':  ('f32', [('encode', 'full'), ('fb', 'b64')]),
    # phantom rows: the layout whatever the hint, the BPTT form of the call before; the shape grows and shrinks on one handle
    'phantom':      ('f32', [('encode', 'low'), ('fb', 'b20'), ('fb', 'b100v'), ('fb', 'b20')]),
    # between 0.40 and 0.60: the exchange without the probe round trip, the gather BPTT
    'mid-ragged':   ('f32', [('fb', 'mid'), ('fb', 'b64')]),
    'mid-full':     ('f32', [('fb', 'mid'), ('fb', 'b64full')]),
    # one "epoch": the shape changes at every step, and every other kind of call sits between the steps
    'epoch':        ('f32', [('fb', 'b64'), ('eval', 'low'), ('fb', 'b20'), ('encode', 'b20'), ('decode', 'b20'), ('fb', 'b64full'),
                             ('fb', 'low'), ('fb', 'b100v'), ('score', 'b20'), ('fb', 'b64'), ('fb', 'full'), ('fb', 'b100v'),
                             ('encode', 'mid'), ('knn', 'mid'), ('fb', 'low'), ('fb', 'b64full'), ('fb', 'mid'), ('fb', 'b20'),
                             ('eval', 'full'), ('decode', 'mid'), ('fb', 'b64')]),
    'low-full-bf16':    ('bf16', [('fb', 'low'), ('fb', 'b64full'), ('fb', 'b64full')]),
    'full-ragged-bf16': ('bf16', [('encode', 'full'), ('fb', 'b64')]),
    'chain-f32s':       ('f32s', [('fb', 'low'), ('fb', 'b64full'), ('fb', 'b20'), ('fb', 'b64')]),
}


def expected_route(batch, prev, dtype):
    """step_route() of a forward_backward on `batch` after a call that left the fill `prev` (None: nothing arrived), options at their defaults"""
    B, _ = shape(batch)
    Bx, pair, one = TEAMS[B]
    compact = Bx != B or (prev is not None and prev < COMPACT_BELOW)
    rs = int(prev is not None and prev < RS_BELOW)
    ring = 0 if dtype == 'bf16' else 4                      # (bf16: no exchange ring, and no reduce-scatter form -- the pick is noted all the same)
    pair, one = SR._team(*pair, ring=ring), SR._team(*one, ring=ring)
    bwd = dict(pair_bwd=SR._rs(pair), one_bwd=SR._rs(one)) if rs and dtype != 'bf16' else {}
    return dict(SR._route(compact=(int(compact),) * 2, Bx=Bx, bwd_rs=rs, pair=pair, one=one, **bwd))


def expected_rows(batch, prev, compact):
    """VAE.row_expect() behind a forward_backward on `batch`: the fill of the call before it scaled to this batch's rows -- (int)(fill * Ss * B)
    source rows, (int)(fill * T * B) decoder rows and tokens (build_compact) --, zeros where the step takes no layout or nothing had arrived"""
    (B, S), f = shape(batch), 0.0 if prev is None else min(1.0, prev)
    return (int(f * S * B), int(f * (S + 1) * B), int(f * (S + 1) * B)) if compact else (0, 0, 0)


def steps(name):
    """the calls of a sequence with what the table derives for each: [(kind, batch, prev fill or None, expected route or None, expected row
    expectations or None)] -- a route and expectations for every checked step (an fb on a probe)"""
    dtype, calls = SEQUENCES[name]
    out, prev = [], None
    for kind, batch in calls:
        route = expected_route(batch, prev, dtype) if kind == 'fb' and batch in PROBES else None
        out.append((kind, batch, prev, route, expected_rows(batch, prev, route['compact'][0]) if route else None))
        if kind in FEEDS:
            prev = fill(batch)
    return out


# ------------------------------------------------------------------------------------------ sequences whose hint is LATE
# tests/test_gpu_stream.py part C: the steps of a training loop that does not synchronise.  A call's hint lands when the stream reaches its
# copy, so a step enqueued behind a busy stream plans from whatever had landed when IT began -- the fill of an earlier call, or nothing.
# Third field of a call, `when`:
#   'sync'    the stream is synchronised behind the call: its hint has arrived before the next call starts (every call of SEQUENCES)
#   'late'    the call is enqueued on a stalled stream, and nothing synchronises behind it unless the NEXT call is not 'late' (then the run of late
#             calls is over: the test synchronises there to read the last step).  Every call of one run sees what had arrived before the run.
#   'nohint'  the call runs with option compact forced to 1 (the hint is sent under compact = 2 alone, build_row_orders), synchronised, and
#             the option goes back to 2: the handle has been used and nothing is on its way.  The first forward_backward of a handle
#             synchronises once by itself (model.cpp first_step_checked), so a step that is to see NOTHING cannot be the second call behind a
#             first step that feeds -- that first step's hint has always arrived.
# The step that is checked against the oracle is the LAST of a run of late calls and every 'sync' fb on a probe: losses(), train_ce() and the
# gradient hold the last step only.
LATE_SEQUENCES = {
    # 1. a used handle, nothing arrived: `low`'s hint sits behind the stall, so the FULL batch takes no layout and the gather BPTT --
    #    with low's hint it would take the compact layout and the reduce-scatter form ('low-full' above)
    'late-nothing':      ('f32', [('fb', 'low', 'nohint'), ('fb', 'low', 'late'), ('fb', 'b64full', 'late')]),
    'late-nothing-bf16': ('bf16', [('fb', 'low', 'nohint'), ('fb', 'low', 'late'), ('fb', 'b64full', 'late')]),
    # 2. one step stale: b20 plans from low's fill (reduce-scatter BPTT, a fifth of the rows expected), not from b64full's 1.0 (gather, all
    #    rows) whose copy is still queued.  3. caught up: the last hint copied in stream order is that of the run's LAST call, b20 itself
    #    (each call's copy overwrites the pinned pair when the stream reaches it; b64full's landed first and b20's over it)
    'late-stale':        ('f32', [('fb', 'low', 'sync'), ('fb', 'b64full', 'late'), ('fb', 'b20', 'late'), ('fb', 'b20', 'sync')]),
}


def late_steps(name):
    """the calls of a late sequence with what the table derives for each: [(kind, batch, when, fill that HAD ARRIVED or None, expected route,
    expected row expectations, checked)] -- route and rows for every fb on a probe, checked: the step is read back and held to the oracle"""
    dtype, calls = LATE_SEQUENCES[name]
    out, arrived, queued = [], None, None
    for i, (kind, batch, when) in enumerate(calls):
        assert when in ('sync', 'late', 'nohint'), when
        probe = kind == 'fb' and batch in PROBES
        forced = when == 'nohint'           # compact = 1: the layout whatever the hint, zero expectations if nothing has arrived
        route = expected_route(batch, arrived, dtype) if probe and not forced else None
        ends_run = when != 'late' or i + 1 == len(calls) or calls[i + 1][2] != 'late'
        out.append((kind, batch, when, arrived, route, expected_rows(batch, arrived, route['compact'][0]) if route else None,
                    bool(route) and ends_run))
        if kind in FEEDS and not forced:
            queued = fill(batch)
        if ends_run:
            arrived = queued
    return out


def spec(prev):
    """spec_pick of a call after the fill `prev` (not part of step_route(): the anchors run with gru_spec = 0 either way)"""
    return int(prev is not None and prev < SPEC_BELOW)
