"""No GPU: the table of the step-history tests (tests/step_history.py) against itself and against the planners the launchers call -- the
fills and their margins, the primers' hint, every expected GRU plan, and the gemm_plan branch a stale row expectation reaches."""
import ctypes as C

import numpy as np
import pytest

import step_history as SH
import step_routes as SR

BIG = 1 << 40           # floats of exchange scratch: the step's own always holds what a D = 512 launch needs (model.cpp layout)
THRESHOLDS = (SH.RS_BELOW, SH.SPEC_BELOW, SH.COMPACT_BELOW)


def _gru_plan(l, njobs, steps, B, bx, fwd, dtype, rs, dec):
    ints = [njobs, steps, B, SR.D, 3 * SR.D * (1 if dec else 2), SR.D * (1 if dec else 2), bx, 0, 0, 0, steps, 2, int(dtype == 'bf16'), rs, BIG]
    out = (C.c_int64 * 10)()
    assert l.avae_debug_gru_plan((C.c_int64 * 15)(*ints), fwd, 1, out) == 0
    return int(out[0]), int(out[1]), int(out[2]), int(out[5]), int(out[9])


def test_fills_are_the_batches_own_and_clear_of_every_threshold():
    assert set(SH.FILL) == set(SH.PROBES) | set(SH.PRIMERS) and not set(SH.PROBES) & set(SH.PRIMERS)
    for name, want in SH.FILL.items():
        f = SH.fill(name)
        assert abs(f - want) < 1e-3, (name, f)
        for th in THRESHOLDS:
            assert abs(f - th) >= SH.MARGIN, (name, f, th)
    # the bands the sequences are written for
    assert SH.fill('low') < SH.RS_BELOW - SH.MARGIN
    assert 0.43 <= SH.fill('mid') <= 0.57 and 0.43 <= SH.fill('b20') <= 0.57 and 0.43 <= SH.fill('b100v') <= 0.57
    assert SH.SPEC_BELOW + SH.MARGIN <= SH.fill('b64') <= SH.COMPACT_BELOW - SH.MARGIN
    assert SH.fill('b64full') == 1.0 and SH.fill('full') == 1.0 and SH.shape('full') != SH.shape('b64full')
    # b64 is the batch of the route tests, bit for bit, and every batch carries the same parameters
    for a, b in zip(SH.make('b64')[2:], SR.make('b64')[2:]):
        assert np.array_equal(a, b)
    for name in SH.FILL:
        assert all(np.array_equal(SH.make(name)[1][k], SH.make('b64')[1][k]) for k in SH.make('b64')[1]), name
    # low is larger than every 64-row probe in both directions of the workspace: source rows and target rows
    B, S = SH.shape('low')
    assert all(S > SH.shape(p)[1] for p in SH.PROBES if SH.shape(p)[0] == B)
    # every probe has both first layers table-fed (use_table: tokens >= V), the condition of the compact layout
    for p in SH.PROBES:
        B, S = SH.shape(p)
        assert B * S >= SH.KW['dim_tgt'], p


def test_every_primer_leaves_a_hint():
    """build_row_orders sends the hint with order 0, which exists where the two-direction encoder launch is a team plan: else a primer is inert"""
    from argsim_amd import lib
    l = lib.load()
    for name in SH.FILL:
        B, S = SH.shape(name)
        bx = l.avae_debug_team_batch(B)
        assert bx == SH.TEAMS[B][0] and bx % 16 == 0, name
        assert _gru_plan(l, 2, S, B, bx, 1, 'f32', 0, False)[0] == SR.TEAM, name


def test_sequences_cover_what_they_are_written_for():
    seen = {}
    for name, (dtype, calls) in SH.SEQUENCES.items():
        z = None
        for kind, batch, prev, route, _ in SH.steps(name):
            assert kind in SH.FEEDS + ('decode', 'knn'), (name, kind)
            if kind == 'encode':
                z = batch
            if kind in ('decode', 'knn'):
                assert z == batch, (name, kind, batch)       # (they take the rows the last encode returned)
            assert (route is not None) == (kind == 'fb' and batch in SH.PROBES), (name, kind, batch)
            if route is not None:
                seen.setdefault(name, []).append((batch, prev, route['compact'], route['bwd_rs'], SH.spec(prev)))
    r = lambda name: [(b, c, rs) for b, _, c, rs, _ in seen[name]]
    assert r('fresh') == [('b64', (0, 0), 0), ('b64', (1, 1), 0)]
    assert r('low-full') == [('b64full', (1, 1), 1), ('b64full', (0, 0), 0)] == r('low-full-bf16')
    assert r('full-ragged') == [('b64', (0, 0), 0)] == r('full-ragged-bf16')
    assert r('phantom') == [('b20', (1, 1), 1), ('b100v', (1, 1), 0), ('b20', (1, 1), 0)]
    assert r('mid-ragged') == [('b64', (1, 1), 0)] and r('mid-full') == [('b64full', (1, 1), 0)]
    assert [s[4] for s in seen['mid-ragged'] + seen['mid-full']] == [1, 1]      # gru_spec on, bwd_rs off
    assert r('chain-f32s')[0] == ('b64full', (1, 1), 1)
    # the epoch: at least eight steps, every probe, every primer, every other kind of call, another shape at every step
    ep = SH.steps('epoch')
    assert len(seen['epoch']) >= 8 and {b for b, *_ in seen['epoch']} == set(SH.PROBES)
    assert {b for k, b, *_ in ep if b in SH.PRIMERS} == set(SH.PRIMERS)
    assert {k for k, *_ in ep} == set(SH.FEEDS + ('decode', 'knn'))
    fbs = [SH.shape(b) for k, b, *_ in ep if k == 'fb']
    assert all(a != b for a, b in zip(fbs, fbs[1:]))
    assert {(c, rs) for _, _, c, rs, _ in seen['epoch']} == {((0, 0), 0), ((1, 1), 0), ((1, 1), 1)}
    # a phantom batch behind a full hint, a full batch behind a low one, a ragged batch behind a full one: all in the epoch too
    assert ('b100v', 1.0) in {(b, p) for b, p, *_ in seen['epoch']} and ('b64', 1.0) in {(b, p) for b, p, *_ in seen['epoch']}
    assert any(b == 'b64full' and p is not None and p < SH.RS_BELOW for b, p, *_ in seen['epoch'])


def _table(name):
    """(dtype, [(kind, batch, the fill the step plans from, route, rows)]) of a sequence of either table"""
    if name in SH.SEQUENCES:
        return SH.SEQUENCES[name][0], SH.steps(name)
    return SH.LATE_SEQUENCES[name][0], [(k, b, p, w, r) for k, b, _, p, w, r, _ in SH.late_steps(name)]


@pytest.mark.parametrize('name', list(SH.SEQUENCES) + list(SH.LATE_SEQUENCES))
def test_expected_routes_match_the_planners(name):
    """every GRU plan of every checked step is what gru_plan answers for the launch shape gru_common fills, and Bx what gru_team_batch answers"""
    from argsim_amd import lib
    l = lib.load()
    dtype, steps = _table(name)
    for kind, batch, prev, w, _ in steps:
        if w is None:
            continue
        B, S = SH.shape(batch)
        assert w['Bx'] == l.avae_debug_team_batch(B), (name, batch)
        assert w['table'] == (1, 1) and w['top1'] == 1 and w['compact'][0] == w['compact'][1], (name, batch)
        for key, fwd, njobs, steps in (('enc_fwd', 1, 2, S), ('enc_bwd', 0, 2, S), ('top_fwd', 1, 1, S), ('top_bwd', 0, 1, S),
                                       ('dec_fwd', 1, 1, S + 1), ('dec_bwd', 0, 1, S + 1)):
            dec = key[:3] == 'dec'
            bx = w['Bx'] if w['compact'][1 if dec else 0] else 0
            assert _gru_plan(l, njobs, steps, B, bx, fwd, dtype, w['bwd_rs'], dec) == w[key], (name, batch, key)


def _gemm_plan(l, M, N, K, dyn_kind, expect):
    # GemmShape in its field order: a_mc, b_nc, M, N, K, ldc, accumulate, split_k, thin, dyn_kind, dyn_expect, allow_atomic, rows_are_batch, pair,
    # wgrad, compute_dtype, skinny, dyn_split, dyn_thin -- the nn() product with .rows(count).atomic() and the options at their defaults
    s = np.array([[0, 1, M, N, K, N, 0, 0, -1, dyn_kind, expect, 1, 0, 0, 0, 0, 1, 1, 1]], dtype=np.int32)
    out = np.full((1, 15), -1, dtype=np.int32)
    assert l.avae_debug_gemm_plan(s.ctypes.data, 1, out.ctypes.data) == 0
    assert out[0, 0] == 1
    return dict(thin=int(out[0, 3]), split_k=int(out[0, 4]), zero=int(out[0, 6]), dyn=int(out[0, 7]))


def test_a_stale_row_expectation_reaches_the_k_split_of_the_decoder_dx_product():
    """b64full behind `low`: the input gradient of the decoder's top layer, dx (T x B, D) = dgi (T x B, 3 D) W over the compact rows
    (model.cpp backward: nn(...).rows(ntgt).atomic(), dyn_kind 1).  With the stale expectation int(fill(low) * T * B) gemm_plan takes the
    dyn_expect branch: K slices that add into the cleared first *count rows (kZeroDynRows = 2).  Behind its own hint of 1.0 the batch takes
    no compact layout, the product has no device-side count and runs as one launch without a clear: the branch is the stale hint's.
    (At 448 rows the split itself is the same for any expectation above zero -- 768 workgroups over at most 16 tiles, capped at K / 512 = 3
    slices; the five-fold error would move it only above 10 240 rows, eff_tiles > 320, which no batch the oracle can follow reaches.  What the
    stale hint changes HERE is that a full batch has a layout, a count and an expectation at all.)"""
    from argsim_amd import lib
    l = lib.load()
    B, S = SH.shape('b64full')
    M, N, K = (S + 1) * B, SR.D, 3 * SR.D
    stale = int(SH.fill('low') * (S + 1) * B)
    assert 0 < 5 * stale < M                                # five times too few rows
    p = _gemm_plan(l, M, N, K, 1, stale)
    assert p['split_k'] >= 2 and p['zero'] == 2 and p['dyn'] == 1, p
    q = _gemm_plan(l, M, N, K, 0, 0)                        # the second b64full of 'low-full': hint 1.0, no layout
    assert q['split_k'] == 1 and q['zero'] == 0 and q['dyn'] == 0, q
    # (nothing known about the count -- a forced layout, the anchors of the GPU test: not that branch either)
    u = _gemm_plan(l, M, N, K, 1, 0)
    assert u['zero'] != 2 and u['dyn'] == 1, u
    assert _gemm_plan(l, M, N, K, 1, M) == p                # (a right expectation behind a layout: the same plan at this size)
    # the encoder's top layer the same way: dx (Ss x B, 2 D) over K = 3 D (the one-step top layer: one direction's gate columns)
    p = _gemm_plan(l, S * B, 2 * SR.D, K, 1, int(SH.fill('low') * S * B))
    assert p['split_k'] >= 2 and p['zero'] == 2, p


def test_row_expectations_are_the_stale_fill_scaled_to_the_step():
    """what the GPU test compares VAE.row_expect() with: behind `low` a FULL 64 x 6 batch is expected to hold a fifth of its rows; behind its own
    hint it takes no layout and expects nothing; a phantom batch behind a full hint expects every row"""
    rows = {name: [(b, r) for k, b, p, w, r in SH.steps(name) if r is not None] for name in SH.SEQUENCES}
    assert rows['low-full'] == [('b64full', (73, 85, 85)), ('b64full', (0, 0, 0))]
    assert rows['fresh'] == [('b64', (0, 0, 0)), ('b64', (int(SH.fill('b64') * 384), int(SH.fill('b64') * 448), int(SH.fill('b64') * 448)))]
    assert rows['full-ragged'] == [('b64', (0, 0, 0))]
    assert ('b100v', (1100, 1200, 1200)) in rows['epoch']


def test_late_sequences_plan_from_what_had_arrived():
    """the "late" column: a call of a run of unsynchronised calls plans from the fill that had arrived BEFORE the run, not from the call
    in front of it; behind the run's synchronise the next call plans from the run's last feeding call"""
    assert not set(SH.LATE_SEQUENCES) & set(SH.SEQUENCES)
    col = {n: [(b, w, p, None if r is None else (r['compact'], r['bwd_rs']), rows, chk) for _, b, w, p, r, rows, chk in SH.late_steps(n)]
           for n in SH.LATE_SEQUENCES}
    low, b20 = SH.fill('low'), SH.fill('b20')
    for n in ('late-nothing', 'late-nothing-bf16'):
        # the primer leaves no hint, low's own is queued behind the stall: the FULL batch sees nothing -- no layout, no expectation
        assert col[n] == [('low', 'nohint', None, None, None, False), ('low', 'late', None, None, None, False),
                          ('b64full', 'late', None, ((0, 0), 0), (0, 0, 0), True)], col[n]
    assert SH.LATE_SEQUENCES['late-nothing'][0] == 'f32' and SH.LATE_SEQUENCES['late-nothing-bf16'][0] == 'bf16'
    B, S = SH.shape('b20')
    stale = (int(low * S * B), int(low * (S + 1) * B), int(low * (S + 1) * B))
    own = (int(b20 * S * B), int(b20 * (S + 1) * B), int(b20 * (S + 1) * B))
    assert col['late-stale'] == [('low', 'sync', None, None, None, False),
                                 ('b64full', 'late', low, ((1, 1), 1), (73, 85, 85), False),
                                 ('b20', 'late', low, ((1, 1), 1), stale, True),          # NOT from b64full's 1.0: that would be bwd_rs 0, every row
                                 ('b20', 'sync', b20, ((1, 1), 0), own, True)], col['late-stale']
    # the stale and the caught-up step differ in what the GPU test can see: the BPTT form and the row expectations
    assert stale != own and stale != (B * S, B * (S + 1), B * (S + 1))
    # what each late step WOULD take had the call in front of it been waited for is another route: the test can tell the two apart
    assert SH.expected_route('b64full', low, 'f32') != SH.expected_route('b64full', None, 'f32')
    assert SH.expected_route('b20', 1.0, 'f32') != SH.expected_route('b20', low, 'f32')
    # a run of late calls holds at most one checked step, its last; a 'nohint' call is a primer
    for n in SH.LATE_SEQUENCES:
        calls = SH.late_steps(n)
        for i, (k, b, w, p, r, rows, chk) in enumerate(calls):
            assert k == 'fb' and (w != 'nohint' or b in SH.PRIMERS), (n, i)
            if chk:
                assert w != 'late' or i + 1 == len(calls) or calls[i + 1][2] != 'late', (n, i)
