"""No GPU: the case table of the whole-step route tests (tests/step_routes.py) against the planners the launchers call, the per-block
gradient criterion (helpers.grad_blocks) against itself, and the host half of the route hook."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import step_routes as SR
from helpers import grad_blocks_bad, grad_blocks_ratio, grads_bad
from oracle import vae_torch as vt

TOL = 2e-4
BIG = 1 << 40           # floats of exchange scratch: the step's own always holds what a D = 512 launch needs (model.cpp layout)


# ------------------------------------------------------------------------------------------ the table against the planners
def test_case_ids_are_unique_and_every_listed_route_is_there():
    ids = [c.id for c in SR.CASES]
    assert len(ids) == len(set(ids))
    assert {c.batch for c in SR.CASES} == set(SR.BATCHES)
    for c in SR.CASES:
        assert [k for k, _ in c.options] == list(SR.OPTIONS), c.id                     # every case forces every option
        assert (c.opt('compact') == 2 or c.opt('bwd_rs') == 2) == (c.calls == 2), c.id  # only AUTO leaves a choice to the fill hint
        assert c.opt('gru_spec') in (0, 1), c.id


def test_fills_are_the_batches_own():
    for name, want in SR.FILL.items():
        assert abs(SR.fill(name) - want) < 1e-3, (name, SR.fill(name))
        assert SR.SPEC.get(name, 0) == int(want < 0.60) and 0.40 <= want < 0.92, name      # what "default" forces (model.cpp spec_pick, rs_pick, build_compact)


@pytest.mark.parametrize('c', SR.CASES, ids=lambda c: c.id)
def test_table_matches_the_planners(c):
    """every GRU plan of the table is what gru_plan answers for the launch shape gru_common fills (G = 0: gru_geometry's groups), and Bx what
    gru_team_batch answers"""
    from argsim_amd import lib
    l = lib.load()
    V, L, B, S, _ = SR.BATCHES[c.batch]
    w = c.want()
    assert w['Bx'] == l.avae_debug_team_batch(B), c.id
    assert w['top1'] == int(c.opt('enc_top1') and L >= 2), c.id
    assert (w['top_fwd'] is None) == (w['top_bwd'] is None) == (not w['top1']), c.id
    for kind, fwd, njobs, steps in SR.launches(c):
        bx = w['Bx'] if w['compact'][0 if kind[:3] != 'dec' else 1] else 0
        ints = [njobs, steps, B, SR.D, 3 * SR.D * (1 if kind[:3] == 'dec' else 2), SR.D * (1 if kind[:3] == 'dec' else 2), bx, 0, 0, 0, steps,
                c.opt('gru_item'), int(c.dtype == 'bf16'), int(w['bwd_rs'] != 0), BIG]
        out = (C.c_int64 * 10)()
        assert l.avae_debug_gru_plan((C.c_int64 * 15)(*ints), fwd, c.opt('persistent'), out) == 0
        got = (int(out[0]), int(out[1]), int(out[2]), int(out[5]), int(out[9]) if c.opt('gru_ring') else 0)      # (the hook plans with the ring on)
        assert got == w[kind], (c.id, kind, got, w[kind])


def test_bpipe_is_the_smallest_batch_with_both_launch_kinds_pipelined():
    """GruPlan::pipe read off the planner: at 512 rows the encoder pair is row-block pipelined and the one-job launches are not; at 1024 both"""
    from argsim_amd import lib
    l = lib.load()

    def pipe(njobs, B, S=4):
        ints = [njobs, S, B, SR.D, 3 * SR.D * njobs, SR.D * njobs, B, 0, 0, 0, S, 2, 0, 0, BIG]
        out = (C.c_int64 * 10)()
        assert l.avae_debug_gru_plan((C.c_int64 * 15)(*ints), 1, 1, out) == 0 and int(out[0]) == SR.TEAM
        return int(out[5])
    assert (pipe(2, 512), pipe(1, 512)) == (1, 0) and (pipe(2, 1024), pipe(1, 1024)) == (1, 1)
    assert SR.BATCHES['bpipe'][2] == 1024


# ------------------------------------------------------------------------------------------ the hook's host half
def test_route_hook_without_a_handle_and_its_decoding():
    from argsim_amd import lib
    from argsim_amd.model import ROUTE_GRU, ROUTE_INTS, route_dict
    l = lib.load()
    out = (C.c_int32 * ROUTE_INTS)()
    assert l.avae_debug_step_route(None, out) != 0
    assert ROUTE_INTS == 37
    v = [1, 0, 1, 0, 128, 1, 1] + [3, 2, 8, 0, 4] + [4, 2, 8, 0, 0] + [-1] * 10 + [3, 2, 4, 0, 4] + [4, 2, 4, 0, 0]
    r = route_dict(v)
    assert r == dict(table=(1, 0), compact=(1, 0), Bx=128, bwd_rs=1, top1=1, enc_fwd=(3, 2, 8, 0, 4), enc_bwd=(4, 2, 8, 0, 0), top_fwd=None,
                     top_bwd=None, dec_fwd=(3, 2, 4, 0, 4), dec_bwd=(4, 2, 4, 0, 0))
    assert set(r) == set(dict(SR.CASES[0].route)) and set(ROUTE_GRU) < set(r)
    with pytest.raises(ValueError):
        route_dict(v[:-1])


# ------------------------------------------------------------------------------------------ the criterion against itself
@functools.lru_cache(maxsize=None)
def _oracle(dtype):
    import torch
    cfg, P, src, tgt, keep, eps = SR.make('b20')
    return vt.loss_and_grads(P, cfg, src, tgt, SR.STEP, keep, eps, dtype={'f64': torch.float64, 'f32': torch.float32}[dtype])[1]


def test_the_float32_oracle_stays_far_inside_the_bound():
    """the reference's own error: the float32 run of the oracle against the float64 run, below 1 / 50 of the bound in every block"""
    g64, g32 = _oracle('f64'), _oracle('f32')
    worst = {k: grad_blocks_ratio(g32[k], g64[k], TOL) for k in g64}
    worst['embed/embedding rows'] = grad_blocks_ratio(g32['embed/embedding'], g64['embed/embedding'], TOL, rows=1)
    k = max(worst, key=worst.get)
    print('RATIO float32 oracle worst', k, worst[k])
    assert worst[k] < 1.0 / 50.0, (k, worst[k])
    assert not grads_bad(g32, g64, TOL)


def test_one_wrong_tile_of_one_gate_is_reported_with_its_block():
    """a 16-row block of one R scaled by 1.01 -- invisible to the relative L2 of the variable at 2e-4 -- is the one block reported"""
    g64 = _oracle('f64')
    k = 'decode/rnn/l1/R'
    for blk in (0, 37, g64[k].shape[0] // 16 - 1):
        got = g64[k].copy()
        got[16 * blk:16 * blk + 16] *= 1.01
        bad = grad_blocks_bad(got, g64[k], TOL)
        assert [b[0] for b in bad] == [blk], bad
    # the dead direction of the top encoder layer: exactly zero in the oracle, so anything else is reported
    z = 'encode/rnn2/bwd/R'
    assert not g64[z].any()
    got = g64[z].copy()
    assert not grad_blocks_bad(got, g64[z], TOL) and grad_blocks_ratio(got, g64[z], TOL) == 0.0
    got[40, 7] = 1e-30
    assert [b[0] for b in grad_blocks_bad(got, g64[z], TOL)] == [2] and grad_blocks_ratio(got, g64[z], TOL) == np.inf
    got[40, 7] = np.nan
    assert [b[0] for b in grad_blocks_bad(got, g64[z], TOL)] == [2]


def test_a_one_percent_error_is_reported_everywhere_where_the_fixture_criteria_pass_it():
    """Why the route tests exist.  The committed D = 512 fixtures pin two scalars per variable, the gradient norm and one Gaussian projection
    (tests/test_gpu_round2.py test_production_kernels_against_oracle_fixture, restated HERE alone): a random error of 1 % of a variable's norm
    moves the norm by 5e-5 of itself and the projection by 0.01 / sqrt(numel) of its bound's scale, so most variables pass; the block
    criterion reports every one of them."""
    g64 = _oracle('f64')
    rng = np.random.default_rng(5)
    live = [k for k in g64 if g64[k].any()]
    assert sorted(set(g64) - set(live)) == ['encode/rnn2/bwd/R']
    passed = []
    for k in live:
        g = g64[k]
        e = rng.standard_normal(g.shape)
        got = g + e * (0.01 * np.linalg.norm(g) / np.linalg.norm(e))
        assert grad_blocks_bad(got, g, TOL), k
        n = np.linalg.norm(g)
        p = np.random.default_rng(zlib.crc32(k.encode())).standard_normal(g.shape)
        if abs(np.linalg.norm(got) - n) <= TOL * n and abs(float((got * p).sum()) - float((g * p).sum())) <= TOL * n * np.linalg.norm(p):
            passed.append(k)
    print('fixture criteria pass %d of %d variables carrying a 1 %% error' % (len(passed), len(live)))
    assert len(passed) > len(live) // 2, passed
