"""beam-search decoding without a GPU: the float64 reference of tests/beam_ref.py against exhaustive enumeration and the oracle's greedy
loop, the frozen-hypothesis and length rules on a hand-built example, the argument checks of VAE.beam, and a check of the INPUTS of
tests/test_gpu_beam.py (few near-ties at the selection boundary)."""
import numpy as np
import pytest

import beam_ref as br
from oracle import vae_numpy as vn


def test_a_beam_as_wide_as_the_tree_is_exhaustive_enumeration():
    """V = 32, 3 steps, width 1024 >= V^(steps - 1): nothing is pruned before the last step, so the final beam is the 1024 best of
    ALL 3-token paths (frozen after an eos), in the order of the contract"""
    cfg, P, z = br.params('tiny', 2.0)
    for r in (0, 3):
        res = br.search(P, cfg, z[r:r + 1], 3, 1024)
        seqs, cum = br.exhaustive(P, cfg, z[r], 3)
        assert len(seqs) > 1024 and (seqs[:, :-1] == cfg['eos']).any()          # paths through an eos are among them
        order = np.argsort(-cum, kind='stable')[:1024]
        assert res['seqs'].shape == (1, 1024, 3)
        assert np.array_equal(res['seqs'][0], seqs[order])
        assert np.allclose(res['cum_last'][0], cum[order], rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ['tiny', 'mid'])
def test_width_1_is_the_greedy_loop_up_to_each_rows_first_eos(name):
    cfg, P, z = br.params(name, 2.0)
    b = 8
    want = vn.decode_greedy(P, cfg, z[:b], steps=24)
    res = br.search(P, cfg, z[:b], 24, 1)
    ids, score, cum, ln = br.backtrack(res['lat_parent'], res['lat_token'], res['cum'].astype(np.float32), cfg['eos'])
    ended = 0
    for r in range(b):
        e = np.flatnonzero(ids[r, 0] == cfg['eos'])
        n = e[0] + 1 if len(e) else ids.shape[2]
        ended += bool(len(e))
        m = min(n, want.shape[1])
        assert np.array_equal(ids[r, 0, :m], want[r, :m]), r
        assert (ids[r, 0, n:] == cfg['eos']).all() and ln[r, 0] == n
        if n > want.shape[1]:          # the greedy result excludes the step at which every row emitted eos
            assert n == want.shape[1] + 1 and ids[r, 0, n - 1] == cfg['eos']
    assert ended >= 2


def test_frozen_hypotheses_and_lengths_on_a_hand_built_example():
    """two steps, V = 4, eos = 1, width 3.  Step 0 from one row; step 1: slot 0 is finished (it took eos) and offers itself alone"""
    eos = 1
    lp0 = np.log(np.array([[0.1, 0.5, 0.3, 0.1]]))                   # slots after step 0: eos (0.5), 2 (0.3), 0 (0.1; first of the tie with 3)
    p, k, sc, gap = br.select(lp0, np.ones((1, 4), bool), 3)
    assert p.tolist() == [0, 0, 0] and k.tolist() == [1, 2, 0] and np.isclose(gap, 0.0)
    cum = sc
    fin = k == eos
    lp1 = np.log(np.array([[0.7, 0.1, 0.1, 0.1], [0.25, 0.6, 0.1, 0.05], [0.4, 0.4, 0.1, 0.1]]))
    scores = cum[:, None] + lp1
    valid = np.ones((3, 4), bool)
    valid[0] = False; valid[0, eos] = True; scores[0, eos] = cum[0]  # the frozen one: cum unchanged, whatever its row says
    p, k, sc, gap = br.select(scores, valid, 3)
    # 0.5 (frozen) > 0.3 * 0.6 = 0.18 (2, eos) > 0.3 * 0.25 = 0.075 (2, 0) > 0.1 * 0.4 twice
    assert p.tolist() == [0, 1, 1] and k.tolist() == [1, 1, 0]
    assert np.allclose(np.exp(sc), [0.5, 0.18, 0.075]) and np.isclose(gap, np.log(0.075) - np.log(0.04))
    lat_parent = np.array([[[0, 0, 0]], [p]]); lat_token = np.array([[[1, 2, 0]], [k]])
    lat_cum = np.array([[cum], [sc]], np.float32)
    ids, score, c, ln = br.backtrack(lat_parent, lat_token, lat_cum, eos, 0.0)
    assert ids[0].tolist() == [[1, 1], [2, 1], [2, 0]] and ln[0].tolist() == [1, 2, 2]      # closing eos counted; unfinished: n
    assert np.array_equal(score, c)
    ids, score, c, ln = br.backtrack(lat_parent, lat_token, lat_cum, eos, 2.0)               # log 0.18 / 4 > log 0.075 / 4 > log 0.5 / 1
    assert ids[0].tolist() == [[2, 1], [2, 0], [1, 1]] and ln[0].tolist() == [2, 2, 1]
    assert np.array_equal(score[0], c[0] / (ln[0] * ln[0]).astype(np.float32)) and score.dtype == np.float32
    # equal scores: the lower parent first, then the lower token
    tie = np.zeros((2, 4))
    p, k, _, gap = br.select(tie, np.ones((2, 4), bool), 5)
    assert p.tolist() == [0, 0, 0, 0, 1] and k.tolist() == [0, 1, 2, 3, 0] and gap == 0.0


def test_beam_refuses_bad_arguments_before_any_device_work():
    from argsim_amd import model
    m = model.VAE.__new__(model.VAE)              # no device behind it: the checks must come first
    m.cfg = dict(dim_rep=8, dim_tgt=16)
    z = np.zeros((2, 8), np.float32)
    for kw in (dict(steps=0), dict(steps=(1 << 20) + 1), dict(steps=2.5), dict(width=0), dict(width=33), dict(width=1.5), dict(width=True),
               dict(length_alpha=-0.1), dict(length_alpha=float('nan')), dict(length_alpha=float('inf')), dict(width=17)):
        with pytest.raises(ValueError):
            m.beam(z, **kw)
        with pytest.raises(ValueError):
            model.beam(m, z, **kw)
    assert model._check_beam_args(np.int64(7), np.int32(32), 0) == (7, 32, 0.0)
    assert model._check_beam_args(1 << 20, 1, np.float32(0.5)) == (1 << 20, 1, 0.5)


@pytest.mark.parametrize("case", br.CASES, ids=lambda c: '%s-b%d-w%d-lean%g' % c)
def test_inputs_of_the_gpu_test_have_few_near_ties(case):
    """What is counted: the (sentence, step) selections of the REFERENCE'S OWN float64 search of the case (every case of
    tests/test_gpu_beam.py: tiny, mid and the production geometry are all affordable here) whose gap -- the width-th minus the
    (width + 1)-th candidate score -- is at most 1e-4 (t + 1), the ceiling the device tolerance may reach.  At most 1 % of the case's
    selections; the case must also do what it is there for (hypotheses that finish where eos_lean > 0)."""
    name, b, W, lean = case
    cfg, P, z = br.params(name, lean)
    res = br.search(P, cfg, z[:b], br.STEPS[name], W)
    gap = res['gap']
    near = int((gap <= 1e-4 * (np.arange(res['n']) + 1)[None, :]).sum())
    print("%s: %d steps, %d selections, %d near a tie, %.0f %% of the final slots finished" % (case, res['n'], gap.size, near, 100 * res['fin'].mean()))
    assert near <= 0.01 * gap.size, (near, gap.size)
    if lean:
        assert res['fin'].any()
