"""importance-weighted sentence likelihood without a GPU: the float64 reference of tests/score_ref.py checked against itself and the
oracle, the C ABI (header, exports, ctypes table), the argument rules and the training driver's flag."""
import ctypes
import os
import re

import numpy as np
import pytest

import score_ref
from helpers import make_case
from oracle import vae_numpy as vn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(name, k=3):
    cfg, P, ids = make_case(name)[:3]
    B, R = len(ids), cfg['dim_rep']
    e = np.random.default_rng(3).standard_normal((k, B, R))
    return cfg, P, ids, e


@pytest.mark.parametrize("name", ['tiny', 'mid'])
def test_bound_is_at_least_the_elbo_estimate(name):
    cfg, P, ids, e = _case(name)
    o = score_ref.score(P, cfg, ids, ids, e)
    assert o['logw'].shape == e.shape[:2] and o['bound'].shape == (len(ids),)
    assert (o['bound'] >= o['logw'].mean(0) - 1e-12).all()          # Jensen
    assert (o['bound'] <= o['logw'].max(0) + 1e-12).all()
    assert np.isfinite(o['bound']).all() and (o['logpx'] < 0).all()


def test_first_draws_of_k_are_the_draws_of_a_smaller_k_and_rows_are_independent():
    a, b = score_ref.eps_all(7, 8, 5, 16), score_ref.eps_all(7, 4, 5, 16)
    assert np.array_equal(a[:4], b)
    assert np.array_equal(score_ref.eps_all(7, 4, 8, 16)[:, 3], b[:, 3])
    assert not np.array_equal(score_ref.eps_all(8, 4, 5, 16), b)
    big = score_ref.eps_all(1, 64, 16, 64)
    assert np.isfinite(big).all() and abs(big.mean()) < 0.02 and abs(big.std() - 1.0) < 0.02 and np.abs(big).max() <= 5.9


@pytest.mark.parametrize("name", ['tiny', 'mid'])
def test_one_draw_at_eps_zero_is_the_row_sum_of_the_valid_forward(name):
    cfg, P, ids, _ = _case(name)
    B, R = len(ids), cfg['dim_rep']
    o = score_ref.score(P, cfg, ids, ids, np.zeros((1, B, R)))
    f = vn.forward(P, cfg, ids, ids, mode='valid')
    ce = np.zeros(f['msk_tgt'].shape)
    ce[f['msk_tgt']] = f['loss_gen_samp']                               # scattered back: time-major boolean_mask order
    assert np.allclose(o['logpx'][0], -ce.sum(0), rtol=1e-12, atol=1e-12)
    assert np.array_equal(o['ntok'], f['msk_tgt'].sum(0))
    assert np.array_equal(o['ntok'], (ids != cfg['eos']).sum(1) + 1)
    # eps = 0: z = mu, the latent term is 1/2 sum (mu^2 - lv)
    assert np.allclose(o['logw'][0], o['logpx'][0] - 0.5 * (o['mu'] ** 2 - o['lv']).sum(1), rtol=1e-12)
    assert np.allclose(o['bound'], o['logw'][0], rtol=1e-12)


def test_a_row_of_all_eos_scores_one_position():
    cfg, P, ids, e = _case('tiny')
    tgt = ids.copy()
    tgt[2] = cfg['eos']
    o = score_ref.score(P, cfg, ids, tgt, e)
    assert o['ntok'][2] == 1 and np.isfinite(o['bound']).all()


def test_log_mean_exp_survives_weights_whose_exponential_underflows():
    lw = np.array([[-600.0, -900.0], [-601.0, -850.0]])
    assert np.allclose(score_ref.log_mean_exp(lw), [-600.0 + np.log((1 + np.exp(-1.0)) / 2), -850.0 + np.log((1 + np.exp(-50.0)) / 2)])


# ------------------------------------------------------------------------------------------ ABI
def _header():
    src = open(os.path.join(ROOT, 'include', 'argsim_vae.h')).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_header_declares_both_entries_and_the_config():
    h = _header()
    assert re.search(r'\bint\s+avae_score\s*\(', h) and re.search(r'\bint\s+avae_score_z\s*\(', h)
    assert re.search(r'typedef struct avae_score_config\s*\{\s*int32_t k;\s*uint64_t seed;\s*\}', h)


def test_library_exports_and_signatures_cover_them():
    from argsim_amd import lib
    lib.build()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for s in ('avae_score', 'avae_score_z'):
        assert hasattr(cdll, s), s
        assert s in lib.SIGNATURES
    assert len(lib.SIGNATURES['avae_score'][1]) == 13 and len(lib.SIGNATURES['avae_score_z'][1]) == 7
    assert ctypes.sizeof(lib.AvaeScoreConfig) == 16
    lib.load()


def test_score_arguments_are_checked_before_the_device():
    from argsim_amd.model import _check_score_args
    assert _check_score_args(1, 0) == (1, 0) and _check_score_args(1 << 20, (1 << 64) - 1) == (1 << 20, (1 << 64) - 1)
    assert _check_score_args(np.int64(4), np.int64(9)) == (4, 9)
    for bad in ((0, 0), ((1 << 20) + 1, 0), (True, 0), (2.5, 0), (4, -1), (4, True), (4, 1 << 64)):
        with pytest.raises(ValueError):
            _check_score_args(*bad)


def test_training_driver_takes_the_iw_flag():
    from argsim_amd.train import parse_args
    assert parse_args([]).iw == 0
    assert parse_args(['--iw', '8']).iw == 8
    for bad in ('-1', str((1 << 20) + 1)):
        with pytest.raises(SystemExit):
            parse_args(['--iw', bad])


class _ScoreStub:
    """VAE.score on the host: values that depend only on the ids"""
    def score(self, src, tgt=None, k=1, seed=0, eps=None, return_parts=False):
        ntok = ((src != 1).sum(1) + 1).astype(np.int32)
        r = np.random.default_rng(int(src.sum()) + k + seed)
        return dict(bound=(-3.0 * ntok * (1 + r.random(len(src)))).astype(np.float32), ntok=ntok)


def test_summ_iw_is_the_sums_formed_by_hand():
    from argsim_amd.train import summ_iw
    rng = np.random.default_rng(2)
    valid = np.ones((23, 9), np.int32)
    for b in range(23):
        n = int(rng.integers(1, 10)); valid[b, :n] = rng.integers(3, 50, n)
    nll, ppl = summ_iw(_ScoreStub(), valid, 5, 4, 7)
    parts = [_ScoreStub().score(valid[i:i + 5], None, 4, 7) for i in range(0, 23, 5)]
    b = sum(float(p['bound'].astype(np.float64).sum()) for p in parts)
    n = sum(int(p['ntok'].sum()) for p in parts)
    assert nll == pytest.approx(-b / 23, rel=1e-12) and ppl == pytest.approx(np.exp(-b / n), rel=1e-12)
