"""aggregate-posterior diagnostics, the part that needs no GPU: the entries are declared and bound, the argument rules of
VAE.log_q / VAE.latent_moments / VAE.posterior_stats, the float64 reference of tests/agg_ref.py against closed forms, and the
conditions on the inputs of tests/test_gpu_agg.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import agg_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_signature():
    from argsim_amd import lib
    src = open(os.path.join(ROOT, 'include', 'argsim_vae.h')).read()
    assert re.search(r'\bavae_agg_logq\s*\(', src) and re.search(r'\bavae_latent_moments\s*\(', src) and 'avae_agg_config' in src
    assert len(lib.SIGNATURES['avae_agg_logq'][1]) == 10 and len(lib.SIGNATURES['avae_latent_moments'][1]) == 6
    assert [f[0] for f in lib.AvaeAggConfig._fields_] == ['self_base', 'reserved'] and ctypes.sizeof(lib.AvaeAggConfig) == 16
    for word in ('self_base', 'agg_chunk', 'DIRECT', 'unbiased', 'logqx'):
        assert word in src, word
    l = lib.load()
    assert hasattr(l, 'avae_agg_logq') and hasattr(l, 'avae_latent_moments')


def test_one_row_bank_is_the_gaussian_density():
    rng = np.random.default_rng(3)
    for dim in (4, 20):
        mu, lv = rng.standard_normal((1, dim)), rng.uniform(-3, 1, (1, dim))
        z = rng.standard_normal((6, dim))
        want = (-0.5 * ((z - mu) ** 2 / np.exp(lv) + lv + np.log(2 * np.pi))).sum(1)
        assert np.abs(ar.logq64(z, mu, lv) - want).max() <= 1e-12 * np.abs(want).max()
        logq, logqx = ar.logq64(z[:1], mu, lv, self_base=0)
        assert abs(logq[0] - want[0]) <= 1e-12 * abs(want[0]) and abs(logqx[0] - want[0]) <= 1e-12 * abs(want[0])
    # a row of -inf terms gives -inf, a NaN stays a NaN
    assert np.isneginf(ar.logsumexp64(np.array([[-np.inf, -np.inf]]))[0]) and np.isnan(ar.logsumexp64(np.array([[0.0, np.nan]]))[0])


def test_reference_is_invariant_under_a_bank_permutation():
    for regime in ar.REGIMES:
        z, mu, lv = ar.case_inputs((33, 777, 20), regime)
        perm = np.random.default_rng(4).permutation(777)
        a, b = ar.logq64(z, mu, lv), ar.logq64(z, mu[perm], lv[perm])
        assert np.abs(a - b).max() <= 1e-11 * np.abs(a).max()


def test_case_list_holds_what_the_issue_names():
    for case in ((1, 1, 4), (5, 129, 4), (33, 777, 20), (65, 300, 128), (130, 4099, 128), (3, 127, 512), (7, 257, 1024)):
        assert case in ar.CASES
    ns, Ns = {c[0] % 128 for c in ar.CASES}, {c[1] % 64 for c in ar.CASES}
    assert {1, 127} <= ns and 129 in {c[0] for c in ar.CASES} and {1, 63} <= Ns and 65 in {c[1] for c in ar.CASES}
    for case in ar.CASES:
        for regime in ar.REGIMES:
            z, mu, lv = ar.case_inputs(case, regime)
            assert z.dtype == mu.dtype == lv.dtype == np.float32 and z.shape == (case[0], case[2]) and mu.shape == lv.shape == (case[1], case[2])
            assert all(np.isfinite(x).all() for x in ar.case_ref(case, regime))


def test_broad_cases_exercise_the_logsumexp():
    for case, (share_med, count_min) in ar.BROAD_SPREAD.items():
        share, count = ar.spread(case, 'broad')
        print(case, "max-term share %.3f .. %.3f, rows weighing > 1e-3 of the max: %.1f on average" % (share.min(), share.max(), count.mean()))
        assert np.median(share) <= share_med and count.mean() >= count_min, (case, float(np.median(share)), count.mean())
    share, count = ar.spread((7, 257, 1024), 'broad')          # one term holds the mass at dim 1024: that shape checks the pair term
    assert np.median(share) > 0.9


def test_no_moments_variance_sits_near_the_threshold():
    for N in ar.MOMENT_N:
        for dim in ar.MOMENT_DIM:
            var = ar.moments64(*ar.moment_inputs(N, dim))[1]
            near = (var > ar.AU_THRESHOLD / 2) & (var < ar.AU_THRESHOLD * 2)
            assert not near.any(), (N, dim, var[near])
            if N == 1:
                assert (var == 0).all()
            else:
                assert int((var > ar.AU_THRESHOLD).sum()) == dim // 2


def test_moments_reference_matches_numpy():
    mu, lv = ar.moment_inputs(257, 20)
    m = ar.moments64(mu, lv)
    assert np.allclose(m[1], np.var(mu.astype(np.float64), axis=0, ddof=1), rtol=1e-12, atol=0)
    assert np.allclose(m[0], mu.astype(np.float64).mean(0), rtol=1e-12, atol=1e-15)


def test_argument_checks():
    import torch
    from argsim_amd.model import VAE, _check_agg_args, _check_stats_args, latent_moments, log_q, posterior_stats
    z, mu, lv = np.zeros((3, 8), np.float32), np.zeros((5, 8), np.float32), np.zeros((5, 8), np.float32)
    assert _check_agg_args(z, mu, lv) == -1 and _check_agg_args(z, mu, lv, None) == -1
    assert _check_agg_args(z, mu, lv, True) == 0 and _check_agg_args(z, mu, lv, 2) == 2 and _check_agg_args(z, mu, lv, 0) == 0
    assert _check_agg_args(torch.zeros(3, 8), torch.zeros(5, 8), torch.zeros(5, 8), 1) == 1
    huge = np.broadcast_to(np.zeros((1, 8), np.float32), (1 << 31, 8))
    off = torch.zeros(5 * 8 + 1)[1:].view(5, 8)                # starts 4 bytes into its storage
    assert off.data_ptr() % 16
    bad = [dict(z=None), dict(mu=None), dict(lv=None), dict(z=[[0.0] * 8]),                                    # a missing array
           dict(z=np.zeros((0, 8), np.float32)),                                                               # n < 1
           dict(mu=np.zeros((0, 8), np.float32), lv=np.zeros((0, 8), np.float32)),                             # N < 1
           dict(mu=huge, lv=huge),                                                                             # N too large
           dict(z=np.zeros((3, 6), np.float32), mu=np.zeros((5, 6), np.float32), lv=np.zeros((5, 6), np.float32)),          # dim % 4
           dict(z=np.zeros((3, 1028), np.float32), mu=np.zeros((5, 1028), np.float32), lv=np.zeros((5, 1028), np.float32)), # dim > 1024
           dict(z=np.zeros((3, 12), np.float32)), dict(lv=np.zeros((4, 8), np.float32)),                       # mismatched shapes
           dict(z=z.astype(np.float64)), dict(lv=lv.astype(np.float16)), dict(z=np.zeros(8, np.float32)),
           dict(mu=off), dict(lv=off), dict(z=off[:3]),                                                        # a misaligned pointer
           dict(self_index=-1), dict(self_index=-2), dict(self_index=1.5),                                     # self_base < -1 and its like
           dict(self_index=3), dict(z=np.zeros((5, 8), np.float32), self_index=1)]                             # self_base + n > N
    for kw in bad:
        args = dict(z=z, mu=mu, lv=lv, self_index=None)
        args.update(kw)
        with pytest.raises(ValueError):
            _check_agg_args(**args)
    assert _check_stats_args(1, 0, 128, 0.01) == (1, 0, 128, 0.01)
    for kw in (dict(samples=0), dict(samples=1.5), dict(samples=True), dict(seed=-1), dict(batch=0), dict(au_threshold=-1.0), dict(au_threshold=float('nan'))):
        args = dict(samples=1, seed=0, batch=128, au_threshold=0.01)
        args.update(kw)
        with pytest.raises(ValueError):
            _check_stats_args(**args)
    for f in (latent_moments, log_q, posterior_stats, VAE.latent_moments, VAE.log_q, VAE.posterior_stats):
        assert callable(f)
