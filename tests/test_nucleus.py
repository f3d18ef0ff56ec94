"""nucleus sampling without a GPU: the ABI of avae_decode_sample_p, the argument rule, the float64 reference of tests/nucleus_ref.py on
hand-made rows, the distribution of its draws, and the conditions that tests/test_gpu_nucleus.py puts on its own inputs (checked
on the reference alone: the crafted rows are decidable, the model cases have few near-ties)."""
import ctypes
import os
import re

import numpy as np
import pytest

import nucleus_ref as nr
import sampling_ref as sr
import test_gpu_nucleus as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_exports_and_ctypes_agree_on_the_two_entries_and_the_struct():
    from argsim_amd import lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'argsim_vae.h')).read(), flags=re.S)
    assert re.search(r'typedef struct avae_sample_p_config \{ float temperature; int32_t top_k; uint64_t seed; float top_p; int32_t reserved; \}', src)
    for name in ('avae_decode_sample_p', 'avae_debug_sample_rows_p'):
        assert re.search(r'\b%s\s*\(' % name, src) and name in lib.SIGNATURES, name
    S = lib.AvaeSamplePConfig
    assert ctypes.sizeof(S) == 24 and S.top_p.offset == 16 and S.reserved.offset == 20 and S.seed.offset == 8
    assert [f[0] for f in S._fields_[:3]] == [f[0] for f in lib.AvaeSampleConfig._fields_]
    lib.build()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(cdll, 'avae_decode_sample_p') and hasattr(cdll, 'avae_debug_sample_rows_p')
    assert len(lib.SIGNATURES['avae_decode_sample_p'][1]) == 9 and len(lib.SIGNATURES['avae_debug_sample_rows_p'][1]) == 10


def test_check_top_p_and_the_public_signatures():
    from argsim_amd import model
    for ok in (0, 0.9, 1, 2.5):
        assert model._check_top_p(ok) == float(ok)
    for bad in (-0.1, float('nan'), True):
        with pytest.raises(ValueError):
            model._check_top_p(bad)
    m = model.VAE.__new__(model.VAE)              # no device behind it: the checks must come first
    m.cfg = dict(dim_rep=8)
    z = np.zeros((2, 8), np.float32)
    for bad in (-0.1, float('nan')):
        with pytest.raises(ValueError):
            m.sample(z, top_p=bad)
        with pytest.raises(ValueError):
            m.generate(2, top_p=bad)
        with pytest.raises(ValueError):
            model.sample(m, z, top_p=bad)
    assert model._check_sample_args(7, 0, 3, 5) == (7, 3, 5)


ROW = np.array([0.5, 2.0, 2.0, -1.0, 1.0, 0.0, -3.0, 1.5])


@pytest.mark.parametrize("T,k,p", [(1.0, 0, 0.0), (1.0, 3, 1.0), (0.7, 0, 2.5), (0.0, 0, 0.5), (0.7, 1, 0.5)])
def test_with_the_nucleus_off_the_reference_is_sampling_refs_position(T, k, p):
    a, b = nr.position(ROW, T, k, p, 5, 1, 2), sr.position(ROW, T, k, 5, 1, 2)
    assert a['nkept'] == -1 and a['nucleus'] is None
    for key, v in b.items():
        assert np.array_equal(np.asarray(a[key]), np.asarray(v)), key


def test_kept_set_grows_with_top_p_holds_the_first_maximum_and_whole_tie_groups():
    rng = np.random.default_rng(0)
    for trial in range(20):
        l = np.round(2.0 * rng.standard_normal(40), 1)             # rounded: ties everywhere
        T, k = (1.0, 0) if trial % 2 else (0.7, 12)
        prev = None
        for p in (0.05, 0.3, 0.5, 0.8, 0.9, 0.99, 1.0 - 2.0 ** -24):
            q = nr.position(l, T, k, p, trial, 0, 0)
            kept, nu = q['kept'], q['nucleus']
            assert kept[int(np.argmax(l))] and q['nkept'] == kept.sum() >= 1
            assert not (np.isin(l[~kept & q['k0']], l[kept])).any()                         # no tie group is split
            assert kept[q['token']] and np.isclose(np.exp(q['logp'][kept]).sum(), 1.0)
            assert nu['cum_j'] >= p > nu['cum_jm1']                                          # the smallest such prefix
            if prev is not None:
                assert (prev <= kept).all()
            prev = kept
        assert (q['kept'] <= sr.kept_set(l, k)[0]).all()


def test_a_dominant_token_is_kept_alone_and_ties_at_the_threshold_are_all_kept():
    l = np.array([0.0, 5.0, 0.1, -0.2, 0.3])
    q = nr.position(l, 1.0, 0, 0.9, 1, 0, 0)
    assert q['kept'].tolist() == [False, True, False, False, False] and q['token'] == 1 and q['logp'][1] == 0.0
    l = np.array([1.0, 3.0, 1.0, 1.0, -2.0, 3.0])                  # two maxima hold 0.79 of the mass: 0.9 needs the three 1.0 too
    q = nr.position(l, 1.0, 0, 0.9, 1, 0, 0)
    assert q['kept'].tolist() == [True, True, True, True, False, True] and q['nkept'] == 5
    assert nr.position(l, 1.0, 0, 0.75, 1, 0, 0)['kept'].tolist() == [False, True, False, False, False, True]


def test_nan_is_absent_plus_inf_is_kept_alone_and_a_row_of_minus_inf_has_no_token():
    l = np.array([np.nan, 1.0, 0.5, np.nan, -np.inf, 0.0])
    q = nr.position(l, 1.0, 0, 0.99, 1, 0, 0)
    assert not q['kept'][[0, 3]].any() and q['kept'][[1, 2, 5]].all() and q['token'] in (1, 2, 5)
    q = nr.position(l, 1.0, 2, 0.99, 1, 0, 0)
    assert q['kept'].tolist() == [False, True, True, False, False, False]
    l = np.array([0.0, np.inf, 3.0, np.nan])
    q = nr.position(l, 0.7, 0, 0.9, 1, 0, 0)
    assert q['kept'].tolist() == [False, True, False, False] and q['token'] == 1 and q['logp'][1] == 0.0
    q = nr.position(np.full(6, -np.inf), 1.0, 0, 0.9, 1, 0, 0)
    assert q['token'] == 0 and np.isnan(q['logp']).all() and q['nkept'] == 6
    j = nr.judge(q, 6, 0)
    assert j['viol'] == 0.0 and j['same'] and np.isnan(j['logp'])


def test_judge_measures_a_foreign_set_by_its_violation():
    l = np.array([3.0, 2.0, 2.0, 1.0, 0.0, -1.0])
    q = nr.position(l, 1.0, 0, 0.9, 1, 0, 0)
    cum = q['nucleus']['cum']
    assert q['nkept'] == 4 and nr.judge(q, 4, 0)['viol'] == 0.0 and nr.judge(q, 4, 0)['same']      # cum = .515, .895, .965, ...
    assert nr.judge(q, 2, 0)['viol'] == np.inf                                              # splits the tie group
    assert np.isclose(nr.judge(q, 1, 0)['viol'], 0.9 - cum[0]) and np.isclose(nr.judge(q, 3, 0)['viol'], 0.9 - cum[1])
    assert np.isclose(nr.judge(q, 5, 0)['viol'], cum[2] - 0.9)
    j = nr.judge(q, 3, 2)
    assert np.isclose(j['logp'], 2.0 - np.log(np.exp([3.0, 2.0, 2.0]).sum())) and not j['same']
    assert nr.judge(q, 3, 3)['deficit'] == np.inf                                           # token 3 is outside that set


N_SEEDS = 20000


def test_draws_follow_the_renormalised_nucleus_distribution():
    """one fixed V = 16 row, seeds 0..19999 (a fixed list: deterministic).  Every count is a binomial(N, q_v): with the normal
    bound |count - N q| <= 4.5 sqrt(N q (1 - q)) + 1 a single cell fails a correct generator with probability < 7e-6 (under 1e-4 over
    the kept cells); nothing outside the nucleus is ever drawn."""
    l = np.array([2.0, 1.5, 1.5, 1.0, 0.7, 0.4, 0.0, -0.3, -0.5, -1.0, -1.2, -2.0, -2.5, -3.0, -4.0, -6.0])[np.random.default_rng(1).permutation(16)]
    T, p = 0.8, 0.9
    q0 = nr.position(l, T, 0, p, 0, 0, 0)
    kept = q0['kept']
    assert 1 < kept.sum() < 16
    prob = np.where(kept, np.exp(q0['logp']), 0.0)
    assert np.isclose(prob.sum(), 1.0)
    counts = np.zeros(16)
    x = np.where(kept, l / T, -np.inf)
    for seed in range(N_SEEDS):
        counts[int(np.argmax(x + sr.gumbel(seed, 0, 0, 16)))] += 1
    assert nr.position(l, T, 0, p, 77, 0, 0)['token'] == int(np.argmax(x + sr.gumbel(77, 0, 0, 16)))      # (the loop above IS position's draw)
    assert counts[~kept].sum() == 0
    bound = 4.5 * np.sqrt(N_SEEDS * prob * (1 - prob)) + 1
    print("largest |count - N q| / bound: %.3f" % (np.abs(counts - N_SEEDS * prob)[kept] / bound[kept]).max())
    assert (np.abs(counts - N_SEEDS * prob) <= bound).all(), (counts, N_SEEDS * prob)


@pytest.mark.parametrize("V", G.CRAFT_V)
def test_crafted_gpu_rows_are_decidable(V):
    """every crafted row of tests/test_gpu_nucleus.py: boundary margin >= 1e-3 and top-2 score margin >= 1e-3 at every config"""
    x, lead = G.crafted(V)
    assert lead[7] == 1 and np.isinf(x[5]).all() and np.isnan(x[3]).any() and np.isinf(x[3]).any() and (x[4] == np.inf).sum() == 1
    for T, k, p in G.CRAFT_CFG:
        ref = G.crafted_ref(V, T, k, p)
        for r, q in ref.items():
            if r == 5 or r not in G.CRAFT_ROWS.get((k, p), G.LIVE):
                continue
            assert G.crafted_margin(q) >= 1e-3, (V, T, k, p, G.ROW_NAMES[r], G.crafted_margin(q))
            assert q['margin'] >= 1e-3 or q['nkept'] == 1, (V, T, k, p, G.ROW_NAMES[r], q['margin'])
        if k == 0 and p == 0.9:
            t = ref[2]
            assert t['nucleus']['sizes'][t['nucleus']['j']] == 6 and t['nkept'] == 6         # the tie group straddles the boundary and is kept whole
            assert ref[6]['nkept'] == 1 and ref[4]['nkept'] == 1
        if p > 0.99:
            assert k == 0 or [ref[r]['nkept'] for r in (0, 1, 2, 3, 4)] == [8, 8, 8, 8, 1]
            assert ref[8]['nkept'] == 6 and ref[8]['nucleus']['cum_j'] == 1.0                # top_k 8 holds two weightless tokens more: not kept


@pytest.mark.parametrize("name", ['tiny', 'mid', 'prod'])
def test_model_cases_have_few_near_ties_in_the_references_own_run(name):
    """at most 2 % of the positions of every model case of tests/test_gpu_nucleus.py have a top-2 score margin <= 1e-4 (a row's draws
    and history do not depend on the rows after it: the b-row case is the first b rows of the largest run)"""
    cfg, P, z = G.params(name)
    bs = sorted({g[1] for g in G.GEOMS if g[0] == name})
    for T, k, p in G.CONFIGS:
        res = nr.sample(P, cfg, z[:bs[-1]], G.STEPS[name], T, k, G.f32(p), seed=1)
        for b in bs:
            live = res['live'][:b]
            close = live & (res['margin'][:b] <= 1e-4)
            print("%s b %d %s: %d of %d positions with a top-2 margin <= 1e-4; min boundary margin %.2e" %
                  (name, b, (T, k, p), close.sum(), live.sum(), res['bmargin'][:b][live].min()))
            assert close.sum() <= 0.02 * live.sum(), (name, b, T, k, p)
