"""No GPU: the references of tests/ops_ref.py against independent formulations, the conditions that the inputs of
tests/test_gpu_ops.py have to meet (stated there, checked here), and the test hooks' presence in the built library."""
import ctypes

import numpy as np
import pytest

import ops_ref as R
import test_gpu_ops as G
from oracle import vae_numpy as vn


# ------------------------------------------------------------------------------------------ references against other formulations
@pytest.mark.parametrize('train', (0, 1))
@pytest.mark.parametrize('shape', ((1, 1, 1), (5, 3, 7), (100, 12, 12)), ids=str)
def test_prep_ids_matches_the_oracle(shape, train):
    """rows without holes (all eos, full, ragged prefixes): the oracle's own trim / mask / compaction says the same"""
    B, Ss, St = shape
    src, tgt, keep = G.prep_inputs(B, Ss, St, 0)
    for x in (src, tgt):          # close the holes: everything behind a row's first eos is eos
        for b in range(B):
            e = np.flatnonzero(x[b] == G.EOS)
            if e.size:
                x[b, e[0]:] = G.EOS
    ref = R.prep_ids(src, tgt, G.EOS, G.BOS, train, keep)
    cfg = dict(eos=G.EOS, bos=G.BOS)
    src_tm, _, len_src = vn.trim(src.T, G.EOS)
    tgt_tm, not_eos, len_tgt = vn.trim(tgt.T, G.EOS)
    S = tgt_tm.shape[0]
    lead, gold, msk = vn.prep_decoder_io(tgt_tm, not_eos, cfg, keep[:S] if train else None)
    assert np.array_equal(ref['lens_src'], len_src) and np.array_equal(ref['lens_tgt'], len_tgt)
    assert np.array_equal(ref['src_tm'][:src_tm.shape[0]], src_tm) and (ref['src_tm'][src_tm.shape[0]:] == G.EOS).all()
    assert np.array_equal(ref['lead'][:S + 1], lead) and np.array_equal(ref['gold'][:S + 1], gold)
    assert np.array_equal(ref['mask'][:S + 1], msk) and not ref['mask'][S + 1:].any()
    assert ref['ntok'] == int(msk.sum())
    # boolean_mask over the time-major array: the compact row of a kept position is its place among the kept ones
    vals = np.arange((St + 1) * B).reshape(St + 1, B)
    assert np.array_equal(ref['cidx'], vals[:S + 1][msk])
    assert np.array_equal(ref['rank'][:S + 1][msk], np.arange(ref['ntok'])) and (ref['rank'][~ref['mask']] == -1).all()


def test_prep_ids_rows_with_holes():
    """an eos between real ids masks its own successor position only; the length runs to the last real id"""
    tgt = np.int32([[5, 1, 6, 1], [1, 1, 1, 1], [4, 4, 4, 4]])
    ref = R.prep_ids(tgt[:, :2], tgt, 1, 2, 1, np.uint8([[1, 1, 0], [1, 1, 1], [0, 1, 1], [1, 1, 1]]))
    assert ref['lens_tgt'].tolist() == [3, 0, 4] and ref['lens_src'].tolist() == [1, 0, 2]
    assert ref['mask'].T.tolist() == [[1, 1, 0, 1, 0], [1, 0, 0, 0, 0], [1, 1, 1, 1, 1]]
    assert ref['lead'].T.tolist() == [[2, 5, 1, 0, 1], [2, 1, 1, 1, 1], [2, 0, 4, 4, 4]]
    assert ref['gold'].T.tolist() == [[5, 1, 6, 1, 1], [1, 1, 1, 1, 1], [4, 4, 4, 4, 1]]
    assert ref['cidx'].tolist() == [0, 1, 2, 3, 5, 8, 9, 11, 14] and ref['ntok'] == 9


@pytest.mark.parametrize('B,geom', G.ORDER_CASES)
def test_row_order_matches_stable_argsort(B, geom):
    T, cpj = geom
    rng = np.random.default_rng(B)
    for kind in range(3):
        for Breal in (B, B - 1, max(B - 28, 1), 1):
            lens, add, S = G.order_lens(rng, B, 12, kind), kind % 2, 12
            perm, slens, tot = R.row_order(lens, add, T, cpj, Breal, B, S)
            steps = np.where(np.arange(B) < Breal, np.clip(lens + add, 1, S), 1)
            order = np.argsort(-steps, kind='stable')
            slots = np.array([R.order_slot(r // 16, T, cpj) * 16 + r % 16 for r in range(B)])
            assert sorted(slots.tolist()) == list(range(B))
            assert np.array_equal(perm[slots], order) and np.array_equal(slens[slots], steps[order]) and tot == steps[:Breal].sum()
            # phantom rows sort behind every real row
            real_pos = np.flatnonzero(order < Breal)
            first_phantom = np.flatnonzero(order >= Breal)[:1]
            assert real_pos.size == Breal and (first_phantom.size == 0 or (steps[order][first_phantom[0]:] == 1).all())


def test_row_order_rejects_a_geometry_that_is_no_permutation():
    with pytest.raises(AssertionError):
        R.row_order(np.ones(32, np.int32), 0, 2, 2, 32, 32, 5)


@pytest.mark.parametrize('B,S,add', ((1, 1, 0), (7, 5, 1), (257, 40, 0), (600, 5, 1)))
def test_row_map_matches_cumsum(B, S, add):
    lens = np.random.default_rng(B).integers(0, S + 1, B)
    m, nact, count = R.row_map(lens, add, S, B)
    mask = np.arange(S)[:, None] < (lens + add)[None, :]
    want = np.where(mask, np.cumsum(mask.ravel()).reshape(S, B) - 1, -1)
    assert np.array_equal(m, want) and np.array_equal(nact, mask.sum(1)) and count == mask.sum()


@pytest.mark.parametrize('D', (32, 64, 512))
def test_g16_round_trip(D):
    x = np.arange(3 * D * 4, dtype=np.float32).reshape(3 * D, 4)
    g = R.g16_permute(x, D, True)
    assert np.array_equal(R.g16_permute(g, D, False), x) and not np.array_equal(g, x)
    assert np.array_equal(g[48 + 3 * 5 + 2], x[2 * D + 16 + 5])      # G16 row ht 1, unit 5, gate n


def test_id_groups_matches_unique():
    rng = np.random.default_rng(0)
    ids = rng.integers(-5, 60, 400)
    rank, uid, nuniq = R.id_groups(ids, 50)
    u = np.unique(np.clip(ids, 0, 49))
    assert np.array_equal(uid, u) and nuniq == u.size and np.array_equal(rank[u], np.arange(u.size)) and (rank >= 0).sum() == u.size


def test_adam_reference_is_the_tf_formula():
    (m, v, p), _ = R.adam_tf([1.0], [0.5], [0.25], [0.04], 0.5, 0.5, 0.75, 0.0)
    assert np.allclose([m[0], v[0], p[0]], [0.375, 0.0925, 1.0 - 0.5 * 0.375 / np.sqrt(0.0925)])


# ------------------------------------------------------------------------------------------ conditions of the GPU tests' inputs
@pytest.mark.parametrize('V,n', [(c[1], c[2] + c[3]) for c in G.SCATTER_CASES] + [(c[1], c[2]) for c in G.GROUP_SUM_CASES])
def test_ladder_counts_are_exact(V, n):
    ids, counts = R.ladder_ids(np.random.default_rng(1), V, n)
    assert ids.size == n and counts.sum() == n
    assert np.array_equal(np.bincount(R.clamp_ids(ids, V), minlength=V), counts)
    assert ids.min() < 0 or counts[0] == 0 or n < 2
    fits = [c for c, tot in zip(R.LADDER, np.cumsum(R.LADDER)) if tot <= n]
    assert all(c in counts for c in fits)
    if n >= sum(R.LADDER):
        assert ids.max() >= V and set(R.LADDER) <= set(counts.tolist())


def test_class_a_sums_are_exact_in_fp32():
    """integers of at most INT_MAX_ABS times 2^-3: the largest partial sum any order can form stays below 2^24 units"""
    for terms in (G.SCATTER_MAX_TERMS, G.COLSUM_MAX_TERMS, G.FINALIZE_MAX_TERMS + 7, max(G.FINALIZE_NKS) * 2, 3):
        assert R.int_sum_is_exact(terms)
    x = R.int_valued(np.random.default_rng(0), 10000)
    assert np.array_equal(x * 8, np.round(x * 8)) and np.abs(x * 8).max() <= R.INT_MAX_ABS
    loss, kld = G.finalize_inputs(20000, 4096, 0.02, 'a')
    assert np.abs(loss * 8).max() <= R.INT_MAX_ABS and np.abs(kld * 8).max() <= R.INT_MAX_ABS + 1 and kld.min() > 0.02


@pytest.mark.parametrize('free_bits', (0.0, 0.02))
def test_no_element_sits_on_the_free_bits_gate(free_bits):
    for seed in (0, 1):
        mu, lv = R.latent_inputs(np.random.default_rng(seed), 37 * 70, free_bits)
        assert np.count_nonzero(~R.gate_clear(mu, lv, free_bits)) == 0
    for n in G.FINALIZE_NS:
        for nk in G.FINALIZE_NKS:
            mu, lv = R.latent_inputs(np.random.default_rng(n + nk), nk, free_bits)
            assert np.count_nonzero(~R.gate_clear(mu, lv, free_bits)) == 0
            loss, kld = G.finalize_inputs(n, nk, free_bits, 'b')
            k = kld.astype(np.float64)
            assert np.count_nonzero(np.abs(k - float(np.float32(free_bits))) <= R.GATE_MARGIN / 2 * (1 + k)) == 0


# ------------------------------------------------------------------------------------------ the hooks
def test_hooks_are_declared_and_exported():
    from argsim_amd import lib
    lib.build()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for s in ('avae_debug_op', 'avae_debug_op_layout'):
        assert s in lib.SIGNATURES and hasattr(cdll, s), s


def test_layout_hook_reports_the_scratch_views():
    from argsim_amd import lib
    l = lib.load()
    o = (ctypes.c_int64 * 6)()
    for n, V in ((1, 1), (1025, 1000), (5000, 12288)):
        assert l.avae_debug_op_layout(n, V, o) == 0
        scatter, groups, rank, uid, count, ok = list(o)
        assert ok == 1 and scatter <= rank < uid < count < groups and uid - rank >= V and count - uid >= V
    assert l.avae_debug_op_layout(8, 12289, o) == 0 and o[5] == 0
    assert l.avae_debug_op_layout(-1, 8, o) != 0
