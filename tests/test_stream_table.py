"""No GPU: the case table of tests/test_gpu_stream.py (tests/stream_stall.py) against the signature table of argsim_amd/lib.py.  Every entry of
the C ABI that is not a debug hook has a case on the stalled stream or stands in EXEMPT with a reason -- a new entry point without either
fails HERE.  And the table against itself: every decoy is a valid input of the true input's shape and dtype that differs from it."""
import numpy as np

import step_history as SH
import step_routes as SR
import stream_stall as SS
from argsim_amd import lib

# what the issue behind the table names, entry by entry
WANTED = ('avae_set_tensor avae_get_tensor avae_forward_backward avae_adam_step avae_train_step avae_get_losses avae_eval avae_encode '
          'avae_decode_init avae_decode_step avae_decode_greedy avae_decode_sample avae_decode_sample_p avae_decode_beam avae_score avae_score_z '
          'avae_knn avae_agg_logq avae_latent_moments avae_probe_fit avae_probe_fit_l1 avae_probe_decision avae_ward avae_ward_cut avae_affinity '
          'avae_tsne avae_kmeans avae_gmm_fit avae_gmm_score avae_silhouette avae_dbscan avae_pca_fit avae_pca_transform avae_mmd avae_mmd_relabel '
          'avae_debug_train_ce avae_debug_present_ids avae_timing_collect').split()


def _covered():
    return {e for c in SS.CASES for e in c.entries}


def test_every_entry_has_a_case_or_a_reason():
    covered = _covered()
    assert covered <= set(lib.SIGNATURES), covered - set(lib.SIGNATURES)
    assert set(SS.EXEMPT) <= set(lib.SIGNATURES), set(SS.EXEMPT) - set(lib.SIGNATURES)
    assert not covered & set(SS.EXEMPT), covered & set(SS.EXEMPT)
    assert all(isinstance(r, str) and len(r) > 10 for r in SS.EXEMPT.values())
    public = {n for n in lib.SIGNATURES if n.startswith('avae_') and not n.startswith('avae_debug_')}
    missing = sorted(public - covered - set(SS.EXEMPT))
    assert not missing, 'entry points without a case on the stalled stream and without an exemption: %s' % missing
    assert set(WANTED) <= covered, sorted(set(WANTED) - covered)
    assert {e for e in covered if e.startswith('avae_debug_')} == set(SS.DEBUG_WITH_CASE)


def test_the_table_is_well_formed():
    ids = [c.id for c in SS.CASES]
    assert len(ids) == len(set(ids))
    for c in SS.CASES:
        assert c.entries and callable(c.inputs) and callable(c.outputs) and callable(c.call), c.id
        assert set(c.state_in) <= {'grads', 'adam_m', 'adam_v'} and set(c.state_out) <= {'params', 'grads', 'adam_m', 'adam_v'}, c.id
        assert c.model or not (c.state_in or c.state_out or c.warm), c.id
        assert not c.warm or not c.sync, c.id                   # (the warm step is there so that the stalled step does NOT synchronise)
        assert all(k.endswith('_chunk') or k.endswith('_form') or k == 'timing' for k, _ in c.options), c.id
    # both forms of the calls that have two
    for key in ('ward_form', 'pca_form'):
        assert {dict(c.options)[key] for c in SS.CASES if key in dict(c.options)} == {1, 2}, key
    # every latent-row call that has a part option runs with it set
    part = dict(avae_knn='knn_chunk', avae_agg_logq='agg_chunk', avae_probe_fit='probe_chunk', avae_probe_fit_l1='probe_chunk',
                avae_probe_decision='probe_chunk', avae_tsne='tsne_chunk', avae_kmeans='kmeans_chunk', avae_gmm_fit='gmm_chunk',
                avae_gmm_score='gmm_chunk', avae_silhouette='sil_chunk', avae_dbscan='dbscan_chunk', avae_pca_fit='pca_chunk',
                avae_pca_transform='pca_chunk', avae_mmd='mmd_chunk')
    for c in SS.CASES:
        for e in c.entries:
            if e in part:
                assert dict(c.options).get(part[e], 0) > 0, (c.id, part[e])
    # the model of the model calls is that of the step-history tests
    assert (SH.KW['dim_tgt'], SH.KW['dim_emb'], SH.KW['dim_rep'], SH.KW['rnn_layers']) == (256, 512, 32, 2) == (256, SR.D, SR.R, 2)
    assert SH.shape('b64') == (64, 6)
    assert SS.stall_ms(0.0) == SS.STALL_MIN_MS and SS.stall_ms(10.0) == SS.STALL_MAX_MS and SS.stall_ms(0.01) == 40.0


def test_every_decoy_is_a_valid_input_that_differs():
    V = SH.KW['dim_tgt']
    eos = SH.make('b64')[0]['eos']
    rng = np.random.default_rng(0)
    aux = dict(ref_grads=rng.standard_normal(4096).astype(np.float32))
    for c in SS.CASES:
        t, d = c.inputs('true', aux), c.inputs('decoy', aux)
        assert set(t) == set(d), c.id
        assert set(c.state_in) <= set(t), c.id
        for k in t:
            a, b = np.asarray(t[k]), np.asarray(d[k])
            assert a.shape == b.shape and a.dtype == b.dtype, (c.id, k)
            if a.dtype.kind == 'f':
                assert np.isfinite(a).all() and np.isfinite(b).all(), (c.id, k)
            if not (c.id == 'adam_step' and k in ('adam_m', 'adam_v')) and k != 'valid':
                assert a.tobytes() != b.tobytes(), (c.id, k, 'the decoy is the true input')
        for w in (t, d):
            for k in ('src', 'tgt', 'lead'):
                if k in w:
                    assert w[k].dtype == np.int32 and w[k].min() >= 0 and w[k].max() < V, (c.id, k)
            if 'src' in w:          # the same lengths: the same eos positions
                assert np.array_equal(w['src'] == eos, t['src'] == eos), c.id
            if 'label' in w:
                assert w['label'].min() >= -1 and w['label'].max() < SS.SIL_K, c.id
            if 'label_in' in w:
                assert w['label_in'].min() >= 0 and w['label_in'].max() < SS.GM_K, c.id
            if 'covars' in w:
                assert (w['covars'] > 0).all() and (w['weights'] > 0).all() and abs(w['weights'].sum() - 1) < 1e-12, c.id
            if 'adam_v' in w:
                assert (w['adam_v'] >= 0).all(), c.id
            if 'pair' in w:         # a valid merge list per group: a < b, every b merged away once, a still alive
                for g in range(3):
                    n = SS.GROUP_OFF[g + 1] - SS.GROUP_OFF[g]
                    p = w['pair'][SS.GROUP_OFF[g] - g:SS.GROUP_OFF[g + 1] - g - 1]
                    alive = set(range(n))
                    for a_, b_ in p:
                        assert 0 <= a_ < b_ < n and a_ in alive and b_ in alive, (c.id, g)
                        alive.discard(int(b_))
                    assert alive == {0}, (c.id, g)
            if 's' in w and c.id.startswith('probe'):
                assert w['s'].shape[1] == SS.N_ROWS and (np.abs(w['s']) > 0).all(), c.id
        outs = c.outputs(t)
        assert all(len(v) == 2 and np.dtype(v[1]).kind in 'fi' for v in outs.values()), c.id
        assert not set(outs) & set(t) or c.id in SS.INOUT, c.id
    # mmd: every relabeling keeps the sizes of the observed samples, inside the valid rows
    for which in ('true', 'decoy'):
        g = SS._mmd_groups(which)
        I = SS._mmd_inputs(which, None)
        bits = np.unpackbits(I['inA'].view(np.uint8), axis=-1, bitorder='little')[..., :SS.N_ROWS].astype(bool)
        assert bits.shape == (SS.MMD_G, 1 + SS.MMD_P, SS.N_ROWS)
        for i in range(SS.MMD_G):
            assert (bits[i, 0] == (g[i] == 0)).all()
            assert all(bits[i, p].sum() == bits[i, 0].sum() and not (bits[i, p] & (g[i] < 0)).any() for p in range(1 + SS.MMD_P))
