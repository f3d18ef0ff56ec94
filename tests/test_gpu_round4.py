"""GPU tests added in round 4: the reduce-scatter form of the BPTT team kernels (gru_rs.hip) against the other form and the oracle
fixtures, the train-forward per-token cross-entropy against the fixtures of the big configurations, bit-reproducible loss scalars."""
import os

import numpy as np
import pytest

from helpers import big_extras, make_case, rel_l2

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ('dim_tgt', 'dim_emb', 'dim_rep', 'rnn_layers', 'accelerate', 'learn_rate', 'bos', 'eos')


def _vae(cfg, P, mode='train', **kw):
    from argsim_amd.model import VAE
    m = VAE(mode, init=False, **{k: cfg[k] for k in KEYS}, **kw)
    m.set_params(P)
    return m


def _gold(name):
    with np.load(os.path.join(HERE, 'golden', 'oracle_%s.npz' % name), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _probe(name, shape):
    import zlib
    return np.random.default_rng(zlib.crc32(name.encode())).standard_normal(shape)


# ------------------------------------------------------------------------------------------ reduce-scatter BPTT (gru_rs.hip)
@pytest.mark.parametrize("name", ['prod64', 'prod512', 'headline'])
def test_reduce_scatter_bptt_against_the_oracle_fixture(name):
    """model.py:15,120-121,160 (CudnnGRU BPTT).  bwd_rs = 1 forces the reduce-scatter form of the backward team kernels (a workgroup
    multiplies its own 48 gate-gradient columns by its resident slice of R; the 32 partial dH rows are summed on the consumer's
    side through a two-slot ring tagged in the last mantissa bit) at B = 64 (4-team encoder launches of one row block, ragged),
    B = 512 (row-block-pipelined instantiations) and the bench batch (B = 256 FULL: 4-team encoder, 2-team decoder launches):
    every gradient against the float64 oracle's fixture -- norm and one fixed projection per variable -- at the fp32 tolerances."""
    gold = _gold(name)
    cfg, P, ids, keep, eps = make_case(name)
    extra = big_extras(name) if name != 'prod64' else {}
    m = _vae(cfg, P, **extra)
    m.step = 20000
    m.set_option('bwd_rs', 1)
    m.forward_backward(ids, ids, keep_mask=keep, eps=eps)
    lo = m.losses()[2]
    assert abs(lo - float(gold['loss'])) <= 2e-5 * abs(float(gold['loss']))
    for k, g in m.get_grads().items():
        g = g.astype(np.float64)
        n = float(gold['gnorm/' + k])
        assert abs(np.linalg.norm(g) - n) <= 2e-4 * n, (name, k)
        p = _probe(k, g.shape)
        assert abs(float((g * p).sum()) - float(gold['gdot/' + k])) <= 2e-4 * n * np.linalg.norm(p), (name, k)
    m.close()


@pytest.mark.parametrize("B,S,ragged", [(256, 20, True), (100, 40, True), (1024, 6, False), (64, 3, True)])
def test_reduce_scatter_bptt_equals_the_other_form(B, S, ragged):
    """The two decompositions of the backward recurrence compute the same sums in another order: every gradient agrees per
    variable to fp32 rounding (the tag bit moves a partial sum by at most one unit in the last place), the forward is untouched
    (same z and losses, bit for bit), and a gradient that is exactly zero in one form -- dR of the top encoder layer's dead
    direction (enc_top1 = 0: all S steps run) -- is exactly zero in the other: a cleared tag bit leaves an exact zero an exact zero.
    Shapes: ragged 256 rows (padding skip, compact layout), 100 rows (phantom rows of the 128-slot geometry), 1024 FULL rows
    (row-block-pipelined), a 3-step sequence (ring slots used once or twice)."""
    from argsim_amd import synth
    from argsim_amd.model import VAE
    V = 8192
    ids = synth.batch(B, S, V, ragged=ragged, seed=3)
    m = VAE('train', seed=0, dim_tgt=V, dim_emb=512, dim_rep=128, rnn_layers=3)
    m.step = 20000
    m.set_option('enc_top1', 0)
    out = {}
    for rs in (0, 1):
        m.set_option('bwd_rs', rs)
        m.forward_backward(ids, ids, seed=7)
        out[rs] = (m.losses(), m.get_grads(), m.encode(ids))
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][2], out[1][2])
    for k in out[0][1]:
        a, b = out[1][1][k], out[0][1][k]
        if k == 'encode/rnn3/bwd/R':
            assert not a.any() and not b.any(), k
            continue
        assert rel_l2(a, b) <= 2e-5, (k, rel_l2(a, b))
    m.close()


def test_auto_choice_of_the_bptt_form_follows_the_fill():
    """bwd_rs = 2 (default): the host takes the reduce-scatter form where the fill it expects is low (a ragged batch with a long tail:
    below 0.40, the measured break-even) and the other form on fuller batches; either way the gradients are those of the forced forms."""
    from argsim_amd import synth
    from argsim_amd.model import VAE
    V = 8192
    m = VAE('train', seed=0, dim_tgt=V, dim_emb=512, dim_rep=128, rnn_layers=3)
    m.step = 20000
    for B, S, ragged in ((256, 24, False), (64, 24, True)):
        ids = synth.batch(B, S, V, ragged=ragged, seed=5)
        g = {}
        for rs in (2, 2, 0, 1):       # (the second auto call has seen the first one's fill)
            m.set_option('bwd_rs', rs)
            m.forward_backward(ids, ids, seed=9)
            g[rs] = m.get_grads()
        for k in g[0]:
            assert min(rel_l2(g[2][k], g[0][k]), rel_l2(g[2][k], g[1][k])) <= 2e-5, (B, k)
    m.close()


# ------------------------------------------------------------------------------------------ what the fixtures pin
@pytest.mark.parametrize("name,dtype,tol", [('headline', 'f32', 1e-4), ('prod512', 'f32', 1e-4), ('cfg0', 'f32', 1e-4),
                                            ('cfg4', 'f32', 1e-4), ('prod512', 'bf16', 6e-2)])
def test_train_forward_per_token_ce_against_the_oracle_fixture(name, dtype, tol):
    """model.py:174-181: loss_gen_samp of the TRAIN forward (word dropout through the injected keep mask, z = mu + exp(lv / 2) eps)
    at the geometries of the big configurations -- B >= 32, D 512, V 8192 -- against the per-token values the float64 oracle
    stored in the fixture (tests/golden/make_oracle_golden.py), token by token in tf.boolean_mask order; round 3 compared only
    the three scalar losses there although the docstrings said per-token CE."""
    gold = _gold(name)
    cfg, P, ids, keep, eps = make_case(name)
    m = _vae(cfg, P, dtype=dtype, **big_extras(name))
    m.step = 20000
    m.forward_backward(ids, ids, keep_mask=keep, eps=eps)
    ce = m.train_ce()
    want = gold['loss_gen_samp'].astype(np.float64)
    assert ce.shape == want.shape, (ce.shape, want.shape)
    assert np.abs(ce - want).max() <= tol, float(np.abs(ce - want).max())
    assert abs(float(ce.astype(np.float64).mean()) - float(gold['loss_gen'])) <= 2e-5 * float(gold['loss_gen']) + (1e-2 if dtype == 'bf16' else 0.0)
    m.close()


@pytest.mark.parametrize("opts", [{}, {'bwd_rs': 1}])
def test_same_seed_gives_bit_identical_losses_at_the_bench_geometry(opts):
    """a determinism test for the persistent kernels -- same seed => bit-identical loss.  The bench geometry
    (B 256 x S 64 FULL, D 512, V 8192, persistent team kernels, counter RNG for the dropout mask and the latent draw), the three
    loss scalars (summed in a fixed order by finalize_losses: no float atomics), z and the per-token CE of two runs of ONE seed are
    the same bits; another seed moves them.  (Weight gradients carry float-atomic order and are compared elsewhere, to 1e-6.)"""
    from argsim_amd import synth
    from argsim_amd.model import VAE
    ids = synth.batch(256, 64, 8192, seed=0)
    m = VAE('train', seed=0, dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3)
    m.step = 20000
    for k, v in opts.items():
        m.set_option(k, v)
    runs = []
    for seed in (11, 11, 12):
        m.forward_backward(ids, ids, seed=seed)
        runs.append((np.asarray(m.losses(), np.float32).tobytes(), m.train_ce().tobytes()))
    assert runs[0] == runs[1]
    assert runs[0][0] != runs[2][0] and runs[0][1] != runs[2][1]
    z = [m.encode(ids).tobytes() for _ in range(2)]
    assert z[0] == z[1]
    m.close()


# ------------------------------------------------------------------------------------------ phantom rows, per variable
def test_phantom_row_geometry_against_the_oracle_fixture():
    """A batch WITHOUT a team-kernel geometry of its own (100 rows, the reference's batch_train, src/config.json:26): the GRU
    launches run with 128 slots of which 28 hold phantom rows, in the compact layout whatever the fill, with table-fed first layers
    below the vocabulary size (1 200 tokens >= 1 024) -- the id-grouped summation of dE and of layer 1's dW.  Round 3 held this path
    against the register-form path by ONE global gradient-norm ratio; here every variable is checked against the float64 oracle's
    fixture (norm and a fixed projection), so a dead or wrong small block -- a bias, one direction's R -- cannot hide."""
    gold = _gold('phantom100')
    cfg, P, ids, keep, eps = make_case('phantom100')
    assert np.array_equal(ids, gold['ids'])
    m = _vae(cfg, P)
    m.step = 20000
    z = m.encode(ids)
    assert np.abs(z - gold['mu']).max() <= 2e-5
    m.forward_backward(ids, ids, keep_mask=keep, eps=eps)
    assert m.present_ids()[0] > 0 and m.present_ids()[1] > 0                  # table-fed below the vocabulary size
    lg, lk, lo = m.losses()
    for got, key in ((lo, 'loss'), (lg, 'loss_gen'), (lk, 'loss_kld')):
        assert abs(got - float(gold[key])) <= 2e-5 * abs(float(gold[key])) + 1e-7, key
    assert np.abs(m.train_ce() - gold['loss_gen_samp']).max() <= 1e-4
    bad = {}
    for k, g in m.get_grads().items():
        g = g.astype(np.float64)
        n = float(gold['gnorm/' + k])
        p = _probe(k, g.shape)
        e = max(abs(np.linalg.norm(g) - n) / n if n > 0 else float(np.abs(g).max()),
                abs(float((g * p).sum()) - float(gold['gdot/' + k])) / (n * np.linalg.norm(p)) if n > 0 else 0.0)
        if e > 2e-4:
            bad[k] = e
    assert not bad, bad
    m.close()


# ------------------------------------------------------------------------------------------ BASELINE configs[0] as worded
def test_configs0_real_text_parity_step_against_the_oracle_fixture():
    """BASELINE configs[0]: "src/config.json defaults, 1k-sentence IAC subset, SentencePiece vocab 8k, seq_len 64, batch 32".  One
    training step at the config.json dimensions (dim_rep 1024, src/config.json:10-21) over rows 0..31 of the 1 000 IAC posts of
    tests/golden/configs0_ids.npz -- real text from the reference's docs/results_iac/clustering.csv, tokenised in the build
    container with the 8k SentencePiece model trained there on the reference's trainer flags (util_sp.py:24-39) and capped to 64
    pieces (util_sp.py:42-63; make_configs0_golden.py) -- against the float64 oracle's fixture: losses, mu, log sigma^2, per-token
    CE, every gradient (norm and one projection per variable)."""
    gold = _gold('cfg0real')
    cfg, P, ids, keep, eps = make_case('cfg0real')
    assert np.array_equal(ids, gold['ids']) and cfg['dim_rep'] == 1024 and ids.shape[0] == 32
    m = _vae(cfg, P)
    m.step = 20000
    z, lv = m.encode(ids, return_lv=True)
    assert np.abs(z - gold['mu']).max() <= 2e-5 and np.abs(lv - gold['lv']).max() <= 2e-5
    m.forward_backward(ids, ids, keep_mask=keep, eps=eps)
    lg, lk, lo = m.losses()
    for got, key in ((lo, 'loss'), (lg, 'loss_gen'), (lk, 'loss_kld')):
        assert abs(got - float(gold[key])) <= 2e-5 * abs(float(gold[key])) + 1e-7, key
    assert np.abs(m.train_ce() - gold['loss_gen_samp']).max() <= 1e-4
    for k, g in m.get_grads().items():
        g = g.astype(np.float64)
        n = float(gold['gnorm/' + k])
        assert abs(np.linalg.norm(g) - n) <= 2e-4 * n, k
        p = _probe(k, g.shape)
        assert abs(float((g * p).sum()) - float(gold['gdot/' + k])) <= 2e-4 * n * np.linalg.norm(p), k
    m.close()


def test_configs0_training_driver_over_the_real_text(tmp_path):
    """The same configuration through argsim_amd.train.main (src/train.py:54-121): train.txt is the DECODE of the capped ids, as
    src/data_iac.py:40-41 writes it, the vocabulary is the committed 8k model, the model section is src/config.json's (dim_rep
    1024), batch 32, max_len 64; the batch generator tokenises the text again (encode_capped over the 8k vocabulary, vpack, the
    prefetch pipe), the loop trains 60 steps, validates twice over 96 held-out posts and writes a checkpoint.  The re-tokenised
    rows must be the committed ids (SentencePiece decode / encode round trip), the validation CE must fall."""
    import json
    from argsim_amd import train, util_sp
    here = os.path.join(HERE, 'golden')
    vocab = util_sp.load_spm(os.path.join(here, 'configs0_vocab.model'))
    assert vocab.get_piece_size() == 8192
    with np.load(os.path.join(here, 'configs0_ids.npz'), allow_pickle=False) as f:
        ids = f['ids'].astype(np.int32)
    assert ids.shape == (1000, 64)
    rows = [[int(t) for t in r if t != 1] for r in ids]
    lines = [vocab.decode_ids(r) for r in rows]
    same = sum(util_sp.encode_capped(vocab, t, cap=64) == r for t, r in zip(lines, rows))
    assert same >= 990, same                      # (a handful of rows may re-segment across a removed piece boundary)
    d = tmp_path
    (d / 'data').mkdir()
    open(d / 'data' / 'train.txt', 'w').write('\n'.join(lines[:904]) + '\n')
    np.save(d / 'data' / 'valid.npy', ids[904:])
    cfgj = {"paths": {"log": str(d / 'log'), "vocab": os.path.join(here, 'configs0_vocab.model'), "train": str(d / 'data' / 'train.txt'),
                      "valid": str(d / 'data' / 'valid.npy'), "ckpt": str(d / 'ckpt')},
            "model": {"accelerate": 1e-4, "learn_rate": 1e-3, "dim_tgt": 8192, "dim_emb": 512, "dim_rep": 1024, "rnn_layers": 3,
                      "bidirectional": True, "bidir_stacked": True, "attentive": False, "logit_use_embed": True},      # src/config.json:10-21
            "train": {"seed": 0, "max_len": 64, "batch_train": 32, "batch_valid": 32, "total_valid": 96}}
    json.dump(cfgj, open(d / 'config.json', 'w'))
    train.main(['--config', str(d / 'config.json'), '--trial', 'c0', '--rounds', '1', '--steps-per-round', '60', '--valid-every', '30', '--prefetch', '4'])
    recs = [json.loads(l) for l in open(d / 'log' / 'c0.jsonl')]
    assert [r['step'] for r in recs] == [30, 60]
    assert all(np.isfinite([r['step_errt'], r['step_loss_gen'], r['step_loss_kld'], r['sentences_per_sec']]).all() for r in recs)
    assert recs[1]['step_loss_gen'] < recs[0]['step_loss_gen'] < np.log(8192.0) + 0.5
    assert (d / 'ckpt' / 'c00.npz').exists()


# ------------------------------------------------------------------------------------------ launch shaping that must not change results
def test_ragged_split_k_and_shared_device_turns_change_only_the_summation_order():
    """Two round-4 knobs that shape launches only.  dyn_split: on a ragged batch in the compact layout the narrow backward GEMMs over few
    EXPECTED rows (dho = dlogits E, the decoder's dx, dE of the present ids) split K with float atomics instead of leaving the chip at one
    workgroup per CU -- the expectation comes from an earlier call's fill and never decides a value: same losses bit for bit, gradients to
    float-atomic order.  shared_device: persistent launches taken in turn across processes (a lock file and one synchronisation per
    launch) -- the same kernels in the same order: z, losses and per-token CE bit for bit."""
    from argsim_amd import synth
    from argsim_amd.model import VAE
    ids = synth.batch(256, 48, 8192, ragged=True, seed=21)
    m = VAE('train', seed=0, dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3)
    m.step = 20000
    m.set_option('compact', 1)
    out = {}
    for key in ((1, 0), (1, 0), (0, 0), (1, 1)):          # (dyn_split, shared_device); the second call has seen the first one's fill
        m.set_option('dyn_split', key[0]); m.set_option('shared_device', key[1])
        m.forward_backward(ids, ids, seed=3)
        out[key] = (m.losses(), m.train_ce(), m.grads.clone(), m.encode(ids))
    base = out[(0, 0)]
    for key in ((1, 0), (1, 1)):
        assert out[key][0] == base[0] and np.array_equal(out[key][1], base[1]) and np.array_equal(out[key][3], base[3])
        d = float((out[key][2] - base[2]).norm() / base[2].norm())
        assert d <= 1e-5, (key, d)
    assert os.path.exists('/tmp/argsim_vae_dev%d.lock' % m.device.index)
    m.close()


# ------------------------------------------------------------------------------------------ phased persistent bf16 NT GEMM (gemm_bf16_p8.hip)
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,bias,acc,split,dyn", [
    (8200, 4104, 512, True, 0, 1, 0),       # 33 x 17 tiles on 256 workgroups: whole tiles (counted epilogue) and edge tiles (drained) follow each other
    (16384, 1536, 128, False, 0, 1, 0),     # two K tiles per item: every look-ahead crosses into the next item
    (5000, 768, 1024, True, 1, 1, 0),       # C += : the epilogue reads C
    (2048, 1024, 8192, True, 0, 5, 0),      # K split into uneven slices (128 K tiles over 5), float atomics, bias added once
    (9000, 2048, 576, False, 0, 1, 7777),   # device-side row count below M: fewer tiles than the grid was sized for
    (70000, 512, 1536, True, 0, 1, 0),      # two tile columns: groups of 8 x 2 tiles
])
def test_bf16_phased_gemm_matches_the_register_staged_kernel(M, N, K, bias, acc, split, dyn):
    """compute_dtype 1: the persistent LDS-DMA kernel against float64 products of the same bf16-rounded operands AND against the
    register-staged 256x256 kernel (option bf16_nt8 = 0) on the same call."""
    import ctypes as C
    import torch
    from argsim_amd.model import VAE
    m = VAE('train', dtype='bf16', dim_tgt=64, dim_emb=16, dim_rep=8, rnn_layers=1)
    g = torch.Generator(device='cuda').manual_seed(M + N + K)
    A = torch.randn((M, K), device='cuda', generator=g) * 0.5
    B = torch.randn((N, K), device='cuda', generator=g) * 0.5
    bv = torch.randn((N,), device='cuda', generator=g)
    C0 = torch.randn((M, N), device='cuda', generator=g)
    rows = dyn if dyn else M
    m._stream()
    out = []
    for form in (1, 0):
        m.set_option('bf16_nt8', form)
        Cm = C0.clone() if acc else torch.zeros((M, N), device='cuda')
        if dyn:
            cnt = torch.tensor([dyn], dtype=torch.int32, device='cuda')
            rc = m._l.avae_debug_gemm_dyn(m._h, C.c_void_p(A.data_ptr()), C.c_void_p(B.data_ptr()), C.c_void_p(Cm.data_ptr()), M, N, K, C.c_void_p(cnt.data_ptr()))
        else:
            rc = m._l.avae_debug_gemm(m._h, 0, 0, C.c_void_p(A.data_ptr()), C.c_void_p(B.data_ptr()), C.c_void_p(Cm.data_ptr()),
                                      C.c_void_p(bv.data_ptr()) if bias else None, M, N, K, K, K, N, 0.5 if not dyn else 1.0, acc, split)
        assert rc == 0, m._l.avae_last_error(m._h)
        torch.cuda.synchronize()
        out.append(Cm)
    alpha = 1.0 if dyn else 0.5
    ref = alpha * (A[:rows].bfloat16().double() @ B.bfloat16().double().t())
    if bias and not dyn: ref = ref + bv.double()
    if acc: ref = ref + C0[:rows].double()
    tol = 2e-4 * max(1.0, float(ref.abs().max()))
    assert float((out[0][:rows].double() - ref).abs().max()) <= tol
    assert float((out[0][:rows] - out[1][:rows]).abs().max()) <= tol
    if dyn: assert float(out[0][rows:].abs().max()) == 0.0          # rows beyond the device-side count are not written
    m.close()


# ------------------------------------------------------------------------------------------ fp16 logits panel of the training forward (bf16 mode)
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,dyn", [
    (8200, 8192, 512, 0),         # 33 x 32 tiles: whole tiles (16 counted stores per wave) and the edge tile row (8-byte predicated stores)
    (16384, 4096, 128, 0),        # two K tiles per item
    (9000, 8192, 576, 7777),      # device-side row count below M: rows beyond it are not written
])
def test_bf16_phased_gemm_fp16_panel_is_the_fp32_result_rounded_once(M, N, K, dyn):
    """GemmArgs::c16 (gemm_bf16_p8.hip, H16): the same accumulators as the fp32-output kernel, rounded to fp16 (nearest even) in the epilogue
    and stored as one 2-byte panel -- bit for bit torch's .half() of the fp32 output, over exactly the rows the device-side count names."""
    import ctypes as C
    import torch
    from argsim_amd.model import VAE
    m = VAE('train', dtype='bf16', dim_tgt=64, dim_emb=16, dim_rep=8, rnn_layers=1)
    g = torch.Generator(device='cuda').manual_seed(M + N + K)
    A = torch.randn((M, K), device='cuda', generator=g) * 0.5
    B = torch.randn((N, K), device='cuda', generator=g) * 0.5
    m._stream()
    rows = dyn if dyn else M
    cnt = torch.tensor([rows], dtype=torch.int32, device='cuda')
    C32 = torch.zeros((M, N), device='cuda')
    if dyn:
        rc = m._l.avae_debug_gemm_dyn(m._h, C.c_void_p(A.data_ptr()), C.c_void_p(B.data_ptr()), C.c_void_p(C32.data_ptr()), M, N, K, C.c_void_p(cnt.data_ptr()))
    else:
        rc = m._l.avae_debug_gemm(m._h, 0, 0, C.c_void_p(A.data_ptr()), C.c_void_p(B.data_ptr()), C.c_void_p(C32.data_ptr()), None, M, N, K, K, K, N, 1.0, 0, 1)
    assert rc == 0, m._l.avae_last_error(m._h)
    C16 = torch.full((M, N), 7.0, dtype=torch.float16, device='cuda')
    rc = m._l.avae_debug_gemm_c16(m._h, C.c_void_p(A.data_ptr()), C.c_void_p(B.data_ptr()), C.c_void_p(C16.data_ptr()), M, N, K, 1.0, C.c_void_p(cnt.data_ptr()) if dyn else None)
    assert rc == 0, m._l.avae_last_error(m._h)
    torch.cuda.synchronize()
    assert torch.equal(C16[:rows], C32[:rows].half())
    if dyn: assert bool((C16[rows:] == 7.0).all())
    ref = A[:rows].bfloat16().double() @ B.bfloat16().double().t()
    assert float((C16[:rows].double() - ref).abs().max()) <= 1e-3 * max(1.0, float(ref.abs().max()))
    m.close()


@pytest.mark.gpu
def test_fp16_logits_panel_changes_the_training_step_by_less_than_the_bf16_gradient_rounding():
    """compute_dtype 1, training forward (option logits16, default on): the logits leave the phased GEMM as an fp16 panel and softmax_ce turns
    that panel into the bf16 gradient (softmax - onehot)/N in place; no fp32 logits exist.  Against logits16 = 0 on the same batch: z bit for
    bit (the encoder does not see it), loss and per-token CE to fp16 accuracy of the logits (2^-11 relative on |logit| <~ 10), gradients well
    inside the bf16 mode's own tolerance (the gradient panel itself carries 2^-9)."""
    import numpy as np
    from argsim_amd import synth
    from argsim_amd.model import VAE
    ids = synth.batch(64, 64, 8192, ragged=True, seed=5)
    m = VAE('train', seed=0, dtype='bf16', dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3)
    m.step = 20000
    out = {}
    for v in (1, 0):
        m.set_option('logits16', v)
        m.forward_backward(ids, ids, seed=3)
        out[v] = (m.losses(), m.train_ce().copy(), m.grads.clone(), m.encode(ids))
    assert np.array_equal(out[1][3], out[0][3])
    assert abs(out[1][0][0] - out[0][0][0]) <= 2e-4 * abs(out[0][0][0]), (out[1][0], out[0][0])
    assert float(np.abs(out[1][1] - out[0][1]).max()) <= 2e-2
    assert float(np.abs(out[1][1] - out[0][1]).mean()) <= 2e-3
    d = float((out[1][2] - out[0][2]).norm() / out[0][2].norm())
    assert d <= 1e-2, d
    m.close()
