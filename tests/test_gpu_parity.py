"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on identical inputs.

Tolerances (fp32 path vs float64 oracle; stated per quantity as SURVEY 8c asks):
    z, mu, lv               <= 2e-5 abs
    loss_gen, loss_kld      <= 2e-5 rel
    per-sample CE           <= 1e-4 abs
    gradients               <= 2e-4 relative L2 per variable, and per 16-row block of every variable (helpers.grad_blocks)
    one Adam update         <= 1e-5 abs on the parameters (update magnitude is ~lr = 1e-3)
    pred / errt             exact (integer) -- ties are vanishingly unlikely with random weights
"""
import ctypes as C

import numpy as np
import pytest

from helpers import CASES, grads_bad, make_case, rel_l2
from oracle import vae_numpy as vn
from oracle import vae_torch as vt

pytestmark = pytest.mark.gpu


def _vae(cfg, P, **kw):
    from argsim_amd.model import VAE
    keys = ('dim_tgt', 'dim_emb', 'dim_rep', 'rnn_layers', 'accelerate', 'learn_rate', 'bos', 'eos')
    m = VAE('train', init=False, **{k: cfg[k] for k in keys}, **kw)
    m.set_params(P)
    return m


@pytest.mark.parametrize("a_mc,b_nc", [(0, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (200, 72, 52), (4, 8, 16), (333, 260, 132), (1000, 512, 96),
                                   (333, 256, 2048), (384, 128, 3072), (1280, 640, 1600)])     # buffer-load staging path
def test_gemm(a_mc, b_nc, M, N, K):
    import torch
    from argsim_amd import lib
    l = lib.load()
    if a_mc:
        M = (M + 3) // 4 * 4
    if b_nc:
        N = (N + 3) // 4 * 4
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = rng.standard_normal((K, N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    C0 = rng.standard_normal((M, N)).astype(np.float32)
    ref = 0.5 * (A.astype(np.float64) @ B.astype(np.float64)) + bias
    cfg = lib.AvaeConfig(32, 16, 8, 1, 1e-4, 1e-3, 2, 1, 0, 0, 1.0, 0.0, 0)
    h = C.c_void_p()
    assert l.avae_create(C.byref(cfg), 0, C.byref(h)) == 0
    dev = torch.device('cuda', 0)
    At = torch.tensor(A.T.copy() if a_mc else A, device=dev)
    Bt = torch.tensor(B if b_nc else B.T.copy(), device=dev)
    bt = torch.tensor(bias, device=dev)
    lda = M if a_mc else K
    ldb = N if b_nc else K
    for acc, split in ((0, 1), (1, 1), (0, 3), (0, -1), (1, -1), (0, -3), (1, -3)):      # split -1: thin 32x128 tile variant; -3: skinny form (A k-contiguous), else thin
        Ct = torch.tensor(C0, device=dev) if acc else torch.zeros((M, N), device=dev)
        rc = l.avae_debug_gemm(h, a_mc, b_nc, At.data_ptr(), Bt.data_ptr(), Ct.data_ptr(), bt.data_ptr(),
                               M, N, K, lda, ldb, N, 0.5, acc, split)
        assert rc == 0, l.avae_last_error(h)
        torch.cuda.synchronize()
        want = ref + (C0 if acc else 0.0)
        got = Ct.cpu().numpy()
        assert np.abs(got - want).max() <= 2e-5 * max(1.0, np.abs(want).max()), (acc, split)
    l.avae_destroy(h)


@pytest.mark.parametrize("case", ['split', 'split_bf16_keep', 'dyn_rows_split', 'paired_wgrad'])
def test_gemm_whole_call(case):
    """one product through gemm() as the model calls it -- plan, clears, launches (avae_debug_gemm_call) -- at the smallest shapes
    where the plan moves pointers, against float64 at the tolerances of test_gemm / test_gemm_bf16_operands:
    split: 9472 x 512 x 64 = 296 tiles, 256 in the main launch + 40 in the tail: result rows on both sides of row 8192;
    split_bf16_keep: the same in bf16 mode with GemmCall::keep_a16: the kept panel is the bf16 rounding of ALL 9472 rows of A;
    dyn_rows_split: backward form, 2048 static rows of which *count = 700 exist (expected: 700), K = 1536: the first 700 rows are
    cleared and K-split, the rows from 700 on keep the sentinel; paired_wgrad: two 128 x 128 weight gradients over K = 2048 in one launch"""
    import torch
    from argsim_amd import lib
    l = lib.load()
    bf16 = case == 'split_bf16_keep'
    M, N, K = {'split': (9472, 512, 64), 'split_bf16_keep': (9472, 512, 64), 'dyn_rows_split': (2048, 512, 1536), 'paired_wgrad': (128, 128, 2048)}[case]
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = rng.standard_normal((K, N)).astype(np.float32)
    cfg = lib.AvaeConfig(32, 16, 8, 1, 1e-4, 1e-3, 2, 1, 0, 0, 1.0, 0.0, 1 if bf16 else 0)
    h = C.c_void_p()
    assert l.avae_create(C.byref(cfg), 0, C.byref(h)) == 0
    dev = torch.device('cuda', 0)
    shape = np.array([[0, 0, M, N, K, N, 0, 0, -1, 0, 0, 0, 0, 0, 0, int(bf16), 1, 1, 1]], dtype=np.int32)      # (GemmShape: tests/test_gemm_plan.py)
    plan = np.zeros((1, 15), dtype=np.int32)

    def call(a_mc, b_nc, At, Bt, Ct, flags=0, count=None, expect=0, pair=(None, None, None), keep=None):
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = l.avae_debug_gemm_call(h, a_mc, b_nc, At.data_ptr(), Bt.data_ptr(), Ct.data_ptr(), None, M, N, K, At.shape[1], Bt.shape[1], N, 1.0, 0,
                                    flags, ptr(count), expect, ptr(pair[0]), ptr(pair[1]), ptr(pair[2]), ptr(keep))
        assert rc == 0, l.avae_last_error(h)
        torch.cuda.synchronize()
        return Ct.cpu().numpy()

    def close(got, want, tol):
        err = np.abs(got - want).max()
        print(case, 'max abs error', err, 'bound', tol * max(1.0, np.abs(want).max()))
        assert err <= tol * max(1.0, np.abs(want).max())

    if case in ('split', 'split_bf16_keep'):
        assert l.avae_debug_gemm_plan(shape.ctypes.data, 1, plan.ctypes.data) == 0
        assert plan[0, 0] == 2 and plan[0, 8] == 8192 and plan[0, 9] == M - 8192, plan      # main + tail, the tail from row 8192
        At, Bt = torch.tensor(A, device=dev), torch.tensor(B.T.copy(), device=dev)
        Ct = torch.full((M, N), 777.0, device=dev)
        if bf16:
            keep = torch.full((M, K), 777.0, device=dev, dtype=torch.bfloat16)
            got = call(0, 0, At, Bt, Ct, keep=keep)
            assert torch.equal(keep.view(torch.int16), At.to(torch.bfloat16).view(torch.int16))
            Ar, Br = (torch.tensor(x).to(torch.bfloat16).to(torch.float64).numpy() for x in (A, B))
            close(got, Ar @ Br, 3e-5)
        else:
            close(call(0, 0, At, Bt, Ct), A.astype(np.float64) @ B.astype(np.float64), 2e-5)
    elif case == 'dyn_rows_split':
        shape[0, 1] = 1; shape[0, 9] = 1; shape[0, 10] = 700; shape[0, 11] = 1
        assert l.avae_debug_gemm_plan(shape.ctypes.data, 1, plan.ctypes.data) == 0
        assert plan[0, 0] == 1 and plan[0, 4] >= 2 and plan[0, 6] == 2 and plan[0, 7] == 1, plan      # K slices into the cleared first *count rows
        At, Bt = torch.tensor(A, device=dev), torch.tensor(B, device=dev)
        Ct = torch.full((M, N), 777.0, device=dev)
        count = torch.tensor([700], dtype=torch.int32, device=dev)
        got = call(0, 1, At, Bt, Ct, flags=1, count=count, expect=700)
        close(got[:700], A[:700].astype(np.float64) @ B.astype(np.float64), 2e-5)
        assert (got[700:] == 777.0).all()
    else:
        A2 = rng.standard_normal((K, M)).astype(np.float32)
        B2 = rng.standard_normal((K, N)).astype(np.float32)
        At, Bt, A2t, B2t = (torch.tensor(x, device=dev) for x in (A.T.copy(), B, A2, B2))
        Ct, C2t = torch.zeros((M, N), device=dev), torch.zeros((M, N), device=dev)      # (the zero-filled gradients)
        got = call(1, 1, At, Bt, Ct, flags=4, pair=(A2t, B2t, C2t))
        close(got, A.astype(np.float64) @ B.astype(np.float64), 2e-5)
        close(C2t.cpu().numpy(), A2.T.astype(np.float64) @ B2.astype(np.float64), 2e-5)
    l.avae_destroy(h)


@pytest.mark.parametrize("name", list(CASES))
def test_encode_z(name):
    cfg, P, ids, keep, eps = make_case(name)
    m = _vae(cfg, P)
    z, lv = m.encode(ids, return_lv=True)
    o = vn.forward(P, cfg, ids, ids, 'valid')
    assert np.abs(z - o['mu']).max() <= 2e-5
    assert np.abs(lv - o['lv']).max() <= 2e-5
    # the stepwise (one launch per time step) and persistent GRU kernels must agree bit for bit
    m.set_option('persistent', 0)
    z2 = m.encode(ids)
    assert np.array_equal(z, z2)


@pytest.mark.parametrize("name", list(CASES))
def test_eval_outputs(name):
    cfg, P, ids, keep, eps = make_case(name)
    m = _vae(cfg, P)
    errt, lgen, lkld = m.eval(ids, ids)
    o = vn.forward(P, cfg, ids, ids, 'valid')
    assert errt.shape == o['errt_samp'].shape
    assert np.abs(lgen - o['loss_gen_samp']).max() <= 1e-4
    assert np.abs(lkld - o['loss_kld_samp']).max() <= 2e-5
    assert np.array_equal(errt, o['errt_samp'])
    lg, lk, lo = m.losses()
    assert abs(lg - o['loss_gen']) <= 2e-5 * abs(o['loss_gen'])
    assert abs(lk - o['loss_kld']) <= 2e-5 * abs(o['loss_kld']) + 1e-7


@pytest.mark.parametrize("name", ['mid', 'tab'])
def test_eos_in_the_middle_of_a_row(name):
    """source != target and an eos id in the MIDDLE of a row, real ids behind it: the source length is the COUNT of non-eos ids
    (util_tf.py:54-57: a prefix of that many positions enters the encoder, eos ids included), the decoder mask is per position
    (model.py:161: the step behind the eos is dropped from the loss, the steps behind it are not, and the recurrence runs
    through) -- losses, per-sentence outputs and gradients against the live oracle."""
    cfg, P, ids, keep, eps = make_case(name)
    src, tgt = ids.copy(), ids.copy()
    full = [b for b in range(ids.shape[0]) if (ids[b] != cfg['eos']).sum() >= 9]
    src[full[0], 4] = cfg['eos']
    tgt[full[1], 5] = cfg['eos']
    tgt[full[1], 2] = cfg['eos']
    step = 20000
    m = _vae(cfg, P)
    m.step = step
    errt, lgen, lkld = m.eval(src, tgt)
    o = vn.forward(P, cfg, src, tgt, 'valid')
    assert np.array_equal(errt, o['errt_samp'])
    assert np.abs(lgen - o['loss_gen_samp']).max() <= 1e-4
    assert np.abs(lkld - o['loss_kld_samp']).max() <= 2e-5
    m.forward_backward(src, tgt, keep_mask=keep, eps=eps)
    lg, lk, lo = m.losses()
    outs, grads = vt.loss_and_grads(P, cfg, src, tgt, step, keep, eps)
    assert abs(lg - outs['loss_gen']) <= 2e-5 * abs(outs['loss_gen'])
    assert abs(lk - outs['loss_kld']) <= 2e-5 * abs(outs['loss_kld'])
    got = m.get_grads()
    bad = {k: rel_l2(got[k], grads[k]) for k in grads if rel_l2(got[k], grads[k]) > 2e-4}
    assert not bad, bad
    bad = grads_bad(got, grads, 2e-4)          # block by block (helpers.grad_blocks): a wrong slice is not diluted by the rest of its variable
    assert not bad, bad


@pytest.mark.parametrize("persistent", [1, 0])
@pytest.mark.parametrize("name", list(CASES))
def test_gradients(name, persistent):
    cfg, P, ids, keep, eps = make_case(name)
    step = 20000                                   # anneal = tanh(2) so the KL backward is live
    m = _vae(cfg, P)
    m.set_option('persistent', persistent)
    m.step = step
    m.forward_backward(ids, ids, keep_mask=keep, eps=eps)
    lg, lk, lo = m.losses()
    outs, grads = vt.loss_and_grads(P, cfg, ids, ids, step, keep, eps)
    assert abs(lg - outs['loss_gen']) <= 2e-5 * abs(outs['loss_gen'])
    assert abs(lk - outs['loss_kld']) <= 2e-5 * abs(outs['loss_kld'])
    assert abs(lo - outs['loss']) <= 2e-5 * abs(outs['loss'])
    got = m.get_grads()
    bad = {k: rel_l2(got[k], grads[k]) for k in grads if rel_l2(got[k], grads[k]) > 2e-4}
    assert not bad, bad
    bad = grads_bad(got, grads, 2e-4)          # block by block (helpers.grad_blocks): a wrong slice is not diluted by the rest of its variable
    assert not bad, bad


@pytest.mark.parametrize("name", ['tiny', 'mid'])
def test_train_steps_match_oracle(name):
    """three full steps (fwd + bwd + TF Adam + step increment) track the float64 oracle"""
    cfg, P, ids, keep, eps = make_case(name)
    m = _vae(cfg, P)
    step0 = 12345
    m.step = step0
    Pn = {k: v.copy() for k, v in P.items()}
    mo = {k: np.zeros_like(v) for k, v in P.items()}
    vo = {k: np.zeros_like(v) for k, v in P.items()}
    for i in range(3):
        m.train_step(ids, ids, keep_mask=keep, eps=eps)
        outs, grads = vt.loss_and_grads(Pn, cfg, ids, ids, step0 + i, keep, eps)
        lr = vn.schedule(step0 + i, cfg['accelerate'], cfg['learn_rate'])[2]
        Pn, mo, vo = vn.adam_tf(Pn, grads, mo, vo, i, lr)
        # NB: TF's beta powers count optimizer applications, the library counts global_step;
        # the library therefore uses t = step + 1.  Compare with that convention:
    assert m.step == step0 + 3
    # the oracle above used n_updates = i; the library uses global_step -- re-run the oracle the same way
    Pn = {k: v.copy() for k, v in P.items()}
    mo = {k: np.zeros_like(v) for k, v in P.items()}
    vo = {k: np.zeros_like(v) for k, v in P.items()}
    for i in range(3):
        outs, grads = vt.loss_and_grads(Pn, cfg, ids, ids, step0 + i, keep, eps)
        lr = vn.schedule(step0 + i, cfg['accelerate'], cfg['learn_rate'])[2]
        Pn, mo, vo = vn.adam_tf(Pn, grads, mo, vo, step0 + i, lr)
    got = m.get_params()
    for k in Pn:
        assert np.abs(got[k] - Pn[k]).max() <= 1e-5, k


def test_adam_first_update_from_step0():
    cfg, P, ids, keep, eps = make_case('tiny')
    m = _vae(cfg, P)
    m.train_step(ids, ids, keep_mask=keep, eps=eps)
    outs, grads = vt.loss_and_grads(P, cfg, ids, ids, 0, keep, eps)
    z = {k: np.zeros_like(v) for k, v in P.items()}
    Pn, _, _ = vn.adam_tf(P, grads, z, z, 0, vn.schedule(0)[2])
    got = m.get_params()
    for k in Pn:
        assert np.abs(got[k] - Pn[k]).max() <= 1e-5, k
    assert m.step == 1


@pytest.mark.parametrize("name", ['tiny', 'mid'])
def test_decode_greedy(name):
    cfg, P, ids, keep, eps = make_case(name)
    m = _vae(cfg, P)
    o = vn.forward(P, cfg, ids, ids, 'valid')
    want = vn.decode_greedy(P, cfg, o['mu'], steps=12)
    got = m.decode(o['mu'].astype(np.float32), steps=12)
    assert got.shape == want.shape and np.array_equal(got, want)
    # single step entry: state_in from z, one step from bos
    s = m.decode_init(o['mu'].astype(np.float32))
    assert np.abs(s.cpu().numpy() - o['state_in']).max() <= 2e-5
    pred, s2 = m.decode_step(np.full((1, len(ids)), cfg['bos'], np.int32), s)
    assert np.array_equal(pred.cpu().numpy()[0], want[:, 0]) or want.shape[1] == 0


def test_untrimmed_input_same_result():
    """util_tf.trim drops all-eos tail columns; feeding them anyway must not change z or the losses"""
    import torch
    cfg, P, ids, keep, eps = make_case('mid', pad=5)
    m = _vae(cfg, P)
    z1 = m.encode(ids)
    z2 = m.encode(torch.as_tensor(ids).cuda())          # device tensors are not trimmed on the host
    assert np.array_equal(z1, z2)
    e1 = m.eval(ids, ids)
    e2 = m.eval(torch.as_tensor(ids).cuda(), torch.as_tensor(ids).cuda())
    for a, b in zip(e1, e2):
        assert np.array_equal(a, b)


def test_random_draws_are_seeded_and_sane():
    """without injected mask/eps the library draws its own: same seed -> same loss, different seed -> different"""
    cfg, P, ids, keep, eps = make_case('mid')
    m = _vae(cfg, P)
    m.forward_backward(ids, ids, seed=11)
    a = m.losses()
    m.forward_backward(ids, ids, seed=11)
    b = m.losses()
    m.forward_backward(ids, ids, seed=12)
    c = m.losses()
    # the loss sums are accumulated with float atomics: equal up to summation order
    assert abs(a[0] - b[0]) <= 1e-5 * abs(a[0]) and abs(a[1] - b[1]) <= 1e-5 * abs(a[1])
    assert abs(a[0] - c[0]) > 1e-4 * abs(a[0])


@pytest.mark.parametrize("enc_top1", [0, 1])
def test_bench_scale_persistent_equals_stepwise(enc_top1):
    """BASELINE configs[1] geometry (B=256, S=64, D=512: 512 co-resident workgroups per GRU launch): the
    persistent kernels' in-launch hand-offs must reproduce the one-launch-per-step results bit for bit
    on the forward (z, per-token CE), and the gradients up to float-atomic summation order.
    enc_top1 = 0: every encoder launch carries both directions (4-team form, the K split of the one-launch-per-step kernels):
    z bit for bit.  enc_top1 = 1 (default): the top layer's forward direction is a one-job launch, which at B = 256 runs the
    2-team form whose K is split over 8 waves -- same products, another summation tree: z to rounding."""
    from argsim_amd import synth
    from argsim_amd.model import VAE
    m = VAE('train', seed=3, dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3)
    m.set_option('enc_top1', enc_top1)
    ids = synth.batch(256, 64, 8192, ragged=True, seed=5)
    m.step = 20000
    same = np.array_equal if not enc_top1 else (lambda a, b: np.abs(np.asarray(a, np.float64) - b).max() <= 2e-6)
    # every forward-kernel variant (0 generic, 1 item pipeline, 2 four-team LDS-weight kernel) must reproduce
    # the one-launch-per-step encoder bit for bit
    m.set_option('persistent', 0)
    z_ref = m.encode(ids)
    m.set_option('persistent', 1)
    for item in (0, 1, 2):
        m.set_option('gru_item', item)
        assert same(m.encode(ids), z_ref), item
    m.set_option('gru_item', 2)
    res = {}
    for mode in (1, 0, 1):
        m.set_option('persistent', mode)
        m.set_option('gru_force_slow', 1 if len(res.get(1, [])) else 0)   # 2nd persistent pass: sc1-only exchange
        z = m.encode(ids)
        ev = m.eval(ids, ids)
        m.forward_backward(ids, ids, seed=9)
        g = m.grads.clone()
        res.setdefault(mode, []).append((z, ev, g))
    (z1, e1, g1), (z0, e0, g0), (z2, e2, g2) = res[1][0], res[0][0], res[1][1]
    assert same(z1, z0) and np.array_equal(z1, z2)
    # decoder layers (one job, B = 256) run the 2-team form whose K is split over 8 waves instead of 4: same products,
    # another summation tree, so per-token CE agrees to rounding (errt and the KL terms, encoder only, exactly)
    for a, b in zip(e1[1:], e0[1:]):
        assert np.allclose(a, b, rtol=0, atol=2e-5)
    if not enc_top1:
        assert np.array_equal(e1[0], e0[0]) and np.array_equal(e1[2], e0[2])
    else:
        assert np.abs(e1[0] - e0[0]).mean() <= 1e-3        # (a rounding-level change of z can flip an argmax at a near tie)
    for a, b in zip(e1, e2):
        assert np.array_equal(a, b)                    # persistent vs persistent (sc1-only exchange): bit for bit
    import torch
    d = (g1 - g0).norm() / g0.norm()
    assert float(d) < 1e-5, float(d)


@pytest.mark.parametrize("name", list(CASES))
def test_against_committed_golden(name):
    """the HIP path against the committed fixtures (tests/golden/oracle_*.npz), not only the live oracle"""
    import os
    path = os.path.join(os.path.dirname(__file__), 'golden', 'oracle_%s.npz' % name)
    with np.load(path, allow_pickle=False) as f:
        gold = {k: f[k] for k in f.files}
    cfg, P, ids, keep, eps = make_case(name)
    m = _vae(cfg, P)
    m.step = 20000
    z = m.encode(gold['ids'])
    assert np.abs(z - gold['mu']).max() <= 2e-5
    m.forward_backward(gold['ids'], gold['ids'], keep_mask=gold['keep'], eps=gold['eps'])
    lg, lk, lo = m.losses()
    assert abs(lo - float(gold['loss'])) <= 2e-5 * abs(float(gold['loss']))
    if name != 'full2':
        g = m.get_grads()
        for k, v in g.items():
            want = float(gold['gnorm/' + k])
            assert abs(np.linalg.norm(v.astype(np.float64)) - want) <= 2e-4 * max(want, 1e-12), k


def test_reference_config_dims_and_odd_batch():
    """src/config.json defaults (dim_rep 1024, dim_emb 512, vocab 8192) with a batch that is no multiple of
    16 and long rows: z against the oracle"""
    cfg = vn.make_cfg()                                     # reference defaults
    rng = np.random.default_rng(5)
    P = {k: v.astype(np.float32).astype(np.float64) for k, v in vn.init_params(cfg, 5, bias_scale=0.05).items()}
    B, S = 5, 40
    ids = np.full((B, S), cfg['eos'], np.int32)
    for b, n in enumerate([40, 1, 17, 33, 8]):
        ids[b, :n] = rng.integers(3, cfg['dim_tgt'], n)
    m = _vae(cfg, P)
    z = m.encode(ids)
    o = vn.forward(P, cfg, ids, ids, 'valid')
    assert np.abs(z - o['mu']).max() <= 2e-5
    errt, lgen, lkld = m.eval(ids, ids)
    assert np.abs(lgen - o['loss_gen_samp']).max() <= 1e-4


def test_large_batch_rows_are_independent():
    """B = 1024 (the per-GPU batch of BASELINE configs[3]; 128 rows per GRU workgroup = 4 super-chunks):
    every row's z must equal the z of the same row encoded in a small batch"""
    from argsim_amd import synth
    from argsim_amd.model import VAE
    m = VAE('train', seed=1, dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3)
    ids = synth.batch(1024, 24, 8192, ragged=True, seed=2)
    z = m.encode(ids)
    for lo in (0, 500, 1008):
        zs = m.encode(ids[lo:lo + 16])
        assert np.array_equal(z[lo:lo + 16], zs), lo
    # and a full training step at that size stays finite and reduces the loss
    m.step = 20000
    l0 = None
    for i in range(3):
        m.train_step(ids, ids, seed=i)
        lg, lk, lo_ = m.losses()
        assert np.isfinite(lo_)
        l0 = l0 if l0 is not None else lo_
    assert lo_ < l0


def test_data_parallel_path_single_rank(tmp_path):
    """the NCCL/RCCL bucket hook + side stream path with world_size 1 must reproduce the plain step"""
    import torch
    import torch.distributed as dist
    from argsim_amd.dist import DataParallel
    cfg, P, ids, keep, eps = make_case('mid')
    a, b = _vae(cfg, P), _vae(cfg, P)
    a.step = b.step = 20000
    if not dist.is_initialized():
        dist.init_process_group('nccl', init_method='file://%s' % (tmp_path / 'rdv'), rank=0, world_size=1,
                                device_id=torch.device('cuda', 0))
    dp = DataParallel(b)
    fired = []
    orig = dp.reducer.reduce_bucket
    dp.reducer.reduce_bucket = lambda i: (fired.append(i), orig(i))[1]
    n_glob = float((ids != cfg['eos']).sum() + len(ids))
    a.train_step(ids, ids, keep_mask=keep, eps=eps)
    dp.train_step(ids, ids, n_glob, float(len(ids)), keep_mask=keep, eps=eps)
    torch.cuda.synchronize()
    nb = len(b.buckets())                                             # every bucket once, in the FIXED announcement order of
    assert fired == list(range(nb - 2)) + [nb - 1, nb - 2]           # include/argsim_vae.h: the embedding before encode/rnn1
    covered = sum(c for _, c in b.buckets())
    assert covered == b.params.numel()
    assert float((a.params - b.params).abs().max()) <= 1e-6
    dist.destroy_process_group()


def test_beta_and_free_bits_extension():
    """BASELINE configs[4] extensions: reduce exactly to the reference at (1, 0) -- every other test -- and
    match the extended oracle otherwise (latent 512 here as in that config)"""
    kw = dict(dim_tgt=256, dim_emb=64, dim_rep=512, rnn_layers=3)
    cfg = vn.make_cfg(**kw)
    rng = np.random.default_rng(3)
    P = {k: v.astype(np.float32).astype(np.float64) for k, v in vn.init_params(cfg, 3, bias_scale=0.1).items()}
    B, S = 6, 10
    ids = np.full((B, S), cfg['eos'], np.int32)
    for b, n in enumerate([10, 3, 7, 10, 1, 5]):
        ids[b, :n] = rng.integers(3, 256, n)
    keep = (rng.random((10, B)) < 0.7).astype(np.uint8)
    eps = rng.standard_normal((B, 512)).astype(np.float32)
    beta, fb = 4.0, 0.02
    m = _vae(cfg, P, kl_beta=beta, free_bits=fb)
    m.step = 20000
    m.forward_backward(ids, ids, keep_mask=keep, eps=eps)
    outs, grads = vt.loss_and_grads(P, cfg, ids, ids, 20000, keep, eps, kl_beta=beta, free_bits=fb)
    lg, lk, lo = m.losses()
    assert abs(lo - outs['loss']) <= 2e-5 * abs(outs['loss'])
    got = m.get_grads()
    bad = {k: rel_l2(got[k], grads[k]) for k in grads if rel_l2(got[k], grads[k]) > 2e-4}
    assert not bad, bad


def test_checkpoint_roundtrip_and_resume(tmp_path):
    """save -> restore into a fresh model -> identical next step (params, Adam slots, global_step): the
    counterpart of tf.train.Saver save/restore in src/train.py:92-96,121"""
    from argsim_amd import ckpt
    cfg, P, ids, keep, eps = make_case('mid')
    a = _vae(cfg, P)
    a.step = 777
    a.train_step(ids, ids, keep_mask=keep, eps=eps)
    path = ckpt.save(a, str(tmp_path / 'trial1'))
    b = _vae(cfg, {k: np.zeros_like(v) for k, v in P.items()})
    ckpt.restore(b, path)
    assert b.step == a.step == 778
    a.train_step(ids, ids, keep_mask=keep, eps=eps)
    b.train_step(ids, ids, keep_mask=keep, eps=eps)
    pa, pb = a.get_params(), b.get_params()
    for k in pa:
        assert np.abs(pa[k] - pb[k]).max() <= 1e-7, k
    # an 'infer' restore without slots (eval_embed_reason.py:24-27) is a partial, name-based restore
    p2 = ckpt.save(a, str(tmp_path / 'noslots'), slots=False)
    c = _vae(cfg, {k: np.zeros_like(v) for k, v in P.items()})
    ckpt.restore(c, p2)
    assert np.array_equal(c.encode(ids), a.encode(ids))


def test_training_driver_end_to_end(tmp_path):
    """argsim_amd.train.main on a tiny corpus: BASELINE configs[0] plumbing (SentencePiece vocab, batch
    generator, prefetch pipe, 250-step-style loop, validation summary, checkpoint) on the GPU path"""
    import json
    from argsim_amd import train, util_sp
    from argsim_amd.util_np import vpack
    rng = np.random.default_rng(0)
    words = ['argument', 'stance', 'abortion', 'rights', 'gun', 'control', 'people', 'think', 'because', 'evidence',
             'the', 'a', 'of', 'and', 'is', 'not', 'that', 'should', 'we', 'they', 'law', 'state', 'debate', 'claim']
    lines = [' '.join(' '.join(rng.choice(words, int(rng.integers(4, 10)))) + '.' for _ in range(int(rng.integers(1, 4)))) for _ in range(300)]
    d = tmp_path
    (d / 'data').mkdir()
    open(d / 'data' / 'train.txt', 'w').write('\n'.join(lines) + '\n')
    vocab = util_sp.spm(str(d / 'data' / 'vocab'), str(d / 'data' / 'train.txt'), size=48)
    val = [util_sp.encode_capped(vocab, t, cap=24) for t in lines[:40]]
    np.save(d / 'data' / 'valid.npy', vpack(val, (len(val), max(map(len, val))), vocab.eos_id(), np.int32))
    cfgj = {"paths": {"log": str(d / 'log'), "vocab": str(d / 'data' / 'vocab.model'), "train": str(d / 'data' / 'train.txt'),
                      "valid": str(d / 'data' / 'valid.npy'), "ckpt": str(d / 'ckpt')},
            "model": {"accelerate": 1e-4, "learn_rate": 1e-3, "dim_tgt": 48, "dim_emb": 64, "dim_rep": 16, "rnn_layers": 2,
                      "bidirectional": True, "bidir_stacked": True, "attentive": False, "logit_use_embed": True},
            "train": {"seed": 0, "max_len": 24, "batch_train": 16, "batch_valid": 12, "total_valid": 40}}
    json.dump(cfgj, open(d / 'config.json', 'w'))
    train.main(['--config', str(d / 'config.json'), '--trial', 't', '--rounds', '1', '--steps-per-round', '40', '--valid-every', '20', '--prefetch', '4'])
    recs = [json.loads(l) for l in open(d / 'log' / 't.jsonl')]
    assert [r['step'] for r in recs] == [20, 40]
    assert all(np.isfinite([r['step_errt'], r['step_loss_gen'], r['step_loss_kld']]).all() for r in recs)
    assert recs[1]['step_loss_gen'] < recs[0]['step_loss_gen']          # it learns
    assert (d / 'ckpt' / 't0.npz').exists()                              # <trial><step // 10000>, src/train.py:121


# ---------------------------------------------------------------- bf16 GEMM-operand mode (BASELINE configs[2])
@pytest.mark.parametrize("a_mc,b_nc", [(0, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (200, 72, 52), (333, 260, 132), (64, 512, 1000), (4099, 3100, 200), (1024, 768, 8192)])
def test_gemm_bf16_operands(a_mc, b_nc, M, N, K):
    """bf16 mode: operands rounded to bf16 (RNE), products accumulated in fp32.  Against float64 products of the
    SAME rounded operands the only error left is fp32 accumulation order.  The last two shapes run the 256x256-tile
    kernel (ragged edges, one slice; K split into atomically added slices)."""
    import torch
    from argsim_amd import lib
    l = lib.load()
    if a_mc:
        M = (M + 3) // 4 * 4
    if b_nc:
        N = (N + 3) // 4 * 4
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = rng.standard_normal((K, N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    Ar = torch.tensor(A).to(torch.bfloat16).to(torch.float64).numpy()
    Br = torch.tensor(B).to(torch.bfloat16).to(torch.float64).numpy()
    ref = 0.5 * (Ar @ Br) + bias
    cfg = lib.AvaeConfig(32, 16, 8, 1, 1e-4, 1e-3, 2, 1, 0, 0, 1.0, 0.0, 1)
    h = C.c_void_p()
    assert l.avae_create(C.byref(cfg), 0, C.byref(h)) == 0
    dev = torch.device('cuda', 0)
    At = torch.tensor(A.T.copy() if a_mc else A, device=dev)
    Bt = torch.tensor(B if b_nc else B.T.copy(), device=dev)
    bt = torch.tensor(bias, device=dev)
    for acc, split in ((0, 1), (0, 3)):
        Ct = torch.zeros((M, N), device=dev)
        rc = l.avae_debug_gemm(h, a_mc, b_nc, At.data_ptr(), Bt.data_ptr(), Ct.data_ptr(), bt.data_ptr(),
                               M, N, K, M if a_mc else K, N if b_nc else K, N, 0.5, acc, split)
        assert rc == 0, l.avae_last_error(h)
        torch.cuda.synchronize()
        got = Ct.cpu().numpy()
        assert np.abs(got - ref).max() <= 3e-5 * max(1.0, np.abs(ref).max()), (acc, split)
    l.avae_destroy(h)


@pytest.mark.parametrize("name", ['mid', 'wide', 'full2'])
def test_bf16_mode_tracks_the_oracle(name):
    """whole path with bf16 GEMM operands (fp32 accumulate, fp32 recurrence / state / Adam): stated bf16
    tolerances -- z <= 3e-2 abs, losses <= 1e-2 rel, gradients <= 5e-2 relative L2 per variable"""
    cfg, P, ids, keep, eps = make_case(name)
    m = _vae(cfg, P, dtype='bf16')
    o = vn.forward(P, cfg, ids, ids, 'valid')
    z = m.encode(ids)
    assert np.abs(z - o['mu']).max() <= 3e-2
    m.step = 20000
    m.forward_backward(ids, ids, keep_mask=keep, eps=eps)
    lg, lk, lo = m.losses()
    outs, grads = vt.loss_and_grads(P, cfg, ids, ids, 20000, keep, eps)
    assert abs(lo - outs['loss']) <= 1e-2 * abs(outs['loss'])
    got = m.get_grads()
    bad = {k: rel_l2(got[k], grads[k]) for k in grads if rel_l2(got[k], grads[k]) > 5e-2}
    assert not bad, bad


# ---------------------------------------------------------------- fp32 on the bf16 matrix cores (compute_dtype 2)
@pytest.mark.parametrize("a_mc,b_nc", [(0, 0), (0, 1), (1, 1), (1, 0)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (200, 72, 52), (4, 8, 16), (333, 260, 132), (1000, 512, 96), (256, 384, 4100),
                                   # long K, tile-aligned where the layout needs it: the buffer-load staging path and the
                                   # persistent wave-specialised kernel (ragged M through num_records, 300+ tiles per launch)
                                   (333, 256, 2048), (1000, 512, 1536), (384, 128, 3072), (4224, 1280, 1600)])
def test_gemm_split_bf16_is_fp32_accurate(a_mc, b_nc, M, N, K):
    """the 3 x bf16 split GEMM (6 partial products, fp32 accumulate) against float64 products of the SAME fp32
    operands, at the tolerance of the exact-fp32 kernel's test (2e-5 of the result scale), on wide-range data"""
    import torch
    from argsim_amd import lib
    l = lib.load()
    if a_mc:
        M = (M + 3) // 4 * 4
    if b_nc:
        N = (N + 3) // 4 * 4
    rng = np.random.default_rng(M * 7 + N * 3 + K + 1)
    A = (rng.standard_normal((M, K)) * np.exp(rng.standard_normal((M, K)))).astype(np.float32)
    B = (rng.standard_normal((K, N)) * np.exp(rng.standard_normal((K, N)))).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    C0 = rng.standard_normal((M, N)).astype(np.float32)
    ref = 0.5 * (A.astype(np.float64) @ B.astype(np.float64)) + bias
    scale = 0.5 * (np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)) + 1.0
    cfg = lib.AvaeConfig(32, 16, 8, 1, 1e-4, 1e-3, 2, 1, 0, 0, 1.0, 0.0, 2)
    h = C.c_void_p()
    assert l.avae_create(C.byref(cfg), 0, C.byref(h)) == 0
    dev = torch.device('cuda', 0)
    At = torch.tensor(A.T.copy() if a_mc else A, device=dev)
    Bt = torch.tensor(B if b_nc else B.T.copy(), device=dev)
    bt = torch.tensor(bias, device=dev)
    for acc, split in ((0, 1), (1, 1), (0, 3)):
        Ct = torch.tensor(C0, device=dev) if acc else torch.zeros((M, N), device=dev)
        rc = l.avae_debug_gemm(h, a_mc, b_nc, At.data_ptr(), Bt.data_ptr(), Ct.data_ptr(), bt.data_ptr(),
                               M, N, K, M if a_mc else K, N if b_nc else K, N, 0.5, acc, split)
        assert rc == 0, l.avae_last_error(h)
        torch.cuda.synchronize()
        want = ref + (C0 if acc else 0.0)
        got = Ct.cpu().numpy()
        assert np.abs(got - want).max() <= 2e-5 * max(1.0, np.abs(want).max()), (acc, split)
        # and in units of the fp32 accumulation error bound: a few 2^-24 of sum |a||b|
        assert (np.abs(got - want) / scale).max() <= 2e-6, (acc, split)
    l.avae_destroy(h)


@pytest.mark.parametrize("name", list(CASES))
def test_split_bf16_mode_meets_the_fp32_tolerances(name):
    """the whole path with compute_dtype 2 is held to the SAME tolerances as the exact-fp32 path"""
    cfg, P, ids, keep, eps = make_case(name)
    m = _vae(cfg, P, dtype='f32s')
    o = vn.forward(P, cfg, ids, ids, 'valid')
    z, lv = m.encode(ids, return_lv=True)
    assert np.abs(z - o['mu']).max() <= 2e-5
    assert np.abs(lv - o['lv']).max() <= 2e-5
    errt, lgen, lkld = m.eval(ids, ids)
    assert np.abs(lgen - o['loss_gen_samp']).max() <= 1e-4
    assert np.abs(lkld - o['loss_kld_samp']).max() <= 2e-5
    step = 20000
    m.step = step
    m.forward_backward(ids, ids, keep_mask=keep, eps=eps)
    lg, lk, lo = m.losses()
    outs, grads = vt.loss_and_grads(P, cfg, ids, ids, step, keep, eps)
    assert abs(lg - outs['loss_gen']) <= 2e-5 * abs(outs['loss_gen'])
    assert abs(lk - outs['loss_kld']) <= 2e-5 * abs(outs['loss_kld'])
    got = m.get_grads()
    bad = {k: rel_l2(got[k], grads[k]) for k in grads if rel_l2(got[k], grads[k]) > 2e-4}
    assert not bad, bad


def test_split_bf16_mode_at_bench_scale_tracks_exact_fp32():
    """B=256, S=64, D=512, V=8192: z and the gradients of the split mode against the exact-fp32 MFMA path on the
    same batch -- the difference must be of the size of fp32 rounding (both are fp32 computations of one graph)"""
    import torch
    from argsim_amd import synth
    from argsim_amd.model import VAE
    kw = dict(dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3, seed=0)
    ids = synth.batch(256, 64, 8192, seed=0)
    rng = np.random.default_rng(0)
    keep = (rng.random((64, 256)) < 0.88).astype(np.uint8)
    eps = rng.standard_normal((256, 128)).astype(np.float32)
    res = {}
    for dt in ('f32', 'f32s'):
        m = VAE('train', dtype=dt, **kw)
        m.step = 20000
        z = m.encode(ids)
        m.forward_backward(ids, ids, keep_mask=keep, eps=eps)
        res[dt] = (z, m.losses(), m.get_grads())
        del m
        torch.cuda.empty_cache()
    assert np.abs(res['f32'][0] - res['f32s'][0]).max() <= 2e-5
    for a, b in zip(res['f32'][1], res['f32s'][1]):
        assert abs(a - b) <= 2e-6 * abs(a)
    bad = {k: rel_l2(res['f32s'][2][k], v) for k, v in res['f32'][2].items() if rel_l2(res['f32s'][2][k], v) > 1e-4}
    assert not bad, bad


def test_tf_checkpoint_files_roundtrip(tmp_path):
    """save_tf -> TF V2 checkpoint files (index table + data shard, canonical CudnnGRU names, opaque Adam slots)
    -> restore into a fresh model: parameters, Adam slots, step and z are reproduced exactly except that TF's
    canonical form stores the r/u biases summed (restored as bW = sum, bR = 0: the same function)"""
    from argsim_amd import ckpt, tf_bundle
    cfg, P, ids, keep, eps = make_case('mid')
    m = _vae(cfg, P)
    m.step = 777
    for i in range(2):
        m.train_step(ids, ids, keep_mask=keep, eps=eps)
    z0 = m.encode(ids)
    prefix = ckpt.save_tf(m, str(tmp_path / 'ckpt' / 'trial_3'))
    names = set(tf_bundle.read_bundle(prefix))
    assert 'global_step' in names and 'embed/embedding' in names and 'train/beta1_power' in names
    assert 'encode/rnn1/fwd/cudnn_gru/rnn/multi_rnn_cell/cell_0/cudnn_compatible_gru_cell/gates/kernel' in names
    assert 'train/decode/rnn/cudnn_gru/opaque_kernel/Adam_1' in names
    m2 = _vae(cfg, {k: np.zeros_like(v) for k, v in P.items()})
    ckpt.restore(m2, prefix)                       # auto-detects the TF prefix
    assert m2.step == m.step
    assert np.abs(m2.encode(ids) - z0).max() <= 1e-6
    a, b = m.get_params(), m2.get_params()
    for k in a:
        if k.endswith('/bW') or k.endswith('/bR'):
            continue
        assert np.array_equal(a[k], b[k]), k
    from argsim_amd.model import ADAM_M, ADAM_V
    for kind in (ADAM_M, ADAM_V):
        sa, sb = m.get_params(kind), m2.get_params(kind)
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), (kind, k)
    # and training continues from the restored state like from the original
    m.train_step(ids, ids, keep_mask=keep, eps=eps)
    m2.train_step(ids, ids, keep_mask=keep, eps=eps)
    assert abs(m.losses()[2] - m2.losses()[2]) <= 1e-5 * abs(m.losses()[2])


def test_split_bf16_mode_ragged_batch_at_bench_scale():
    """ragged lengths at B=256, S=64, D=512, V=8192: the device-side row counts (dyn M / dyn K), the skipped tiles of
    the persistent wave-specialised kernel and the buffer-bound predicates of the fast staging path, against the
    exact-fp32 path on the same batch"""
    import torch
    from argsim_amd.model import VAE
    kw = dict(dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3, seed=0)
    rng = np.random.default_rng(3)
    lens = np.clip(np.round(rng.lognormal(np.log(24), 0.5, 256)), 2, 64).astype(int)
    ids = np.ones((256, 64), np.int32)                      # eos padded
    for b, n in enumerate(lens):
        ids[b, :n] = rng.integers(3, 8192, n)
    keep = (rng.random((int(lens.max()), 256)) < 0.88).astype(np.uint8)
    eps = rng.standard_normal((256, 128)).astype(np.float32)
    res = {}
    for dt in ('f32', 'f32s'):
        m = VAE('train', dtype=dt, **kw)
        m.step = 20000
        z = m.encode(ids)
        errt, lgen, lkld = m.eval(ids, ids)
        m.forward_backward(ids, ids, keep_mask=keep, eps=eps)
        res[dt] = (z, lgen, m.losses(), m.get_grads())
        del m
        torch.cuda.empty_cache()
    assert res['f32'][1].shape == (int(lens.sum()) + 256,)
    assert np.abs(res['f32'][0] - res['f32s'][0]).max() <= 2e-5
    assert np.abs(res['f32'][1] - res['f32s'][1]).max() <= 1e-4
    for a, b in zip(res['f32'][2], res['f32s'][2]):
        assert abs(a - b) <= 2e-6 * abs(a)
    bad = {k: rel_l2(res['f32s'][3][k], v) for k, v in res['f32'][3].items() if rel_l2(res['f32s'][3][k], v) > 1e-4}
    assert not bad, bad


@pytest.mark.parametrize("ragged", [False, True])
def test_bench_scale_backward_persistent_equals_stepwise(ragged):
    """B=256, S=64, D=512: gradients of the persistent GRU kernels (LDS-weight team kernels for the encoder, register
    form for the decoder) against one launch per step, on a FULL and on a ragged batch -- same arithmetic, so the
    difference is float-atomic ordering only"""
    import torch
    from argsim_amd import synth
    from argsim_amd.model import VAE
    kw = dict(dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3, seed=0)
    rng = np.random.default_rng(5)
    ids = synth.batch(256, 64, 8192, seed=1)
    if ragged:
        lens = np.clip(np.round(rng.lognormal(np.log(24), 0.5, 256)), 2, 64).astype(int)
        lens[0] = 64
        for b, n in enumerate(lens):
            ids[b, n:] = 1
    keep = (rng.random((64, 256)) < 0.88).astype(np.uint8)
    eps = rng.standard_normal((256, 128)).astype(np.float32)
    m = VAE('train', **kw)
    m.step = 20000
    out = {}
    for persistent in (1, 0):
        m.set_option('persistent', persistent)
        m.forward_backward(ids, ids, keep_mask=keep, eps=eps)
        out[persistent] = (m.losses(), m.get_grads())
    for x, y in zip(out[1][0], out[0][0]):              # (the two scalar loss sums are float atomics)
        assert abs(x - y) <= 2e-6 * abs(y)
    bad = {k: rel_l2(out[1][1][k], v) for k, v in out[0][1].items() if rel_l2(out[1][1][k], v) > 2e-6}
    assert not bad, bad
