"""shared fixtures for the parity tests: seeded ragged batches and oracle parameter sets."""
import numpy as np

from oracle import vae_numpy as vn

CASES = {
    # name: (cfg kwargs, B, S, lens or None(full))
    'tiny':  (dict(dim_tgt=32, dim_emb=16, dim_rep=8, rnn_layers=3), 4, 7, [7, 1, 3, 5]),
    'mid':   (dict(dim_tgt=256, dim_emb=64, dim_rep=32, rnn_layers=3), 8, 16, [16, 2, 9, 16, 1, 5, 12, 7]),
    'wide':  (dict(dim_tgt=512, dim_emb=256, dim_rep=64, rnn_layers=2), 20, 9, None),
    'full2': (dict(dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3), 2, 64, [64, 23]),
    # five word ids for 288 tokens: every id owns several 32-row segments of the grouped embedding-gradient scatter
    'hot':   (dict(dim_tgt=8, dim_emb=16, dim_rep=8, rnn_layers=1), 24, 12, None),
    # more tokens than vocabulary entries: the layers fed by embedding rows project the table and gather / scatter by id
    'tab':   (dict(dim_tgt=64, dim_emb=64, dim_rep=16, rnn_layers=2), 12, 10, [10, 3, 7, 10, 1, 5, 9, 2, 10, 6, 4, 8]),
    # the other widths the register-form GRU kernels are instantiated for (dim_emb 32 and 128)
    'd32':   (dict(dim_tgt=128, dim_emb=32, dim_rep=16, rnn_layers=2), 6, 9, [9, 1, 4, 9, 2, 7]),
    'd128':  (dict(dim_tgt=384, dim_emb=128, dim_rep=48, rnn_layers=3), 10, 11, [11, 2, 6, 11, 1, 9, 4, 8, 3, 10]),
    # a vocabulary beyond the scatter's LDS histogram: the per-element atomic fallback
    'bigv':  (dict(dim_tgt=12800, dim_emb=16, dim_rep=8, rnn_layers=1), 4, 6, [6, 2, 4, 1]),
}
# production geometry (D = 512, V = 8192, B = 64: one full 64-row block per GRU workgroup, so the LDS-weight team
# kernels, the fast-staging and split-K GEMM paths run).  Too large for the live float64 oracle inside a test:
# compared with committed reduced fixtures only (tests/golden/make_oracle_golden.py).
PROD_CASES = {
    'prod64':  (dict(dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3), 64, 64, 'ragged'),
    'prod128': (dict(dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3), 64, 128, 'ragged'),
}
# round 3: what the BIG configurations run, reduced fixtures only.  Fifth field: extras
#   prod512  B = 512: every GRU launch is a row-block-pipelined (PIPE) team instantiation, fp32 and bf16 (configs[2]/[3])
#   cfg0     the reference's own config.json dims (R = 1024, src/config.json:10-21) through backward
#   cfg4     BASELINE configs[4]: R = 512 with the beta / free-bits extension live
#   headline the bench batch itself: B 256 x S 64 FULL Zipf ids of argsim_amd.synth (seed 0), step 20000
BIG_CASES = {
    'prod512':  (dict(dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3), 512, 14, 'ragged', {}),
    'cfg0':     (dict(dim_tgt=8192, dim_emb=512, dim_rep=1024, rnn_layers=3), 32, 64, 'ragged', {}),
    'cfg4':     (dict(dim_tgt=8192, dim_emb=512, dim_rep=512, rnn_layers=3), 64, 32, 'ragged', dict(kl_beta=0.5, free_bits=0.02)),
    'headline': (dict(dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3), 256, 64, 'synth', {}),
    # round 4: a batch WITHOUT a team-kernel geometry of its own -- 100 rows run in the 128-slot geometry with 28 phantom
    # rows, the compact layout whatever the fill, table-fed first layers below the vocabulary size (1 200 tokens >= 1 024)
    'phantom100': (dict(dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3), 100, 12, 'ragged', {}),
    # BASELINE configs[0] as worded: src/config.json dims, batch 32, rows 0..31 of the 1 000 IAC posts encoded with the 8k SentencePiece
    # model trained in the build container and capped to 64 pieces (tests/golden/make_configs0_golden.py)
    'cfg0real': (dict(dim_tgt=8192, dim_emb=512, dim_rep=1024, rnn_layers=3), 32, 64, 'configs0', {}),
}


def big_extras(name):
    return dict(BIG_CASES[name][4])


def make_case(name, seed=0, pad=2, bias_scale=0.1):
    kw, B, S, lens = (CASES.get(name) or PROD_CASES.get(name) or BIG_CASES[name][:4])
    return make_batch(kw, B, S, lens, seed, pad, bias_scale)


def make_batch(kw, B, S, lens, seed=0, pad=2, bias_scale=0.1):
    """the batch of make_case for a geometry that is in none of the tables above (tests/step_routes.py)"""
    cfg = vn.make_cfg(**kw)
    rng = np.random.default_rng(seed + 17)
    V, R = cfg['dim_tgt'], cfg['dim_rep']
    ids = np.full((B, S + pad), cfg['eos'], np.int32)
    if lens is None:
        lens = [S] * B
    elif lens == 'ragged':             # a few full rows, a length-1 row, the rest uniform in [2, S]
        lens = rng.integers(2, S + 1, B)
        lens[[0, B // 2]] = S
        lens[1] = 1
    if isinstance(lens, str) and lens == 'configs0':   # real text: the committed ids of tests/golden/configs0_ids.npz
        import os
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'configs0_ids.npz'), allow_pickle=False) as f:
            real = f['ids'][:B].astype(np.int32)
        ids[:, :S] = real
        lens = [int((r != cfg['eos']).sum()) for r in real]
    elif isinstance(lens, str) and lens == 'synth':      # the bench batch (FULL Zipf rows), eos-padded like every other case
        from argsim_amd import synth
        ids[:, :S] = synth.batch(B, S, V, seed=0)
        lens = [S] * B
    else:
      for b, n in enumerate(lens):
        ids[b, :n] = rng.integers(3, V, n)
    smax = max(lens)
    keep = (rng.random((smax, B)) < 0.6).astype(np.uint8)
    eps = rng.standard_normal((B, R)).astype(np.float32)
    P = vn.init_params(cfg, seed, bias_scale=bias_scale)
    P = {k: v.astype(np.float32).astype(np.float64) for k, v in P.items()}   # exactly representable in fp32
    return cfg, P, ids, keep, eps


def rel_l2(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    d = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (d if d > 0 else 1.0)


def grad_blocks(got, want, tol, rows=16):
    """the per-block gradient criterion: a variable flattened to (shape[0], -1) and cut into blocks of `rows` leading rows (16 rows = one
    hidden tile of one gate in the natural layout get_grads() returns; a bias vector: 16 elements) -> (err, bound) per block,
    err = |got_blk - want_blk|, bound = tol * max(|want_blk|, |want| * sqrt(blk.size / want.size)): the tolerance relative to the block's
    own norm or to its fair share of the variable's norm, whichever is larger.  Where the reference is exactly zero the bound is zero."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    got, want = got.reshape(want.shape[0], -1), want.reshape(want.shape[0], -1)
    edges = np.arange(0, want.shape[0], rows)
    err = np.sqrt(np.add.reduceat(((got - want) ** 2).sum(1), edges))
    blk = np.sqrt(np.add.reduceat((want ** 2).sum(1), edges))
    size = np.diff(np.append(edges, want.shape[0])) * want.shape[1]
    return err, tol * np.maximum(blk, np.linalg.norm(want) * np.sqrt(size / want.size))


def grad_blocks_bad(got, want, tol, rows=16):
    """-> [(block index, err, bound)] of the blocks of grad_blocks that miss their bound (a non-finite error misses it)"""
    err, bound = grad_blocks(got, want, tol, rows)
    return [(int(i), float(err[i]), float(bound[i])) for i in np.flatnonzero(~(err <= bound))]


def grad_blocks_ratio(got, want, tol, rows=16):
    """the worst err / bound over the blocks of grad_blocks (0 / 0 = 0, x / 0 = inf: an exact zero of the reference must be an exact zero)"""
    err, bound = grad_blocks(got, want, tol, rows)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(np.where(np.isnan(r), np.inf, r)))


def grads_bad(got, want, tol):
    """every variable of a gradient set through grad_blocks_bad: 16-row blocks, and single rows (one token id each) for the embedding
    -> {(name, rows): [(block, err, bound)]} of the variables with a bad block"""
    bad = {}
    for k in want:
        for rows in ((16, 1) if k == 'embed/embedding' else (16,)):
            b = grad_blocks_bad(got[k], want[k], tol, rows)
            if b:
                bad[(k, rows)] = b[:8]
    return bad


def ce_scale(inv_n, n_dev, n_max):
    """the gradient scale softmax_ce applies (kernels.h CeArgs): inv_n itself (as the fp32 value the kernel receives), or
    1 / n over the rows it processes, n = min(n_max, *n_dev), when inv_n <= 0"""
    if inv_n > 0:
        return float(np.float32(inv_n))
    return 1.0 / max(min(n_max, n_dev), 1)


def softmax_ce_reference(x, labels, scale):
    """float64 restatement of model.py:170-181 on the given logit values, row by row (torch tensors, any device).
    x: (n, V) logits -- pass the values the kernel reads (an fp16 panel widened exactly); labels: (n,) ints.
    -> loss = logsumexp(x) - x[label], pred = FIRST argmax, errt = (pred != label), grad = (softmax(x) - onehot(label)) * scale."""
    import torch
    x = x.to(torch.float64)
    labels = labels.to(device=x.device, dtype=torch.long)
    m = x.max(-1, keepdim=True).values
    e = torch.exp(x - m)
    s = e.sum(-1, keepdim=True)
    loss = (m + torch.log(s))[:, 0] - x.gather(1, labels[:, None])[:, 0]
    col = torch.arange(x.shape[1], device=x.device).expand_as(x)
    pred = torch.where(x == m, col, torch.full_like(col, x.shape[1])).min(-1).values      # the first maximum, whatever argmax does on ties
    errt = (pred != labels).to(torch.float64)
    grad = e / s
    grad[torch.arange(x.shape[0], device=x.device), labels] -= 1.0
    return loss, pred, errt, grad * scale
