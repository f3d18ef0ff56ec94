"""float64 reference of beam-search decoding (include/argsim_vae.h, avae_decode_beam): numpy only.

The decoder step is oracle.vae_numpy.decoder_rnn.  search() runs its own search, or REPLAYS a device lattice: then at every step the
hypotheses (their tokens, their states, and the float64 cum along their paths) are the device's, so every selection is judged on the
device's own history and one near-tie cannot cascade into another beam.  backtrack() is the host twin of the device's final ranking
and back-walk, in the arithmetic the contract names (fp32 cum, len^alpha in double rounded to fp32, fp32 division).

CASES / STEPS / params() are the models and shapes of tests/test_gpu_beam.py; tests/test_beam.py checks on the CPU that they are fit
to judge a device with (few near-ties at the selection boundary)."""
import math

import numpy as np

from helpers import make_case
from oracle import vae_numpy as vn

# (geometry, sentences, width, eos_lean).  tiny / mid: make_case; prod: V 8192, D 512, L 3.  widths 1, 2, 4, 8, 16 (32 on mid), b = 1, 5, 40;
# ('mid', 40, 32) has 1280 hypotheses: two groups of 32 and 8 sentences.  eos_lean > 0: hypotheses finish, at different steps.  The
# eos_lean of a case is the one of 0, 2, 3, 4 at which the reference's own search has the fewest selections closer to a tie than
# 1e-4 (t + 1) (tests/test_beam.py counts them: at most 1 % of a case's steps).
CASES = [('tiny', 4, 1, 0.0), ('tiny', 4, 2, 0.0), ('tiny', 4, 2, 3.0), ('tiny', 4, 4, 2.0), ('tiny', 4, 8, 2.0),
         ('mid', 1, 4, 3.0), ('mid', 5, 1, 2.0), ('mid', 5, 2, 0.0), ('mid', 5, 2, 4.0), ('mid', 5, 4, 2.0), ('mid', 5, 8, 4.0), ('mid', 5, 32, 4.0),
         ('mid', 40, 4, 3.0), ('mid', 40, 32, 4.0),
         ('prod', 1, 4, 3.0), ('prod', 5, 8, 3.0), ('prod', 5, 1, 0.0), ('prod', 1, 16, 3.0), ('prod', 40, 2, 4.0)]
STEPS = {'tiny': 16, 'mid': 16, 'prod': 12}
_PARAMS = {}


def first_logits(P, cfg, z):
    D, L = cfg['dim_emb'], cfg['rnn_layers']
    E = P['embed/embedding']
    h0 = np.asarray(z, np.float64) @ P['latent/ex/kernel'] + P['latent/ex/bias']
    hd, _ = vn.decoder_rnn(P, cfg, E[np.full((1, len(z)), cfg['bos'], np.int32)], np.stack([h0] * L))
    hd = hd.reshape(-1, D) @ P['decode/out/kernel'] + P['decode/out/bias']
    return hd @ ((D ** -0.5) * E.T)


def params(name, eos_lean=0.0):
    """(cfg, P, z (40, R)) of a geometry: the `out` affine scaled so that the first step's max |logit| is 8 (as tests/test_gpu_sampling.py
    does); eos_lean adds that much of the unit eos embedding to the out bias, so that hypotheses end"""
    key = (name, eos_lean)
    if key not in _PARAMS:
        if name == 'prod':
            cfg = vn.make_cfg(dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3)
            P = {k: v.astype(np.float32).astype(np.float64) for k, v in vn.init_params(cfg, 4, bias_scale=0.1).items()}
        else:
            cfg, P = make_case(name)[:2]
        z = np.random.default_rng(11).standard_normal((40, cfg['dim_rep'])).astype(np.float32)
        f = 8.0 / float(np.abs(first_logits(P, cfg, z)).max())
        for k in ('decode/out/kernel', 'decode/out/bias'):
            P[k] = (P[k] * f).astype(np.float32).astype(np.float64)
        if eos_lean:
            e = P['embed/embedding'][cfg['eos']]
            P['decode/out/bias'] = (P['decode/out/bias'] + eos_lean * np.sqrt(cfg['dim_emb']) * e / (e @ e)).astype(np.float32).astype(np.float64)
        _PARAMS[key] = (cfg, P, z)
    return _PARAMS[key]


def select(scores, valid, width, by=None):
    """the `width` best of the valid candidates of one sentence.  scores, valid: (Win, V).  Order: score descending, parent ascending,
    token ascending (a stable sort of the row-major candidates).  by: rank by these values instead (width 1: the logits themselves).
    -> (parent (width), token (width), score (width), gap = width-th minus (width+1)-th score, inf without a (width+1)-th)"""
    Win, V = scores.shape
    flat = np.flatnonzero(valid.ravel())
    key = (scores if by is None else by).ravel()[flat]
    order = flat[np.argsort(-key, kind='stable')]
    width = min(width, len(order))                        # (a beam wider than the candidates there are: the reference alone)
    top = order[:width]
    sc = scores.ravel()
    with np.errstate(invalid='ignore'):
        gap = float(sc[order[width - 1]] - sc[order[width]]) if len(order) > width else np.inf
    return top // V, top % V, sc[top], gap


def search(P, cfg, z, steps, width, replay=None):
    """the search over b sentences.  replay: (lat_parent, lat_token) of the device, (n, b, width) each; the loop then runs those n steps on
    the device's hypotheses.  Without replay the loop ends as the contract says (every slot finished, or steps).
    -> dict: n; per (sentence, step): gap (b, n), margin (b, n, width - 1) between neighbours of the reference's chosen set, ref_parent /
       ref_token / ref_score (b, n, width) the reference's choice in its order, kth (b, n) = ref_score[..., -1]; lat_parent, lat_token
       (n, b, width) and cum (n, b, width) float64: the lattice the loop FOLLOWED (the device's on replay, with the reference's float64 cum
       along the device's paths; -inf where the device took something that is no candidate); fin, len (b, width), seqs (b, width, n) the token paths and cum_last (b, width) after the last step.  (A width above the number of
       candidates of a step takes them all; the per-step entries then stay lists.)"""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    D, L, V, eos = cfg['dim_emb'], cfg['rnn_layers'], cfg['dim_tgt'], cfg['eos']
    E = P['embed/embedding']
    b, W = len(z), width
    n_cap = steps if replay is None else replay[0].shape[0]
    h0 = np.asarray(z, np.float64) @ P['latent/ex/kernel'] + P['latent/ex/bias']
    s = np.stack([h0] * L)                                   # (L, b * Win, D)
    x = np.full((b, 1), cfg['bos'], np.int32)                # last tokens (b, Win)
    cum = np.zeros((b, 1)); fin = np.zeros((b, 1), bool); ln = np.zeros((b, 1), np.int64)
    out = {k: [] for k in ('gap', 'margin', 'ref_parent', 'ref_token', 'ref_score', 'lat_parent', 'lat_token', 'cum')}
    n = 0
    seqs = np.zeros((b, 1, 0), np.int64)
    for t in range(n_cap):
        Win = x.shape[1]
        hd, s_new = vn.decoder_rnn(P, cfg, E[x.reshape(1, -1)], s)
        hd = hd.reshape(-1, D) @ P['decode/out/kernel'] + P['decode/out/bias']
        logits = (hd @ ((D ** -0.5) * E.T)).reshape(b, Win, V)
        mx = logits.max(-1, keepdims=True)
        logp = (logits - mx) - np.log(np.exp(logits - mx).sum(-1, keepdims=True))
        scores = cum[:, :, None] + logp
        valid = np.ones((b, Win, V), bool)
        for r, w in zip(*np.nonzero(fin)):                   # a finished hypothesis offers itself
            valid[r, w] = False; valid[r, w, eos] = True; scores[r, w, eos] = cum[r, w]
        col = {k: [] for k in out}
        Wt = min(W, int(valid.reshape(b, -1).sum(1).min()))
        par = np.zeros((b, Wt), np.int64); tok = np.zeros((b, Wt), np.int64); new_cum = np.zeros((b, Wt))
        for r in range(b):
            p, k, sc, gap = select(scores[r], valid[r], Wt, by=logits[r] if W == 1 else None)
            col['gap'].append(gap); col['margin'].append(sc[:-1] - sc[1:])
            col['ref_parent'].append(p); col['ref_token'].append(k); col['ref_score'].append(sc)
            if replay is not None:
                p, k = replay[0][t, r].astype(np.int64), replay[1][t, r].astype(np.int64)
                ok = (p >= 0) & (p < Win) & (k >= 0) & (k < V)
                p, k = np.where(ok, p, 0), np.where(ok, k, 0)
                sc = np.where(ok & valid[r, p, k], scores[r, p, k], -np.inf)
            par[r], tok[r], new_cum[r] = p, k, sc
        for key in ('gap', 'margin', 'ref_parent', 'ref_token', 'ref_score'):
            out[key].append(np.array(col[key]))
        out['lat_parent'].append(par.copy()); out['lat_token'].append(tok.copy()); out['cum'].append(new_cum.copy())
        rows = (np.arange(b)[:, None] * Win + par).ravel()
        s = s_new[:, rows]
        pf = np.take_along_axis(fin, par, 1)
        ln = np.where(pf, np.take_along_axis(ln, par, 1), np.take_along_axis(ln, par, 1) + 1)
        fin = pf | (tok == eos)
        cum, x = new_cum, tok.astype(np.int32)
        seqs = np.concatenate([np.take_along_axis(seqs, par[:, :, None], 1), tok[:, :, None]], 2)
        n = t + 1
        if replay is None and fin.all():
            break
    same = len({a.shape for a in out['lat_parent']}) == 1        # (the beam has `width` slots from the first step on)
    res = {k: np.stack(v, 1) if same else v for k, v in out.items() if k in ('gap', 'margin', 'ref_parent', 'ref_token', 'ref_score')}
    for k in ('lat_parent', 'lat_token', 'cum'):
        res[k] = np.stack(out[k], 0) if same else out[k]
    if same:
        res['kth'] = res['ref_score'][..., -1]
    res.update(n=n, fin=fin, len=ln, seqs=seqs, cum_last=cum)
    return res


def backtrack(lat_parent, lat_token, lat_cum, eos, length_alpha=0.0):
    """host twin of the device's end: lattice (n, b, width), lat_cum fp32 -> ids (b, width, n) best first, score, cum (b, width) fp32,
    len (b, width).  len: tokens up to and including the first eos of the path, n without one.  score = cum / fp32(len ** alpha) in fp32
    (cum itself at alpha 0); ranking: score descending, ties to the lower slot."""
    n, b, W = lat_parent.shape
    ids = np.full((b, W, n), eos, np.int32)
    for r in range(b):
        for j in range(W):
            slot = j
            for t in range(n - 1, -1, -1):
                ids[r, j, t] = lat_token[t, r, slot]
                slot = lat_parent[t, r, slot]
    is_eos = ids == eos
    ln = np.where(is_eos.any(-1), is_eos.argmax(-1) + 1, n).astype(np.int32)
    cum = np.asarray(lat_cum[n - 1], np.float32)
    if length_alpha:
        a = float(np.float32(length_alpha))                  # (libm pow in double on the fp32 alpha, rounded to fp32)
        score = cum / np.array([math.pow(float(v), a) for v in ln.ravel()]).reshape(ln.shape).astype(np.float32)
    else:
        score = cum.copy()
    order = np.stack([np.argsort(-score[r].astype(np.float64), kind='stable') for r in range(b)])
    take = lambda a: np.take_along_axis(a, order, 1)
    return np.take_along_axis(ids, order[:, :, None], 1), take(score), take(cum), take(ln)


def exhaustive(P, cfg, z1, steps):
    """every sequence of `steps` tokens of ONE sentence with the frozen-hypothesis rule (nothing but eos after an eos), scored in float64:
    -> (tokens (N, steps), cum (N)) in lexicographic token order"""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    D, L, V, eos = cfg['dim_emb'], cfg['rnn_layers'], cfg['dim_tgt'], cfg['eos']
    E = P['embed/embedding']
    h0 = np.asarray(z1, np.float64).reshape(1, -1) @ P['latent/ex/kernel'] + P['latent/ex/bias']
    seqs, cum, s = np.zeros((1, 0), np.int64), np.zeros(1), np.stack([h0] * L)
    x = np.full(1, cfg['bos'], np.int64)
    fin = np.zeros(1, bool)
    for t in range(steps):
        hd, s_new = vn.decoder_rnn(P, cfg, E[x.reshape(1, -1)], s)
        hd = hd.reshape(-1, D) @ P['decode/out/kernel'] + P['decode/out/bias']
        logits = hd @ ((D ** -0.5) * E.T)
        mx = logits.max(-1, keepdims=True)
        logp = (logits - mx) - np.log(np.exp(logits - mx).sum(-1, keepdims=True))
        par = np.concatenate([[i] if fin[i] else [i] * V for i in range(len(x))]).astype(np.int64)
        tok = np.concatenate([[eos] if fin[i] else np.arange(V) for i in range(len(x))]).astype(np.int64)
        add = np.concatenate([[0.0] if fin[i] else logp[i] for i in range(len(x))])
        seqs = np.concatenate([seqs[par], tok[:, None]], 1)
        cum = cum[par] + add
        fin = fin[par] | (tok == eos)
        s, x = s_new[:, par], tok
    return seqs, cum
