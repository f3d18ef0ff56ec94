"""float64 reference of sampled decoding (include/argsim_vae.h, avae_decode_sample): numpy only.

The counter generator (mix64, the 23-bit uniform of stream 3) is restated in uint64 arithmetic; the decoder step is
oracle.vae_numpy.decoder_rnn.  sample() runs the loop on its own tokens, or REPLAYS given tokens (the device's): then
every position is judged with the device's own history, so that one near-tie cannot cascade into another continuation."""
import numpy as np

from oracle import vae_numpy as vn

M64 = (1 << 64) - 1
STREAM = 3 * 0xD6E8FEB86659FD93 & M64


def mix64(x):
    """splitmix64 finaliser on uint64 arrays (wrapping)"""
    x = np.asarray(x, np.uint64)
    with np.errstate(over='ignore'):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def u23(x):
    """the uniform of a 64-bit draw: ((x >> 41) + 0.5) 2^-23, exact in fp32 (and float64), strictly inside (0, 1)"""
    return ((np.asarray(x, np.uint64) >> np.uint64(41)).astype(np.float64) + 0.5) * 2.0 ** -23


def draws(seed, r, t, V):
    """the V 64-bit draws of row r, step t"""
    assert V <= 1 << 20 and 0 <= t < 1 << 20
    key = mix64(np.array([(int(seed) ^ STREAM) & M64], np.uint64))
    idx = np.uint64((((int(r) << 20) + int(t)) << 20) & M64) + np.arange(V, dtype=np.uint64)
    with np.errstate(over='ignore'):
        return mix64(key + idx)


def gumbel(seed, r, t, V):
    return -np.log(-np.log(u23(draws(seed, r, t, V))))


def kept_set(l, top_k):
    """{v: l[v] >= k-th largest}, ties kept; everything for top_k = 0 or >= V.  -> (mask, gap = l_(k) - l_(k+1), inf without top-k)"""
    V = len(l)
    if not 0 < top_k < V:
        return np.ones(V, bool), np.inf
    srt = np.sort(l)[::-1]
    with np.errstate(invalid='ignore'):               # (-inf) - (-inf): no gap to speak of
        return l >= srt[top_k - 1], float(srt[top_k - 1] - srt[top_k])


def position(l, T, top_k, seed, r, t):
    """one row's step from its float64 logits l -> dict: token, scores (V, -inf outside the kept set), kept, margin (top-2 score gap),
    gap ((l_(k) - l_(k+1)) / T, inf without top-k), logp (V: log-softmax of l / T over the kept set, -inf outside)"""
    V = len(l)
    if T == 0:
        top_k, Tn = 0, 1.0
    else:
        Tn = float(T)
    kept, gap = kept_set(l, top_k)
    x = l / Tn
    noise = T != 0 and top_k != 1
    sc = x + gumbel(seed, r, t, V) if noise else l.copy()
    raw = sc.copy()
    sc[~kept] = -np.inf
    tok = int(np.argmax(sc))                          # numpy: the first maximum
    two = np.partition(sc, V - 2)[V - 2:] if V > 1 else np.array([-np.inf, sc[0]])
    xm = np.where(kept, x, -np.inf)
    mx = xm.max()
    logp = xm - (mx + np.log(np.exp(xm - mx).sum()))
    return dict(token=tok, scores=sc, raw_scores=raw, kept=kept, margin=float(two[1] - two[0]), gap=gap / Tn, logp=logp, x=x)


def sample(P, cfg, z, steps, T=1.0, top_k=0, seed=0, replay=None, full=False):
    """the sampled loop.  replay: (b, n) device tokens (eos-padded rows as avae_decode_sample returns them, n <= steps) fed as the lead
    ids instead of the reference's own; the loop then runs n + 1 positions (capped at steps): the last one is the closing eos of the
    longest rows.
    -> dict of (b, n_pos) arrays: token (the reference's choice given the history), margin, gap, logp_ref (at the reference's token),
       live (the row had not finished before the position); with replay also dev (the device token judged), logp_dev (the reference's
       logp at it, over the reference's kept set), deficit (best score - the device token's raw score), below ((k-th largest l - l[dev]) / 1,
       <= 0 when the device token is in the kept set); n_steps; with full=True also 'pos': the position() dicts [r][t]."""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    D, L, eos = cfg['dim_emb'], cfg['rnn_layers'], cfg['eos']
    E = P['embed/embedding']
    b = len(z)
    n_pos = steps if replay is None else min(replay.shape[1] + 1, steps)
    x = np.full((1, b), cfg['bos'], np.int32)
    h0 = np.asarray(z, np.float64) @ P['latent/ex/kernel'] + P['latent/ex/bias']
    s = np.stack([h0] * L)
    fin = np.zeros(b, bool)
    keys = ('token', 'margin', 'gap', 'logp_ref', 'live', 'dev', 'logp_dev', 'deficit', 'below')
    out = {k: [] for k in keys}
    pos = [[] for _ in range(b)]
    n_steps = steps
    for t in range(n_pos):
        hd, s = vn.decoder_rnn(P, cfg, E[x], s)
        hd = hd.reshape(-1, D) @ P['decode/out/kernel'] + P['decode/out/bias']
        logits = hd @ ((D ** -0.5) * E.T)
        col = {k: np.zeros(b) for k in keys}
        nxt = np.full(b, eos, np.int32)
        for r in range(b):
            col['live'][r] = not fin[r]
            if fin[r]:
                col['token'][r] = col['dev'][r] = eos
                col['margin'][r] = col['gap'][r] = np.inf
                pos[r].append(None)
                continue
            p = position(logits[r], T, top_k, seed, r, t)
            col['token'][r], col['margin'][r], col['gap'][r] = p['token'], p['margin'], p['gap']
            col['logp_ref'][r] = p['logp'][p['token']]
            nxt[r] = p['token']
            if replay is not None:
                d = int(replay[r, t]) if t < replay.shape[1] else eos
                mx = np.where(p['kept'], p['x'], -np.inf)
                col['dev'][r] = d
                col['logp_dev'][r] = p['x'][d] - (mx.max() + np.log(np.exp(mx - mx.max()).sum()))
                col['deficit'][r] = p['scores'][p['token']] - p['raw_scores'][d]
                col['below'][r] = logits[r][p['kept']].min() - logits[r][d]
                nxt[r] = d
            if full:
                pos[r].append(p)
            else:
                pos[r].append(None)
        for k in keys:
            out[k].append(col[k])
        fin |= nxt == eos
        x = nxt.reshape(1, b)
        if fin.all():
            n_steps = t
            break
    res = {k: np.stack(v, 1) for k, v in out.items()}
    res['token'] = res['token'].astype(np.int32)
    res['dev'] = res['dev'].astype(np.int32)
    res['live'] = res['live'].astype(bool)
    res['n_steps'] = n_steps
    if full:
        res['pos'] = pos
    return res


def ids_of(res, eos):
    """the reference's own run as avae_decode_sample returns it: (b, n_steps), eos after a row's end"""
    tok = res['token'][:, :res['n_steps']].copy()
    tok[~res['live'][:, :res['n_steps']]] = eos
    return tok
