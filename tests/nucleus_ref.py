"""float64 reference of nucleus sampling (include/argsim_vae.h, avae_decode_sample_p): numpy only.

The generator, the top-k set and the loop are sampling_ref's; only the nucleus is restated here, and in exact float64 shares of
mass instead of the device's 2^40 fixed-point weights: the distinct logit values of K0, descending, with cum_j = the share of
the mass at or above the j-th value; the reference set is the first j with cum_j >= top_p.  A device run is judged on ITS set:
nkept must be the size of a prefix of whole tie groups j', and its violation max(p - cum_j', cum_(j'-1) - p, 0) says by how much
of the mass that prefix is not the smallest one that holds top_p (0 for the reference's own set)."""
import contextlib

import numpy as np

import sampling_ref as sr


_top_k_position = sr.position          # (sample() below puts position() in its place for the time of a run)


def nucleus_on(T, top_k, top_p):
    return 0.0 < top_p < 1.0 and T != 0 and top_k != 1


def _shares(x, mask):
    """exp(x - max) over mask, the maximum itself exactly 1 (so +inf, and a row of -inf only, weigh 1 each); 0 outside"""
    m = x[mask].max() if mask.any() else -np.inf
    with np.errstate(invalid='ignore', over='ignore'):
        e = np.where(x == m, 1.0, np.exp(x - m))
    return np.where(mask, e, 0.0)


def nucleus(l, x, k0, top_p):
    """l (V) float64 logits without NaN, x = l / T, k0 (V) bool: the set the nucleus is taken of
    -> dict: values (distinct l over k0, descending), sizes (tokens in the first j + 1 tie groups), cum (share of mass at or above
    values[j]), j (the reference's group), kept (V bool), cum_j, cum_jm1, bmargin = min(cum_j - p, p - cum_(j-1))"""
    if not k0.any():
        return dict(values=np.zeros(0), sizes=np.zeros(0, int), cum=np.zeros(0), j=-1, kept=k0.copy(), cum_j=1.0, cum_jm1=0.0, bmargin=np.inf)
    e = _shares(x, k0)
    values, inv, counts = np.unique(l[k0], return_inverse=True, return_counts=True)
    values, counts = values[::-1], counts[::-1]
    mass = np.bincount(len(values) - 1 - inv, weights=e[k0], minlength=len(values))
    cum = np.cumsum(mass) / mass.sum()
    cum[-1] = 1.0
    j = int(np.argmax(cum >= top_p))
    cjm1 = float(cum[j - 1]) if j else 0.0
    return dict(values=values, sizes=np.cumsum(counts), cum=cum, j=j, kept=k0 & (l >= values[j]), cum_j=float(cum[j]), cum_jm1=cjm1,
                bmargin=float(min(cum[j] - top_p, top_p - cjm1)))


def over(p, kept):
    """the fields of sampling_ref.position that depend on the kept set, over `kept`: token, scores, kept, margin, logp (NaN where
    there is no number to choose: every score -inf)"""
    V = len(kept)
    sc = np.where(kept, p['raw_scores'], -np.inf)
    two = np.partition(sc, V - 2)[V - 2:] if V > 1 else np.array([-np.inf, sc[0]])
    with np.errstate(invalid='ignore'):
        margin = float(two[1] - two[0]) if two[1] > -np.inf else 0.0
    if sc.max() == -np.inf:
        logp = np.full(V, np.nan)
    else:
        xm = np.where(kept, p['x'], -np.inf)
        mx = xm.max()
        with np.errstate(invalid='ignore', divide='ignore'):
            logp = np.where(xm == mx, 0.0, xm - mx) - np.log(_shares(p['x'], kept).sum())
        logp[~kept] = -np.inf
    return dict(token=int(np.argmax(sc)), scores=sc, kept=kept, margin=margin, logp=logp)


def position(l, T, top_k, top_p, seed, r, t):
    """sampling_ref.position with the nucleus: the same dict over the nucleus' set, plus 'nucleus' (the dict of nucleus(), None
    when the nucleus is off) and 'nkept' (the size of the kept set, -1 when off); with the nucleus on also l (the logits, NaN as
    -inf), k0 and top_p, for judge().  A NaN logit is absent."""
    l = np.asarray(l, np.float64)
    nan = np.isnan(l)
    p = _top_k_position(np.where(nan, -np.inf, l), T, top_k, seed, r, t)
    if not nucleus_on(T, top_k, top_p):
        p.update(nucleus=None, nkept=-1)
        return p
    lc, k0 = np.where(nan, -np.inf, l), p['kept'] & ~nan
    nu = nucleus(lc, p['x'], k0, top_p)
    p.update(over(p, nu['kept']), nucleus=nu, nkept=int(nu['kept'].sum()), l=lc, k0=k0, top_p=top_p)
    return p


def judge(p, nkept, tok):
    """a device's (nkept, token) at the position p = position(...) with the nucleus on -> dict: viol (inf: nkept is no prefix of whole
    tie groups; the other figures are then over the reference's set), same (the device's set is the reference's), logp (float64,
    of the device token over the device's set), win / margin (the Gumbel winner over the device's set and its top-2 margin),
    deficit (best score over that set - the device token's; inf outside the set), tie (the device's prefix ends BEHIND the reference's
    group: how far its last value lies under the reference's last one, in l / T -- two logits that are one tie group in fp32 and two in
    float64 make the device keep the second with the first; inf where the prefix ends elsewhere)"""
    nu, top_p = p['nucleus'], p['top_p']
    hit = np.flatnonzero(nu['sizes'] == nkept)
    tie = np.inf
    if len(hit) == 0:
        o, viol, same = p, np.inf, False
    else:
        jd = int(hit[0])
        o = over(p, p['k0'] & (p['l'] >= nu['values'][jd]))
        viol = float(max(top_p - nu['cum'][jd], (nu['cum'][jd - 1] if jd else 0.0) - top_p, 0.0))
        same = jd == nu['j']
        if jd > nu['j']:
            tie = float(p['x'][p['l'] == nu['values'][nu['j']]][0] - p['x'][p['l'] == nu['values'][jd]][0])
    with np.errstate(invalid='ignore'):
        deficit = float(o['scores'][o['token']] - o['scores'][tok]) if o['kept'][tok] else np.inf
    return dict(viol=viol, same=same, logp=float(o['logp'][tok]), win=o['token'], margin=o['margin'], deficit=deficit, tie=tie)


@contextlib.contextmanager
def _position_of(fn):
    """sampling_ref.sample looks its position() up when it runs: run it with fn in that place"""
    old = sr.position
    sr.position = fn
    try:
        yield
    finally:
        sr.position = old


FIELDS = ('bmargin', 'nkept_ref', 'viol', 'same', 'logp_set', 'win', 'margin_set', 'deficit_set', 'tie')


def sample(P, cfg, z, steps, T=1.0, top_k=0, top_p=0.0, seed=0, replay=None, nkept=None):
    """sampling_ref.sample with the nucleus (its dict, over the reference's set), plus (b, n_pos) arrays: bmargin, nkept_ref, and
    with replay and the device's nkept (b, >= n_pos) the figures of judge(): viol, same, logp_set, win, margin_set, deficit_set, tie"""
    on = nucleus_on(T, top_k, top_p)
    rec = {}

    def pos(l, T_, k_, seed_, r, t):
        p = position(l, T_, k_, top_p, seed_, r, t)
        d = dict(bmargin=p['nucleus']['bmargin'] if on else np.inf, nkept_ref=p['nkept'])
        if replay is not None and nkept is not None and on:
            tok = int(replay[r, t]) if t < replay.shape[1] else cfg['eos']
            jd = judge(p, int(nkept[r, t]), tok)
            d.update(viol=jd['viol'], same=jd['same'], logp_set=jd['logp'], win=jd['win'], margin_set=jd['margin'], deficit_set=jd['deficit'], tie=jd['tie'])
        rec[(r, t)] = d
        return p

    with _position_of(pos):
        res = sr.sample(P, cfg, z, steps, T, top_k, seed, replay=replay)
    b, n_pos = res['live'].shape
    for k in FIELDS:
        a = np.zeros((b, n_pos))
        for (r, t), d in rec.items():
            if k in d:
                a[r, t] = d[k]
        res[k] = a
    res['bmargin'][~res['live']] = np.inf
    res['tie'][~res['live']] = np.inf
    return res
