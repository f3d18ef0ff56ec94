"""Ward clustering of latent rows: the clustering evaluation of the reference's src/eval_clustering.py:82-103 (AgglomerativeClustering,
Ward linkage, per selection; adjusted Rand score and V-measure) with the trees built on the device (include/argsim_vae.h, avae_ward).
Everything here is the host side, numpy in float64:

    gather_groups(groups, N)            the row order and group_off of one avae_ward call
    linkage_matrix(pair, delta, size)   a group's merges as scipy's Z (cluster ids n + t, height sqrt(2 Delta))
    relabel(slots)                      slot labels -> 0 .. k - 1 by first appearance
    adjusted_rand(a, b), v_measure(a, b)
    ward(vae, z, groups), ward_cut(vae, res, k), cluster_eval(vae, z, gold, groups)
"""
import ctypes as C

import numpy as np

MAX_GROUP = 1 << 15
MAX_GROUPS = 1 << 16


def gather_groups(groups, N):
    """groups: None (all N rows, one group keyed 0), an (N,) array of group labels (a partition; groups in order of first appearance)
    or a dict {key: row numbers} (selections that may overlap) -> (keys, rows, group_off): rows[g] the row numbers of group g in
    ascending order (a dict's in the order given), group_off (G + 1) int32 their running count"""
    if groups is None:
        keys, rows = [0], [np.arange(N)]
    elif isinstance(groups, dict):
        keys, rows = list(groups), [np.asarray(groups[k]) for k in groups]
        for k, r in zip(keys, rows):
            if r.ndim != 1 or not np.issubdtype(r.dtype, np.integer) or (len(r) and (r.min() < 0 or r.max() >= N)):
                raise ValueError("group %r must be a 1-d integer array of row numbers in [0, %d)" % (k, N))
    else:
        groups = np.asarray(groups)
        if groups.shape != (N,):
            raise ValueError("groups must be (N,) = (%d,), got %s" % (N, groups.shape))
        uniq, first, inv = np.unique(groups, return_index=True, return_inverse=True)
        order = np.argsort(first)
        keys = [uniq[i].item() if hasattr(uniq[i], 'item') else uniq[i] for i in order]
        rows = [np.flatnonzero(inv == i) for i in order]
    if not 1 <= len(keys) <= MAX_GROUPS:
        raise ValueError("between 1 and 2^16 groups per call, got %d" % len(keys))
    for k, r in zip(keys, rows):
        if not 1 <= len(r) <= MAX_GROUP:
            raise ValueError("group %r has %d rows: a group holds between 1 and 2^15" % (k, len(r)))
    off = np.zeros(len(keys) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    if off[-1] > (1 << 31) - 1:
        raise ValueError("at most 2^31 - 1 gathered rows per call")
    return keys, rows, off.astype(np.int32)


def linkage_matrix(pair, delta, size):
    """the merges of ONE group (slots a < b, Delta, member counts) -> scipy's linkage matrix Z (n - 1, 4) float64: the two cluster
    ids (leaves 0 .. n - 1, merge t makes cluster n + t; the smaller id first), the height sqrt(2 Delta), the member count"""
    pair, delta, size = np.asarray(pair), np.asarray(delta, np.float64), np.asarray(size)
    n = pair.shape[0] + 1
    cid = np.arange(n)
    Z = np.zeros((n - 1, 4))
    for t, (a, b) in enumerate(pair):
        Z[t] = (min(cid[a], cid[b]), max(cid[a], cid[b]), np.sqrt(2.0 * delta[t]), size[t])
        cid[a] = n + t
    return Z


def relabel(slots):
    """labels -> 0 .. k - 1 in order of first appearance"""
    slots = np.asarray(slots)
    _, first, inv = np.unique(slots, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[inv.reshape(slots.shape)]


def _contingency(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 1 or a.shape != b.shape:
        raise ValueError("two label arrays of one length, got %s and %s" % (a.shape, b.shape))
    _, ia = np.unique(a, return_inverse=True)
    _, ib = np.unique(b, return_inverse=True)
    M = np.zeros((ia.max() + 1 if len(ia) else 0, ib.max() + 1 if len(ib) else 0), np.int64)
    np.add.at(M, (ia, ib), 1)
    return M


def adjusted_rand(a, b):
    """sklearn.metrics.adjusted_rand_score: from the pair counts, in exact integers until the last division"""
    M = _contingency(a, b)
    n = int(M.sum())
    same_both = sum(int(v) * int(v) for v in M.ravel()) - n          # ordered pairs together in both
    same_a = sum(int(v) ** 2 for v in M.sum(1)) - n
    same_b = sum(int(v) ** 2 for v in M.sum(0)) - n
    tp, fp, fn = same_both, same_b - same_both, same_a - same_both
    tn = n * (n - 1) - tp - fp - fn
    if fn == 0 and fp == 0:
        return 1.0
    return 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def _entropy(counts):
    c = np.asarray(counts, np.float64)
    c = c[c > 0]
    n = c.sum()
    return float(-(c / n * (np.log(c) - np.log(n))).sum()) if len(c) else 0.0


def v_measure(a, b):
    """sklearn.metrics.v_measure_score (beta = 1): the harmonic mean of homogeneity and completeness, natural logarithms"""
    M = _contingency(a, b).astype(np.float64)
    if M.size == 0:
        return 1.0
    n, ra, cb = M.sum(), M.sum(1), M.sum(0)
    ha, hb = _entropy(ra), _entropy(cb)
    i, j = np.nonzero(M)
    v = M[i, j]
    # conditional entropies, so that a perfect clustering scores exactly 1: H(a | b) = -sum n_ij / n log(n_ij / b_j)
    h_ab = max(float(-(v / n * (np.log(v) - np.log(cb[j]))).sum()), 0.0)
    h_ba = max(float(-(v / n * (np.log(v) - np.log(ra[i]))).sum()), 0.0)
    hom = max(1.0 - h_ab / ha, 0.0) if ha else 1.0
    com = max(1.0 - h_ba / hb, 0.0) if hb else 1.0
    return 0.0 if hom + com == 0.0 else 2.0 * hom * com / (hom + com)


def _check_rows(z):
    import torch
    if not isinstance(z, (np.ndarray, torch.Tensor)):
        raise ValueError("z must be a numpy array or a torch tensor, got %s" % type(z).__name__)
    if z.dtype not in (np.float32, torch.float32):
        raise ValueError("z must be float32, got %s" % z.dtype)
    if len(z.shape) != 2 or z.shape[0] < 1 or not 1 <= z.shape[1] <= 1024:
        raise ValueError("z must be (rows, dim) with at least one row and 1 <= dim <= 1024, got %s" % (tuple(z.shape),))


def gathered(z, rows):
    """the rows of every group one after the other, as float32 numpy; the columns padded with zeros to a multiple of 4 (a zero
    column changes no distance)"""
    import torch
    x = z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else z
    x = x[np.concatenate(rows)]
    pad = -x.shape[1] % 4
    return np.ascontiguousarray(np.pad(x, ((0, 0), (0, pad))) if pad else x, dtype=np.float32)


def ward_raw(vae, x, group_off):
    """avae_ward as it stands: x (N, dim) float32 numpy, group_off (G + 1) int32 -> (pair (N - G, 2), delta, size) numpy"""
    import torch
    from . import lib as _lib
    N, G = x.shape[0], len(group_off) - 1
    dx = torch.as_tensor(x).to(vae.device)
    pair = torch.zeros((max(N - G, 1), 2), dtype=torch.int32, device=vae.device)
    delta = torch.zeros((max(N - G, 1),), dtype=torch.float32, device=vae.device)
    size = torch.zeros((max(N - G, 1),), dtype=torch.int32, device=vae.device)
    off = (C.c_int32 * (G + 1))(*[int(v) for v in group_off])
    wc = _lib.AvaeWardConfig()
    vae._stream()
    vae._ck(vae._l.avae_ward(vae._h, C.c_void_p(dx.data_ptr()), x.shape[1], off, G, C.byref(wc), C.c_void_p(pair.data_ptr()),
                             C.c_void_p(delta.data_ptr()), C.c_void_p(size.data_ptr())))
    return pair.cpu().numpy()[:N - G], delta.cpu().numpy()[:N - G], size.cpu().numpy()[:N - G]


def cut_raw(vae, pair, group_off, k):
    """avae_ward_cut: pair (N - G, 2) int32 numpy as ward_raw returned it, k (G) -> slot labels (N,) int32 of the gathered rows"""
    import torch
    G, N = len(group_off) - 1, int(group_off[-1])
    dp = torch.as_tensor(np.ascontiguousarray(pair, dtype=np.int32).reshape(-1, 2)).to(vae.device)
    if dp.shape[0] == 0:
        dp = torch.zeros((1, 2), dtype=torch.int32, device=vae.device)
    label = torch.zeros((N,), dtype=torch.int32, device=vae.device)
    off = (C.c_int32 * (G + 1))(*[int(v) for v in group_off])
    ks = (C.c_int32 * G)(*[int(v) for v in k])
    vae._stream()
    vae._ck(vae._l.avae_ward_cut(vae._h, C.c_void_p(dp.data_ptr()), off, G, ks, C.c_void_p(label.data_ptr())))
    return label.cpu().numpy()


def split_result(keys, rows, group_off, pair, delta, size):
    """the call's outputs per group -> {key: dict(rows, pair, delta, size, Z)}"""
    out = {}
    for g, key in enumerate(keys):
        lo, hi = int(group_off[g]) - g, int(group_off[g + 1]) - g - 1
        p, d, s = pair[lo:hi], delta[lo:hi], size[lo:hi]
        out[key] = dict(rows=rows[g], pair=p, delta=d, size=s, Z=linkage_matrix(p, d, s))
    return out


def ward(vae, z, groups=None, raw=ward_raw):
    """the Ward tree of every group of rows of z in ONE device call -> dict(keys, group_off, groups {key: dict(rows, pair, delta,
    size, Z)}): pair the merged slots a < b (positions within rows), delta the increase of the within-cluster sum of squares, size
    the member count, Z scipy's linkage matrix of the group"""
    _check_rows(z)
    keys, rows, off = gather_groups(groups, z.shape[0])
    pair, delta, size = raw(vae, gathered(z, rows), off)
    return dict(keys=keys, group_off=off, groups=split_result(keys, rows, off, pair, delta, size), n_rows=z.shape[0])


def _per_group(res, k):
    keys = res['keys']
    if isinstance(k, dict):
        k = [k[key] for key in keys]
    elif np.ndim(k) == 0:
        k = [k] * len(keys)
    k = [int(v) for v in k]
    if len(k) != len(keys):
        raise ValueError("k must be one number, one per group or a dict by group key")
    for key, v in zip(keys, k):
        n = len(res['groups'][key]['rows'])
        if not 1 <= v <= n:
            raise ValueError("group %r: k must be in [1, %d], got %d" % (key, n, v))
    return k


def ward_cut(vae, res, k, raw=cut_raw):
    """the clusters after cutting every group's tree of `res` (ward's result) at k clusters (one number, one per group in res['keys']
    order, or a dict by key) -> {key: labels 0 .. k - 1 by first appearance, aligned with that group's rows}"""
    k = _per_group(res, k)
    off = res['group_off']
    pair = np.concatenate([res['groups'][key]['pair'] for key in res['keys']], axis=0)
    slots = raw(vae, pair, off, k)
    return {key: relabel(slots[off[g]:off[g + 1]]) for g, key in enumerate(res['keys'])}


def cluster_eval(vae, z, gold, groups=None, raw=ward_raw, raw_cut=cut_raw):
    """src/eval_clustering.py:95-102 for every group at once: Ward clusters, as many as the group has distinct gold labels, scored
    against them -> {key: (adjusted Rand score, V-measure)}"""
    gold = np.asarray(gold)
    if gold.shape != (z.shape[0],):
        raise ValueError("gold must be (N,) = (%d,), got %s" % (z.shape[0], gold.shape))
    res = ward(vae, z, groups, raw)
    k = {key: len(np.unique(gold[res['groups'][key]['rows']])) for key in res['keys']}
    labels = ward_cut(vae, res, k, raw_cut)
    return {key: (adjusted_rand(gold[res['groups'][key]['rows']], labels[key]), v_measure(gold[res['groups'][key]['rows']], labels[key]))
            for key in res['keys']}
