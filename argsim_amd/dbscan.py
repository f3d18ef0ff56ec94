"""Density clustering of latent rows on the device (include/argsim_vae.h, avae_dbscan): scikit-learn's DBSCAN(algorithm='brute') in ONE
call -- no cluster count, clusters of any shape, and the rows that belong to no cluster at -1, which VAE.silhouette takes as "left out".
The labels are an exact function of the rows: clusters are numbered by their lowest core row, a border row takes the lowest cluster number
among the core rows within eps of it.

    dbscan_raw(vae, x, cfg, want_count)                the C entry as it stands
    dbscan(vae, z, eps, min_samples, metric, ...)      dict(labels, core_sample_indices, n_clusters, n_noise, n_border, counts, rounds)
    kdist(vae, z, k, metric)                           the ascending k-distance curve (VAE.neighbors): the usual way to pick eps
    sweep_eps(vae, z, eps_list, ...)                   one dbscan call per eps, ONE silhouette call over all of them -> the table, the best eps
"""
import ctypes as C
import math

import numpy as np

METRICS = {'euclidean': 0, 'cosine': 1}
MAX_ROWS, MAX_ROUNDS, MAX_EPS = 1 << 17, 4096, 64


def dbscan_raw(vae, x, cfg, want_count=True):
    """avae_dbscan: x (N, dim) float32, numpy or a tensor on the device; cfg a lib.AvaeDbscanConfig -> dict(label (N,) int32, stat (8,)
    int32 and, with want_count, count (N,) int32)"""
    import torch
    N, dim = x.shape
    dev = vae.device
    dx = x if isinstance(x, torch.Tensor) else torch.as_tensor(x)
    dx = dx.to(dev).contiguous()
    label = torch.zeros((N,), dtype=torch.int32, device=dev)
    stat = torch.zeros((8,), dtype=torch.int32, device=dev)
    count = torch.zeros((N,), dtype=torch.int32, device=dev) if want_count else None
    ptr = lambda v: C.c_void_p(v.data_ptr()) if v is not None else None
    vae._stream()
    vae._ck(vae._l.avae_dbscan(vae._h, ptr(dx), N, dim, C.byref(cfg), ptr(label), ptr(count), ptr(stat)))
    out = dict(label=label.cpu().numpy(), stat=stat.cpu().numpy())
    if want_count:
        out['count'] = count.cpu().numpy()
    return out


def _check_dbscan_args(z, eps, min_samples, metric, max_rounds=0):
    import torch
    if not isinstance(z, (np.ndarray, torch.Tensor)):
        raise ValueError("z must be a numpy array or a torch tensor, got %s" % type(z).__name__)
    if z.dtype not in (np.float32, torch.float32):
        raise ValueError("z must be float32, got %s" % z.dtype)
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, got %r" % (sorted(METRICS), metric))
    if len(z.shape) != 2 or not 1 <= z.shape[0] <= MAX_ROWS:
        raise ValueError("z must be (rows, dim) with 1 <= rows <= 2^17, got %s" % (tuple(z.shape),))
    if not 1 <= z.shape[1] <= 1024:
        raise ValueError("z must have 1 <= dim <= 1024, got %s" % (tuple(z.shape),))
    if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)) or not (eps > 0 and math.isfinite(eps)):
        raise ValueError("eps must be a finite number > 0, got %r" % (eps,))
    if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)) or not 1 <= min_samples < (1 << 31):
        raise ValueError("min_samples must be an integer >= 1, got %r" % (min_samples,))
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or not 0 <= max_rounds <= MAX_ROUNDS:
        raise ValueError("max_rounds must be an integer in [0, 4096] (0: the planner's default), got %r" % (max_rounds,))


def _pad_cols(a, pad):
    return np.ascontiguousarray(np.pad(a, [(0, 0), (0, pad)]) if pad else a, dtype=np.float32)


def dbscan(vae, z, eps, min_samples=5, metric='euclidean', max_rounds=0, raw=dbscan_raw):
    """sklearn's DBSCAN(eps, min_samples, metric, algorithm='brute') of the rows of z in ONE device call -> dict(labels (N,) int64 with
    -1 = noise, core_sample_indices, n_clusters, n_noise, n_border, counts (N,) = the rows within eps of a row, itself included, rounds =
    the rounds the components took).  metric: 'euclidean' or 'cosine' (1 - cos <= eps).  max_rounds: 0 for the planner's default;
    RuntimeError if the components had not settled within it.  A tensor on the device whose dim is a multiple of 4 is taken as it is;
    anything else is uploaded, its columns padded with zeros to a multiple of 4 (a zero column changes no pair value)."""
    import torch
    from . import lib as _lib
    _check_dbscan_args(z, eps, min_samples, metric, max_rounds)
    pad = -z.shape[1] % 4
    if isinstance(z, torch.Tensor) and z.is_cuda and not pad:
        x = z.detach()
    else:
        x = _pad_cols(z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else z, pad)
    cfg = _lib.AvaeDbscanConfig(metric=METRICS[metric], min_samples=int(min_samples), max_rounds=int(max_rounds), reserved=0, eps=float(eps))
    res = raw(vae, x, cfg, want_count=True)
    stat = res['stat']
    if stat[5]:
        raise RuntimeError("dbscan: the components had not settled after %d rounds; call again with a larger max_rounds (it was %s)"
                           % (int(stat[4]), max_rounds if max_rounds else "the planner's default"))
    counts = res['count'].astype(np.int64)
    return dict(labels=res['label'].astype(np.int64), core_sample_indices=np.flatnonzero(counts >= min_samples), n_clusters=int(stat[0]),
                n_noise=int(stat[3]), n_border=int(stat[2]), counts=counts, rounds=int(stat[4]))


def kdist(vae, z, k, metric='euclidean'):
    """the ascending curve of every row's distance to its k-th nearest OTHER row (VAE.neighbors, exclude_self): eps is usually read off
    its knee.  'euclidean': the distance; 'cosine': 1 - cos, from the normalised rows' squared distance / 2"""
    import torch
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, got %r" % (sorted(METRICS), metric))
    if len(z.shape) != 2 or z.shape[0] < 2:
        raise ValueError("z must be (rows, dim) with at least 2 rows, got %s" % (tuple(z.shape),))
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= min(32, z.shape[0] - 1):
        raise ValueError("k must be an integer in [1, min(32, rows - 1) = %d], got %r" % (min(32, z.shape[0] - 1), k))
    if isinstance(z, torch.Tensor) and z.is_cuda and z.dtype == torch.float32 and metric == 'euclidean' and z.shape[1] % 4 == 0:
        _, d2 = vae.neighbors(z.detach(), z.detach(), k=int(k), metric='euc', exclude_self=True, return_distance=True)      # in place
        return np.sort(np.sqrt(np.maximum(d2[:, k - 1].double().cpu().numpy(), 0.0)))
    x = z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else np.asarray(z)
    x = np.asarray(x, np.float32)
    if metric == 'cosine':
        rn = np.sqrt((x.astype(np.float64) ** 2).sum(1))
        x = np.divide(x, rn[:, None], out=np.zeros(x.shape, np.float64), where=rn[:, None] > 0).astype(np.float32)
    x = _pad_cols(x, -x.shape[1] % 4)
    _, d2 = vae.neighbors(x, x, k=int(k), metric='euc', exclude_self=True, return_distance=True)
    d2 = np.maximum(np.asarray(d2, np.float64)[:, k - 1], 0.0)
    return np.sort(d2 / 2.0 if metric == 'cosine' else np.sqrt(d2))


def sweep_eps(vae, z, eps_list, min_samples=5, metric='euclidean'):
    """which eps?  One vae.dbscan call per eps in eps_list (at most 64), then ONE vae.silhouette call over the labelings that have
    2 <= clusters <= labelled rows - 1, noise left at -1 (left out of the scores) -> dict(eps, n_clusters, n_noise, score, ch, db
    (len(eps_list),), NaN where a labeling cannot be scored, labels (len(eps_list), N), best = the eps with the largest silhouette, the first
    of equals, None if none can be scored)"""
    eps_list = [float(e) for e in eps_list]
    if not 1 <= len(eps_list) <= MAX_EPS:
        raise ValueError("between 1 and 64 values of eps per sweep, got %d" % len(eps_list))
    runs = [vae.dbscan(z, e, min_samples, metric) for e in eps_list]
    labels = np.stack([r['labels'] for r in runs])
    ok = [i for i, r in enumerate(runs) if 2 <= r['n_clusters'] <= int((r['labels'] >= 0).sum()) - 1]
    score, ch, db = (np.full(len(eps_list), np.nan) for _ in range(3))
    if ok:
        q = vae.silhouette(z, labels[ok], metric)
        score[ok], ch[ok], db[ok] = q['score'], q['ch'], q['db']
    best = eps_list[int(np.nanargmax(score))] if ok else None
    return dict(eps=np.array(eps_list), n_clusters=np.array([r['n_clusters'] for r in runs]), n_noise=np.array([r['n_noise'] for r in runs]),
                score=score, ch=ch, db=db, labels=labels, best=best)
