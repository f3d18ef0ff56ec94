"""Affinity propagation of latent rows: the explorative clustering of the reference's src/eval_clustering_explorative.py:69-132
(AffinityPropagation on Euclidean and on cosine similarities, the distances to the cluster centroids, the per-topic purity listing)
with the clustering itself on the device (include/argsim_vae.h, avae_affinity).

    affinity_raw(vae, x, cfg, ...)      the C entry as it stands
    affinity(vae, z, metric, ...)       dict(labels 0 .. K - 1 in ascending exemplar row or all -1, exemplars, n_iter, converged)
    centroids, dist_to_centroids, purity      host helpers, numpy in float64
    decode_centroids(vae, z, labels)    the cluster centroids through the greedy decoder (src/explore_centroids.py)
"""
import ctypes as C

import numpy as np

METRICS = {'euclidean': 0, 'cosine': 1, 'precomputed': 2}
MAX_ROWS = 1 << 14


def affinity_raw(vae, x, cfg, want_s=False, messages=False, a=None, r=None):
    """avae_affinity: x (N, dim) float32 numpy, cfg an lib.AvaeAffinityConfig -> dict(label (N,) int32 rows of the exemplars or -1,
    stat (4,) int32 = iterations, converged, K, 0; with want_s `s` (N, N); with messages (or a and r given, which a warm start
    reads) `a` and `r`)"""
    import torch
    N, dim = x.shape
    dev = vae.device
    dx = torch.as_tensor(x).to(dev)
    label = torch.zeros((N,), dtype=torch.int32, device=dev)
    stat = torch.zeros((4,), dtype=torch.int32, device=dev)
    s = torch.zeros((N, N), dtype=torch.float32, device=dev) if want_s else None
    da = dr = None
    if messages or a is not None:
        da = torch.zeros((N, N), dtype=torch.float32, device=dev) if a is None else torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dev)
        dr = torch.zeros((N, N), dtype=torch.float32, device=dev) if r is None else torch.as_tensor(np.ascontiguousarray(r, np.float32)).to(dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    vae._stream()
    vae._ck(vae._l.avae_affinity(vae._h, ptr(dx), N, dim, C.byref(cfg), ptr(label), ptr(stat), ptr(s), ptr(da), ptr(dr)))
    out = dict(label=label.cpu().numpy(), stat=stat.cpu().numpy())
    if s is not None:
        out['s'] = s.cpu().numpy()
    if da is not None:
        out['a'], out['r'] = da.cpu().numpy(), dr.cpu().numpy()
    return out


def _check_affinity_args(z, metric, preference, damping, max_iter, convergence_iter, seed):
    import torch
    if not isinstance(z, (np.ndarray, torch.Tensor)):
        raise ValueError("z must be a numpy array or a torch tensor, got %s" % type(z).__name__)
    if z.dtype not in (np.float32, torch.float32):
        raise ValueError("z must be float32, got %s" % z.dtype)
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, got %r" % (sorted(METRICS), metric))
    if len(z.shape) != 2 or not 1 <= z.shape[0] <= MAX_ROWS:
        raise ValueError("z must be (rows, dim) with 1 <= rows <= 2^14, got %s" % (tuple(z.shape),))
    if metric == 'precomputed':
        if z.shape[0] != z.shape[1]:
            raise ValueError("a precomputed similarity matrix must be square, got %s" % (tuple(z.shape),))
    elif not 1 <= z.shape[1] <= 1024:
        raise ValueError("z must have 1 <= dim <= 1024, got %s" % (tuple(z.shape),))
    if preference is not None and not np.isfinite(preference):
        raise ValueError("preference must be None (the median similarity) or a finite number, got %r" % (preference,))
    if not 0.5 <= damping < 1:
        raise ValueError("damping must be in [0.5, 1), got %r" % (damping,))
    if not (isinstance(max_iter, (int, np.integer)) and 1 <= max_iter <= 10000):
        raise ValueError("max_iter must be an integer in [1, 10000], got %r" % (max_iter,))
    if not (isinstance(convergence_iter, (int, np.integer)) and 1 <= convergence_iter <= max_iter):
        raise ValueError("convergence_iter must be an integer in [1, max_iter], got %r" % (convergence_iter,))
    if not (isinstance(seed, (int, np.integer)) and 0 <= seed < 1 << 64):
        raise ValueError("seed must be an integer in [0, 2^64), got %r" % (seed,))


def rows_of(z, metric):
    """z as float32 numpy; the columns of rows padded with zeros to a multiple of 4 (a zero column changes neither similarity)"""
    import torch
    from . import cluster
    if metric != 'precomputed':
        return cluster.gathered(z, [np.arange(z.shape[0])])
    return np.ascontiguousarray(z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else z, dtype=np.float32)


def affinity(vae, z, metric='euclidean', preference=None, damping=0.5, max_iter=200, convergence_iter=15, seed=0, noise=True,
             return_messages=False, raw=affinity_raw):
    """sklearn's AffinityPropagation(damping, max_iter, convergence_iter, preference) of the rows of z in ONE device call ->
    dict(labels (N,) 0 .. K - 1 in ascending exemplar row, all -1 without exemplars; exemplars (K,) ascending rows; n_iter; converged),
    with return_messages also s, a, r (N, N)"""
    from . import lib as _lib
    _check_affinity_args(z, metric, preference, damping, max_iter, convergence_iter, seed)
    cfg = _lib.AvaeAffinityConfig(metric=METRICS[metric], max_iter=int(max_iter), convergence_iter=int(convergence_iter),
                                  use_preference=0 if preference is None else 1, noise=1 if noise else 0, warm=0, damping=float(damping),
                                  preference=0.0 if preference is None else float(preference), seed=int(seed))
    res = raw(vae, rows_of(z, metric), cfg, want_s=return_messages, messages=return_messages)
    label = res['label']
    exemplars = np.unique(label[label >= 0]).astype(np.int64)
    out = dict(labels=np.where(label >= 0, np.searchsorted(exemplars, label), -1).astype(np.int64), exemplars=exemplars,
               n_iter=int(res['stat'][0]), converged=bool(res['stat'][1]))
    if return_messages:
        out.update(s=res['s'], a=res['a'], r=res['r'])
    return out


def _clusters(labels):
    labels = np.asarray(labels)
    if labels.ndim != 1:
        raise ValueError("labels must be (N,), got %s" % (labels.shape,))
    return np.unique(labels)


def centroids(z, labels):
    """-> (cluster labels ascending, (K, dim) float64 means of the member rows)"""
    z = np.asarray(z, np.float64)
    ids = _clusters(labels)
    if z.ndim != 2 or z.shape[0] != len(labels):
        raise ValueError("z must be (N, dim) with one row per label, got %s" % (z.shape,))
    return ids, np.stack([z[np.asarray(labels) == c].mean(0) for c in ids]) if len(ids) else np.zeros((0, z.shape[1]))


def dist_to_centroids(z, labels, metric='sqeuclidean'):
    """every row's distance to the centroid of its cluster, in the original row order: 'sqeuclidean' |z - c|^2 or 'cosine'
    1 - z.c / (|z||c|) (scipy.spatial.distance's definitions)"""
    if metric not in ('sqeuclidean', 'cosine'):
        raise ValueError("metric must be 'sqeuclidean' or 'cosine', got %r" % (metric,))
    z = np.asarray(z, np.float64)
    ids, ctr = centroids(z, labels)
    c = ctr[np.searchsorted(ids, np.asarray(labels))]
    if metric == 'sqeuclidean':
        return ((z - c) ** 2).sum(1)
    with np.errstate(invalid='ignore', divide='ignore'):
        return 1.0 - (z * c).sum(1) / (np.sqrt((z * z).sum(1)) * np.sqrt((c * c).sum(1)))


def purity(pred, mask, min_acc=0.5, min_cnt=2):
    """the clusters that lie mostly inside a selection of rows -> [(cluster, members, share of the members inside mask)] for the
    clusters with share >= min_acc and members >= min_cnt, by descending share (stable: first appearance breaks ties)"""
    pred, mask = np.asarray(pred), np.asarray(mask, bool)
    if pred.shape != mask.shape or pred.ndim != 1:
        raise ValueError("pred and mask must be (N,), got %s and %s" % (pred.shape, mask.shape))
    order = list(dict.fromkeys(pred.tolist()))
    rows = [(c, int((pred == c).sum()), int((pred[mask] == c).sum())) for c in order]
    rows = sorted(((c, n, hit / n) for c, n, hit in rows), key=lambda t: -t[2])
    return [(c, n, acc) for c, n, acc in rows if min_acc <= acc and min_cnt <= n]


def decode_centroids(vae, z, labels, steps=512):
    """the sentences at the cluster centroids -> (cluster labels, what model.decode returns for the (K, dim) centroid rows)"""
    from . import model
    ids, ctr = centroids(z, labels)
    return ids, model.decode(vae, ctr.astype(np.float32), steps=steps)
