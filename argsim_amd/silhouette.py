"""Cluster-quality scores of latent rows on the device (include/argsim_vae.h, avae_silhouette): scikit-learn's silhouette_samples /
silhouette_score, calinski_harabasz_score and davies_bouldin_score for MANY labelings of the same rows in ONE call -- every pair distance
is formed once and binned for all of them.  The labelings are whatever kmeans, ward_cut, affinity or gold ids give; a negative label
leaves a row out of that labeling (one labeling per topic with the other topics' rows at -1 scores every topic in the same call).

    silhouette_raw(vae, x, cfg, label, K, want)        the C entry as it stands
    silhouette(vae, z, labels, metric, ...)            dict(score, ch, db, n_clusters, counts, clusters[, samples, a, b, nearest])
    sweep_k(vae, z, ks, metric, ...)                   one kmeans call per k, ONE silhouette call over all of them -> the table, the best k
"""
import ctypes as C

import numpy as np

METRICS = {'euclidean': 0, 'cosine': 1, 'sqeuclidean': 2}
MAX_ROWS, MAX_K, MAX_L = 1 << 18, 4096, 64
WANT = ('sil', 'ab', 'nearest', 'count', 'cluster_mean', 'index')


def silhouette_raw(vae, x, cfg, label, K, want=WANT):
    """avae_silhouette: x (N, dim) float32, numpy or a tensor on the device; cfg a lib.AvaeSilhouetteConfig; label (L, N) int32; K (L)
    int32 on the host; want: the optional outputs to ask for -> dict(score (L,) float64 and, as asked, sil (L, N), ab (L, N, 2), nearest
    (L, N) int32, count (L, Kmax) int32, cluster_mean (L, Kmax), index (L, 2) = CH, DB)"""
    import torch
    N, dim = x.shape
    dev = vae.device
    L = cfg.L
    K = np.ascontiguousarray(K, np.int32)
    kmax = int(K.max())
    dx = x if isinstance(x, torch.Tensor) else torch.as_tensor(x)
    dx = dx.to(dev).contiguous()
    dl = torch.as_tensor(np.ascontiguousarray(label, np.int32).reshape(L, N)).to(dev)
    shapes = dict(sil=((L, N), torch.float64), ab=((L, N, 2), torch.float64), nearest=((L, N), torch.int32), count=((L, kmax), torch.int32),
                  cluster_mean=((L, kmax), torch.float64), index=((L, 2), torch.float64))
    score = torch.zeros((L,), dtype=torch.float64, device=dev)
    t = {n: (torch.zeros(s, dtype=dt, device=dev) if n in want else None) for n, (s, dt) in shapes.items()}
    ptr = lambda v: C.c_void_p(v.data_ptr()) if v is not None else None
    vae._stream()
    vae._ck(vae._l.avae_silhouette(vae._h, ptr(dx), N, dim, C.byref(cfg), ptr(dl), K.ctypes.data_as(C.POINTER(C.c_int32)), ptr(score),
                                   *[ptr(t[n]) for n in WANT]))
    out = dict(score=score.cpu().numpy())
    out.update({n: v.cpu().numpy() for n, v in t.items() if v is not None})
    return out


def _check_silhouette_args(z, labels, metric):
    import torch
    if not isinstance(z, (np.ndarray, torch.Tensor)):
        raise ValueError("z must be a numpy array or a torch tensor, got %s" % type(z).__name__)
    if z.dtype not in (np.float32, torch.float32):
        raise ValueError("z must be float32, got %s" % z.dtype)
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, got %r" % (sorted(METRICS), metric))
    if len(z.shape) != 2 or not 2 <= z.shape[0] <= MAX_ROWS:
        raise ValueError("z must be (rows, dim) with 2 <= rows <= 2^18, got %s" % (tuple(z.shape),))
    if not 1 <= z.shape[1] <= 1024:
        raise ValueError("z must have 1 <= dim <= 1024, got %s" % (tuple(z.shape),))
    lab = np.asarray(labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else labels)
    if lab.dtype.kind not in 'iu':
        raise ValueError("labels must be integers, got %s" % lab.dtype)
    if lab.ndim not in (1, 2) or lab.shape[-1] != z.shape[0]:
        raise ValueError("labels must be (rows,) or (L, rows) with rows = %d, got %s" % (z.shape[0], lab.shape))
    if lab.ndim == 2 and not 1 <= lab.shape[0] <= MAX_L:
        raise ValueError("at most 64 labelings per call, got %d" % lab.shape[0])
    return lab.astype(np.int64)


def _pad_cols(a, pad):
    return np.ascontiguousarray(np.pad(a, [(0, 0), (0, pad)]) if pad else a, dtype=np.float32)


def silhouette(vae, z, labels, metric='euclidean', return_samples=False, raw=silhouette_raw):
    """sklearn's silhouette_score, calinski_harabasz_score and davies_bouldin_score of the rows of z for every labeling in `labels`, (N,)
    or (L, N) integers, in ONE device call.  A negative label leaves the row out of that labeling; the other values of a labeling are
    compacted to 0 .. K - 1 on the host.  -> dict(score (L,), ch (L,), db (L,), n_clusters (L,), counts [(K_l,)], clusters [(K_l,) the
    original values]); with return_samples also samples, a, b (L, N) and nearest (L, N) in the original values (-1: none).  For (N,)
    labels every entry loses its leading axis.  metric: 'euclidean', 'cosine' or 'sqeuclidean'.  Like sklearn it raises ValueError for a
    labeling with fewer than 2 clusters or as many clusters as labelled rows.  A tensor on the device whose dim is a multiple of 4 is
    taken as it is; anything else is uploaded, its columns padded with zeros to a multiple of 4 (a zero column changes no distance)."""
    import torch
    from . import lib as _lib
    lab = _check_silhouette_args(z, labels, metric)
    single = lab.ndim == 1
    lab = np.atleast_2d(lab)
    L, N = lab.shape
    comp = np.full((L, N), -1, np.int32)
    clusters = []
    for l in range(L):
        on = lab[l] >= 0
        vals, inv = np.unique(lab[l][on], return_inverse=True)
        if not 2 <= len(vals) <= int(on.sum()) - 1:
            raise ValueError("labeling %d: the number of clusters is %d; it must be in [2, labelled rows - 1 = %d]" % (l, len(vals), int(on.sum()) - 1))
        if len(vals) > MAX_K:
            raise ValueError("labeling %d: at most 4096 clusters, got %d" % (l, len(vals)))
        comp[l][on] = inv
        clusters.append(vals)
    K = np.array([len(v) for v in clusters], np.int32)
    dim = z.shape[1]
    pad = -dim % 4
    if isinstance(z, torch.Tensor) and z.is_cuda and not pad:
        x = z.detach()
    else:
        x = _pad_cols(z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else z, pad)
    cfg = _lib.AvaeSilhouetteConfig(metric=METRICS[metric], L=L, reserved=0, reserved2=0)
    want = ('count', 'index') + (('sil', 'ab', 'nearest') if return_samples else ())
    res = raw(vae, x, cfg, comp, K, want=want)
    out = dict(score=res['score'], ch=res['index'][:, 0], db=res['index'][:, 1], n_clusters=K.astype(np.int64),
               counts=[res['count'][l, :K[l]].astype(np.int64) for l in range(L)], clusters=clusters)
    if return_samples:
        near = np.full((L, N), -1, np.int64)
        for l in range(L):
            m = res['nearest'][l] >= 0
            near[l][m] = clusters[l][res['nearest'][l][m]]
        out.update(samples=res['sil'], a=res['ab'][:, :, 0], b=res['ab'][:, :, 1], nearest=near)
    if single:
        out = {k: v[0] for k, v in out.items()}
    return out


def sweep_k(vae, z, ks, metric='euclidean', n_init=10, seed=0):
    """which k?  One vae.kmeans call per k in ks, then ONE silhouette call over all the labelings -> dict(k, score, ch, db (len(ks),),
    inertia, labels (len(ks), N), best = the k with the largest silhouette, the first of equals).  metric: 'euclidean' or 'cosine'"""
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= MAX_L:
        raise ValueError("between 1 and 64 values of k per sweep, got %d" % len(ks))
    runs = [vae.kmeans(z, k, metric, n_init=n_init, seed=seed) for k in ks]
    labels = np.stack([r['labels'] for r in runs])
    q = vae.silhouette(z, labels, metric)
    return dict(k=np.array(ks), score=q['score'], ch=q['ch'], db=q['db'], inertia=np.array([r['inertia'] for r in runs]), labels=labels,
                best=ks[int(np.argmax(q['score']))])
