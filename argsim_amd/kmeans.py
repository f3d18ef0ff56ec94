"""K-means of latent rows on the device (include/argsim_vae.h, avae_kmeans): scikit-learn's KMeans(algorithm='lloyd') with greedy
k-means++ seeding, n_init restarts side by side in ONE call, Euclidean or cosine (spherical).  The labels are what
affinity.decode_centroids and affinity.dist_to_centroids take.

    kmeans_raw(vae, x, cfg, centers_in, want_all)      the C entry as it stands
    kmeans(vae, z, k, ...)                             dict(labels, centers, inertia, n_iter, stop, best, inertias, relocations)
"""
import ctypes as C

import numpy as np

METRICS = {'euclidean': 0, 'cosine': 1}
STOPS = ('converged', 'tol', 'max_iter')
MAX_ROWS, MAX_K, MAX_INIT, MAX_ITER = 1 << 22, 4096, 64, 10000


def kmeans_raw(vae, x, cfg, centers_in=None, want_all=False):
    """avae_kmeans: x (N, dim) float32, numpy or a tensor on the device; cfg a lib.AvaeKmeansConfig; centers_in (n_init, k, dim) float32
    with cfg.init = 1 -> dict(label (N,) int32, centers (k, dim) float32, stat (4,) int32, inertia (n_init,) float64; with want_all
    label_all (n_init, N), centers_all (n_init, k, dim) float64, stat_all (n_init, 4))"""
    import torch
    N, dim = x.shape
    dev = vae.device
    k, R = cfg.k, cfg.n_init
    dx = x if isinstance(x, torch.Tensor) else torch.as_tensor(x)
    dx = dx.to(dev).contiguous()
    dc = None if centers_in is None else torch.as_tensor(np.ascontiguousarray(centers_in, np.float32)).to(dev)
    label = torch.zeros((N,), dtype=torch.int32, device=dev)
    centers = torch.zeros((k, dim), dtype=torch.float32, device=dev)
    stat = torch.zeros((4,), dtype=torch.int32, device=dev)
    inertia = torch.zeros((R,), dtype=torch.float64, device=dev)
    la = torch.zeros((R, N), dtype=torch.int32, device=dev) if want_all else None
    ca = torch.zeros((R, k, dim), dtype=torch.float64, device=dev) if want_all else None
    sa = torch.zeros((R, 4), dtype=torch.int32, device=dev) if want_all else None
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    vae._stream()
    vae._ck(vae._l.avae_kmeans(vae._h, ptr(dx), N, dim, C.byref(cfg), ptr(dc), ptr(label), ptr(centers), ptr(stat), ptr(inertia), ptr(la),
                               ptr(ca), ptr(sa)))
    out = dict(label=label.cpu().numpy(), centers=centers.cpu().numpy(), stat=stat.cpu().numpy(), inertia=inertia.cpu().numpy())
    if want_all:
        out.update(label_all=la.cpu().numpy(), centers_all=ca.cpu().numpy(), stat_all=sa.cpu().numpy())
    return out


def _check_kmeans_args(z, k, metric, n_init, max_iter, tol, seed, init):
    import torch
    if not isinstance(z, (np.ndarray, torch.Tensor)):
        raise ValueError("z must be a numpy array or a torch tensor, got %s" % type(z).__name__)
    if z.dtype not in (np.float32, torch.float32):
        raise ValueError("z must be float32, got %s" % z.dtype)
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, got %r" % (sorted(METRICS), metric))
    if len(z.shape) != 2 or not 1 <= z.shape[0] <= MAX_ROWS:
        raise ValueError("z must be (rows, dim) with 1 <= rows <= 2^22, got %s" % (tuple(z.shape),))
    if not 1 <= z.shape[1] <= 1024:
        raise ValueError("z must have 1 <= dim <= 1024, got %s" % (tuple(z.shape),))
    if not (isinstance(k, (int, np.integer)) and 1 <= k <= min(z.shape[0], MAX_K)):
        raise ValueError("k must be an integer in [1, min(rows, 4096)], got %r" % (k,))
    if not (isinstance(n_init, (int, np.integer)) and 1 <= n_init <= MAX_INIT):
        raise ValueError("n_init must be an integer in [1, 64], got %r" % (n_init,))
    if not (isinstance(max_iter, (int, np.integer)) and 1 <= max_iter <= MAX_ITER):
        raise ValueError("max_iter must be an integer in [1, 10000], got %r" % (max_iter,))
    if not (isinstance(tol, (int, float, np.floating, np.integer)) and tol >= 0):
        raise ValueError("tol must be a number >= 0, got %r" % (tol,))
    if not (isinstance(seed, (int, np.integer)) and 0 <= seed < 1 << 64):
        raise ValueError("seed must be an integer in [0, 2^64), got %r" % (seed,))
    if isinstance(init, str):
        if init != 'k-means++':
            raise ValueError("init must be 'k-means++' or an array of centres, got %r" % (init,))
    else:
        shape = tuple(np.shape(init))
        if shape not in ((k, z.shape[1]), (n_init, k, z.shape[1])):
            raise ValueError("init centres must be (k, dim) or (n_init, k, dim) = %s, got %s" % ((n_init, k, z.shape[1]), shape))


def _pad_cols(a, pad):
    return np.ascontiguousarray(np.pad(a, [(0, 0)] * (a.ndim - 1) + [(0, pad)]) if pad else a, dtype=np.float32)


def kmeans(vae, z, k, metric='euclidean', n_init=10, max_iter=300, tol=1e-4, seed=0, init='k-means++', return_all=False, raw=kmeans_raw):
    """sklearn's KMeans(k, n_init, max_iter, tol, algorithm='lloyd') of the rows of z in ONE device call -> dict(labels (N,) int64,
    centers (k, dim) float32, inertia, n_iter, stop 'converged' | 'tol' | 'max_iter', best, inertias (n_init,), relocations); with
    return_all also labels_all (n_init, N), centers_all (n_init, k, dim) float64 and stats_all [(n_iter, stop, relocations)].  init:
    'k-means++' (greedy, from seed) or the centres, (k, dim) -- one restart -- or (n_init, k, dim).  A tensor on the device whose dim is a
    multiple of 4 is taken as it is; anything else is uploaded, its columns padded with zeros to a multiple of 4 (a zero column changes no
    distance; tol is scaled so that its absolute value is that of the unpadded rows)."""
    import torch
    from . import lib as _lib
    given = not isinstance(init, str)
    if given and np.ndim(init) in (2, 3):                   # the centres say how many restarts there are
        n_init = 1 if np.ndim(init) == 2 else int(np.shape(init)[0])
    _check_kmeans_args(z, k, metric, n_init, max_iter, tol, seed, init)
    dim = z.shape[1]
    pad = -dim % 4
    if isinstance(z, torch.Tensor) and z.is_cuda and not pad:
        x = z.detach()
    else:
        x = _pad_cols(z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else z, pad)
    cin = None
    if given:
        cin = init.detach().cpu().numpy() if isinstance(init, torch.Tensor) else np.asarray(init)
        cin = _pad_cols(cin.astype(np.float32).reshape(n_init, k, dim), pad)
    cfg = _lib.AvaeKmeansConfig(k=int(k), n_init=int(n_init), max_iter=int(max_iter), metric=METRICS[metric], init=1 if given else 0,
                                reserved=0, tol=float(tol) * (dim + pad) / dim, seed=int(seed))
    res = raw(vae, x, cfg, cin, want_all=return_all)
    stat = res['stat']
    out = dict(labels=res['label'].astype(np.int64), centers=res['centers'][:, :dim], inertia=float(res['inertia'][stat[0]]), n_iter=int(stat[1]),
               stop=STOPS[stat[2]], best=int(stat[0]), inertias=res['inertia'], relocations=int(stat[3]))
    if return_all:
        out.update(labels_all=res['label_all'].astype(np.int64), centers_all=res['centers_all'][:, :, :dim],
                   stats_all=[(int(s[0]), STOPS[s[1]], int(s[2])) for s in res['stat_all']])
    return out
