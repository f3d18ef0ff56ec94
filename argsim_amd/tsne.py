"""Exact t-SNE of latent rows: the embedding plot of the reference's src/eval_clustering_explorative.py:45-66
(TSNE(n_components=2, perplexity=40, n_iter=20000) over the post embeddings, scattered by topic) with the whole fit on the device
(include/argsim_vae.h, avae_tsne).

    tsne_raw(vae, x, cfg, ...)      the C entry as it stands
    tsne(vae, z, perplexity, ...)   dict(y (N, 2), kl, n_iter, stop; optionally p, beta, trace)
    pca_init(z)                     sklearn's init='pca' start, numpy in float64
    plot(path, y, topics)           the reference's scatter by topic, through matplotlib's Agg backend

The reference's era of sklearn started at random: init='random' is what it ran.  A fit is chaotic -- two runs that differ in one
rounding part ways within a hundred iterations -- so runs are compared by their kl and their neighbourhoods, never point by point."""
import ctypes as C

import numpy as np

MAX_ROWS = 1 << 14
MAX_ITER = 1 << 15
STOPS = ('max_iter', 'no_progress', 'grad_norm')
COLOURS = {'obama': 'r', 'gayRights': 'b', 'abortion': 'g', 'marijuana': 'k'}      # the reference's; other topics take matplotlib's cycle


def tsne_raw(vae, x, cfg, p_in=None, y=None, want_p=False, want_beta=False, want_trace=False, want_grad=False, ug=None, prog=None, state=False):
    """avae_tsne: x (N, dim) float32 numpy or None with p_in (N, N) float64; cfg an lib.AvaeTsneConfig; y (N, 2) float32 the start of
    init 0 -> dict(y, kl (2), stat (4); with the flags p, beta, trace (2, max_iter), grad; with state (or ug and prog given, which a
    warm call reads) ug (2, N, 2) and prog (4))"""
    import torch
    dev = vae.device
    N = x.shape[0] if x is not None else p_in.shape[0]
    dim = x.shape[1] if x is not None else 0
    put = lambda v, dt: None if v is None else torch.as_tensor(np.ascontiguousarray(v, dt)).to(dev)
    new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    dx, dp = put(x, np.float32), put(p_in, np.float64)
    dy = new((N, 2), torch.float32) if y is None else put(y, np.float32)
    kl, stat = new((2,), torch.float64), new((4,), torch.int32)
    p = new((N, N), torch.float64) if want_p else None
    beta = new((N,), torch.float64) if want_beta and x is not None else None
    trace = new((2, max(cfg.max_iter, 1)), torch.float64) if want_trace else None
    grad = new((N, 2), torch.float32) if want_grad else None
    dug = dprog = None
    if state or ug is not None:
        dug = new((2, N, 2), torch.float32) if ug is None else put(ug, np.float32)
        dprog = new((4,), torch.float64) if prog is None else put(prog, np.float64)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    vae._stream()
    vae._ck(vae._l.avae_tsne(vae._h, ptr(dx), N, dim, C.byref(cfg), ptr(dp), ptr(dy), ptr(kl), ptr(stat), ptr(p), ptr(beta), ptr(trace),
                             ptr(grad), ptr(dug), ptr(dprog)))
    out = dict(y=dy.cpu().numpy(), kl=kl.cpu().numpy(), stat=stat.cpu().numpy())
    for name, t in (('p', p), ('beta', beta), ('trace', trace), ('grad', grad), ('ug', dug), ('prog', dprog)):
        if t is not None:
            out[name] = t.cpu().numpy()
    if trace is not None:
        out['trace'] = out['trace'][:, :cfg.max_iter]
    return out


def pca_init(z):
    """sklearn's init='pca': the first two principal components of the rows -- numpy's SVD of the centred rows in double, the signs
    fixed so that each left vector's entry of largest magnitude is positive -- scaled so that the first column's standard deviation is
    1e-4 -> (N, 2) float32"""
    x = np.asarray(z, np.float64)
    x = x - x.mean(0)
    U, S, _ = np.linalg.svd(x, full_matrices=False)
    k = min(2, U.shape[1])
    U, S = U[:, :k], S[:k]
    U = U * np.sign(U[np.abs(U).argmax(0), np.arange(k)])
    y = np.zeros((x.shape[0], 2))
    y[:, :k] = U * S
    sd = y[:, 0].std()
    return (y / sd * 1e-4 if sd > 0 else y).astype(np.float32)


def _is_int(v, lo, hi):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool) and lo <= v <= hi


def _check_tsne_args(z, perplexity, max_iter, init, seed, learning_rate, early_exaggeration, exaggeration_iter, n_iter_check,
                     n_iter_without_progress, min_grad_norm, p):
    import torch
    if p is not None:
        if not isinstance(p, np.ndarray) or p.dtype != np.float64 or p.ndim != 2 or p.shape[0] != p.shape[1]:
            raise ValueError("p must be a square float64 numpy array")
        N = p.shape[0]
        if z is not None and z.shape[0] != N:
            raise ValueError("p must be (rows, rows) for the rows of z")
    else:
        if not isinstance(z, (np.ndarray, torch.Tensor)):
            raise ValueError("z must be a numpy array or a torch tensor, got %s" % type(z).__name__)
        if z.dtype not in (np.float32, torch.float32):
            raise ValueError("z must be float32, got %s" % z.dtype)
        if len(z.shape) != 2 or not 1 <= z.shape[1] <= 1024:
            raise ValueError("z must be (rows, dim) with 1 <= dim <= 1024, got %s" % (tuple(z.shape),))
        N = z.shape[0]
        if not (isinstance(perplexity, (int, float, np.floating, np.integer)) and 0 < perplexity < N):
            raise ValueError("perplexity must be in (0, rows), got %r" % (perplexity,))
    if not 2 <= N <= MAX_ROWS:
        raise ValueError("t-SNE needs 2 <= rows <= 2^14, got %d" % N)
    if not _is_int(max_iter, 0, MAX_ITER):
        raise ValueError("max_iter must be an integer in [0, 32768], got %r" % (max_iter,))
    if isinstance(init, str):
        if init not in ('pca', 'random'):
            raise ValueError("init must be 'pca', 'random' or an (rows, 2) array, got %r" % (init,))
        if init == 'pca' and z is None:
            raise ValueError("init='pca' needs z")
    elif not isinstance(init, np.ndarray) or init.shape != (N, 2):
        raise ValueError("init must be 'pca', 'random' or an (rows, 2) array")
    if not _is_int(seed, 0, (1 << 64) - 1):
        raise ValueError("seed must be an integer in [0, 2^64), got %r" % (seed,))
    if learning_rate != 'auto' and not (isinstance(learning_rate, (int, float, np.floating)) and 0 < learning_rate < float('inf')):
        raise ValueError("learning_rate must be 'auto' or a positive number, got %r" % (learning_rate,))
    if not (isinstance(early_exaggeration, (int, float, np.floating)) and 1 <= early_exaggeration < float('inf')):
        raise ValueError("early_exaggeration must be a number >= 1, got %r" % (early_exaggeration,))
    if not _is_int(exaggeration_iter, 0, MAX_ITER):
        raise ValueError("exaggeration_iter must be an integer in [0, 32768], got %r" % (exaggeration_iter,))
    if not _is_int(n_iter_check, 1, MAX_ITER):
        raise ValueError("n_iter_check must be an integer in [1, 32768], got %r" % (n_iter_check,))
    if not _is_int(n_iter_without_progress, 0, MAX_ITER):
        raise ValueError("n_iter_without_progress must be an integer in [0, 32768], got %r" % (n_iter_without_progress,))
    if not (isinstance(min_grad_norm, (int, float, np.floating)) and min_grad_norm >= 0):
        raise ValueError("min_grad_norm must be a number >= 0, got %r" % (min_grad_norm,))


def tsne(vae, z, perplexity=30.0, max_iter=1000, init='pca', seed=0, learning_rate='auto', early_exaggeration=12.0, exaggeration_iter=250,
         n_iter_check=50, n_iter_without_progress=300, min_grad_norm=1e-7, p=None, return_p=False, return_trace=False, raw=tsne_raw):
    """sklearn's TSNE(method='exact', n_components=2) of the rows of z in ONE device call -> dict(y (N, 2) float32, kl sklearn's
    kl_divergence_, n_iter sklearn's n_iter_, stop 'max_iter' | 'no_progress' | 'grad_norm'; with return_p p (N, N) float64 and beta;
    with return_trace trace (2, max_iter): the error and gradient norm where they were computed).  p: a joint matrix from an earlier
    call -- the distances and the bisection do not run (one P, several seeds); z may then be None unless init='pca'."""
    from . import affinity
    from . import lib as _lib
    _check_tsne_args(z, perplexity, max_iter, init, seed, learning_rate, early_exaggeration, exaggeration_iter, n_iter_check,
                     n_iter_without_progress, min_grad_norm, p)
    y0 = pca_init(affinity.rows_of(z, 'euclidean')) if isinstance(init, str) and init == 'pca' else (None if isinstance(init, str) else init)
    cfg = _lib.AvaeTsneConfig(perplexity=float(perplexity), early_exaggeration=float(early_exaggeration), min_grad_norm=float(min_grad_norm),
                              learning_rate=0.0 if learning_rate == 'auto' else float(learning_rate), max_iter=int(max_iter), it0=0,
                              exaggeration_iter=int(exaggeration_iter), n_iter_check=int(n_iter_check),
                              n_iter_without_progress=int(n_iter_without_progress), init=1 if y0 is None else 0, warm=0, seed=int(seed))
    x = None if p is not None else affinity.rows_of(z, 'euclidean')
    res = raw(vae, x, cfg, p_in=p, y=y0, want_p=return_p, want_beta=return_p, want_trace=return_trace)
    out = dict(y=res['y'], kl=float(res['kl'][0]), n_iter=int(res['stat'][0]) + 1, stop=STOPS[int(res['stat'][1])])
    if return_p:
        out['p'] = res['p']
        if 'beta' in res:
            out['beta'] = res['beta']
    if return_trace:
        out['trace'] = res['trace']
    return out


def plot(path, y, topics):
    """the scatter of eval_clustering_explorative.py:53-66: one colour per topic (COLOURS), in order of first appearance, with the
    legend in the lower right"""
    try:
        import matplotlib
    except ImportError as e:
        raise RuntimeError("--tsne-plot needs matplotlib, which is not installed; --tsne alone writes the embedding as .npy") from e
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    topics = np.asarray(topics)
    fig = plt.figure(figsize=(8, 8))
    for topic in dict.fromkeys(topics.tolist()):
        pick = topics == topic
        plt.scatter(y[pick, 0], y[pick, 1], s=8, c=COLOURS.get(str(topic)), label=str(topic))
    plt.legend(loc=4)
    fig.savefig(path)
    plt.close(fig)
