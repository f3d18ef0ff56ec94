"""Gaussian mixture of latent rows on the device (include/argsim_vae.h, avae_gmm_fit / avae_gmm_score): scikit-learn's
GaussianMixture(covariance_type='diag' | 'spherical') with n_init restarts side by side in ONE call.

    gmm_raw(vae, x, cfg, ...)            the C entry as it stands
    gmm(vae, z, k, ...)                  dict(weights, means, covariances, labels, logp, lower_bound, ..., bic, aic)
    gmm_score(vae, z, model)             log p(z_i) under a fitted model (and labels; responsibilities on request)
    sweep_gmm(vae, z, ks, ...)           one fit per k, BIC / AIC, the best k
    sample(model, n, seed)               rows drawn from the mixture on the host

Columns: the C entry takes a column count that is a multiple of 4.  Other rows are padded with zero columns and the handle's option
gmm_pad is set for the call: a padding column has variance 1 whatever it holds, no share in the spherical mean or in the (dim / 2) log 2 pi
constant, and a zero column with a zero mean adds exactly nothing to a row's q_ic -- the result over the real columns is that of the
unpadded rows, and the padding columns are stripped from what is returned."""
import ctypes as C

import numpy as np

COVS = {'diag': 0, 'spherical': 1}
STOPS = ('converged', 'max_iter', 'degenerate')
MAX_ROWS, MAX_K, MAX_INIT, MAX_ITER = 1 << 22, 1024, 16, 10000
DEGENERATE = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance caused by "
              "singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or scale the input data.")


def _dev(vae, a, dtype):
    import torch
    if isinstance(a, torch.Tensor):
        return a.detach().to(device=vae.device, dtype=dtype).contiguous()
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=vae.device, dtype=dtype).contiguous()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _Pad:
    """the handle's gmm_pad for the length of one call"""
    def __init__(self, vae, pad):
        self.vae, self.pad = vae, pad

    def __enter__(self):
        if self.pad:
            self.vae._ck(self.vae._l.avae_set_option(self.vae._h, b'gmm_pad', self.pad))

    def __exit__(self, *exc):
        if self.pad:
            self.vae._l.avae_set_option(self.vae._h, b'gmm_pad', 0)


def gmm_raw(vae, x, cfg, label_in=None, params_in=None, want_logp=True, want_resp=False, want_all=False, want_trace=False, pad=0):
    """avae_gmm_fit: x (N, dim) float32, numpy or a tensor on the device; cfg a lib.AvaeGmmConfig; label_in (n_init, N) int32 with
    cfg.init = 0, params_in = (w (n_init, k), mu, cov (n_init, k, dim)) float64 with cfg.init = 1 -> dict(weights (k,), means, covars
    (k, dim), label (N,), stat (4,), lower (n_init,); logp (N,), resp (N, k), weights_all, means_all, covars_all, stat_all (n_init, 4),
    trace (n_init, max_iter) as asked for)"""
    import torch
    N, dim = x.shape
    dev = vae.device
    k, R, T = cfg.k, cfg.n_init, cfg.max_iter
    dx = _dev(vae, x, torch.float32)
    dl = None if label_in is None else _dev(vae, label_in, torch.int32)
    dp = [None] * 3 if params_in is None else [_dev(vae, p, torch.float64) for p in params_in]
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    o = dict(weights=f64(k), means=f64(k, dim), covars=f64(k, dim), label=i32(N), stat=i32(4), lower=f64(R),
             logp=f64(N) if want_logp else None, resp=f64(N, k) if want_resp else None,
             weights_all=f64(R, k) if want_all else None, means_all=f64(R, k, dim) if want_all else None,
             covars_all=f64(R, k, dim) if want_all else None, stat_all=i32(R, 4) if want_all else None,
             trace=f64(R, max(T, 1))[:, :T].contiguous() if want_trace else None)
    vae._stream()
    with _Pad(vae, pad):
        vae._ck(vae._l.avae_gmm_fit(vae._h, _ptr(dx), N, dim, C.byref(cfg), _ptr(dl), *[_ptr(p) for p in dp], *[_ptr(t) for t in o.values()]))
    return {n: t.cpu().numpy() for n, t in o.items() if t is not None}


def score_raw(vae, x, weights, means, covars, want_resp=False, pad=0):
    """avae_gmm_score -> dict(logp (n,), label (n,), resp (n, k) if asked for)"""
    import torch
    n, dim = x.shape
    k = int(np.shape(weights)[0])
    dx = _dev(vae, x, torch.float32)
    dp = [_dev(vae, p, torch.float64) for p in (weights, means, covars)]
    logp = torch.zeros((n,), dtype=torch.float64, device=vae.device)
    label = torch.zeros((n,), dtype=torch.int32, device=vae.device)
    resp = torch.zeros((n, k), dtype=torch.float64, device=vae.device) if want_resp else None
    vae._stream()
    with _Pad(vae, pad):
        vae._ck(vae._l.avae_gmm_score(vae._h, _ptr(dx), n, dim, k, *[_ptr(p) for p in dp], _ptr(logp), _ptr(label), _ptr(resp)))
    out = dict(logp=logp.cpu().numpy(), label=label.cpu().numpy())
    if want_resp:
        out['resp'] = resp.cpu().numpy()
    return out


def _check_rows(z):
    import torch
    if not isinstance(z, (np.ndarray, torch.Tensor)):
        raise ValueError("z must be a numpy array or a torch tensor, got %s" % type(z).__name__)
    if z.dtype not in (np.float32, torch.float32):
        raise ValueError("z must be float32, got %s" % z.dtype)
    if len(z.shape) != 2 or not 1 <= z.shape[1] <= 1024:
        raise ValueError("z must be (rows, dim) with 1 <= dim <= 1024, got %s" % (tuple(z.shape),))


def _check_gmm_args(z, k, covariance='diag', n_init=1, max_iter=100, tol=1e-3, reg_covar=1e-6, seed=0, init='kmeans'):
    """the argument rules of VAE.gmm, checked before anything touches the device (ValueError)"""
    _check_rows(z)
    if not 2 <= z.shape[0] <= MAX_ROWS:
        raise ValueError("z must have 2 <= rows <= 2^22, got %s" % (tuple(z.shape),))
    if covariance not in COVS:
        raise ValueError("covariance must be one of %s, got %r" % (sorted(COVS), covariance))
    if not (isinstance(k, (int, np.integer)) and 1 <= k <= min(z.shape[0], MAX_K)):
        raise ValueError("k must be an integer in [1, min(rows, 1024)], got %r" % (k,))
    if not (isinstance(n_init, (int, np.integer)) and 1 <= n_init <= MAX_INIT):
        raise ValueError("n_init must be an integer in [1, 16], got %r" % (n_init,))
    if not (isinstance(max_iter, (int, np.integer)) and 0 <= max_iter <= MAX_ITER):
        raise ValueError("max_iter must be an integer in [0, 10000], got %r" % (max_iter,))
    for name, v in (('tol', tol), ('reg_covar', reg_covar)):
        if not (isinstance(v, (int, float, np.floating, np.integer)) and v >= 0):
            raise ValueError("%s must be a number >= 0, got %r" % (name, v))
    if not (isinstance(seed, (int, np.integer)) and 0 <= seed < 1 << 63):
        raise ValueError("seed must be an integer in [0, 2^63), got %r" % (seed,))
    N, dim = z.shape
    if isinstance(init, str):
        if init != 'kmeans':
            raise ValueError("init must be 'kmeans', labels or a dict of parameters, got %r" % (init,))
    elif isinstance(init, dict):
        if sorted(init) != ['covariances', 'means', 'weights']:
            raise ValueError("init parameters must be dict(weights, means, covariances), got keys %s" % sorted(init))
        w, mu, cov = (np.shape(init[n]) for n in ('weights', 'means', 'covariances'))
        cshape = (k, dim) if covariance == 'diag' else (k,)
        if not ((w, mu, cov) == ((k,), (k, dim), cshape) or (w, mu, cov) == ((n_init, k), (n_init, k, dim), (n_init,) + cshape)):
            raise ValueError("init parameters must be weights (k,), means (k, dim), covariances %s, or each with a leading n_init, got %s"
                             % (cshape, (w, mu, cov)))
    else:
        shape = tuple(np.shape(init))
        if shape not in ((N,), (n_init, N)):
            raise ValueError("init labels must be (rows,) or (n_init, rows) = %s, got %s" % ((n_init, N), shape))
        if not np.issubdtype(np.asarray(init).dtype, np.integer):
            raise ValueError("init labels must be integers, got %s" % np.asarray(init).dtype)


def _padded(z, pad):
    import torch
    if isinstance(z, torch.Tensor) and z.is_cuda and not pad:
        return z.detach()
    a = z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else z
    return np.ascontiguousarray(np.pad(a, ((0, 0), (0, pad))) if pad else a, dtype=np.float32)


def n_parameters(k, dim, covariance):
    """sklearn's GaussianMixture._n_parameters"""
    return int((k * dim if covariance == 'diag' else k) + k * dim + k - 1)


def _full_cov(cov, k, dim, covariance):
    """a model's covariances as the C entry takes them: (.., k, dim)"""
    cov = np.asarray(cov, np.float64)
    return np.repeat(cov[..., None], dim, -1) if covariance == 'spherical' else cov


def gmm(vae, z, k, covariance='diag', n_init=1, max_iter=100, tol=1e-3, reg_covar=1e-6, seed=0, init='kmeans', return_resp=False,
        return_all=False, raw=gmm_raw):
    """sklearn's GaussianMixture(k, covariance_type, n_init, max_iter, tol, reg_covar) of the rows of z in ONE device call ->
    dict(weights (k,), means (k, dim), covariances (k, dim) or (k,) for 'spherical', covariance, labels (N,), logp (N,), lower_bound,
    lower_bounds (n_init,), n_iter, stop 'converged' | 'max_iter', converged, best, n_parameters, bic, aic); with return_resp also resp (N, k);
    with return_all also weights_all, means_all, covariances_all, stats_all [(n_iter, stop)] and trace (n_init, max_iter).  init: 'kmeans'
    (VAE.kmeans(z, k, n_init=1, seed=seed + r) for restart r hands over its labels), labels (N,) -- one restart -- or (n_init, N), or
    dict(weights, means, covariances), each with or without a leading n_init.  A restart whose variances collapse is degenerate; if the best
    one is, ValueError with sklearn's message."""
    from . import lib as _lib
    labels = params = None
    if isinstance(init, dict) and 'weights' in init:
        n_init = 1 if np.ndim(init['weights']) == 1 else int(np.shape(init['weights'])[0])
    elif not isinstance(init, (str, dict)) and np.ndim(init) in (1, 2):
        n_init = 1 if np.ndim(init) == 1 else int(np.shape(init)[0])
    _check_gmm_args(z, k, covariance, n_init, max_iter, tol, reg_covar, seed, init)
    N, dim = z.shape
    pad = -dim % 4
    x = _padded(z, pad)
    if isinstance(init, str):
        labels = np.stack([vae.kmeans(x, k, n_init=1, seed=seed + r)['labels'] for r in range(n_init)]).astype(np.int32)
    elif isinstance(init, dict):
        w = np.asarray(init['weights'], np.float64).reshape(n_init, k)
        mu = np.asarray(init['means'], np.float64).reshape(n_init, k, dim)
        cov = _full_cov(np.asarray(init['covariances'], np.float64).reshape((n_init, k) + ((dim,) if covariance == 'diag' else ())), k, dim, covariance)
        grow = lambda a: np.ascontiguousarray(np.pad(a, ((0, 0), (0, 0), (0, pad)), constant_values=0.0))
        params = (np.ascontiguousarray(w), grow(mu), grow(cov))
    else:
        labels = np.ascontiguousarray(np.asarray(init).reshape(n_init, N), np.int32)
    cfg = _lib.AvaeGmmConfig(k=int(k), n_init=int(n_init), max_iter=int(max_iter), covariance=COVS[covariance], init=0 if params is None else 1,
                             reserved=0, tol=float(tol), reg_covar=float(reg_covar))
    res = raw(vae, x, cfg, labels, params, want_logp=True, want_resp=return_resp, want_all=return_all, want_trace=return_all, pad=pad)
    stat = res['stat']
    if stat[2] == 2:
        raise ValueError(DEGENERATE)
    cut = lambda a: a[..., :dim] if covariance == 'diag' else a[..., 0]
    lower = float(res['lower'][stat[0]])
    npar = n_parameters(k, dim, covariance)
    out = dict(weights=res['weights'], means=res['means'][:, :dim], covariances=cut(res['covars']), covariance=covariance,
               labels=res['label'].astype(np.int64), logp=res['logp'], lower_bound=lower, lower_bounds=res['lower'], n_iter=int(stat[1]),
               stop=STOPS[stat[2]], converged=bool(stat[2] == 0), best=int(stat[0]), n_parameters=npar,
               bic=float(-2.0 * res['logp'].sum() + npar * np.log(N)), aic=float(-2.0 * res['logp'].sum() + 2 * npar))
    if return_resp:
        out['resp'] = res['resp']
    if return_all:
        out.update(weights_all=res['weights_all'], means_all=res['means_all'][:, :, :dim], covariances_all=cut(res['covars_all']),
                   stats_all=[(int(s[0]), STOPS[s[1]]) for s in res['stat_all']], trace=res['trace'])
    return out


def _model_params(model, dim):
    for n in ('weights', 'means', 'covariances'):
        if n not in model:
            raise ValueError("a mixture model is dict(weights, means, covariances), as VAE.gmm returns it; %r is missing" % n)
    w = np.asarray(model['weights'], np.float64)
    mu = np.asarray(model['means'], np.float64)
    cov = np.asarray(model['covariances'], np.float64)
    k = w.shape[0]
    if w.ndim != 1 or mu.shape != (k, dim) or cov.shape not in ((k,), (k, dim)):
        raise ValueError("the model's weights (k,), means (k, %d) and covariances (k,) or (k, %d) do not fit: %s %s %s"
                         % (dim, dim, w.shape, mu.shape, cov.shape))
    return w, mu, (np.repeat(cov[:, None], dim, 1) if cov.ndim == 1 else cov)


def gmm_score(vae, z, model, return_resp=False, raw=score_raw):
    """log p(z_i) of the rows of z under a model of VAE.gmm -> dict(logp (n,), labels (n,)); with return_resp also resp (n, k)"""
    _check_rows(z)
    if not 1 <= z.shape[0] <= MAX_ROWS:
        raise ValueError("z must have 1 <= rows <= 2^22, got %s" % (tuple(z.shape),))
    dim = z.shape[1]
    w, mu, cov = _model_params(model, dim)
    pad = -dim % 4
    grow = lambda a: np.ascontiguousarray(np.pad(a, ((0, 0), (0, pad))))
    res = raw(vae, _padded(z, pad), w, grow(mu), grow(cov), want_resp=return_resp, pad=pad)
    out = dict(logp=res['logp'], labels=res['label'].astype(np.int64))
    if return_resp:
        out['resp'] = res['resp']
    return out


def sweep_gmm(vae, z, ks, **kw):
    """one VAE.gmm per k in ks -> dict(k, bic, aic, lower_bound, models, best): best is the k with the smallest BIC (the first of equals)"""
    ks = [int(k) for k in ks]
    if not ks:
        raise ValueError("ks must name at least one k")
    models = [gmm(vae, z, k, **kw) for k in ks]
    bic = np.array([m['bic'] for m in models])
    return dict(k=ks, bic=bic, aic=np.array([m['aic'] for m in models]), lower_bound=np.array([m['lower_bound'] for m in models]),
                models=models, best=ks[int(np.argmin(bic))])


def sample(model, n, seed=0):
    """n rows from the mixture, on the host, from np.random.default_rng(seed): the component by choice(p=weights), then
    mean + sqrt(cov) * standard_normal -> (z (n, dim) float32, component (n,))"""
    mu = np.asarray(model['means'], np.float64)
    w, mu, cov = _model_params(model, mu.shape[1])
    rng = np.random.default_rng(seed)
    comp = rng.choice(w.shape[0], size=int(n), p=w / w.sum())
    z = mu[comp] + np.sqrt(cov[comp]) * rng.standard_normal((int(n), mu.shape[1]))
    return z.astype(np.float32), comp
