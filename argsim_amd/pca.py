"""Principal components of latent rows on the device (include/argsim_vae.h, avae_pca_fit / avae_pca_transform): the mean, the covariance
and its eigen-decomposition in double in ONE call, the projection in another.  The components carry scikit-learn's sign convention
(the entry of largest magnitude of each is positive) and its explained_variance (the divisor is N - 1).

    pca_raw(vae, x, cfg)                               the C entry as it stands
    pca(vae, z, n_components, whiten, max_sweeps)      the model: a dict of numpy float64 arrays and Python numbers
    transform(vae, z, model)                           (n, k) float32 on the device where z is, else numpy
    inverse_transform(model, y)                        numpy float64 on the host (a handful of rows to decode: no kernel)
    reduce(vae, z, k, whiten)                          fit + transform -> (y, model)
"""
import ctypes as C

import numpy as np

MAX_ROWS, MAX_SWEEPS = 1 << 22, 256


def _ptr(v):
    return C.c_void_p(v.data_ptr()) if v is not None else None


def pca_raw(vae, x, cfg):
    """avae_pca_fit: x (N, dim) float32, numpy or a tensor on the device; cfg a lib.AvaePcaConfig -> dict(mean (dim,), var (dim,), comp
    (dim, dim) float64 and stat (8,) int32); what the call leaves untouched (the padding) is zero"""
    import torch
    N, dim = x.shape
    dev = vae.device
    dx = x if isinstance(x, torch.Tensor) else torch.as_tensor(x)
    dx = dx.to(dev).contiguous()
    mean = torch.zeros((dim,), dtype=torch.float64, device=dev)
    var = torch.zeros((dim,), dtype=torch.float64, device=dev)
    comp = torch.zeros((dim, dim), dtype=torch.float64, device=dev)
    stat = torch.zeros((8,), dtype=torch.int32, device=dev)
    vae._stream()
    vae._ck(vae._l.avae_pca_fit(vae._h, _ptr(dx), N, dim, C.byref(cfg), _ptr(mean), _ptr(var), _ptr(comp), _ptr(stat)))
    return dict(mean=mean.cpu().numpy(), var=var.cpu().numpy(), comp=comp.cpu().numpy(), stat=stat.cpu().numpy())


def transform_raw(vae, x, mean, comp, scale):
    """avae_pca_transform: x (n, dim) float32, numpy or a tensor on the device; mean (dim,), comp (k, dim), scale (k,) or None, float64
    numpy -> y (n, k) float32 on the device"""
    import torch
    n, dim = x.shape
    k = comp.shape[0]
    dev = vae.device
    dx = x if isinstance(x, torch.Tensor) else torch.as_tensor(x)
    dx = dx.to(dev).contiguous()
    up = lambda v: torch.as_tensor(np.ascontiguousarray(v, np.float64)).to(dev) if v is not None else None
    dm, dc, ds = up(mean), up(comp), up(scale)
    y = torch.zeros((n, k), dtype=torch.float32, device=dev)
    vae._stream()
    vae._ck(vae._l.avae_pca_transform(vae._h, _ptr(dx), n, dim, _ptr(dm), _ptr(dc), _ptr(ds), k, _ptr(y)))
    return y


def _check_pca_args(z, n_components=None, whiten=False, max_sweeps=0, fit=True):
    import torch
    if not isinstance(z, (np.ndarray, torch.Tensor)):
        raise ValueError("z must be a numpy array or a torch tensor, got %s" % type(z).__name__)
    if z.dtype not in (np.float32, torch.float32):
        raise ValueError("z must be float32, got %s" % z.dtype)
    if len(z.shape) != 2 or not (2 if fit else 1) <= z.shape[0] <= MAX_ROWS:
        raise ValueError("z must be (rows, dim) with %d <= rows <= 2^22, got %s" % (2 if fit else 1, tuple(z.shape)))
    if not 1 <= z.shape[1] <= 1024:
        raise ValueError("z must have 1 <= dim <= 1024, got %s" % (tuple(z.shape),))
    if not isinstance(whiten, (bool, np.bool_)):
        raise ValueError("whiten must be True or False, got %r" % (whiten,))
    if isinstance(max_sweeps, bool) or not isinstance(max_sweeps, (int, np.integer)) or not 0 <= max_sweeps <= MAX_SWEEPS:
        raise ValueError("max_sweeps must be an integer in [0, 256] (0: the planner's default), got %r" % (max_sweeps,))
    top = min(z.shape[0] - 1, z.shape[1])
    if n_components is None:
        return
    if isinstance(n_components, bool) or not isinstance(n_components, (int, float, np.integer, np.floating)):
        raise ValueError("n_components must be None, an integer or a fraction in (0, 1), got %r" % (n_components,))
    if isinstance(n_components, (int, np.integer)):
        if not 1 <= n_components <= top:
            raise ValueError("n_components must be in [1, min(rows - 1, dim) = %d], got %r" % (top, n_components))
    elif not 0.0 < n_components < 1.0:
        raise ValueError("a fractional n_components must be in (0, 1), got %r" % (n_components,))


def _pad_cols(a, pad):
    return np.ascontiguousarray(np.pad(a, [(0, 0), (0, pad)]) if pad else a, dtype=np.float32)


def _rows(z, pad):
    """the rows as the C entries take them: a device tensor whose dim is a multiple of 4 as it is, anything else uploaded and padded"""
    import torch
    if isinstance(z, torch.Tensor) and z.is_cuda and not pad:
        return z.detach()
    return _pad_cols(z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else z, pad)


def pca(vae, z, n_components=None, whiten=False, max_sweeps=0, raw=pca_raw):
    """PCA of the rows of z in ONE device call -> dict(mean (dim,), components (k, dim), explained_variance (k,),
    explained_variance_ratio (k,), singular_values (k,) = sqrt(var (N - 1)), noise_variance = the mean of the dropped variances (0 if
    none), effective_dim = (sum var)^2 / sum var^2 over ALL components, n_samples, rank, sweeps, whiten).  n_components: None (all dim),
    an integer in [1, min(N - 1, dim)], or a fraction in (0, 1): the smallest count whose cumulative ratio exceeds it (scikit-learn's
    rule).  RuntimeError if the eigen-solve had not converged within max_sweeps (0: the planner's default)."""
    from . import lib as _lib
    _check_pca_args(z, n_components, whiten, max_sweeps)
    N, dim = z.shape
    pad = -dim % 4
    cfg = _lib.AvaePcaConfig(pad=pad, max_sweeps=int(max_sweeps), reserved=0, reserved2=0)
    res = raw(vae, _rows(z, pad), cfg)
    stat = res['stat']
    if not stat[1]:
        raise RuntimeError("pca: the eigen-solve had not converged after %d sweeps; call again with a larger max_sweeps (it was %s)"
                           % (int(stat[0]), max_sweeps if max_sweeps else "the planner's default"))
    var = np.asarray(res['var'], np.float64)[:dim]
    total = var.sum()
    ratio = var / total if total > 0 else np.zeros_like(var)
    if n_components is None:
        k = dim
    elif isinstance(n_components, (int, np.integer)):
        k = int(n_components)
    else:
        k = min(int(np.searchsorted(np.cumsum(ratio), n_components, side='right')) + 1, dim)
    sq = (var * var).sum()
    return dict(mean=np.asarray(res['mean'], np.float64)[:dim].copy(), components=np.asarray(res['comp'], np.float64)[:k, :dim].copy(),
                explained_variance=var[:k].copy(), explained_variance_ratio=ratio[:k].copy(), singular_values=np.sqrt(var[:k] * (N - 1)),
                noise_variance=float(var[k:].mean()) if k < dim else 0.0, effective_dim=float(total * total / sq) if sq > 0 else 0.0,
                n_samples=int(N), rank=int(stat[3]), sweeps=int(stat[0]), whiten=bool(whiten))


def _check_model(model, dim):
    need = ('mean', 'components', 'explained_variance', 'whiten')
    if not isinstance(model, dict) or any(n not in model for n in need):
        raise ValueError("model must be what pca() returns: a dict with %s" % ', '.join(need))
    k, d = model['components'].shape
    if d != dim or model['mean'].shape != (dim,) or model['explained_variance'].shape != (k,):
        raise ValueError("the model is for rows of dim %d, k = %d; got rows of dim %d" % (d, k, dim))
    if model['whiten'] and not (model['explained_variance'] > 0).all():
        raise ValueError("a whitening model needs every kept variance > 0; keep at most rank = %d components" % int((model['explained_variance'] > 0).sum()))
    return k


def transform(vae, z, model, raw=transform_raw):
    """y[i][c] = scale_c sum_j (z_ij - mean_j) components[c][j] in double, rounded once to float32; scale_c = 1 / sqrt(var_c) with a
    whitening model, else 1.  -> (n, k) float32: a tensor on the device where z is one, else a numpy array"""
    import torch
    _check_pca_args(z, fit=False)
    dim = z.shape[1]
    k = _check_model(model, dim)
    pad = -dim % 4
    mean = np.pad(np.asarray(model['mean'], np.float64), (0, pad))
    comp = np.pad(np.asarray(model['components'], np.float64), [(0, 0), (0, pad)])
    scale = 1.0 / np.sqrt(np.asarray(model['explained_variance'], np.float64)) if model['whiten'] else None
    y = raw(vae, _rows(z, pad), mean, comp, scale)
    return y if isinstance(z, torch.Tensor) and z.is_cuda else np.asarray(y.cpu().numpy() if isinstance(y, torch.Tensor) else y)


def inverse_transform(model, y):
    """the rows a transform came from, up to the dropped components: y / scale @ components + mean, numpy float64 on the host"""
    import torch
    y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
    k, dim = model['components'].shape
    if y.ndim != 2 or y.shape[1] != k:
        raise ValueError("y must be (rows, k = %d), got %s" % (k, tuple(y.shape)))
    y = y.astype(np.float64)
    if model['whiten']:
        y = y * np.sqrt(np.asarray(model['explained_variance'], np.float64))
    return y @ np.asarray(model['components'], np.float64) + np.asarray(model['mean'], np.float64)


def reduce(vae, z, k, whiten=False):
    """fit + transform: the rows of z in their leading k principal directions -> (y (N, k) float32, model)"""
    model = vae.pca(z, n_components=k, whiten=whiten)
    return vae.pca_transform(z, model), model
