"""Kernel two-sample test of latent rows on the device (include/argsim_vae.h, avae_mmd / avae_mmd_relabel): do two sets of rows come from
the same distribution?  The unbiased statistic MMD^2_u with a permutation null for MANY comparisons of the same rows in ONE call -- every
kernel value is formed once per pass and added for all relabelings of the pass; the relabelings themselves are generated on the device.
With kernel 'energy' the statistic is the energy distance.

    mmd_raw(vae, x, cfg, valid, inA, want)             the C entry as it stands
    relabel_raw(vae, N, valid, a0, P, seed)            avae_mmd_relabel: relabeling 0 from the host, 1 .. P written on the device
    mmd(vae, z, groups, kernel, gamma, ...)            dict(stat, pvalue, m, n[, null, witness])
    mmd2(vae, za, zb, ...)                             the same for two arrays
    median_gamma(vae, z, max_rows)                     the median heuristic (on the host: the one step that downloads rows)
    prior_match(vae, z, n_perm, seed)                  z against as many N(0, I) rows: MMD(q(z), p(z))
"""
import ctypes as C

import numpy as np

KERNELS = {'rbf': 0, 'energy': 1}
METRICS = {'euclidean': 0, 'cosine': 1}
MAX_ROWS, MAX_G, MAX_Q, MAX_BW = 1 << 17, 64, 16384, 8
WANT = ('sums', 'ull', 'witness')


def pack_bits(bits):
    """(.., N) bool -> (.., ceil(N / 64)) uint64: bit i % 64 of word i / 64 is row i"""
    bits = np.asarray(bits, bool)
    N = bits.shape[-1]
    W = (N + 63) // 64
    b = np.zeros(bits.shape[:-1] + (64 * W,), np.uint8)
    b[..., :N] = bits
    return np.ascontiguousarray(np.packbits(b, axis=-1, bitorder='little')).view('<u8').reshape(bits.shape[:-1] + (W,))


def _words(vae, w):
    """uint64 words -> an int64 tensor on the device (the same bits)"""
    import torch
    if isinstance(w, torch.Tensor):
        return w.to(vae.device).contiguous()
    return torch.from_numpy(np.ascontiguousarray(w, '<u8').view(np.int64)).to(vae.device)


def relabel_raw(vae, N, valid, a0, P, seed):
    """avae_mmd_relabel: valid (G, W) and a0 (G, W) uint64 words (numpy) -> the (G, 1 + P, W) int64 tensor of mask words on the device,
    relabeling 0 = a0, relabelings 1 .. P generated there"""
    import torch
    G, W = valid.shape
    dv = _words(vae, valid)
    din = torch.zeros((G, 1 + P, W), dtype=torch.int64, device=vae.device)
    din[:, 0] = _words(vae, a0)
    vae._stream()
    vae._ck(vae._l.avae_mmd_relabel(vae._h, N, G, P, C.c_void_p(dv.data_ptr()), C.c_void_p(din.data_ptr()), C.c_uint64(int(seed) & (2 ** 64 - 1))))
    return din


def mmd_raw(vae, x, cfg, valid, inA, want=WANT):
    """avae_mmd: x (N, dim) float32, numpy or a tensor on the device; cfg a lib.AvaeMmdConfig; valid (G, W) and inA (G, 1 + P, W) mask words,
    numpy uint64 or int64 tensors on the device; want: the optional outputs to ask for -> dict(stat (G, 1 + P), pvalue (G,), counts
    (G, 2) int32, stat_out int and, as asked, sums (G, 1 + P, 2), ull (G,), witness (G, N))"""
    import torch
    N, dim = x.shape
    dev = vae.device
    G, P1 = cfg.G, 1 + cfg.P
    dx = x if isinstance(x, torch.Tensor) else torch.as_tensor(x)
    dx = dx.to(dev).contiguous()
    dv, din = _words(vae, valid), _words(vae, inA)
    stat = torch.zeros((G, P1), dtype=torch.float64, device=dev)
    pvalue = torch.zeros((G,), dtype=torch.float64, device=dev)
    counts = torch.zeros((G, 2), dtype=torch.int32, device=dev)
    stat_out = torch.zeros((1,), dtype=torch.int32, device=dev)
    shapes = dict(sums=(G, P1, 2), ull=(G,), witness=(G, N))
    t = {n: (torch.zeros(s, dtype=torch.float64, device=dev) if n in want else None) for n, s in shapes.items()}
    ptr = lambda v: C.c_void_p(v.data_ptr()) if v is not None else None
    vae._stream()
    vae._ck(vae._l.avae_mmd(vae._h, ptr(dx), N, dim, C.byref(cfg), ptr(dv), ptr(din), ptr(stat), ptr(pvalue), ptr(counts),
                            *[ptr(t[n]) for n in WANT], ptr(stat_out)))
    out = dict(stat=stat.cpu().numpy(), pvalue=pvalue.cpu().numpy(), counts=counts.cpu().numpy(), stat_out=int(stat_out.cpu()[0]))
    out.update({n: v.cpu().numpy() for n, v in t.items() if v is not None})
    return out


def _gammas(gamma):
    """gamma as numbers -> a list of 1 .. 8 finite positive floats (ValueError otherwise)"""
    g = np.atleast_1d(np.asarray(gamma, np.float64)).ravel()
    if not 1 <= len(g) <= MAX_BW:
        raise ValueError("between 1 and 8 bandwidths, got %d" % len(g))
    if not (np.isfinite(g).all() and (g > 0).all()):
        raise ValueError("every gamma must be finite and > 0, got %s" % (g.tolist(),))
    return [float(v) for v in g]


def _check_mmd_args(z, groups, kernel, gamma, metric, n_perm):
    import torch
    if not isinstance(z, (np.ndarray, torch.Tensor)):
        raise ValueError("z must be a numpy array or a torch tensor, got %s" % type(z).__name__)
    if z.dtype not in (np.float32, torch.float32):
        raise ValueError("z must be float32, got %s" % z.dtype)
    if kernel not in KERNELS:
        raise ValueError("kernel must be one of %s, got %r" % (sorted(KERNELS), kernel))
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, got %r" % (sorted(METRICS), metric))
    if len(z.shape) != 2 or not 2 <= z.shape[0] <= MAX_ROWS:
        raise ValueError("z must be (rows, dim) with 2 <= rows <= 2^17, got %s" % (tuple(z.shape),))
    if not 1 <= z.shape[1] <= 1024:
        raise ValueError("z must have 1 <= dim <= 1024, got %s" % (tuple(z.shape),))
    grp = np.asarray(groups.detach().cpu().numpy() if isinstance(groups, torch.Tensor) else groups)
    if grp.dtype.kind not in 'iu':
        raise ValueError("groups must be integers, got %s" % grp.dtype)
    if grp.ndim not in (1, 2) or grp.shape[-1] != z.shape[0]:
        raise ValueError("groups must be (rows,) or (G, rows) with rows = %d, got %s" % (z.shape[0], grp.shape))
    if grp.ndim == 2 and not 1 <= grp.shape[0] <= MAX_G:
        raise ValueError("between 1 and 64 comparisons per call, got %d" % grp.shape[0])
    grp = grp.astype(np.int64)
    if (grp > 1).any():
        raise ValueError("groups holds 0 (sample A), 1 (sample B) or a negative value (left out)")
    G = 1 if grp.ndim == 1 else grp.shape[0]
    if isinstance(n_perm, bool) or not isinstance(n_perm, (int, np.integer)) or n_perm < 0 or G * (1 + int(n_perm)) > MAX_Q:
        raise ValueError("n_perm must be an integer >= 0 with G (1 + n_perm) <= 16384, got %r for %d comparisons" % (n_perm, G))
    for g, row in enumerate(np.atleast_2d(grp)):
        m, n = int((row == 0).sum()), int((row == 1).sum())
        if m < 2 or n < 2:
            raise ValueError("comparison %d has %d rows in A and %d in B; both samples need at least 2" % (g, m, n))
    if kernel == 'rbf' and not (isinstance(gamma, str) and gamma == 'median'):
        if isinstance(gamma, str):
            raise ValueError("gamma must be 'median' or numbers, got %r" % gamma)
        _gammas(gamma)
    return grp


def median_gamma(vae, z, max_rows=2048):
    """the median heuristic: 1 / the median of the squared Euclidean distances among an evenly strided subsample of at most max_rows rows
    of z, in float64 ON THE HOST.  It is the one step of this module that downloads rows (at most max_rows of them); mmd, mmd2 and
    prior_match skip it whenever gamma is given as numbers."""
    import torch
    N = z.shape[0]
    step = max(1, -(-N // int(max_rows)))
    s = z[::step]
    s = np.asarray(s.detach().cpu().numpy() if isinstance(s, torch.Tensor) else s, np.float64)
    d2 = ((s[:, None, :] - s[None, :, :]) ** 2).sum(-1)[np.triu_indices(len(s), 1)]
    med = float(np.median(d2))
    if not med > 0:
        raise ValueError("the median squared distance of the subsample is %r: give gamma as a number" % med)
    return 1.0 / med


def mmd(vae, z, groups, kernel='rbf', gamma='median', metric='euclidean', n_perm=999, seed=0, return_null=False, return_witness=False,
        raw=mmd_raw, relabel=relabel_raw):
    """the unbiased kernel two-sample statistic MMD^2_u of the rows of z with groups == 0 (sample A) against those with groups == 1
    (sample B) and its permutation p-value, for every row of `groups`, (N,) or (G, N) integers, in ONE device call; a negative value
    leaves a row out of that comparison.  kernel 'rbf': sum_b exp(-gamma_b d^2), gamma 'median' (median_gamma: the one step that
    downloads rows, skipped whenever gamma is a number or up to 8 numbers); kernel 'energy': -d, the energy distance.  metric
    'euclidean' or 'cosine' (the rows divided by their norms).  The n_perm relabelings are generated on the device from seed.
    -> dict(stat (G,), pvalue (G,), m (G,), n (G,)); with return_null also null (G, n_perm), with return_witness witness (G, N): for each
    row the mean kernel value to A minus that to B (large: typical of A).  For (N,) groups every entry loses its leading axis.  A tensor
    on the device whose dim is a multiple of 4 is taken as it is; anything else is uploaded, its columns padded with zeros to a multiple
    of 4 (a zero column changes no distance)."""
    import torch
    from . import lib as _lib
    from .silhouette import _pad_cols
    grp = _check_mmd_args(z, groups, kernel, gamma, metric, n_perm)
    single = grp.ndim == 1
    grp = np.atleast_2d(grp)
    G, N = grp.shape
    P = int(n_perm)
    gam = []
    if kernel == 'rbf':
        gam = [median_gamma(vae, z)] if isinstance(gamma, str) else _gammas(gamma)
    pad = -z.shape[1] % 4
    if isinstance(z, torch.Tensor) and z.is_cuda and not pad:
        x = z.detach()
    else:
        x = _pad_cols(z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else z, pad)
    valid, a0 = pack_bits(grp >= 0), pack_bits(grp == 0)
    cfg = _lib.AvaeMmdConfig(kernel=KERNELS[kernel], metric=METRICS[metric], G=G, P=P, nbw=len(gam), reserved=0)
    for b, v in enumerate(gam):
        cfg.gamma[b] = v
    inA = relabel(vae, N, valid, a0, P, seed)
    res = raw(vae, x, cfg, valid, inA, want=('witness',) if return_witness else ())
    if res['stat_out'] != 0:
        raise RuntimeError("mmd: relabeling %d does not have the size of the observed sample" % (res['stat_out'] - 1))
    out = dict(stat=res['stat'][:, 0], pvalue=res['pvalue'], m=res['counts'][:, 0].astype(np.int64), n=res['counts'][:, 1].astype(np.int64))
    if return_null:
        out['null'] = res['stat'][:, 1:]
    if return_witness:
        out['witness'] = res['witness']
    if single:
        out = {k: v[0] for k, v in out.items()}
    return out


def mmd2(vae, za, zb, kernel='rbf', gamma='median', metric='euclidean', n_perm=999, seed=0, return_null=False, return_witness=False):
    """mmd for two arrays of rows with the same dim: za is sample A, zb sample B (the witness covers the rows of za, then those of zb)"""
    import torch
    for v in (za, zb):
        if not isinstance(v, (np.ndarray, torch.Tensor)):
            raise ValueError("za and zb must be numpy arrays or torch tensors, got %s" % type(v).__name__)
        if v.dtype not in (np.float32, torch.float32):
            raise ValueError("za and zb must be float32, got %s" % v.dtype)
    if len(za.shape) != 2 or len(zb.shape) != 2 or za.shape[1] != zb.shape[1]:
        raise ValueError("za and zb must be (rows, dim) with the same dim, got %s and %s" % (tuple(za.shape), tuple(zb.shape)))
    if isinstance(za, torch.Tensor) and isinstance(zb, torch.Tensor):
        z = torch.cat([za.detach(), zb.detach().to(za.device)])
    else:
        z = np.concatenate([v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v for v in (za, zb)])
    groups = np.concatenate([np.zeros(za.shape[0], np.int64), np.ones(zb.shape[0], np.int64)])
    return mmd(vae, z, groups, kernel, gamma, metric, n_perm, seed, return_null, return_witness)


def prior_match(vae, z, n_perm=999, seed=0):
    """does the aggregate posterior match the prior?  The rows of z against as many rows of N(0, I) drawn with
    numpy.random.default_rng(seed) as float32: MMD(q(z), p(z)), the InfoVAE diagnostic, with the rbf kernel at the median bandwidth
    -> dict(stat, pvalue, m, n)"""
    prior = np.random.default_rng(seed).standard_normal(tuple(z.shape)).astype(np.float32)
    return mmd2(vae, z, prior, 'rbf', 'median', 'euclidean', n_perm, seed)
