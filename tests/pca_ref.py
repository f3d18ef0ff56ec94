"""Principal components in float64 numpy: the contract of avae_pca_fit / avae_pca_transform (include/argsim_vae.h) restated.

    covariance(x, pad)        column means and the two-pass covariance of the centred rows, / (N - 1)
    jacobi(C, max_sweeps)     two-sided cyclic Jacobi, round by round, as the device runs it (the rule is in the header)
    fit(x, pad, max_sweeps)   dict(mean, var, comp, sweeps, rotations, converged, rank, thr)
    transform(x, model, k, scale)
    certificates(x, model)    residual, orthogonality, eigenvalue and mean error against numpy from the rows themselves
and the makers of the test cases.  DEFAULT_SWEEPS is the planner's default (kPcaSweeps, kernels.h): twice the largest count of MEASURED
below, which test_pca.py re-measures (all but the 1024-column case, which takes minutes in numpy)."""
import numpy as np

EPS = 2.0 ** -52
# sweeps jacobi() takes: the cases of test_gpu_pca.py / test_pca.py (the largest over them) and 300 x 1024 designed rows
MEASURED = {'tests': 22, '300x1024': 29}
DEFAULT_SWEEPS = 2 * max(MEASURED.values())


def covariance(x, pad=0):
    """-> mean (dreal,), C (dreal, dreal): the columns behind dreal = dim - pad are ignored"""
    x = np.asarray(x, np.float64)
    d = x.shape[1] - pad
    x = x[:, :d]
    mean = x.sum(0) / len(x)
    xc = x - mean
    return mean, xc.T @ xc / (len(x) - 1)


def partners(n, r):
    """round r of the round-robin order over n columns: partner[j], or >= n for the bye.  m = n rounded up to even; column m - 1 plays
    column r, every other column j plays (2 r - j) mod (m - 1)"""
    m = n + (n & 1)
    j = np.arange(n)
    p = (2 * r - j) % (m - 1)
    p = np.where(p == j, m - 1, p)
    if n == m:
        p[m - 1] = r
    return p


def rounds(n):
    return n + (n & 1) - 1


def jacobi(C, max_sweeps=DEFAULT_SWEEPS):
    """-> dict(var descending and clipped at 0, comp (row c = component c, sign fixed), sweeps, rotations, converged, rank, thr, diag (the
    eigenvalues as the solve left them, sorted))"""
    A = np.array(C, np.float64)
    n = len(A)
    V = np.eye(n)                                           # row j = column j of the accumulated rotations
    thr = EPS * np.sqrt((A * A).sum()) / n
    sweeps = rotations = 0
    converged = False
    idx = np.arange(n)
    while sweeps < max_sweeps and not converged:
        rot_sweep = 0
        for r in range(rounds(n)):
            p = partners(n, r)
            live = p < n
            ps = np.where(live, p, idx)
            lo, hi = np.minimum(idx, ps), np.maximum(idx, ps)
            apq, app, aqq = A[lo, hi], A[lo, lo], A[hi, hi]
            rot = live & (np.abs(apq) > thr)
            if not rot.any():
                continue
            with np.errstate(all='ignore'):
                theta = (aqq - app) / (2.0 * apq)
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(1.0 + theta * theta))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
            is_lo = idx == lo
            w = np.where(rot, c, 1.0)
            u = np.where(rot, np.where(is_lo, -s, s), 0.0)
            dd = np.where(rot, np.where(is_lo, -t * apq, t * apq), 0.0)
            B = A * w[None, :] + A[:, ps] * u[None, :]
            An = w[:, None] * B + u[:, None] * B[ps, :]
            An = np.triu(An) + np.triu(An, 1).T            # the device evaluates (min, max) and mirrors
            An[idx, idx] = A[idx, idx] + dd
            An[idx[rot], ps[rot]] = 0.0
            A = An
            V = w[:, None] * V + u[:, None] * V[ps, :]
            rot_sweep += int(rot.sum()) // 2
        sweeps += 1
        rotations += rot_sweep
        converged = rot_sweep == 0
    d = np.diag(A).copy()
    order = np.argsort(-d, kind='stable')
    comp = V[order]
    big = np.argmax(np.abs(comp), 1)
    comp = comp * np.where(comp[np.arange(n), big] < 0, -1.0, 1.0)[:, None]
    var = np.maximum(d[order], 0.0)
    return dict(var=var, comp=comp, sweeps=sweeps, rotations=rotations, converged=converged, rank=int((var > thr).sum()), thr=thr, diag=d[order])


def fit(x, pad=0, max_sweeps=DEFAULT_SWEEPS):
    mean, C = covariance(x, pad)
    out = jacobi(C, max_sweeps)
    out['mean'] = mean
    return out


def transform(x, mean, comp, k, scale=None):
    """float64 (x - mean) comp[:k]^T scale over the leading len(mean) columns"""
    d = len(mean)
    y = (np.asarray(x, np.float64)[:, :d] - mean) @ np.asarray(comp, np.float64)[:k, :d].T
    return y if scale is None else y * np.asarray(scale, np.float64)[:k]


def certificates(x, model, pad=0):
    """-> dict(res, orth, eig, mean): what the header's contract promises, measured against float64 numpy from the rows"""
    mean, C = covariance(x, pad)
    d = len(mean)
    var, V = np.asarray(model['var'], np.float64)[:d], np.asarray(model['comp'], np.float64)[:d, :d]
    lam = np.linalg.eigvalsh(C)[::-1]
    top = max(lam[0], np.finfo(np.float64).tiny)
    return dict(res=float(np.abs(C @ V.T - V.T * var[None, :]).max() / top), orth=float(np.abs(V @ V.T - np.eye(d)).max()),
                eig=float(np.abs(var - np.maximum(lam, 0.0)).max() / top),
                mean=float(np.abs(np.asarray(model['mean'], np.float64)[:d] - mean).max() / max(np.abs(mean).max(), 1.0)))


def signs_ok(comp):
    """every row's entry of largest magnitude (the first of equals) is positive"""
    comp = np.asarray(comp)
    return bool((comp[np.arange(len(comp)), np.argmax(np.abs(comp), 1)] > 0).all())


# ---------------------------------------------------------------- the cases
def _pad(x, pad):
    """pad columns of rubbish behind the real ones: the device must ignore them"""
    if not pad:
        return np.ascontiguousarray(x, np.float32)
    junk = np.full((len(x), pad), 1e6, np.float32) * (1 + np.arange(len(x), dtype=np.float32))[:, None]
    return np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32), junk], 1))


def random_rows(N, dim, pad=0, seed=0):
    """dense correlated rows with a decaying spectrum and a modest offset; the last pad columns are rubbish"""
    rng = np.random.RandomState(1000 * N + dim + 7 * pad + seed)
    d = dim - pad
    mix = rng.standard_normal((d, d)) * (0.8 ** np.arange(d))[:, None]
    x = rng.standard_normal((N, d)) @ mix + rng.standard_normal(d)
    return _pad(x.astype(np.float32), pad)


def designed(N, dim, spectrum, seed=0):
    """rows whose covariance has (nearly) the eigenvalues `spectrum` (len <= min(N - 1, dim), well separated) along a random basis"""
    rng = np.random.RandomState(seed)
    k = len(spectrum)
    Q = np.linalg.qr(rng.standard_normal((dim, dim)))[0][:, :k]
    U = np.linalg.qr(rng.standard_normal((N, k + 1)) - 0.0)[0]
    U = U - U.mean(0)
    U = np.linalg.qr(U)[0][:, :k]                          # orthonormal, centred columns
    x = (U * np.sqrt(np.asarray(spectrum, np.float64) * (N - 1))[None, :]) @ Q.T
    return np.ascontiguousarray(x + 0.5, np.float32)


def collapsed(N, dim, seed=0):
    """three quarters of the columns scaled by 1e-4 (collapsed units), an offset of 3"""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((N, dim)) @ rng.standard_normal((dim, dim))
    x[:, dim // 4:] *= 1e-4
    return np.ascontiguousarray(x + 3.0, np.float32)


def offset(N, dim, seed=0, shift=1000.0):
    """rows + 1000: a one-pass covariance loses seven digits here"""
    return np.ascontiguousarray(random_rows(N, dim, 0, seed).astype(np.float64) * 0.25 + shift, np.float32)


def rank_deficient(N, dim, seed=0):
    """a duplicated column and a zero column.  The rows are small integers and their negatives (N even): every column sum is 0 and every
    sum of products an integer below 2^53, so the mean and the covariance are exact whatever the order of the sums -- the device and the
    reference start the solve from the same matrix, and the count of eigenvalues above thr (the rank) is the same on both sides although
    the null eigenvalue of the duplicate is rounding noise"""
    rng = np.random.RandomState(seed + 5)
    half = rng.randint(-8, 9, (N // 2, dim)).astype(np.float32)
    x = np.concatenate([half, -half])
    x[:, 1] = x[:, 0]
    x[:, dim - 1] = 0.0
    return np.ascontiguousarray(x)


def dense(N, dim, pad=0, seed=0):
    """well-conditioned rows (every eigenvalue of the covariance far above thr when N > dreal): the rank does not hang on rounding"""
    rng = np.random.RandomState(77 * N + dim + seed)
    d = dim - pad
    x = rng.standard_normal((N, d)) @ (np.eye(d) + 0.5 * rng.standard_normal((d, d)) / np.sqrt(d)) + rng.standard_normal(d)
    return _pad(x.astype(np.float32), pad)


def axis_rows(scales):
    """rows +s_j e_j and -s_j e_j: C is diagonal with entries 2 s_j^2 / (N - 1), N = 2 len(scales)"""
    d = len(scales)
    x = np.zeros((2 * d, d), np.float32)
    for j, s in enumerate(scales):
        x[2 * j, j], x[2 * j + 1, j] = s, -s
    return x


def block_rows():
    """4 rows whose covariance over columns (0, 1) is [[a, b], [b, a]], a = 10 / 3, b = 8 / 3; columns 2, 3 are zero"""
    x = np.zeros((4, 4), np.float32)
    x[:, 0] = [2, -2, 1, -1]
    x[:, 1] = [1, -1, 2, -2]
    return x


SHAPES = [(N, dim, pad) for N in (2, 3, 63, 64, 65, 257) for dim in (4, 36, 132) for pad in (0, 3)]


def test_cases():
    """name -> (x, pad): every case whose sweeps count toward DEFAULT_SWEEPS"""
    out = {}
    for N, dim, pad in SHAPES:
        out['random-%dx%d-%d' % (N, dim, pad)] = (random_rows(N, dim, pad), pad)
    out['dense-300x260'] = (dense(300, 260), 0)
    out['designed-200x36'] = (designed(200, 36, 2.0 ** -np.arange(12)), 0)
    out['designed-300x132'] = (designed(300, 132, 3.0 ** -np.arange(10)), 0)
    out['collapsed-257x132'] = (collapsed(257, 132), 0)
    out['offset-257x36'] = (offset(257, 36), 0)
    out['rankdef-64x36'] = (rank_deficient(64, 36), 0)
    out['rankdef-256x132'] = (rank_deficient(256, 132), 0)
    out['dense-257x132'] = (dense(257, 132, 3), 3)
    out['few-40x64'] = (random_rows(40, 64), 0)
    out['few-7x8'] = (random_rows(7, 8, 3), 3)
    return out
