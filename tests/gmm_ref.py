"""float64 restatement of the contract of avae_gmm_fit / avae_gmm_score (include/argsim_vae.h): scikit-learn 1.7.2's GaussianMixture with
'diag' or 'spherical' covariances -- the E-step, the M-step, the start, the loop with its stops, restarts and the best of them; the margins
under which the device must reproduce every decision; the derived one-step error bounds; the inputs of the test cases.

Bounds (derived from operation counts, none measured; EPS = 2^-53, a double sum of n terms is good to n EPS of the sum of magnitudes, an
exp or a log to 2 EPS relative).  All are bounds on ONE step from the same input parameters:
  q_ic       the rows are fp32 numbers, exact as doubles.  A term (x - mu)^2 p: the difference EPS, the square EPS, p = 1 / cov EPS, the fma
             EPS, each relative to at most (|x| + |mu|)^2 p; the chain over dim terms adds dim EPS of the sum of magnitudes:
             q_bound = (3 dim + 8) EPS sum_j (|x_j| + |mu_j|)^2 p_j.
  t_ic       half of q_bound, and (dim + 8) EPS (|log w| + 1/2 sum_j |log cov_j| + (dim / 2) log 2 pi + q / 2) for the logs (2 EPS each), their
             sum over dim terms and the three subtractions.
  lse_i      lse is a smooth maximum: an error of the t_ic moves it by at most their largest.  Forming it takes k exps (2 EPS, and EPS |t - m|
             of the argument's rounding, weighted by exp(t - m): at most EPS / e each), at most k + 20 rescalings and additions of the running
             pair (4 EPS each, relative to the sum), one log and one addition: max_c t_bound + (5 k + 100) EPS + 2 EPS |lse|.
  r_ic       r expm1(t_bound + lse_bound + EPS |t - lse| + 2 EPS).
  n_c, mu    a sum over N rows is good to (N + 4) EPS of the sum of magnitudes, and moves by sum_i r_bound_ic |term|; the quotient carries
             both errors and EPS of its own.
  cov        the same applied to av = sum r x^2 / n_c and to mu^2; cov = av - mu^2 + reg adds 2 EPS (av + mu^2 + reg).  Nothing here is
             relative to cov itself: this is the cancellation of the one-pass form, stated.  Spherical: the mean of the bounds and
             (dim + 2) EPS of the mean magnitude.
  weights    w_c = n_c / sum n: n_bound_c / sum n + w_c sum_c n_bound / sum n + (k + 4) EPS w_c.
  lower      the mean of lse_bound and (N + 4) EPS of the mean |lse|."""
import numpy as np

from ap_ref import gaussian, pad4, planted      # noqa: F401  (the inputs)

EPS = 2.0 ** -53
MARGIN = 2.0 ** -30
LOG2PI = float(np.log(2.0 * np.pi))
TEN_EPS = 10.0 * 2.0 ** -52
STOPS = ('converged', 'max_iter', 'degenerate')
COVS = {'diag': 0, 'spherical': 1}


def _rel_gap(a, b):
    """|a - b| relative to the larger magnitude (inf where both are 0 or either is not finite: no decision hangs on it)"""
    m = max(abs(a), abs(b))
    return abs(a - b) / m if 0 < m < np.inf else np.inf


# ---------------------------------------------------------------- E, M
def scores(X, w, mu, cov, pad=0):
    """t_ic (N, k).  pad: the last pad columns are padding (their variance is 1 whatever cov holds; the constant counts dim - pad)"""
    X = np.asarray(X, np.float64)
    N, dim = X.shape
    cov = np.array(cov, np.float64)
    if pad:
        cov[:, dim - pad:] = 1.0
    with np.errstate(divide='ignore', invalid='ignore'):            # (a degenerate restart's variances: the result is unspecified)
        prec = 1.0 / cov
        q = np.zeros((N, mu.shape[0]))
        for j in range(dim):
            d = X[:, j, None] - mu[None, :, j]
            q += (d * d) * prec[None, :, j]
        lc = (np.log(w) - 0.5 * np.log(cov).sum(1)) - 0.5 * (dim - pad) * LOG2PI
        return lc[None, :] - 0.5 * q, q


def estep(X, w, mu, cov, pad=0):
    """-> dict(t, q, lse, resp, lower, labels)"""
    t, q = scores(X, w, mu, cov, pad)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        m = t.max(1)
        s = np.zeros(t.shape[0])
        for c in range(t.shape[1]):
            s += np.exp(t[:, c] - m)
        lse = m + np.log(s)
        resp = np.exp(t - lse[:, None])
    return dict(t=t, q=q, lse=lse, resp=resp, lower=lse.sum() / t.shape[0], labels=t.argmax(1))


def mstep(X, resp, reg, spherical, pad=0):
    """-> (weights, means, covars (k, dim), n_c)"""
    X = np.asarray(X, np.float64)
    N, dim = X.shape
    n = resp.sum(0) + TEN_EPS
    mu = (resp.T @ X) / n[:, None]
    cov = (resp.T @ (X * X)) / n[:, None] - mu * mu + reg
    if pad:
        cov[:, dim - pad:] = 1.0
    if spherical:
        cov[:, :dim - pad] = (cov[:, :dim - pad].sum(1) / (dim - pad))[:, None]
    w = n / N
    return w / w.sum(), mu, cov, n


def onehot(lab, k):
    lab = np.asarray(lab)
    r = np.zeros((lab.shape[0], k))
    ok = (lab >= 0) & (lab < k)
    r[np.flatnonzero(ok), lab[ok]] = 1.0
    return r


def _bad(cov):
    return bool((~(cov > 0) | ~np.isfinite(cov)).any())


def em(X, k, spherical, max_iter, tol, reg, w, mu, cov, pad=0):
    """one restart from parameters -> dict(weights, means, covars, n_iter, stop, lower, trace, stop_margin)"""
    trace = np.full(max_iter, -np.inf)
    prev, it, how, margin, lower = -np.inf, 0, 1, np.inf, -np.inf
    if _bad(cov):
        how = 2
    else:
        for it in range(1, max_iter + 1):
            e = estep(X, w, mu, cov, pad)
            w, mu, cov, _ = mstep(X, e['resp'], reg, spherical, pad)
            lower = e['lower']
            trace[it - 1] = lower
            if _bad(cov) or not np.isfinite(lower):
                how, lower = 2, -np.inf
                break
            change = lower - prev
            prev = lower
            if tol > 0 and np.isfinite(change):
                margin = min(margin, abs(abs(change) - tol) / tol)
            if abs(change) < tol:
                how = 0
                break
    return dict(weights=w, means=mu, covars=cov, n_iter=it if max_iter else 0, stop=how, lower=lower, trace=trace, stop_margin=margin)


def start_from_labels(X, lab, k, reg, spherical, pad=0):
    w, mu, cov, _ = mstep(X, onehot(lab, k), reg, spherical, pad)
    return w, mu, cov


def run(x, k, covariance='diag', n_init=1, max_iter=100, tol=1e-3, reg_covar=1e-6, init=None, pad=0):
    """the whole call.  init: labels (n_init, N) or dict(weights (n_init, k), means, covariances (n_init, k, dim)) -> dict(best, runs,
    starts, lowers, stop_margin, label_gap, best_margin) and the best run's fields with labels, logp, resp of its final E-step"""
    X = np.asarray(x, np.float64)
    sph = COVS[covariance]
    runs, starts = [], []
    for r in range(n_init):
        if isinstance(init, dict):
            s = tuple(np.array(np.asarray(init[n], np.float64)[r]) for n in ('weights', 'means', 'covariances'))
        else:
            s = start_from_labels(X, np.asarray(init).reshape(n_init, -1)[r], k, reg_covar, sph, pad)
        starts.append(s)
        runs.append(em(X, k, sph, max_iter, tol, reg_covar, *s, pad=pad))
    lowers = np.array([q['lower'] for q in runs])
    ok = [r for r in range(n_init) if runs[r]['stop'] != 2]
    best = 0
    for r in ok:
        if best not in ok or lowers[r] > lowers[best]:
            best = r
    best_margin = min([_rel_gap(lowers[best], lowers[r]) for r in ok if r != best], default=np.inf)
    out = dict(runs[best])
    b = runs[best]
    fin = estep(X, b['weights'], b['means'], b['covars'], pad)
    gap = np.inf
    if k > 1 and b['stop'] != 2:
        two = np.sort(fin['t'], axis=1)[:, -2:]
        gap = float(((two[:, 1] - two[:, 0]) / np.maximum(np.abs(two).max(1), 1.0)).min())
    out.update(best=best, runs=runs, starts=starts, lowers=lowers, labels=fin['labels'], logp=fin['lse'], resp=fin['resp'],
               stop_margin=min(q['stop_margin'] for q in runs), label_gap=gap, best_margin=best_margin)
    return out


def restarts_have_margins(res):
    """every decision inside the restarts has its margin: the iterations and stop codes of every restart, the best one's labels"""
    return bool(res['stop_margin'] > MARGIN and res['label_gap'] > MARGIN)


def has_margins(res):
    """... and so has the choice of the best restart"""
    return restarts_have_margins(res) and bool(res['best_margin'] > MARGIN)


# ---------------------------------------------------------------- bounds of one step
def estep_bounds(X, w, mu, cov, e, pad=0):
    """bounds on the error of estep's t, lse, resp and lower, given its result e"""
    X = np.asarray(X, np.float64)
    N, dim = X.shape
    k = mu.shape[0]
    cov = np.array(cov, np.float64)
    if pad:
        cov[:, dim - pad:] = 1.0
    qb = np.zeros((N, k))
    for j in range(dim):
        qb += (np.abs(X[:, j, None]) + np.abs(mu[None, :, j])) ** 2 / cov[None, :, j]
    qb *= (3 * dim + 8) * EPS
    const = np.abs(np.log(w)) + 0.5 * np.abs(np.log(cov)).sum(1) + 0.5 * dim * LOG2PI
    tb = 0.5 * qb + (dim + 8) * EPS * (const[None, :] + 0.5 * e['q'])
    lb = tb.max(1) + (5 * k + 100) * EPS + 2 * EPS * np.abs(e['lse'])
    rb = e['resp'] * np.expm1(tb + lb[:, None] + EPS * np.abs(e['t'] - e['lse'][:, None]) + 2 * EPS)
    lowb = lb.mean() + (N + 4) * EPS * np.abs(e['lse']).mean()
    return dict(t=tb, lse=lb, resp=rb, lower=lowb)


def mstep_bounds(X, resp, rb, reg, spherical, pad=0):
    """bounds on the error of mstep(X, resp, ..) where resp itself is good to rb -> dict(weights, means, covars, n)"""
    X = np.asarray(X, np.float64)
    N, dim = X.shape
    k = resp.shape[1]
    A = np.abs(X)
    n = resp.sum(0) + TEN_EPS
    nb = rb.sum(0) + (N + 4) * EPS * n
    nlo = np.maximum(n - nb, 1e-300)[:, None]
    s1b = rb.T @ A + (N + 4) * EPS * (resp.T @ A)
    mu = (resp.T @ X) / n[:, None]
    mub = (s1b + np.abs(mu) * nb[:, None]) / nlo + EPS * np.abs(mu)
    av = (resp.T @ (A * A)) / n[:, None]
    s2b = rb.T @ (A * A) + (N + 4) * EPS * (resp.T @ (A * A))
    avb = (s2b + av * nb[:, None]) / nlo + EPS * av
    sqb = 2 * np.abs(mu) * mub + mub * mub + EPS * mu * mu
    cb = avb + sqb + 2 * EPS * (av + mu * mu + reg)
    if pad:
        cb[:, dim - pad:] = 0.0
    if spherical:
        d = dim - pad
        cb[:, :d] = (cb[:, :d].sum(1) / d + (d + 2) * EPS * (av + mu * mu + reg)[:, :d].sum(1) / d)[:, None]
    w = n / n.sum()
    wb = nb / n.sum() + w * nb.sum() / n.sum() + (k + 4) * EPS * w
    return dict(weights=wb, means=mub, covars=cb, n=nb)


def step_bounds(X, w, mu, cov, reg, spherical, pad=0):
    """one EM step from (w, mu, cov): the reference's result and the bounds on every output of it"""
    e = estep(X, w, mu, cov, pad)
    eb = estep_bounds(X, w, mu, cov, e, pad)
    w2, mu2, cov2, _ = mstep(X, e['resp'], reg, spherical, pad)
    mb = mstep_bounds(X, e['resp'], eb['resp'], reg, spherical, pad)
    return dict(e=e, eb=eb, weights=w2, means=mu2, covars=cov2, mb=mb)


# ---------------------------------------------------------------- inputs
def start_labels(N, k, n_init=1, seed=5):
    """random labels with the first k rows labelled 0 .. k - 1 (no component starts empty)"""
    lab = np.random.default_rng(seed).integers(0, k, (n_init, N)).astype(np.int32)
    lab[:, :k] = np.arange(k)
    return lab


# (name, rows, k): the margin cases; has_margins is asserted for each of them by tests/test_gmm.py
CASES = [('planted96x8', lambda: planted(96, 8, 6, 1), 6), ('gauss37x12', lambda: pad4(gaussian(37, 12, 2)), 3),
         ('planted257x16', lambda: planted(257, 16, 9, 3, spread=2.0), 9), ('gauss200x128', lambda: gaussian(200, 128, 4), 5),
         ('gauss500x32', lambda: gaussian(500, 32, 4), 7)]
CASE_IDS = [c[0] for c in CASES]


# the whole runs of the margin cases: three restarts from different random labels
RUN_KW = dict(n_init=3, max_iter=100, tol=1e-3, reg_covar=1e-6)


def whole_run(name, covariance):
    """-> (x, k, labels (3, N), the reference's run) of a margin case"""
    _, make, k = CASES[CASE_IDS.index(name)]
    x = make()
    lab = start_labels(x.shape[0], k, RUN_KW['n_init'])
    return x, k, lab, run(x, k, covariance, init=lab, **RUN_KW)


def repeated_points():
    """24 rows that are 4 points repeated 6 times, and their exact labels: every variance collapses"""
    return np.tile(gaussian(4, 8, 5), (6, 1)), (np.arange(24) % 4).astype(np.int32)


def bic_aic(lower, N, k, dim, covariance):
    """sklearn's n_parameters, bic and aic from the mean log-likelihood `lower` of N rows"""
    cov_p = k * dim if covariance == 'diag' else k
    n_par = int(cov_p + k * dim + k - 1)
    return n_par, -2.0 * lower * N + n_par * np.log(N), -2.0 * lower * N + 2 * n_par
