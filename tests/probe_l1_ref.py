"""float64 reference of the L1 probes (include/argsim_vae.h, avae_probe_fit_l1): the objective, its minimum-norm subgradient, the
proximal Newton method of the device in numpy (run to tol 1e-10), and the shapes and inputs the CPU and GPU tests share.

Problem p minimises F(w) = |w|_1 + sum_i |s_i| softplus(-sgn(s_i) w . x~_i), x~_i = (x_i, 1), the bias inside the 1-norm (liblinear
with intercept_scaling = 1).  With g = X~^T r the gradient of the smooth part, the minimum-norm subgradient is v_j = g_j + sgn(w_j)
where w_j != 0 and sgn(g_j) max(|g_j| - 1, 0) where w_j = 0; w is optimal iff v(w) = 0."""
import numpy as np

from probe_ref import _sigmoid, _softplus, tilde

_CACHE = {}

# A coordinate of a reference optimum is DECIDED when it is zero with |g_j| <= 1 - GAP_G or nonzero with |w_j| >= GAP_W; the others
# may be at most CAP of dim + 1 per problem (tests/test_probe_l1.py holds every case to it on the CPU)
GAP_G, GAP_W, CAP = 0.04, 0.02, 0.05


def loss64(xt, s, w):
    return float(np.sum(np.abs(s) * _softplus(-np.sign(s) * (xt @ w))))


def objective64(x, s, w):
    """F of one problem: x (N, dim), s (N,) signed costs, w (dim + 1,)"""
    w = np.asarray(w, np.float64)
    return float(np.sum(np.abs(w))) + loss64(tilde(x), np.asarray(s, np.float64), w)


def grad64(x, s, w):
    """the gradient of the smooth part"""
    s, xt = np.asarray(s, np.float64), tilde(x)
    return xt.T @ (-s * _sigmoid(-np.sign(s) * (xt @ np.asarray(w, np.float64))))


def subgrad(g, w):
    return np.where(w != 0, g + np.sign(w), np.sign(g) * np.maximum(np.abs(g) - 1.0, 0.0))


def v64(x, s, w):
    """the minimum-norm subgradient of F at w"""
    return subgrad(grad64(x, s, w), np.asarray(w, np.float64))


def v0_64(x, s):
    """|v(0)|_1 of every problem: s (P, N) -> (P,)"""
    return np.array([np.abs(v64(x, s[p], np.zeros(x.shape[1] + 1))).sum() for p in range(s.shape[0])])


def soft(a, t):
    return np.sign(a) * np.maximum(np.abs(a) - t, 0.0) + 0.0


def prox_newton64(x, s, tol=1e-10, max_newton=200, max_inner=5000, count=None):
    """the method of the device in float64: proximal Newton from w = 0; the inner problem min_d g.d + 1/2 d.Hd + |w + d|_1 by FISTA
    with backtracking on L (from the largest diagonal entry of H) and adaptive restart until |v_q|_1 <= 0.1 |v|_1; Armijo on the
    composite objective; stop at |v(w)|_1 <= tol |v(0)|_1 -> w (dim + 1,).  count: a dict that receives outer / hv"""
    s = np.asarray(s, np.float64)
    xt = tilde(x)
    keep = s != 0
    xt, s = xt[keep], s[keep]
    y, c = np.sign(s), np.abs(s)
    n = xt.shape[1]
    w = np.zeros(n)
    v0 = None
    outer = hv = 0
    for outer in range(max_newton + 1):
        m = y * (xt @ w)
        g = xt.T @ (-s * _sigmoid(-m))
        vn = np.abs(subgrad(g, w)).sum()
        v0 = vn if v0 is None else v0
        if vn <= tol * v0 or outer == max_newton:
            break
        D = c * _sigmoid(m) * _sigmoid(-m)
        L = float(np.max((xt * xt).T @ D))
        d, Hd, yy, Hy, t = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), 1.0
        for _ in range(max_inner):
            cand = soft(w + yy - (g + Hy) / L, 1.0 / L) - w
            Hc = xt.T @ (D * (xt @ cand))
            hv += 1
            delta = cand - yy
            if np.dot(delta, Hc - Hy) > L * np.dot(delta, delta):
                L, t, yy, Hy = 2.0 * L, 1.0, d, Hd
                continue
            restart = np.dot(yy - cand, cand - d) > 0
            tn = 1.0 if restart else 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
            beta = 0.0 if restart else (t - 1.0) / tn
            yy, Hy = cand + beta * (cand - d), Hc + beta * (Hc - Hd)
            d, Hd, t = cand, Hc, tn
            if np.abs(subgrad(g + Hd, w + d)).sum() <= 0.1 * vn:
                break
        u = xt @ d
        z = xt @ w
        w1 = np.abs(w).sum()
        delta = float(np.dot(g, d)) + np.abs(w + d).sum() - w1
        phi = lambda a: np.sum(c * _softplus(-y * (z + a * u)))
        a, phi0 = 1.0, phi(0.0)
        while a > 2.0 ** -21 and (phi(a) - phi0) + (np.abs(w + a * d).sum() - w1) > 0.01 * a * delta:
            a *= 0.5
        w = w + a * d
    if count is not None:
        count.update(outer=outer, hv=hv)
    return w + 0.0


# ---- the cases: (N, dim, K, P, scale, C, seed).  Rows are unit noise around K class centres planted on two columns per class
# (centre value 3), times scale.  Problem p is class p % K against the rest (K = 2: class 1 positive, as liblinear) at cost
# C (1 + 0.1 (p // K)) and no class weights.  The seeds were searched on the CPU for decided coordinates (see GAP_G, GAP_W, CAP).
# The scikit-learn cases have P = K (1 for K = 2) at one C: a LogisticRegression fit of the labels is the same model.
SK_CASES = ((256, 32, 3, 3, 1.0, 0.1, 0), (200, 128, 2, 1, 1.0, 0.1, 0), (384, 64, 4, 4, 0.05, 0.1, 0))
# the device cases: N a partial tile, a tile + 1, two tiles + 1; dim 4 .. 260 (DT 1 and 4, 260 no multiple of 32); P one problem, a
# short tile, a second problem tile
GPU_CASES = ((127, 4, 2, 1, 1.0, 0.1, 0), (129, 32, 3, 3, 1.0, 0.1, 0), (257, 128, 3, 33, 1.0, 0.1, 0), (200, 260, 3, 3, 1.0, 0.1, 0))
CASE_ID = lambda c: 'N%d-d%d-K%d-P%d' % c[:4]


def case_labels(case):
    """-> x (N, dim) float32, labels (N,) int64"""
    if ('xy', case) not in _CACHE:
        N, dim, K, P, scale, C, seed = case
        rng = np.random.default_rng(5000 + 131 * seed + N + 3 * dim + K)
        cls = rng.integers(0, K, N)
        cls[:2 * K] = np.arange(2 * K) % K
        centres = np.zeros((K, dim))
        for k in range(K):
            centres[k, (2 * k) % dim] = centres[k, (2 * k + 1) % dim] = 3.0
        x = ((centres[cls] + rng.standard_normal((N, dim))) * scale).astype(np.float32)
        x.setflags(write=False)
        cls.setflags(write=False)
        _CACHE['xy', case] = (x, cls)
    return _CACHE['xy', case]


def case_inputs(case):
    """-> x (N, dim) float32, s (P, N) float32"""
    if ('in', case) not in _CACHE:
        N, dim, K, P, scale, C, seed = case
        x, cls = case_labels(case)
        s = np.zeros((P, N), np.float64)
        for p in range(P):
            k = 1 if K == 2 else p % K
            s[p] = np.where(cls == k, 1.0, -1.0) * C * (1.0 + 0.1 * (p // K))
        s = s.astype(np.float32)
        s.setflags(write=False)
        _CACHE['in', case] = (x, s)
    return _CACHE['in', case]


def case_ref(case):
    """-> w* (P, dim + 1) float64 of the case, computed once"""
    if ('ref', case) not in _CACHE:
        x, s = case_inputs(case)
        w = np.stack([prox_newton64(x, s[p]) for p in range(s.shape[0])])
        w.setflags(write=False)
        _CACHE['ref', case] = w
    return _CACHE['ref', case]


def decided(x, s, w):
    """-> bool (dim + 1,): the coordinates of the optimum w of one problem whose membership of the support is decided"""
    g = grad64(x, s, w)
    return np.where(w == 0, np.abs(g) <= 1.0 - GAP_G, np.abs(w) >= GAP_W)


def case_decided(case):
    """-> bool (P, dim + 1)"""
    if ('dec', case) not in _CACHE:
        x, s = case_inputs(case)
        ref = case_ref(case)
        _CACHE['dec', case] = np.stack([decided(x, s[p], ref[p]) for p in range(s.shape[0])])
    return _CACHE['dec', case]


def useful_dims(coef):
    """eval_clustering.py:57 with an exact zero: the columns with a nonzero coefficient in any class"""
    return np.flatnonzero((np.asarray(coef) != 0).any(axis=0)).astype(np.int64)
