"""float64 reference of the linear probes (include/argsim_vae.h, avae_probe_fit): the objective, its gradient, an exact-Hessian
Newton method run to |grad f| <= 1e-12, and the shapes and inputs the CPU and GPU tests share.

Problem p minimises f(w) = 1/2 |w|^2 + sum_i |s_i| softplus(-sgn(s_i) w . x~_i), x~_i = (x_i, 1): strongly convex with modulus 1, so
|w - w*| <= |grad f(w)| for any w (the certificate the GPU test checks)."""
import numpy as np

# (N, P, dim): the kernel has ONE tile form -- row tiles of 128, problem tiles of 32 -- and the cases hold the remainders 1,
# tile - 1 and tile + 1 on both axes (N 129 / 257, 127, 129; P 33 / 65, 31, 33), each of the dims 4, 36, 128 and 1024 once, a second
# row tile, a second and third problem tile, and with dim 1024 fewer rows than dims
CASES = ((129, 33, 4), (127, 31, 36), (257, 65, 128), (200, 7, 1024))
CASE_IDS = ['N%d-P%d-d%d' % c for c in CASES]
_CACHE = {}


def tilde(x):
    x = np.asarray(x, np.float64)
    return np.concatenate([x, np.ones((x.shape[0], 1))], axis=1)


def _softplus(t):
    return np.maximum(t, 0.0) + np.log1p(np.exp(-np.abs(t)))


def _sigmoid(t):
    e = np.exp(-np.abs(t))
    return np.where(t >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def objective64(x, s, w):
    """f of one problem: x (N, dim), s (N,) signed costs, w (dim + 1,)"""
    s = np.asarray(s, np.float64)
    m = np.sign(s) * (tilde(x) @ np.asarray(w, np.float64))
    return 0.5 * float(np.dot(w, w)) + float(np.sum(np.abs(s) * _softplus(-m)))


def grad64(x, s, w):
    s = np.asarray(s, np.float64)
    w = np.asarray(w, np.float64)
    xt = tilde(x)
    m = np.sign(s) * (xt @ w)
    return w + xt.T @ (-s * _sigmoid(-m))


def newton64(x, s, tol=1e-12, max_iter=200):
    """exact-Hessian Newton with backtracking from w = 0 until |grad f| <= tol -> w* (dim + 1,)"""
    s = np.asarray(s, np.float64)
    xt = tilde(x)
    keep = s != 0                      # a cost of 0 leaves the row out
    xt, s = xt[keep], s[keep]
    y, c = np.sign(s), np.abs(s)
    n = xt.shape[1]
    w = np.zeros(n)
    f = lambda v: 0.5 * np.dot(v, v) + np.sum(c * _softplus(-y * (xt @ v)))
    for _ in range(max_iter):
        m = y * (xt @ w)
        g = w + xt.T @ (-s * _sigmoid(-m))
        if np.linalg.norm(g) <= tol:
            break
        d = c * _sigmoid(m) * _sigmoid(-m)
        step = -np.linalg.solve(np.eye(n) + xt.T @ (d[:, None] * xt), g)
        # Armijo, or -- where the decrease of f is below its rounding, next to the optimum -- a step that halves the gradient
        a, f0, gp, gn = 1.0, f(w), float(np.dot(g, step)), np.linalg.norm(g)
        grad_at = lambda v: v + xt.T @ (-s * _sigmoid(-y * (xt @ v)))
        while a > 1e-12 and f(w + a * step) > f0 + 1e-4 * a * gp and np.linalg.norm(grad_at(w + a * step)) > 0.5 * gn:
            a *= 0.5
        w = w + a * step
    return w


def case_inputs(case):
    """-> x (N, dim) float32, s (P, N) float32.  The rows are float32 draws around 4 class centres 2.5 apart (unit noise).
    Problem p is class p % 4 against the rest with balanced weights, at C = 0.001 (p even) or C = 1 (p odd), trained on the rows
    outside fold p % 5 -- the held-out rows have cost 0 and lie scattered among the others -- except
        problem 1: every row with a positive cost (one sign);  problem 2 (P > 2): every cost 0;  problem 3 (P > 3): one sign, negative"""
    if ('in', case) in _CACHE:
        return _CACHE['in', case]
    N, P, dim = case
    rng = np.random.default_rng(1000 + N + 7 * P + dim)
    cls = rng.integers(0, 4, N)
    if N >= 8:
        cls[:8] = np.arange(8) % 4
    centres = rng.standard_normal((4, dim))
    centres *= (2.5 / np.sqrt(2.0)) / np.linalg.norm(centres, axis=1, keepdims=True)
    x = (centres[cls] + rng.standard_normal((N, dim))).astype(np.float32)
    fold = rng.integers(0, 5, N)
    s = np.zeros((P, N), np.float64)
    for p in range(P):
        C = 0.001 if p % 2 == 0 else 1.0
        train = fold != p % 5
        if not train.any():
            train[:] = True
        pos = cls == p % 4
        npos, nneg = max(int((pos & train).sum()), 1), max(int((~pos & train).sum()), 1)
        T = float(train.sum())
        s[p] = np.where(train, np.where(pos, C * T / (2.0 * npos), -C * T / (2.0 * nneg)), 0.0)
    if P > 1:
        s[1] = 1.0 + rng.random(N)
    if P > 2:
        s[2] = 0.0
    if P > 3:
        s[3] = -0.001 * (1.0 + rng.random(N))
    x.setflags(write=False)
    s = s.astype(np.float32)
    s.setflags(write=False)
    _CACHE['in', case] = (x, s)
    return x, s


def case_ref(case):
    """-> w* (P, dim + 1) float64 of the case, computed once"""
    if ('ref', case) not in _CACHE:
        x, s = case_inputs(case)
        w = np.stack([newton64(x, s[p]) for p in range(s.shape[0])])
        w.setflags(write=False)
        _CACHE['ref', case] = w
    return _CACHE['ref', case]


def g0_64(x, s):
    """|grad f(0)| of every problem: s (P, N) -> (P,)"""
    return np.array([np.linalg.norm(grad64(x, s[p], np.zeros(x.shape[1] + 1))) for p in range(s.shape[0])])


# ---- the cross-validation case: 2 topics (4 and 2 classes), 5 folds: 5 x 4 + 5 x 1 = 25 problems over 300 rows of dim 36
CV_N, CV_DIM, CV_C, CV_TOL = 300, 36, 0.001, 1e-4


def cv_inputs():
    """-> z (N, dim) float32, labels (N,) strings, folds (N,), groups (N,).  Class centres 4 apart (unit noise): chosen, with C, so
    that under the worst-case certificate 2 tol g0 at most 5 % of the rows are too close to call (tests/test_probe.py asserts it)"""
    if 'cv' in _CACHE:
        return _CACHE['cv']
    rng = np.random.default_rng(77)
    groups = np.where(np.arange(CV_N) < 200, 'a', 'b')
    cls = np.where(groups == 'a', rng.integers(0, 4, CV_N), rng.integers(0, 2, CV_N))
    centres = rng.standard_normal((2, 4, CV_DIM))
    centres *= (4.0 / np.sqrt(2.0)) / np.linalg.norm(centres, axis=2, keepdims=True)
    z = (centres[(groups == 'b').astype(int), cls] + rng.standard_normal((CV_N, CV_DIM))).astype(np.float32)
    labels = np.array(['c%d' % c for c in cls])
    folds = rng.permutation(CV_N) % 5
    for a in (z, labels, folds, groups):
        a.setflags(write=False)
    _CACHE['cv'] = (z, labels, folds, groups)
    return _CACHE['cv']


def decision_bound(x, w):
    """the standard bound on an fp32 dot product of dim + 1 terms summed in any order: (dim + 2) 2^-24 sum_j |w_j| |x~_ij| -> (n, P)"""
    return (x.shape[1] + 2) * 2.0 ** -24 * (np.abs(tilde(x)) @ np.abs(np.asarray(w, np.float64)).T)


def undecided(x, classes, dec, werr, dbound):
    """rows whose prediction a perturbation of the model within its certificate could change: dec (n, P) float64 decisions of one
    job, werr (P,) bounds on |w - w*|, dbound (n, P) the decision's own rounding bound.  The top-two gap (|decision| at K = 2) is
    at most twice the certificate's bound times |x~_i|, plus the decision bound"""
    if len(classes) < 2:
        return np.zeros(x.shape[0], bool)
    norm = np.linalg.norm(tilde(x), axis=1)
    slack = 2.0 * np.max(werr) * norm + 2.0 * np.max(dbound, axis=1)
    if len(classes) == 2:
        return np.abs(dec[:, 0]) <= slack
    top = np.sort(dec, axis=1)
    return top[:, -1] - top[:, -2] <= slack
