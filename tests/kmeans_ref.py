"""float64 restatement of the contract of avae_kmeans (include/argsim_vae.h): the generator's uniforms as the device forms them, greedy
k-means++ seeding, Lloyd iterations with the relocation of empty clusters, the cosine form, restarts and the best of them; the margins
under which the device must reproduce every decision; the derived error bounds; the inputs of the test cases.

Bounds (derived from operation counts, none measured; EPS = 2^-53, a double sum of n terms is good to n EPS of the sum of magnitudes):
  distance   the rows are fp32 numbers, exact as doubles; for the cosine a row is divided by its norm, itself a sum of dim squares and a
             root: (dim + 3) EPS relative per element.  A term (x - c)^2 then errs by at most 2 (dim + 5) EPS (|x| + |c|)^2 and the sum
             over dim terms adds dim EPS of it: dist_bound = (3 dim + 12) EPS sum_j (|x_j| + |c_j|)^2.
  centre     the labels being equal, a centre is a function of its members alone: a sum of n member elements (each (dim + 3) EPS relative
             for the cosine), a relocated row subtracted, one division: (n + dim + 6) EPS sum_members |x_ij| / n per element.  The
             projection of the cosine form divides by the norm: an element error e_j becomes (e_j + |c_j| |e|_2 / |c|_2) / |c|_2, and
             (dim + 4) EPS |c_j| for the norm's own sum and the division.
  inertia    per row dist_bound, the effect of the centre's error 2 sum_j |x_j - c_j| e_j + sum_j e_j^2, and (N + 2) EPS of the sum."""
import math

import numpy as np

from ap_ref import gaussian, mix64, pad4, planted      # noqa: F401  (the inputs and the generator's mixer)

EPS = 2.0 ** -53
MARGIN = 2.0 ** -30
M64 = (1 << 64) - 1
STOPS = ('converged', 'tol', 'max_iter')


# ---------------------------------------------------------------- the counter generator (csrc/sample_dev.h), stream 7
def uniform01(seed, stream, idx):
    """the device's fp32 value as a double: (float)(24 bits + 0.5) 2^-24 -- the cast rounds to even from 2^23 on"""
    with np.errstate(over='ignore'):
        base = mix64(np.uint64(seed) ^ np.uint64((stream * 0xD6E8FEB86659FD93) & M64))
        r = mix64(base + np.asarray(idx, np.uint64))
    return ((r >> np.uint64(40)).astype(np.float64) + 0.5).astype(np.float32).astype(np.float64) / 16777216.0


def seed_index(r, c, t):
    return (((r << 20) + c) << 20) + t


def trials(k):
    return 2 + int(math.floor(math.log(k)))


# ---------------------------------------------------------------- rows, distances
def rows_of(x, metric):
    X = np.asarray(x, np.float64)
    if metric:
        n = np.sqrt((X * X).sum(1))
        X = np.divide(X, n[:, None], out=np.zeros_like(X), where=n[:, None] > 0)
    return X


def sqdist(X, C):
    return ((X[:, None, :] - C[None, :, :]) ** 2).sum(-1)


def tol_abs(X, tol):
    return tol * X.var(axis=0).mean()


def project(C):
    n = np.sqrt((C * C).sum(1))
    return np.divide(C, n[:, None], out=np.zeros_like(C), where=n[:, None] > 0)


def _rel_gap(a, b):
    """|a - b| relative to the larger magnitude (inf where both are 0: no decision hangs on it)"""
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0 else np.inf


# ---------------------------------------------------------------- seeding
def seeding(X, k, seed, r):
    """greedy k-means++ of restart r -> dict(rows, margin): margin is the smallest distance of a threshold to its neighbouring
    cumulative sums, relative to the total, and the smallest relative gap between the best potential and that of another row"""
    N = X.shape[0]
    T = trials(k)
    rows = [min(int(math.floor(float(uniform01(seed, 7, seed_index(r, 0, 0))) * N)), N - 1)]
    closest = ((X - X[rows[0]]) ** 2).sum(1)
    margin = np.inf
    for c in range(1, k):
        cum = np.cumsum(closest)
        total = cum[-1]
        thr = uniform01(seed, 7, [seed_index(r, c, t) for t in range(T)]) * total
        cand = np.minimum(np.searchsorted(cum, thr, side='left'), N - 1)
        for t in range(T):
            near = [abs(cum[cand[t]] - thr[t])] + ([abs(thr[t] - cum[cand[t] - 1])] if cand[t] > 0 else [])
            margin = min(margin, min(near) / total)
        D = np.minimum(closest[None, :], sqdist(X[cand], X))           # (T, N)
        pot = D.sum(1)
        best = int(np.argmin(pot))
        for t in range(T):
            if cand[t] != cand[best]:
                margin = min(margin, _rel_gap(pot[t], pot[best]))
        rows.append(int(cand[best]))
        closest = D[best]
    return dict(rows=np.array(rows), margin=margin)


# ---------------------------------------------------------------- Lloyd
def update(X, lab, d, k, metric):
    """steps 2 to 4 -> (new centres, relocations, counts, the smallest relative gap among the distances that decide a relocation)"""
    N = X.shape[0]
    cnt = np.bincount(lab, minlength=k).astype(np.int64)
    S = np.zeros((k, X.shape[1]))
    np.add.at(S, lab, X)
    empty = np.flatnonzero(cnt == 0)
    gap = np.inf
    if len(empty):
        order = np.lexsort((np.arange(N), -d))
        top = d[order[:len(empty) + 1]]
        for a, b in zip(top[:-1], top[1:]):
            gap = min(gap, _rel_gap(a, b))
        for e, c in enumerate(empty):
            i = order[e]
            S[lab[i]] -= X[i]; cnt[lab[i]] -= 1
            S[c] = X[i]; cnt[c] = 1
    C = np.where(cnt[:, None] > 0, S / np.maximum(cnt, 1)[:, None], S)
    if metric:
        C = project(C)
    return C, len(empty), cnt, gap


def lloyd(X, C0, max_iter, tolabs, metric=0):
    """one restart from centres C0 on prepared rows X -> dict(labels, centers, inertia, n_iter, stop, relocations, margin)"""
    N, k = X.shape[0], C0.shape[0]
    C = np.array(C0, np.float64)
    prev, reloc, margin, how = None, 0, np.inf, 2
    idx = np.arange(N)
    for it in range(max_iter):
        D = sqdist(X, C)
        lab = D.argmin(1)
        d = D[idx, lab]
        if k > 1:
            two = np.partition(D, 1, axis=1)[:, :2]
            with np.errstate(invalid='ignore', divide='ignore'):
                g = (two[:, 1] - two[:, 0]) / two[:, 1]
            margin = min(margin, np.nanmin(np.where(two[:, 1] > 0, g, 0.0)))
        Cn, ne, cnt, gap = update(X, lab, d, k, metric)
        reloc += ne
        margin = min(margin, gap)
        shift = ((Cn - C) ** 2).sum()
        C = Cn
        if prev is not None and np.array_equal(lab, prev):
            how = 0
            break
        margin = min(margin, _rel_gap(shift, tolabs) if shift > 0 or tolabs > 0 else 0.0)      # 0 against 0: rounding decides
        if shift <= tolabs:
            how = 1
            break
        prev = lab
    if how != 0:
        D = sqdist(X, C)
        lab = D.argmin(1)
        if k > 1:
            two = np.partition(D, 1, axis=1)[:, :2]
            with np.errstate(invalid='ignore', divide='ignore'):
                g = (two[:, 1] - two[:, 0]) / two[:, 1]
            margin = min(margin, np.nanmin(np.where(two[:, 1] > 0, g, 0.0)))
    inertia = ((X - C[lab]) ** 2).sum()
    return dict(labels=lab, centers=C, inertia=inertia, n_iter=it + 1, stop=how, relocations=reloc, margin=margin)


def run(x, k, metric=0, n_init=1, max_iter=300, tol=0.0, seed=0, init=None):
    """the whole call: x (N, dim) fp32; init None (k-means++) or (n_init, k, dim) -> dict(best, runs, margin, seeds) and the best run's
    fields"""
    X = rows_of(x, metric)
    ta = tol_abs(X, tol) if tol > 0 else 0.0
    runs, seeds, margin = [], [], np.inf
    for r in range(n_init):
        if init is None:
            s = seeding(X, k, seed, r)
            seeds.append(s['rows'])
            margin = min(margin, s['margin'])
            C0 = X[s['rows']]
        else:
            C0 = np.asarray(init, np.float64).reshape(-1, k, X.shape[1])[r]
        runs.append(lloyd(X, C0, max_iter, ta, metric))
        margin = min(margin, runs[-1]['margin'])
    ine = np.array([q['inertia'] for q in runs])
    best = int(np.argmin(ine))
    best_margin = min([_rel_gap(ine[best], v) for j, v in enumerate(ine) if j != best], default=np.inf)
    out = dict(runs[best])
    out.update(best=best, runs=runs, margin=margin, best_margin=best_margin, seeds=seeds, inertias=ine, tol_abs=ta, X=X)
    return out


def restarts_have_margins(res):
    """every decision inside the restarts has its margin: labels, iterations, stop codes and relocations of every restart are decided"""
    return bool(res['margin'] > MARGIN)


def has_margins(res):
    """... and so has the choice of the best restart: the two smallest inertias differ by the margin as well.  (Two restarts that reach
    the same partition have equal inertias; such a call can be compared restart by restart, but not in its best restart.)"""
    return restarts_have_margins(res) and bool(res['best_margin'] > MARGIN)


# ---------------------------------------------------------------- bounds
def dist_bound(X, C):
    """(N, k) bound on the error of sqdist(X, C)"""
    dim = X.shape[1]
    return (3 * dim + 12) * EPS * ((np.abs(X)[:, None, :] + np.abs(C)[None, :, :]) ** 2).sum(-1)


def centre_bound(X, lab, C, metric):
    """(k, dim) bound on the error of the centres update() gives for these labels (relocations included: they move one row)"""
    k, dim = C.shape
    cnt = np.maximum(np.bincount(lab, minlength=k), 1)
    A = np.zeros((k, dim))
    np.add.at(A, lab, np.abs(X))
    e = (cnt + dim + 6)[:, None] * EPS * (A / cnt[:, None] + np.abs(X).max(0)[None, :])
    if metric:
        raw = np.zeros((k, dim))
        np.add.at(raw, lab, X)
        n = np.maximum(np.sqrt(((raw / cnt[:, None]) ** 2).sum(1)), 1e-300)[:, None]
        e = (e + np.abs(C) * np.sqrt((e * e).sum(1))[:, None]) / n + (dim + 4) * EPS * np.abs(C)
    return e


def inertia_bound(X, lab, C, e):
    N = X.shape[0]
    c = C[lab]
    per = dist_bound(X, C)[np.arange(N), lab] + 2 * (np.abs(X - c) * e[lab]).sum(1) + (e[lab] ** 2).sum(1)
    return per.sum() + (N + 2) * EPS * ((X - c) ** 2).sum()


# ---------------------------------------------------------------- inputs
def far_init(x, k, seed, n_far=1):
    """k random rows as centres, the last n_far replaced by a centre at 1e3: those clusters are empty in iteration 1"""
    r = np.random.default_rng(seed)
    c = np.array(x[r.choice(x.shape[0], k, replace=False)], np.float32)
    c[k - n_far:] = 1e3
    return c


def random_init(x, k, seed, n_init=1):
    r = np.random.default_rng(seed)
    return np.stack([x[r.choice(x.shape[0], k, replace=False)] for _ in range(n_init)]).astype(np.float32)


# (name, rows, k): the margin cases; has_margins is asserted for each of them by tests/test_kmeans.py
CASES = [('planted96x8', lambda: planted(96, 8, 6, 1), 6), ('gauss37x12', lambda: pad4(gaussian(37, 12, 2)), 5),
         ('planted257x16', lambda: planted(257, 16, 9, 3, spread=2.0), 9), ('gauss200x128', lambda: gaussian(200, 128, 4), 70)]
CASE_IDS = [c[0] for c in CASES]


def case_inits(x, k):
    """the starts of a margin case: three random-row restarts, and one start with a centre at 1e3"""
    return dict(rows=random_init(x, k, 11, 3), far=far_init(x, k, 15)[None])
