"""float64 restatement of the contract of avae_silhouette (include/argsim_vae.h): the three distances, the silhouette of every row for
every labeling, its means, the Calinski-Harabasz (CH) and the Davies-Bouldin (DB) index; unlabelled rows; the margins under which
`nearest` must be reproduced exactly; the derived error bounds; the small shapes of the test cases.

Bounds (derived from operation counts, none measured; EPS = 2^-53, a double sum of n terms is good to n EPS of the sum of magnitudes;
the tests allow twice a bound, since the reference errs as well):
  distance   metrics 0 and 2: the rows are fp32 numbers, exact as doubles; a difference, its square and the sum over dim positive terms
             are good to (dim + 3) EPS relative, the root halves that and adds one: (dim + 4) EPS d covers both.  Cosine: an element of
             a unit row errs by (dim + 3) EPS relative (kmeans_ref), a product of two by twice that, the sum adds dim + 1, and
             sum_j |X_ij X_kj| <= 1: (3 dim + 10) EPS absolute.
  a, b       a sum of n distances adds n EPS of itself, the division one more: with nmax the largest cluster
             (3 dim + 10) EPS [cosine] + (dim + 4 [not cosine] + nmax + 1) EPS times the value.  The minimum of perturbed means moves
             by at most the largest relative perturbation of a mean times b itself.
  s          (b - a) / max: (ea + eb) (1 + |s|) / max(a, b) + 2 EPS.
  means      the mean of n values s: the mean of their bounds + (n + 2) EPS of the mean magnitude.
  member mean  an element of m_c: (n_c + dim + 6) EPS (mean_members |X_ij| + max_i |X_ij|), as kmeans_ref.centre_bound; the labelled
             rows' mean likewise with n'.
  trW        a row's |X_i - m_c|^2 errs by 2 sum_j |X_ij - m_cj| (em_cj + ex_ij) + (dim + 3) EPS of itself, ex the element error of
             a cosine row; the sum adds (n' + 1) EPS.  trB likewise from the errors of m_c and m.  CH: the two relative errors + 4 EPS.
  roots      |sqrt(e + t) - sqrt(e)| <= min(|t| / sqrt(e), sqrt(|t|)), + EPS of the root.
  DB         S_c: the mean of the rows' root bounds + (n_c + 1) EPS; R: ((eS + eS') + R eM) / (M - eM) + 2 EPS R; the maximum of
             perturbed values moves by at most the largest perturbation; the mean adds (k' + 1) EPS."""
import numpy as np

from ap_ref import gaussian, pad4, planted      # noqa: F401  (the inputs)
from kmeans_ref import rows_of

EPS = 2.0 ** -53
MARGIN = 2.0 ** -30
METRICS = {'euclidean': 0, 'cosine': 1, 'sqeuclidean': 2}


# ---------------------------------------------------------------- distances
def distances(x, metric):
    """(N, N) d(i, k) on the rows of the contract: by differences for metrics 0 and 2"""
    X = rows_of(x, 1 if metric == 1 else 0)
    if metric == 1:
        return np.minimum(np.maximum(1.0 - X @ X.T, 0.0), 2.0)
    D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    return np.sqrt(D) if metric == 0 else D


def _valid(lab, K):
    lab = np.asarray(lab, np.int64)
    return np.where((lab >= 0) & (lab < K), lab, -1)


# ---------------------------------------------------------------- one labeling
def one(x, metric, lab, K, D=None):
    """the outputs of one labeling -> dict(score, sil, a, b, nearest, count, cluster_mean, ch, db and what the bounds need)"""
    N = len(lab)
    lab = _valid(lab, K)
    on = lab >= 0
    with np.errstate(invalid='ignore'):
        D = np.array(distances(x, metric) if D is None else D)
    np.fill_diagonal(D, 0.0)                                 # k = i is left out of every sum
    cnt = np.bincount(lab[on], minlength=K).astype(np.int64)
    S = np.zeros((N, K))
    for c in range(K):
        m = lab == c
        if m.any():
            S[:, c] = D[:, m].sum(1)
    idx = np.flatnonzero(on)
    a, b, s = np.zeros(N), np.zeros(N), np.zeros(N)
    near = np.full(N, -1, np.int64)
    second = np.full(N, np.inf)
    live = cnt > 0
    for i in idx:
        c = lab[i]
        if cnt[c] > 1:
            a[i] = S[i, c] / (cnt[c] - 1)
        other = live.copy()
        other[c] = False
        if other.any():
            means = np.where(other, S[i] / np.maximum(cnt, 1), np.inf)
            near[i] = int(np.argmin(means))                  # the first of equals
            b[i] = means[near[i]]
            if other.sum() > 1:
                second[i] = np.partition(means, 1)[1]
        mx = max(a[i], b[i])
        if cnt[c] > 1 and other.any() and mx > 0:
            s[i] = (b[i] - a[i]) / mx
    cm = np.array([s[lab == c].mean() if cnt[c] else 0.0 for c in range(K)])
    out = dict(sil=s, a=a, b=b, nearest=near, count=cnt, cluster_mean=cm, score=s[on].mean() if on.any() else 0.0, second=second, label=lab)
    out.update(indices(x, metric, lab, K))
    return out


def indices(x, metric, lab, K):
    """CH and DB of one labeling (lab already validated) -> dict(ch, db, trW, trB, means, gmean, e, S, R (over the non-empty clusters in
    ascending order), kp, n)"""
    X = rows_of(x, 1 if metric == 1 else 0)
    on = lab >= 0
    cnt = np.bincount(lab[on], minlength=K)
    kp, n = int((cnt > 0).sum()), int(on.sum())
    dim = X.shape[1]
    M = np.zeros((K, dim))
    np.add.at(M, lab[on], X[on])
    g = M.sum(0) / n if n else np.zeros(dim)
    M = M / np.maximum(cnt, 1)[:, None]
    e = np.zeros(len(lab))
    e[on] = ((X[on] - M[lab[on]]) ** 2).sum(1)
    trW = e.sum()
    trB = (cnt * ((M - g) ** 2).sum(1))[cnt > 0].sum()
    ch, db = np.nan, np.nan
    if kp >= 2 and n > kp:
        ch = 1.0 if trW == 0 else (trB / (kp - 1)) / (trW / (n - kp))
    Sc = np.zeros(K)
    np.add.at(Sc, lab[on], np.sqrt(e[on]))
    Sc = Sc / np.maximum(cnt, 1)
    live = np.flatnonzero(cnt > 0)                          # R over the non-empty clusters only: (k', k')
    R = np.zeros((kp, kp))
    if kp >= 2:
        Ml, Sl = M[live], Sc[live]
        Mcc = np.sqrt(((Ml[:, None, :] - Ml[None, :, :]) ** 2).sum(-1))
        with np.errstate(divide='ignore', invalid='ignore'):
            R = np.where(Mcc > 0, (Sl[:, None] + Sl[None, :]) / Mcc, 0.0)
        R[np.arange(kp), np.arange(kp)] = 0.0
        db = R.max(1).sum() / kp
    return dict(ch=ch, db=db, trW=trW, trB=trB, means=M, gmean=g, e=e, S=Sc, R=R, kp=kp, n=n)


def run(x, metric, labels, K):
    """the whole call: x (N, dim) fp32, labels (L, N), K (L) -> list of one() per labeling.  Rows unlabelled in a labeling may hold
    anything: only the labelled rows of a labeling enter it"""
    labels = np.atleast_2d(labels)
    out = []
    for lab, k in zip(labels, K):
        lab = _valid(lab, k)
        on = lab >= 0
        xs = np.where(on[:, None], np.asarray(x, np.float64), 0.0).astype(np.float32)      # what is unlabelled here cannot enter
        out.append(one(xs, metric, lab, int(k)))
    return out


def brute(x, metric, lab, K):
    """the silhouette of one labeling by three plain loops -> (a, b, s, nearest)"""
    X = rows_of(x, 1 if metric == 1 else 0)
    N, dim = X.shape
    lab = _valid(lab, K)
    a, b, s, near = [0.0] * N, [0.0] * N, [0.0] * N, [-1] * N
    for i in range(N):
        if lab[i] < 0:
            continue
        tot, num = [0.0] * K, [0] * K
        for k in range(N):
            if lab[k] < 0:
                continue
            num[lab[k]] += 1
            if k == i:
                continue
            if metric == 1:
                d = min(max(1.0 - sum(X[i, j] * X[k, j] for j in range(dim)), 0.0), 2.0)
            else:
                d = sum((X[i, j] - X[k, j]) ** 2 for j in range(dim))
                d = d ** 0.5 if metric == 0 else d
            tot[lab[k]] += d
        c = lab[i]
        if num[c] > 1:
            a[i] = tot[c] / (num[c] - 1)
        best = None
        for q in range(K):
            if q != c and num[q] > 0 and (best is None or tot[q] / num[q] < best):
                best, near[i] = tot[q] / num[q], q
        if best is not None:
            b[i] = best
        if num[c] > 1 and best is not None and max(a[i], b[i]) > 0:
            s[i] = (b[i] - a[i]) / max(a[i], b[i])
    return np.array(a), np.array(b), np.array(s), np.array(near)


def has_margins(ref):
    """on every labelled row the smallest and the second-smallest other-cluster mean differ by a relative 2^-30: nearest is decided"""
    on = (ref['label'] >= 0) & np.isfinite(ref['second'])
    b, s2 = ref['b'][on], ref['second'][on]
    return bool((s2 - b > MARGIN * s2).all())


# ---------------------------------------------------------------- bounds
def bounds(x, metric, ref):
    """-> dict(a, b, s (N,), score, cluster_mean (K,), ch, db): bounds on the error of the fields of one()'s result"""
    X = rows_of(x, 1 if metric == 1 else 0)
    N, dim = X.shape
    lab, cnt = ref['label'], ref['count']
    on = lab >= 0
    K = len(cnt)
    nmax = int(cnt.max()) if K else 0
    absd = (3 * dim + 10) * EPS if metric == 1 else 0.0
    rel = ((0 if metric == 1 else dim + 4) + nmax + 1) * EPS
    ea, eb = absd + rel * ref['a'], absd + rel * ref['b']
    mx = np.maximum(ref['a'], ref['b'])
    es = np.where(mx > 0, (ea + eb) * (1 + np.abs(ref['sil'])) / np.where(mx > 0, mx, 1.0), 0.0) + 2 * EPS
    es = np.where(on, es, 0.0)
    n = int(on.sum())
    score = (es[on].sum() + (n + 2) * EPS * np.abs(ref['sil'][on]).sum()) / max(n, 1)
    cm = np.array([(es[lab == c].sum() + (cnt[c] + 2) * EPS * np.abs(ref['sil'][lab == c]).sum()) / max(cnt[c], 1) for c in range(K)])
    # CH and DB
    ex = (dim + 3) * EPS * np.abs(X) if metric == 1 else np.zeros_like(X)
    A = np.zeros((K, dim))
    np.add.at(A, lab[on], np.abs(X[on]))
    top = np.abs(X[on]).max(0) if n else np.zeros(dim)
    em = (cnt + dim + 6)[:, None] * EPS * (A / np.maximum(cnt, 1)[:, None] + top[None, :])
    eg = (n + dim + 6) * EPS * (A.sum(0) / max(n, 1) + top)
    M, g = ref['means'], ref['gmean']
    ee = np.zeros(N)
    ee[on] = 2 * (np.abs(X[on] - M[lab[on]]) * (em[lab[on]] + ex[on])).sum(1) + (dim + 3) * EPS * ref['e'][on]
    etrW = ee.sum() + (n + 1) * EPS * ref['trW']
    live = cnt > 0
    d2 = ((M - g) ** 2).sum(1)
    etrB = (cnt * (2 * (np.abs(M - g) * (em + eg[None, :])).sum(1) + (dim + 3) * EPS * d2))[live].sum() + (ref['kp'] + 2) * EPS * ref['trB']
    ch = np.nan
    if np.isfinite(ref['ch']):
        ch = 0.0 if ref['trW'] == 0 else ref['ch'] * (etrB / ref['trB'] + etrW / ref['trW'] + 4 * EPS)
    root = np.sqrt(ref['e'])
    with np.errstate(divide='ignore', invalid='ignore'):
        er = np.minimum(np.where(root > 0, ee / root, np.inf), np.sqrt(ee)) + EPS * root
    eS = np.zeros(K)
    np.add.at(eS, lab[on], er[on])
    eS = eS / np.maximum(cnt, 1) + (cnt + 1) * EPS * ref['S']
    db = np.nan
    if np.isfinite(ref['db']):
        Ml, eml, eSl, kp = M[live], em[live], eS[live], ref['kp']
        Mcc = np.sqrt(((Ml[:, None, :] - Ml[None, :, :]) ** 2).sum(-1))
        t = 2 * (np.abs(Ml[:, None, :] - Ml[None, :, :]) * (eml[:, None, :] + eml[None, :, :])).sum(-1) + (dim + 3) * EPS * Mcc ** 2
        with np.errstate(divide='ignore', invalid='ignore'):
            eM = np.minimum(np.where(Mcc > 0, t / Mcc, np.inf), np.sqrt(t)) + EPS * Mcc
            eR = np.where(Mcc > 2 * eM, ((eSl[:, None] + eSl[None, :]) + ref['R'] * eM) / (Mcc - eM) + 2 * EPS * ref['R'], np.inf)
        eR = np.where(Mcc == 0, 0.0, eR)                     # coincident centroids: R = 0 on both sides
        eR[np.arange(kp), np.arange(kp)] = 0.0
        db = eR.max(1).sum() / kp + (kp + 1) * EPS * ref['db']
    return dict(a=np.where(on, ea, 0.0), b=np.where(on, eb, 0.0), s=es, score=score, cluster_mean=cm, ch=ch, db=db)


# ---------------------------------------------------------------- inputs
def labels_of(N, K, seed, empty=()):
    """N labels in [0, K) from the generator, none of them in `empty` (cluster ids with no members)"""
    r = np.random.default_rng(seed)
    ok = np.array([c for c in range(K) if c not in empty])
    return ok[r.integers(0, len(ok), N)].astype(np.int32)


# (name, rows, [K per labeling], cluster ids left without members): the small shapes of tests/test_gpu_silhouette.py; has_margins is
# asserted for each of them and every metric by tests/test_silhouette.py
CASES = [('n2', lambda: gaussian(2, 4, 1), [2], ()),
         ('n3', lambda: gaussian(3, 4, 2), [2, 3, 3], ()),
         ('n65x12', lambda: pad4(gaussian(65, 12, 3)), [2, 3, 7], (1,)),
         ('n130x12', lambda: pad4(gaussian(130, 12, 4)), [3, 7, 70, 2, 7], (5,)),
         ('n257x128', lambda: gaussian(257, 128, 5), [7, 70, 3], (0, 6)),
         ('n130x4', lambda: planted(130, 4, 5, 6), [7], ()),
         ('n65x128', lambda: gaussian(65, 128, 7), [70], (3, 69))]
CASE_IDS = [c[0] for c in CASES]


def case_labels(case):
    name, make, Ks, empty = case
    x = make()
    N = x.shape[0]
    labs = np.stack([labels_of(N, k, 10 * j + N, [e for e in empty if e < k and k > 2]) for j, k in enumerate(Ks)])
    if N <= 3:
        labs = np.stack([np.arange(N, dtype=np.int32) % min(k, N) for k in Ks])          # every cluster of a tiny case has a member
        if N == 3:
            labs[1] = [0, 2, 0]                                                          # and one labeling an empty cluster in between
    return x, labs, np.array(Ks, np.int32)
