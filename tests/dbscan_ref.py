"""float64 restatement of avae_dbscan (include/argsim_vae.h), the cases the tests share, and the CPU model of the device's round rule.

The definition is order-free:
  * p(i, j) = sum_e (v_i[e] - v_j[e])^2 in double, v = double(x), for the cosine divided by the row's norm (a zero row stays zero, and a
    pair with a zero row and i != j has p = 2);
  * within eps iff p <= thr, thr = eps * eps (euclidean) or 2 eps (cosine), inclusive;
  * a row is core when at least min_samples rows, itself included, are within eps of it;
  * core rows within eps of each other share a cluster; clusters are numbered in ascending order of their lowest core row;
  * a non-core row with a core row within eps takes the lowest cluster number among those core rows; every other non-core row is -1.

A "random" case has a margin: every pair's p is at least 1e-9 thr away from thr, far above the error of a double sum of dim <= 1024
terms ((dim + 3) 2^-52), so every correct double evaluation decides every pair the same way.  An "exact" case has small integers as
coordinates and an eps whose double square is an integer: p is exact, and pairs at exactly eps are inside."""
import numpy as np

METRICS = ('euclidean', 'cosine')
MARGIN = 1e-9


def rows_value(x, metric):
    v = np.asarray(x, np.float32).astype(np.float64)
    if metric == 1:
        rn = np.sqrt((v * v).sum(1))
        v = np.divide(v, rn[:, None], out=np.zeros_like(v), where=rn[:, None] > 0)
    return v


def pair_values(x, metric):
    """(N, N) float64 p"""
    v = rows_value(x, metric)
    n = v.shape[0]
    p = np.empty((n, n))
    step = max(1, (1 << 22) // max(1, n * v.shape[1]))
    for b in range(0, n, step):
        d = v[b:b + step, None, :] - v[None, :, :]
        p[b:b + step] = (d * d).sum(2)
    if metric == 1:
        zero = ~(np.asarray(x, np.float32).astype(np.float64) ** 2).sum(1).astype(bool)
        m = zero[:, None] | zero[None, :]
        np.fill_diagonal(m, False)
        p[m] = 2.0
    return p


def threshold(metric, eps):
    eps = float(eps)
    return 2.0 * eps if metric == 1 else eps * eps


def margin(x, metric, eps):
    """the minimum over the pairs i != j of |p - thr| / thr (inf without pairs)"""
    p = pair_values(x, metric)
    thr = threshold(metric, eps)
    off = ~np.eye(p.shape[0], dtype=bool)
    return float(np.min(np.abs(p[off] - thr) / thr)) if off.any() else float('inf')


def dbscan(x, metric, eps, min_samples):
    """-> dict(label (N,), count (N,), core (N,) bool, stat = clusters, core rows, border rows, noise rows)"""
    A = pair_values(x, metric) <= threshold(metric, eps)
    n = A.shape[0]
    count = A.sum(1).astype(np.int64)
    core = count >= min_samples
    root = np.full(n, -1, np.int64)
    for s in np.flatnonzero(core):                      # ascending: a component is found from its lowest core row
        if root[s] >= 0:
            continue
        root[s] = s
        todo = [s]
        while todo:
            i = todo.pop()
            for j in np.flatnonzero(A[i] & core & (root < 0)):
                root[j] = s
                todo.append(j)
    roots = np.unique(root[core])
    number = {int(r): k for k, r in enumerate(roots)}
    label = np.full(n, -1, np.int64)
    label[core] = [number[int(r)] for r in root[core]]
    for i in np.flatnonzero(~core):
        near = np.flatnonzero(A[i] & core)
        if near.size:
            label[i] = label[near].min()
    border = int((~core & (label >= 0)).sum())
    return dict(label=label, count=count, core=core, stat=np.array([len(roots), int(core.sum()), border, int((label < 0).sum())]))


# ---------------------------------------------------------------- cases
def blobs(n, dim, seed):
    """three blobs and a fifth of uniform rows, shuffled"""
    rng = np.random.default_rng(seed)
    c = rng.normal(0.0, 2.0, (3, dim))
    x = c[rng.integers(0, 3, n)] + rng.normal(0.0, 1.0 / np.sqrt(2.0 * dim), (n, dim))
    far = rng.random(n) < 0.2
    x[far] = rng.uniform(-3.0, 3.0, (int(far.sum()), dim))
    return np.ascontiguousarray(x, np.float32)


def _round3(v):
    return float('%.3g' % v)


def pick_eps(x, metric, q=0.12):
    """an eps of three digits near the q-quantile of the pair distances (1 without pairs): some rows core, some border, some noise"""
    p = pair_values(x, metric)
    off = p[~np.eye(p.shape[0], dtype=bool)]
    if off.size == 0:
        return 1.0
    v = float(np.quantile(off, q))
    return max(_round3(v / 2.0 if metric == 1 else np.sqrt(v)), 1e-3)


RANDOM_SHAPES = [(n, dim) for n in (1, 2, 63, 64, 65, 127, 128, 129, 257) for dim in (4, 36, 132)]
_CACHE = {}


def random_case(n, dim, metric):
    """-> (x, eps, min_samples) of the "random" case, with the margin"""
    key = (n, dim, metric)
    if key not in _CACHE:
        x = blobs(n, dim, 1000 * n + dim)
        _CACHE[key] = (x, pick_eps(x, metric), 4)
    return _CACHE[key]


def _grid(w, h, dim=4):
    x = np.zeros((w * h, dim), np.float32)
    x[:, 0] = np.repeat(np.arange(h), w)
    x[:, 2] = np.tile(np.arange(w), h)
    return x


def _line(pos, dim=4, col=1):
    x = np.zeros((len(pos), dim), np.float32)
    x[:, col] = pos
    return x


def bridge():
    """a non-core row between two clusters: it is border, takes cluster 0, and the clusters stay two"""
    pos = [2.0, 2.1, 2.2, 2.3, 2.4, 0.0, -0.1, -0.2, -0.3, -0.4, 1.0]
    return _line(pos, 8, 0), 1.0, 5, [0] * 5 + [1] * 5 + [0], [6, 5, 5, 5, 5, 6, 5, 5, 5, 5, 3]


def numbering():
    """row 0 is a border row of the cluster whose lowest CORE row is 4; the cluster of core row 2 is cluster 0"""
    return _line([20, 0, 1, 2, 21, 22, 23]), 1.0, 3, [1, 0, 0, 0, 1, 1, 1]


def cosine_rows():
    """a row, a zero row, two scaled copies of the first (p = 0 exactly: powers of two) and a row at 1 - cos = 0.59 from them"""
    return np.array([[1, 2, 3, 4], [0, 0, 0, 0], [2, 4, 6, 8], [0.5, 1, 1.5, 2], [-1, 0, 2, 0]], np.float32)


# name -> (x, metric, eps, min_samples): integer coordinates, p exact, pairs at exactly eps
EXACT = {
    'grid_at_eps': (_grid(7, 9), 0, 1.0, 5),
    'grid_pythagoras': (_grid(12, 9), 0, 5.0, 60),
    'grid_two': (_grid(13, 11), 0, 2.0, 13),
    'all_core': (_line([0, 1, 2, 5, 9, 10, 14, 14, 30, 3]), 0, 1.0, 1),
    'all_noise': (_grid(5, 5), 0, 1.0, 26),
    'duplicates': (np.repeat(_line([0, 1, 4, 5, 5, 9]), 3, axis=0), 0, 1.0, 4),
    'two_words': (_line(np.arange(130) // 2 * 2), 0, 2.0, 4),
}


def orders(n, seed=0):
    """name -> where each point of a shape goes: ascending, descending, bit-reversed, random"""
    bits = max(1, int(n - 1).bit_length())
    rev = np.array([int(format(i, '0%db' % bits)[::-1], 2) for i in range(n)])
    return dict(ascending=np.arange(n), descending=np.arange(n)[::-1].copy(), bitrev=np.argsort(np.argsort(rev, kind='stable'), kind='stable'),
                random=np.random.default_rng(seed + n).permutation(n))


def chain(n, order):
    """n integer points 0 .. n - 1 on a line, point k in row order[k]; eps 1, min_samples 3: one cluster, the two ends border"""
    pos = np.empty(n)
    pos[order] = np.arange(n)
    return _line(pos)


def ring(n, order):
    """n points on the integer square ring of side n / 4 (n a multiple of 4), point k in row order[k]: every row has two neighbours at 1"""
    s = n // 4
    k = np.arange(n)
    side, t = k // s, k % s
    px = np.where(side == 0, t, np.where(side == 1, s, np.where(side == 2, s - t, 0)))
    py = np.where(side == 0, 0, np.where(side == 1, t, np.where(side == 2, s, s - t)))
    x = np.zeros((n, 4), np.float32)
    x[order, 0] = px
    x[order, 3] = py
    return x


# ---------------------------------------------------------------- the round rule
def round_model(n, src, dst):
    """The device's rounds on the core graph with the edges (src[k], dst[k]) (both directions given; a row is its own neighbour):
      hook   m_i = min(P[i], min over neighbours j of P[j]); where m_i < P[i]: Q[P[i]] = min(Q[P[i]], m_i), Q[i] = min(Q[i], m_i), from Q = P
      jump   P[i] = the root of i in Q
    until a hook changes nothing -> (P, the number of hooks run).  Minima commute: the result does not depend on an order."""
    P = np.arange(n)
    t = 0
    while True:
        t += 1
        m = P.copy()
        np.minimum.at(m, src, P[dst])
        ch = np.flatnonzero(m < P)
        if ch.size == 0:
            return P, t
        Q = P.copy()
        np.minimum.at(Q, P[ch], m[ch])
        np.minimum.at(Q, ch, m[ch])
        while True:
            R = Q[Q]
            if np.array_equal(R, Q):
                break
            Q = R
        P = Q


def default_rounds(n, a=1, b=1):
    """the planner's default max_rounds: twice a ceil(log2 n) + b"""
    return 2 * (a * int(n - 1).bit_length() + b)


def _both(e):
    e = np.asarray(e, np.int64).reshape(-1, 2)
    return np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])


def shape_edges(kind, n):
    """the edges of an adversarial shape on the points 0 .. n - 1"""
    k = np.arange(n)
    if kind == 'chain':
        return np.stack([k[:-1], k[1:]], 1)
    if kind == 'ring':
        return np.stack([k, (k + 1) % n], 1)
    if kind == 'star':
        return np.stack([np.full(n - 1, n // 2), np.delete(k, n // 2)], 1)
    if kind == 'comb':                                  # a spine of the even points, a tooth on each
        spine = k[::2]
        return np.concatenate([np.stack([spine[:-1], spine[1:]], 1), np.stack([k[1::2] - 1, k[1::2]], 1)])
    if kind == 'tree':                                  # the binary heap's tree
        return np.stack([(k[1:] - 1) // 2, k[1:]], 1)
    raise ValueError(kind)


SHAPES = ('chain', 'ring', 'star', 'comb', 'tree')
FAMILY_N = (2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32, 33, 64, 100, 128, 255, 256, 257, 512, 1000, 1024, 2048, 4095, 4096)


def family_rounds(ns=FAMILY_N):
    """n -> (the worst number of rounds of the model over the shapes and orders, where)"""
    worst = {}
    for n in ns:
        for kind in SHAPES:
            e = shape_edges(kind, n)
            for name, o in orders(n).items():
                src, dst = _both(o[e])
                P, t = round_model(n, src, dst)
                assert (P == 0).all(), (kind, n, name)
                if t > worst.get(n, (0, None))[0]:
                    worst[n] = (t, '%s/%s' % (kind, name))
    return worst
