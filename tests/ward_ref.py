"""float64 reference of the Ward clustering of include/argsim_vae.h (avae_ward, avae_ward_cut): numpy only.

    ward(x)            the contract itself: pair values Delta(A, B) = |A||B| / (|A| + |B|) |c_A - c_B|^2 from double sums, difference
                       first, rounded once to fp32; every step merges the smallest stored value, ties to the lowest a, then the lowest
                       b; a cluster lives in the slot of its smallest member row.  Also reports, per merge, the relative gap between
                       the smallest and the second-smallest DISTINCT stored value and how many alive pairs hold the smallest.
    follow(x, pair)    replays a given merge list: the float64 Delta of every chosen pair and the float64 minimum over all alive pairs
                       at that state -- the certificate the GPU test holds a device's own tree to.  Incremental: O(n dim) per merge
                       plus the rescans of the rows whose cached minimum was retired.
    cut(pair, n, k)    slot labels after the first n - k merges.
CASES are the shapes of tests/test_gpu_ward.py; tests/test_ward.py checks on the CPU that they hold what that file says."""
import numpy as np

MIN_GAP = 2.0 ** -20

# (n, dim, seed): Gaussian rows plus 5 planted centres.  n crosses the wave (64) and the workgroup (256, 1024-thread) boundaries, dims
# 4, 36, 128, 1024 use 1, 9, 32 lanes of a wave and all four chunks.  tests/test_ward.py asserts that every merge of every exact
# case is decided by a gap >= MIN_GAP, so that an fp32 value one ulp off cannot change the tree.
CASES = [(33, 4, 0), (129, 36, 1), (300, 128, 2), (130, 1024, 3)]
CASE_IDS = ['%dx%d' % c[:2] for c in CASES]
# certificate-only inputs: a jittered lattice (near-ties everywhere) and one group of more than 1024 rows, far beyond the planner's one-workgroup threshold
NEAR_TIES = ('lattice', 200, 4, 7)
BIG = (1100, 36, 11)
# groups of one call in the independence test, dim 36
GROUP_SIZES = [1, 2, 3, 64, 65, 200]


def planted(n, dim, seed, k=5):
    r = np.random.default_rng(seed)
    return (r.standard_normal((n, dim)) + 1.5 * r.standard_normal((k, dim))[r.integers(0, k, n)]).astype(np.float32)


def case_inputs(case):
    if case[0] == 'lattice':
        _, n, dim, seed = case
        r = np.random.default_rng(seed)
        return (r.integers(0, 4, (n, dim)) + 1e-6 * r.standard_normal((n, dim))).astype(np.float32)
    return planted(*case)


def tie_inputs(m=9, dim=4, seed=5):
    """m distinct small-integer rows, each 4 times, shuffled: the first 3 m merges have Delta = 0 in any arithmetic"""
    r = np.random.default_rng(seed)
    base = np.unique(r.integers(-3, 4, (4 * m, dim)), axis=0)
    base = base[r.permutation(len(base))[:m]]
    assert len(base) == m
    return np.repeat(base, 4, axis=0)[r.permutation(4 * m)].astype(np.float32)


def _values(S, cnt, a, ks):
    """float64 Delta(a, k) for the slots ks: direct form"""
    ca, ck = S[a] / cnt[a], S[ks] / cnt[ks][:, None]
    return cnt[a] * cnt[ks] / (cnt[a] + cnt[ks]) * ((ca - ck) ** 2).sum(1)


def ward(x):
    """-> dict(pair (n - 1, 2) int32 slots a < b, delta (n - 1) float32, size (n - 1) int32, gap (n - 1), unique (n - 1) bool)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    n = x.shape[0]
    S, cnt, alive = x.copy(), np.ones(n), np.ones(n, bool)
    D = np.full((n, n), np.inf, np.float32)
    for i in range(n - 1):
        D[i, i + 1:] = _values(S, cnt, i, np.arange(i + 1, n)).astype(np.float32)
    pair, delta, size = np.zeros((n - 1, 2), np.int32), np.zeros(n - 1, np.float32), np.zeros(n - 1, np.int32)
    gap, unique = np.full(n - 1, np.inf), np.ones(n - 1, bool)
    for t in range(n - 1):
        a, b = np.unravel_index(np.argmin(D), D.shape)              # row-major first: the lowest a, then the lowest b
        m = D[a, b]
        rest = D[(D > m) & np.isfinite(D)]
        if rest.size and m > 0:
            gap[t] = (float(rest.min()) - float(m)) / float(m)
        unique[t] = (D == m).sum() == 1
        pair[t], delta[t], size[t] = (a, b), m, cnt[a] + cnt[b]
        S[a] += S[b]
        cnt[a] += cnt[b]
        alive[b] = False
        D[b, :] = np.inf
        D[:, b] = np.inf
        ks = np.flatnonzero(alive)
        ks = ks[ks != a]
        if len(ks):
            d = _values(S, cnt, a, ks).astype(np.float32)
            D[ks[ks < a], a] = d[ks < a]
            D[a, ks[ks > a]] = d[ks > a]
    return dict(pair=pair, delta=delta, size=size, gap=gap, unique=unique)


def follow(x, pair):
    """-> (chosen, least) float64, one entry per given merge (a prefix of a tree will do): Delta of merge t's pair and the minimum over
    all alive pairs before merge t"""
    x = np.asarray(x, np.float32).astype(np.float64)
    n = x.shape[0]
    S, cnt, alive = x.copy(), np.ones(n), np.ones(n, bool)
    D = np.full((n, n), np.inf)
    for i in range(n - 1):
        D[i, i + 1:] = _values(S, cnt, i, np.arange(i + 1, n))
    rmin, rarg = D.min(1), D.argmin(1)
    chosen, least = np.zeros(len(pair)), np.zeros(len(pair))
    for t in range(len(pair)):
        a, b = int(pair[t][0]), int(pair[t][1])
        assert 0 <= a < b < n and alive[a] and alive[b], (t, a, b)
        chosen[t], least[t] = D[a, b], rmin[alive].min()
        S[a] += S[b]
        cnt[a] += cnt[b]
        alive[b] = False
        D[b, :] = np.inf
        D[:, b] = np.inf
        ks = np.flatnonzero(alive)
        ks = ks[ks != a]
        if len(ks):
            d = _values(S, cnt, a, ks)
            D[ks[ks < a], a] = d[ks < a]
            D[a, ks[ks > a]] = d[ks > a]
        stale = np.flatnonzero(alive & ((rarg == a) | (rarg == b)) & (np.arange(n) < b))
        for i in set(stale.tolist()) | {a}:
            rmin[i], rarg[i] = D[i].min(), D[i].argmin()
        lo = ks[ks < a]
        better = D[lo, a] < rmin[lo]
        rmin[lo[better]], rarg[lo[better]] = D[lo[better], a], a
    return chosen, least


def cut(pair, n, k):
    """slot of every row's cluster after the first n - k merges"""
    p = np.arange(n)
    for a, b in np.asarray(pair)[:n - k]:
        p[b] = a
    out = np.arange(n)
    for i in range(n):
        while p[out[i]] != out[i]:
            out[i] = p[out[i]]
    return out
