"""float64 reference of the nearest-neighbour contract (include/argsim_vae.h, avae_knn) on the fp32 inputs, the inputs of the
tests, and the judge of a device run.

The device sums in fp32 and the reference in float64, so a device list is judged tolerantly, never by equality with the
reference's list:
    (a) every returned score is within tol of the float64 score of the returned index (a score that is not finite must be the
        same non-finite value);
    (b) the returned set holds every admissible row whose float64 score exceeds the reference's k-th by more than tol and no
        row below it by more than tol, each row once, and as many rows as there are admissible ones (up to k);
    (c) the device list is ordered by ITS OWN scores under order_key, ties to the lower index, real entries first, then
        (-1, -inf).
Nothing is left out of the comparison."""
import functools

import numpy as np

METRICS = ('dot', 'cos', 'euc')
# (n, N, dim, k): query-tile remainders 1, 3, 33, 65, 130; bank-tile remainders 127, 129, 777, 4099; dim 4 .. 1024; k 1 .. 32
CASES = [(3, 129, 20, 5), (33, 1000, 128, 32), (65, 4099, 128, 10), (5, 777, 1024, 32), (1, 127, 4, 1), (130, 2500, 64, 32)]
LOW, NAN_LOW = -1e300, -2e300      # stand-ins for -inf and NaN where scores are compared with a tolerance


def make_inputs(n, N, dim, seed=0):
    """8 cluster centres of norm about 1; every row 0.7 centre + noise, scaled so that norms are about 1, float32.  Planted: two
    duplicates of bank row 1 (at N // 2 and N - 1), bank row 3 zero, q[0] = bank[1]."""
    rng = np.random.default_rng(1000 * seed + 7 * n + 3 * N + dim)
    centres = rng.standard_normal((8, dim)) / np.sqrt(dim)
    noise = np.sqrt(1.0 - 0.49) / np.sqrt(dim)
    def rows(m):
        return (0.7 * centres[rng.integers(0, 8, m)] + noise * rng.standard_normal((m, dim))).astype(np.float32)
    q, bank = rows(n), rows(N)
    if N > 3:
        bank[N // 2] = bank[1]
        bank[N - 1] = bank[1]
        bank[3] = 0.0
    if N > 1:
        q[0] = bank[1]
    return q, bank


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    n, N, dim, k = case
    q, bank = make_inputs(n, N, dim)
    q.setflags(write=False)
    bank.setflags(write=False)
    return q, bank


def scores64(q, bank, metric):
    """(n, N) float64 scores of the contract on the fp32 rows"""
    q, b = np.asarray(q, np.float64), np.asarray(bank, np.float64)
    with np.errstate(all='ignore'):
        d = q @ b.T if b.shape[0] else np.zeros((q.shape[0], 0))
        q2, b2 = (q * q).sum(1), (b * b).sum(1)
        if metric == 'dot':
            return d
        if metric == 'cos':
            nq, nb = np.sqrt(q2), np.sqrt(b2)
            s = d / (nq[:, None] * nb[None, :])
            s[(nq == 0)[:, None] | (nb == 0)[None, :]] = 0.0
            return s
        if metric == 'euc':
            t = (q2[:, None] - 2.0 * d) + b2[None, :]
            t = np.where(t < 0, 0.0, t)           # (a NaN stays a NaN)
            return -t
    raise ValueError(metric)


@functools.lru_cache(maxsize=None)
def case_scores(case, metric):
    s = scores64(*case_inputs(case), metric)
    s.setflags(write=False)
    return s


def comparable(s):
    """scores as float64 values that order like order_key and survive a subtraction: NaN lowest, below -inf"""
    s = np.asarray(s, np.float64)
    with np.errstate(invalid='ignore'):
        v = np.clip(s, LOW, -LOW)
    return np.where(np.isnan(s), NAN_LOW, v)


def order_key(x):
    """the device's order_key on float32 values: larger float, larger key; +-0 equal; NaN = 0, below -inf"""
    x = np.ascontiguousarray(x, np.float32).copy()
    x[x == 0] = 0.0
    u = x.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(x)] = 0
    return key


def topk(scores, k, idx_base=0, self_base=-1, carry=None):
    """the reference list: (idx int64 (n, k), score float64 (n, k)) of the (n, N) scores under (score descending, global index
    ascending), query i never taking global index self_base + i, -1 / -inf in missing slots; carry = (idx, score) of earlier
    calls is merged as one more list"""
    n, N = scores.shape
    out_i = np.full((n, k), -1, np.int64)
    out_s = np.full((n, k), -np.inf)
    for i in range(n):
        gi = idx_base + np.arange(N, dtype=np.int64)
        s = np.asarray(scores[i], np.float64)
        keep = np.ones(N, bool) if self_base < 0 else gi != self_base + i
        gi, s = gi[keep], s[keep]
        if carry is not None:
            have = carry[0][i] >= 0
            gi, s = np.concatenate([gi, carry[0][i][have]]), np.concatenate([s, np.asarray(carry[1][i], np.float64)[have]])
        order = np.lexsort((gi, -comparable(s)))[:k]
        out_i[i, :len(order)], out_s[i, :len(order)] = gi[order], s[order]
    return out_i, out_s


def judge(dev_idx, dev_score, scores, k, tol, idx_base=0, self_base=-1):
    """asserts (a), (b), (c) of the module docstring for a device result over bank rows idx_base .. idx_base + N of `scores`
    (n, N) float64; -> the largest |device score - float64 score| over the finite entries"""
    n, N = scores.shape
    dev_idx, dev_score = np.asarray(dev_idx), np.asarray(dev_score)
    assert dev_idx.shape == (n, k) and dev_idx.dtype == np.int64 and dev_score.shape == (n, k) and dev_score.dtype == np.float32
    ref_i, ref_s = topk(scores, k, idx_base, self_base)
    keys = order_key(dev_score)
    worst = 0.0
    for i in range(n):
        m = int((ref_i[i] >= 0).sum())
        got = dev_idx[i]
        assert (got[:m] >= 0).all() and (got[m:] == -1).all(), (i, got, m)
        assert np.isneginf(dev_score[i, m:]).all(), (i, dev_score[i])
        loc = got[:m] - idx_base
        assert len(set(loc.tolist())) == m and (loc >= 0).all() and (loc < N).all(), (i, got)
        if self_base >= 0:
            assert self_base + i not in got[:m].tolist(), (i, got)
        # (c) the device's own order
        for j in range(m - 1):
            assert keys[i, j] > keys[i, j + 1] or (keys[i, j] == keys[i, j + 1] and got[j] < got[j + 1]), (i, j, got, dev_score[i])
        # (a) the scores
        want, have = scores[i, loc], dev_score[i, :m].astype(np.float64)
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(want), np.isnan(have)) and np.array_equal(want[~fin & ~np.isnan(want)], have[~fin & ~np.isnan(want)]), (i, want, have)
        if fin.any():
            err = np.abs(want[fin] - have[fin])
            assert err.max() <= tol, (i, float(err.max()), tol)
            worst = max(worst, float(err.max()))
        # (b) the set
        if m:
            v = comparable(scores[i])
            kth = comparable(ref_s[i, m - 1])
            adm = np.ones(N, bool)
            if self_base >= 0 and 0 <= self_base + i - idx_base < N:
                adm[self_base + i - idx_base] = False
            must = np.flatnonzero(adm & (v > kth + tol))
            assert np.isin(must, loc).all(), (i, "missing", np.setdiff1d(must, loc))
            assert (v[loc] >= kth - tol).all(), (i, "too low", loc[v[loc] < kth - tol])
    return worst


def small_gaps(scores, k, self_base=-1, eps=1e-5):
    """share of the queries whose k-th / (k+1)-th float64 gap is positive and <= eps"""
    n, N = scores.shape
    ref_i, ref_s = topk(scores, min(k + 1, 64) if k + 1 <= N else k, 0, self_base)
    if ref_s.shape[1] <= k:
        return 0.0
    gap = comparable(ref_s[:, k - 1]) - comparable(ref_s[:, k])
    return float(((gap > 0) & (gap <= eps) & (ref_i[:, k] >= 0)).mean())
