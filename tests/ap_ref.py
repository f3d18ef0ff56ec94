"""float64 restatement of the contract of avae_affinity (include/argsim_vae.h): similarities, the median preference, one message-passing
step, the loop with its stopping rule and the labels; an fp32 numpy emulation of one step (step_fp32); a numpy copy of the counter
generator for the noise bound; the inputs of the test cases.

Step bounds (derived, not measured; u = 2^-24, the fp32 unit roundoff).  From a state (S, A, R) of fp32 numbers:
  R   fl(A + S) errs by u |A + S|, so the row's first and second maximum Y, Y2 err by u max_k' |A_ik' + S_ik'| (a near-tie that
      rounding resolves the other way swaps two values that far apart at most).  S - Y adds u (|S| + |Y|), the product with
      1 - lambda one more relative u, lambda R one u |R|, the final sum one relative u of a value bounded by |R| + |S| + |Y|: in all
      below 5 u (|S_ik| + max_k' |A_ik' + S_ik'| + |R_ik|), stated with 8.
  A   the column sum and R_kk + sum - max(0, R_ik) are formed in double (error ~2^-53 N times the terms) and rounded once: u times at
      most |R_kk| + sum_i max(0, R_ik); the damping adds u |A_ik| and two relative u of the result: below 4 u (|A_ik| + |R_kk| +
      sum_i max(0, R_ik)), stated with 8.  The same bound covers A_kk.
Both are evaluated on the state the step starts from and, for A, on the R the step itself produced."""
import numpy as np

U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
M64 = (1 << 64) - 1


# ---------------------------------------------------------------- the counter generator (csrc/sample_dev.h)
def mix64(x):
    with np.errstate(over='ignore'):                    # arithmetic modulo 2^64
        x = (np.asarray(x, np.uint64) + np.uint64(0x9E3779B97F4A7C15))
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def uniform01(seed, stream, idx):
    with np.errstate(over='ignore'):
        base = mix64(np.uint64(seed) ^ np.uint64((stream * 0xD6E8FEB86659FD93) & M64))
        r = mix64(base + np.asarray(idx, np.uint64))
    return ((r >> np.uint64(40)).astype(np.float64) + 0.5) / 16777216.0


def normal01(seed, stream, idx):
    """float64 value of the device's normal01 (which evaluates the same formula in fp32)"""
    idx = np.asarray(idx, np.uint64)
    u1, u2 = uniform01(seed, stream, np.uint64(2) * idx), uniform01(seed, stream, np.uint64(2) * idx + np.uint64(1))
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


NORMAL_MAX = float(np.sqrt(-2.0 * np.log(0.5 / 16777216.0)))      # the smallest u1 is 2^-25: |normal01| <= 5.887 < 6


def noise_scale(S):
    """what multiplies normal01 in the perturbation: 2^-23 |S| + 100 FLT_MIN"""
    return 2.0 ** -23 * np.abs(np.asarray(S, np.float64)) + 100.0 * FLT_MIN


# ---------------------------------------------------------------- similarities and the preference
def similarity(x, metric):
    """float64: metric 0 -|xi - xk|^2 (the difference first), 1 -(1 - cos), 2 x itself; the diagonal 0 for metrics 0 and 1"""
    x = np.asarray(x, np.float64)
    if metric == 2:
        return x.copy()
    if metric == 0:
        S = np.empty((x.shape[0],) * 2)
        for i in range(x.shape[0]):
            d = x - x[i]
            S[i] = -(d * d).sum(1)
    else:
        n = np.sqrt((x * x).sum(1))
        with np.errstate(invalid='ignore', divide='ignore'):
            S = (x @ x.T) / (n[:, None] * n[None, :]) - 1.0
    np.fill_diagonal(S, 0.0)
    return S


def prepared(x, metric, preference=None):
    """-> (S float64 holding fp32 values with the preference on the diagonal, the preference as fp32): the matrix the iterations
    use without noise"""
    S32 = similarity(x, metric).astype(np.float32)
    pref = np.float32(np.median(S32)) if preference is None else np.float32(preference)
    np.fill_diagonal(S32, pref)
    return S32.astype(np.float64), pref


# ---------------------------------------------------------------- one step
def responsibilities(S, A, R, lam):
    """the contract's R update in the dtype of its arguments (float64)"""
    N = S.shape[0]
    idx = np.arange(N)
    AS = A + S
    I = np.argmax(AS, 1)                                 # the first maximum
    Y = AS[idx, I]
    AS[idx, I] = -np.inf
    Y2 = AS.max(1)
    other = np.repeat(Y[:, None], N, 1)
    other[idx, I] = Y2
    return lam * R + (1 - lam) * (S - other)


def availabilities(A, Rn, lam):
    """the contract's A update from the new responsibilities"""
    Rp = np.maximum(Rn, 0)
    np.fill_diagonal(Rp, 0)
    col = Rp.sum(0)                                      # sum over i' != k of max(0, R_i'k)
    new = np.minimum(0, (np.diag(Rn) + col)[None, :] - Rp)
    np.fill_diagonal(new, col)
    return lam * A + (1 - lam) * new


def step(S, A, R, lam):
    """one iteration -> (A, R, E)"""
    Rn = responsibilities(S, A, R, lam)
    An = availabilities(A, Rn, lam)
    return An, Rn, (np.diag(An) + np.diag(Rn)) > 0


def step_fp32(S, A, R, lam, bug=None):
    """one step as the device takes it: fp32 arrays and arithmetic, the column sums and R_kk + sum - max(0, R_ik) in double, rounded
    once.  bug: 'second' uses the first maximum where the second belongs, 'diag' leaves max(0, R_kk) in the column sums -- the two
    mistakes the step bounds must catch"""
    f = np.float32
    S, A, R, lam = np.asarray(S, f), np.asarray(A, f), np.asarray(R, f), f(lam)
    oml = f(1) - lam
    N = S.shape[0]
    idx = np.arange(N)
    AS = A + S
    I = np.argmax(AS, 1)
    Y = AS[idx, I]
    AS[idx, I] = -np.inf
    Y2 = AS.max(1)
    other = np.repeat(Y[:, None], N, 1)
    if bug != 'second':
        other[idx, I] = Y2
    Rn = lam * R + oml * (S - other)
    Rp = np.maximum(Rn, f(0))
    if bug != 'diag':
        np.fill_diagonal(Rp, 0)
    col = Rp.astype(np.float64).sum(0)
    v = ((np.diag(Rn).astype(np.float64) + col)[None, :] - Rp.astype(np.float64)).astype(f)
    new = np.minimum(f(0), v)
    np.fill_diagonal(new, col.astype(f))
    An = lam * A + oml * new
    assert An.dtype == f and Rn.dtype == f
    return An, Rn, (np.diag(An) + np.diag(Rn)) > 0


def bound_R(S, A, R):
    S, A, R = (np.asarray(v, np.float64) for v in (S, A, R))
    return 8 * U * (np.abs(S) + np.abs(A + S).max(1)[:, None] + np.abs(R))


def bound_A(A, Rn):
    """A: the state the step starts from; Rn: the responsibilities the step produced"""
    A, Rn = np.asarray(A, np.float64), np.asarray(Rn, np.float64)
    return 8 * U * (np.abs(A) + np.abs(np.diag(Rn))[None, :] + np.maximum(Rn, 0).sum(0)[None, :])


def sklearn_step(S, A, R, damping):
    """the array operations of sklearn's _affinity_propagation loop body, restated in place on A and R -> E"""
    n = S.shape[0]
    ind = np.arange(n)
    tmp = A + S
    I = np.argmax(tmp, axis=1)
    Y = tmp[ind, I]
    tmp[ind, I] = -np.inf
    Y2 = np.max(tmp, axis=1)
    tmp = S - Y[:, None]
    tmp[ind, I] = S[ind, I] - Y2
    tmp *= 1 - damping
    R *= damping
    R += tmp
    tmp = np.maximum(R, 0)
    tmp.flat[::n + 1] = R.flat[::n + 1]
    tmp -= np.sum(tmp, axis=0)
    dA = np.diag(tmp).copy()
    tmp.clip(0, np.inf, tmp)
    tmp.flat[::n + 1] = dA
    tmp *= 1 - damping
    A *= damping
    A -= tmp
    return (np.diag(A) + np.diag(R)) > 0


# ---------------------------------------------------------------- the loop and the labels
def assign(S, ex):
    """c_i = the exemplar (row number) with the largest S_ik, lowest k on ties; an exemplar takes itself"""
    ex = np.asarray(ex)
    c = ex[np.argmax(S[:, ex], 1)]
    c[ex] = ex
    return c


def refine_sums(S, c, e):
    """(members, sums): the members of exemplar e's cluster, ascending, and for each member j the sum of S_ij over the cluster"""
    ii = np.flatnonzero(c == e)
    return ii, S[np.ix_(ii, ii)].sum(0)


def labels(S, E):
    """the contract's tail -> (label (row of the exemplar, or all -1), exemplars ascending, margins (assignment, refinement))"""
    N = S.shape[0]
    ex = np.flatnonzero(E)
    if len(ex) == 0:
        return np.full(N, -1), ex, (np.inf, np.inf)
    m_assign, m_ref = np.inf, np.inf
    c = assign(S, ex)
    m_assign = min(m_assign, _gap_rows(S, ex))
    new = []
    for e in ex:
        ii, sums = refine_sums(S, c, e)
        new.append(ii[int(np.argmax(sums))])                 # the first maximum: the lowest member on ties
        m_ref = min(m_ref, _gap(sums))
    ex = np.sort(np.array(new))
    m_assign = min(m_assign, _gap_rows(S, ex))
    return assign(S, ex), ex, (m_assign, m_ref)


def _gap(v):
    """relative gap between the largest and the second largest entry (inf with one entry)"""
    if len(v) < 2:
        return np.inf
    s = np.sort(v)
    return (s[-1] - s[-2]) / max(abs(s[-1]), abs(s[-2]), 1e-300)


def _gap_rows(S, ex):
    rows = np.setdiff1d(np.arange(S.shape[0]), ex)
    return min((_gap(S[i, ex]) for i in rows), default=np.inf)


def run(S, damping=0.5, max_iter=200, convergence_iter=15, A=None, R=None, one=step):
    """the whole call from the matrix S the iterations use -> dict(label, exemplars, n_iter, converged, K, A, R, E (per iteration),
    diag (A_kk + R_kk per iteration), margins).  one: the step (step, or step_fp32 to iterate the emulation)"""
    N = S.shape[0]
    A = np.zeros_like(S) if A is None else A
    R = np.zeros_like(S) if R is None else R
    runlen, prev = np.zeros(N, np.int64), None
    hist, diag, converged = [], [], 0
    for it in range(max_iter):
        A, R, E = one(S, A, R, damping)
        runlen = np.where(E == prev, runlen + 1, 1) if prev is not None else np.ones(N, np.int64)
        prev = E
        hist.append(E)
        diag.append(np.diag(A).astype(np.float64) + np.diag(R))
        if it >= convergence_iter and runlen.min() >= convergence_iter and E.sum() > 0:
            converged = 1
            break
    label, ex, margins = labels(np.asarray(S, np.float64), E)
    window = np.array(diag[-convergence_iter:])
    m_e = float(np.abs(window).min() / np.abs(S).max())
    return dict(label=label, exemplars=ex, n_iter=len(hist), converged=converged, K=int(E.sum()), A=A, R=R, E=np.array(hist),
                margins=(m_e,) + margins)


MARGINS = (2.0 ** -10, 2.0 ** -16, 2.0 ** -16)      # |A_kk + R_kk| / max |S| over the final window; assignment gap; refinement gap


def has_margins(res):
    return all(m >= need for m, need in zip(res['margins'], MARGINS))


# ---------------------------------------------------------------- inputs
def planted(n, dim, k, seed, spread=6.0):
    r = np.random.default_rng(seed)
    return (spread * r.standard_normal((k, dim))[np.arange(n) % k] + r.standard_normal((n, dim))).astype(np.float32)


def gaussian(n, dim, seed):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


# (name, rows, metric): the margin cases, on which fp32 and float64 must agree exactly (has_margins holds for each: tests/test_affinity.py)
CASES = [('planted96x8', lambda: planted(96, 8, 6, 1), 0), ('gauss37x12', lambda: gaussian(37, 12, 2), 1),
         ('gauss200x16', lambda: gaussian(200, 16, 3), 1), ('gauss500x32', lambda: gaussian(500, 32, 4), 0)]
CASE_IDS = [c[0] for c in CASES]


def repeated_points():
    """24 rows that are 4 points repeated 6 times: every similarity within a group ties (noise off, fp32 and float64 may part)"""
    return np.tile(gaussian(4, 8, 5), (6, 1))


def pad4(x):
    pad = -x.shape[1] % 4
    return np.ascontiguousarray(np.pad(x, ((0, 0), (0, pad))) if pad else x, dtype=np.float32)
