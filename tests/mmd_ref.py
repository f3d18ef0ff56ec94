"""float64 restatement of the contract of avae_mmd and avae_mmd_relabel (include/argsim_vae.h): the kernel values, the U sums over
unordered pairs, the statistic, the p-value, the witness, the generated relabelings from their key definition; the margins under which
the p-value must be reproduced exactly; the derived error bounds; the small shapes of the test cases.

Bounds (derived from operation counts, none measured; EPS = 2^-53, a double sum of t terms is good to t EPS of the sum of magnitudes;
the tests allow twice a bound, since the reference errs as well):
  distance   euclidean: the rows are fp32 numbers, exact as doubles; a difference, its square and the sum over dim non-negative terms:
             ed2 = (dim + 4) EPS d2.  Cosine: an element of a unit row errs by (dim + 3) EPS relative (kmeans_ref), so a difference moves
             by that much of |X_ie| + |X_je|; by Cauchy-Schwarz d2 moves by 2 d (dim + 3) EPS (|X_i| + |X_j|) <= 4 (dim + 3) EPS d, and by
             the square of the perturbation, 8 ((dim + 3) EPS)^2, where d itself is that small.
  rbf        exp is taken at its documented 1 ulp = 2 EPS; its argument gamma d2 carries gamma ed2 and one rounding: a term errs by
             exp(-gamma d2) (gamma ed2 + EPS gamma d2 + 2 EPS); the sum over nbw terms adds nbw EPS k.
  energy     |sqrt(d2 + t) - sqrt(d2)| <= min(t / d, sqrt(t)), + EPS d for the root.
  U sums     the sum of the pairs' bounds + t EPS sum |k|, t = the number of pairs of the sum.
  statistic  U_AB = U_LL - U_AA - U_BB: the three bounds + 2 EPS of the three magnitudes.  m (m - 1), n (n - 1), m n and the factor 2
             are exact; a division adds EPS of the term, the two additions 2 EPS of the terms' magnitudes.
  witness    a row's sum over at most m (n) columns: the pairs' bounds + m EPS sum |k|; the division and the difference add EPS each."""
import numpy as np

from kmeans_ref import rows_of

EPS = 2.0 ** -53
U64 = np.uint64
KERNELS = {'rbf': 0, 'energy': 1}
METRICS = {'euclidean': 0, 'cosine': 1}


# ---------------------------------------------------------------- masks as bit rows
def pack(bits):
    """(.., N) bool -> (.., W) uint64, bit i % 64 of word i / 64"""
    bits = np.asarray(bits, bool)
    N = bits.shape[-1]
    W = (N + 63) // 64
    b = np.zeros(bits.shape[:-1] + (64 * W,), np.uint8)
    b[..., :N] = bits
    return np.ascontiguousarray(np.packbits(b, axis=-1, bitorder='little')).view('<u8').reshape(bits.shape[:-1] + (W,))


def unpack(words, N):
    """(.., W) uint64 -> (.., N) bool"""
    w = np.ascontiguousarray(np.asarray(words, '<u8'))
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (-1,)), axis=-1, bitorder='little')[..., :N].astype(bool)


# ---------------------------------------------------------------- the generator (sample_dev.h: mix64; stream 8)
def mix64(x):
    with np.errstate(over='ignore'):
        x = np.asarray(x, U64) + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def relabel_keys(N, seed, g, p):
    with np.errstate(over='ignore'):
        base = mix64(U64(seed) ^ (U64(8) * U64(0xD6E8FEB86659FD93)))
        c = mix64(base + ((U64(g) << U64(32)) | U64(p)))
        return mix64(c + np.arange(N, dtype=U64))


def relabel(valid, a0, P, seed):
    """valid, a0 (G, N) bool -> (G, 1 + P, N) bool: relabeling 0 = valid & a0, relabeling p >= 1 the m valid rows with the smallest (key, row)"""
    valid, a0 = np.asarray(valid, bool), np.asarray(a0, bool)
    G, N = valid.shape
    out = np.zeros((G, 1 + P, N), bool)
    for g in range(G):
        out[g, 0] = valid[g] & a0[g]
        m = int(out[g, 0].sum())
        idx = np.flatnonzero(valid[g])
        for p in range(1, 1 + P):
            k = relabel_keys(N, seed, g, p)[idx]
            out[g, p, idx[np.lexsort((idx, k))[:m]]] = True
    return out


# ---------------------------------------------------------------- kernel values
def sqdist(x, metric):
    X = rows_of(x, metric)
    D = np.zeros((len(X), len(X)))
    for e in range(X.shape[1]):                      # ascending e, as the contract has it
        d = X[:, None, e] - X[None, :, e]
        D += d * d
    return D


def kernel_values(x, kernel, metric, gamma=()):
    """(N, N) k(i, j); rows that hold a NaN give NaN values, which no sum below touches unless the row is valid"""
    D = sqdist(x, metric)
    if kernel == 1:
        return -np.sqrt(D)
    K = np.zeros_like(D)
    for g in gamma:
        K += np.exp(-(float(g) * D))
    return K


# ---------------------------------------------------------------- the statistic
def statistic(uaa, ubb, ull, m, n):
    uab = ull - uaa - ubb
    m, n = float(m), float(n)
    return 2.0 * uaa / (m * (m - 1.0)) + 2.0 * ubb / (n * (n - 1.0)) - 2.0 * uab / (m * n)


def u_sums(K, valid, inA):
    """K (N, N), valid (N,), inA (R, N) bool -> U_AA (R,), U_BB (R,), U_LL: explicit loops over the unordered pairs i < j (j in one
    vector operation per i)"""
    K = np.where(valid[:, None] & valid[None, :], K, 0.0)
    A, B = (inA & valid).astype(np.float64), (~inA & valid).astype(np.float64)
    N = len(valid)
    uaa, ubb, ull = np.zeros(len(inA)), np.zeros(len(inA)), 0.0
    for i in range(N - 1):
        if not valid[i]:
            continue
        row = K[i, i + 1:]
        uaa += A[:, i] * (A[:, i + 1:] @ row)
        ubb += B[:, i] * (B[:, i + 1:] @ row)
        ull += float(row.sum())
    return uaa, ubb, ull


def run(x, kernel, metric, gamma, valid, inA):
    """valid (G, N), inA (G, 1 + P, N) bool -> dict(stat (G, 1 + P), pvalue (G,), counts (G, 2), sums (G, 1 + P, 2), ull (G,), witness (G, N),
    K): everything avae_mmd returns"""
    valid, inA = np.asarray(valid, bool), np.asarray(inA, bool)
    G, P1, N = inA.shape
    K = kernel_values(x, kernel, metric, gamma)
    out = dict(stat=np.zeros((G, P1)), pvalue=np.zeros(G), counts=np.zeros((G, 2), np.int32), sums=np.zeros((G, P1, 2)), ull=np.zeros(G),
               witness=np.zeros((G, N)), K=K)
    for g in range(G):
        v = valid[g]
        a0, b0 = inA[g, 0] & v, ~inA[g, 0] & v
        m, n = int(a0.sum()), int(b0.sum())
        uaa, ubb, ull = u_sums(K, v, inA[g])
        out['counts'][g] = m, n
        out['sums'][g, :, 0], out['sums'][g, :, 1], out['ull'][g] = uaa, ubb, ull
        out['stat'][g] = statistic(uaa, ubb, ull, m, n)
        out['pvalue'][g] = (1 + int((out['stat'][g, 1:] >= out['stat'][g, 0]).sum())) / P1
        Kz = np.where(v[:, None] & v[None, :], K, 0.0)
        np.fill_diagonal(Kz, 0.0)
        sa, sb = Kz @ a0.astype(np.float64), Kz @ b0.astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            out['witness'][g] = np.where(v, sa / (m - a0) - sb / (n - b0), 0.0)
    return out


def mmd2(xa, xb, kernel, metric, gamma, P, seed):
    """two arrays -> run() on their concatenation with generated relabelings (what VAE.mmd2 computes)"""
    x = np.concatenate([xa, xb])
    valid = np.ones((1, len(x)), bool)
    a0 = np.arange(len(x))[None, :] < len(xa)
    return run(x, kernel, metric, gamma, valid, relabel(valid, a0, P, seed))


def median_gamma(z, max_rows=2048):
    z = np.asarray(z, np.float64)
    step = max(1, -(-len(z) // max_rows))
    s = z[::step]
    d2 = ((s[:, None, :] - s[None, :, :]) ** 2).sum(-1)[np.triu_indices(len(s), 1)]
    return 1.0 / float(np.median(d2))


# ---------------------------------------------------------------- bounds
def bounds(x, kernel, metric, gamma, valid, inA, ref):
    """-> dict(sums (G, 1 + P, 2), ull (G,), stat (G, 1 + P), witness (G, N)): bounds on the error of run()'s fields"""
    valid, inA = np.asarray(valid, bool), np.asarray(inA, bool)
    G, P1, N = inA.shape
    dim = np.asarray(x).shape[1]
    anyv = valid.any(0)
    D = np.where(anyv[:, None] & anyv[None, :], sqdist(x, metric), 0.0)
    d = np.sqrt(D)
    ed2 = (dim + 4) * EPS * D
    if metric == 1:
        ed2 = ed2 + 4 * (dim + 3) * EPS * d + 8 * ((dim + 3) * EPS) ** 2
    if kernel == 1:
        with np.errstate(divide='ignore', invalid='ignore'):
            eK = np.minimum(np.where(d > 0, ed2 / d, np.inf), np.sqrt(ed2)) + EPS * d
        absK = d
    else:
        eK, absK = np.zeros_like(D), np.zeros_like(D)
        for gm in gamma:
            t = np.exp(-float(gm) * D)
            eK += t * (float(gm) * ed2 + EPS * float(gm) * D + 2 * EPS)
            absK += t
        eK += len(gamma) * EPS * absK
    out = dict(sums=np.zeros((G, P1, 2)), ull=np.zeros(G), stat=np.zeros((G, P1)), witness=np.zeros((G, N)))
    iu = np.triu(np.ones((N, N), bool), 1)
    for g in range(G):
        v = valid[g]
        m, n = (float(c) for c in ref['counts'][g])

        def usum(side):
            s = side.astype(np.float64)
            pairs = s.sum() * (s.sum() - 1) / 2
            on = iu & side[:, None] & side[None, :]
            return float(eK[on].sum() + pairs * EPS * absK[on].sum())
        ell = usum(v)
        out['ull'][g] = ell
        for p in range(P1):
            ea, eb = usum(inA[g, p] & v), usum(~inA[g, p] & v)
            out['sums'][g, p] = ea, eb
            uaa, ubb = ref['sums'][g, p]
            ull = ref['ull'][g]
            eab = ell + ea + eb + 2 * EPS * (abs(ull) + abs(uaa) + abs(ubb))
            t = np.array([2 * uaa / (m * (m - 1)), 2 * ubb / (n * (n - 1)), 2 * (ull - uaa - ubb) / (m * n)])
            e = np.array([2 * ea / (m * (m - 1)), 2 * eb / (n * (n - 1)), 2 * eab / (m * n)])
            out['stat'][g, p] = e.sum() + 3 * EPS * np.abs(t).sum()
        a0, b0 = inA[g, 0] & v, ~inA[g, 0] & v
        off = ~np.eye(N, dtype=bool)
        for i in np.flatnonzero(v):
            ca, cb = a0 & off[i], b0 & off[i]
            sa = eK[i, ca].sum() + m * EPS * absK[i, ca].sum()
            sb = eK[i, cb].sum() + n * EPS * absK[i, cb].sum()
            ma, nb = max(ca.sum(), 1), max(cb.sum(), 1)
            out['witness'][g, i] = sa / ma + sb / nb + 3 * EPS * (absK[i, ca].sum() / ma + absK[i, cb].sum() / nb)
    return out


def has_margins(ref, bnd):
    """no null statistic lies within twice the bounds (its own and the observed one's) of the observed one: the p-value is decided"""
    s, e = ref['stat'], bnd['stat']
    gap = np.abs(s[:, 1:] - s[:, :1])
    return bool((gap > 2 * (e[:, 1:] + e[:, :1])).all())


# ---------------------------------------------------------------- inputs
def rows(N, dim, seed, shift=0.0):
    r = np.random.default_rng(seed)
    x = r.standard_normal((N, dim)).astype(np.float32)
    x[N // 2:] += np.float32(shift)
    return x


def split(N, G, seed, left_out=True, one_word=False, sizes=None):
    """-> valid, a0 (G, N) bool.  With left_out about a fifth of the rows take part in nothing per comparison; one_word: the last
    comparison has its valid rows in word 0 only; sizes (m, n): the first comparison has exactly m rows in A and n in B"""
    r = np.random.default_rng(seed)
    valid, a0 = np.zeros((G, N), bool), np.zeros((G, N), bool)
    for g in range(G):
        v = r.random(N) >= 0.2 if left_out else np.ones(N, bool)
        a = r.random(N) < 0.45
        allowed = np.ones(N, bool)
        if g == G - 1 and one_word and G > 1:
            allowed[min(N, 64):] = False
            v &= allowed
        if g == 0 and sizes is not None:
            perm = r.permutation(N)
            v[:] = False; a[:] = False
            v[perm[:sizes[0] + sizes[1]]] = True
            a[perm[:sizes[0]]] = True
        for side in (a, ~a):                         # at least two rows on each side
            short = 2 - int((v & side).sum())
            if short > 0:
                v[np.flatnonzero(side & ~v & allowed)[:short]] = True
        valid[g], a0[g] = v, a
    return valid, a0
