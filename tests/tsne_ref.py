"""float64 restatement of the contract of avae_tsne (include/argsim_vae.h): distances, the perplexity bisection, the joint matrix, one
iteration (pair sums in double, the state in fp32 numpy with every operation rounded), the two-phase loop with sklearn's stopping
rule; the margins that make a comparison in bits legitimate; the inputs of the test cases.  The counter generator is ap_ref's.

A fit is chaotic: one fp32 ulp in a few gradient entries moves the embedding by a fifth of its span within a hundred iterations.  So
nothing here compares a fitted embedding with another fit by tolerance: pure functions are compared with float64, ONE iteration from a
given state is compared in bits where the margins below allow it, and a run is checked by certificates on its own outputs.

Margins (derived, not measured; e = 2^-52).
  bisection  A row's decisions are |h - log perplexity| <= tol and the sign of h - log perplexity, h = log s + beta sum_j D_j p_j / s,
             p_j = exp(-D_j beta).  Device and numpy differ in exp (within 1 ulp each), in the rounding of the argument D_j beta (a
             relative e / 2 of the argument: a relative D_j beta e / 2 of p_j) and in the order of the two sums (at most N e / 2
             relative, all terms positive).  With t = beta sum D_j p_j / s and m2 = sum (D_j beta)^2 p_j / s: s errs relatively by at
             most (2 + t + N / 2) e, so log s by that much absolutely; t errs by at most t (6 + N) e + (t + m2) e.  Stated with a
             factor 4:  eval_err = 4 e ((N + 8) (1 + t) + 2 t + 2 m2).  A row whose smallest distance from a decision boundary over its
             steps (`margin`) exceeds the largest eval_err over its steps takes the same decisions on the device: beta, a chain of exact
             operations on those decisions, is then the same in bits.
  gradient   g = fp32(4 (a - b / Z)), a = sum_j P'_ij q_ij d_ij, b = sum_j q_ij^2 d_ij, Z = sum q.  Every TERM is a fixed sequence of IEEE
             operations on the same operands, so the device forms the very same terms; only the ORDER of the sums is free.  A sum of n
             terms in any order errs by at most (n - 1) e / 2 sum |terms|, so two orders differ by at most n e sum |terms|: N e
             sum |terms| for a and for b.  Z has N^2 positive terms, but in a blocked order a term passes through far fewer than N
             additions (a lane's run, the butterfly, the parts, the rows: below 64 + 6 + 256 + 64 + 10 at N = 2^14; numpy's pairwise
             sum fewer still): two such orders differ relatively by at most max(N, 64) e, taken as (N + 4) e with the three
             roundings of the final expression, e / 2 of its operands each.  Hence, with the gradient's factor 4,
                 bound = 4 e ((N + 4) (sum_j |P'_ij q_ij d_ij| + sum_j q_ij^2 |d_ij| / Z) + max(N + 4, 64) |b| / Z).  An entry whose double value lies further than `bound` from
             the nearest fp32 rounding boundary rounds to the same fp32 number on the device."""
import numpy as np

import ap_ref as ar

E = 2.0 ** -52
EPS = 2.0 ** -52                       # sklearn's MACHINE_EPSILON, the floor of P and Q
TOL = float(np.float32(1e-5))          # the bisection's tolerance
SUM0 = float(np.float32(1e-8))         # what a zero sum of p is replaced by
STREAM = 6                             # the generator's stream of the random start
F32 = np.float32


# ---------------------------------------------------------------- inputs
def clusters(N, dim, seed, k=4, sep=6.0):
    """k separated gaussian clusters, rows in round-robin order -> (x float32 (N, dim), labels)"""
    r = np.random.default_rng(seed)
    lab = np.arange(N) % k
    ctr = sep * r.standard_normal((k, dim))
    return (ctr[lab] + r.standard_normal((N, dim))).astype(F32), lab


def start(N, seed, scale=1e-4):
    return (scale * np.random.default_rng(seed).standard_normal((N, 2))).astype(F32)


def random_init(N, seed):
    """float64 value of mode-1 start (the device evaluates normal01 in fp32)"""
    return 1e-4 * ar.normal01(seed, STREAM, np.arange(2 * N)).reshape(N, 2)


# (N, dim, tsne_chunk or 0, perplexity): the shapes of the issue; chunks that give several parts which are no tile multiples
CASES = [(3, 4, 0, 1.5), (37, 8, 5, 10.0), (64, 16, 0, 20.0), (65, 4, 33, 20.0), (96, 16, 40, 30.0), (257, 1024, 100, 40.0)]
STEP_ONLY = (1024, 64, 300, 40.0)


# ---------------------------------------------------------------- distances, conditionals, joint
def distances(x):
    """D_ij in double, the difference first, rounded once to fp32 (returned as float64 values of fp32 numbers)"""
    x = np.asarray(x, np.float64)
    D = np.empty((x.shape[0],) * 2)
    for i in range(x.shape[0]):
        d = x - x[i]
        D[i] = (d * d).sum(1)
    np.fill_diagonal(D, 0.0)
    return D.astype(F32).astype(np.float64)


def entropy(Drow, beta):
    """one evaluation of a row (Drow without the own entry) -> (h, s, p normalised, t, m2)"""
    p = np.exp(-Drow * beta)
    s = p.sum()
    if s == 0.0:
        s = SUM0
    p = p / s
    t = beta * (Drow * p).sum()
    return np.log(s) + t, s, p, t, ((Drow * beta) ** 2 * p).sum()


def conditionals(D, perplexity, steps=100):
    """sklearn's _binary_search_perplexity over the fp32 distances -> dict(C (N, N) conditionals, beta (N) the beta the row's
    conditionals were evaluated at, margin (N), eval_err (N), steps (N) evaluations made)"""
    N = D.shape[0]
    want = np.log(perplexity)
    C = np.zeros((N, N))
    out = dict(C=C, beta=np.zeros(N), margin=np.full(N, np.inf), eval_err=np.zeros(N), steps=np.zeros(N, int))
    for i in range(N):
        row = np.delete(D[i], i)
        beta, lo, hi = 1.0, -np.inf, np.inf
        for l in range(steps):
            h, s, p, t, m2 = entropy(row, beta)
            diff = h - want
            out['steps'][i] = l + 1
            out['margin'][i] = min(out['margin'][i], abs(abs(diff) - TOL), abs(diff))
            out['eval_err'][i] = max(out['eval_err'][i], 4 * E * ((N + 8) * (1 + t) + 2 * t + 2 * m2))
            used = beta
            if abs(diff) <= TOL:
                break
            if diff > 0.0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
        out['beta'][i] = used
        C[i] = np.insert(p, i, 0.0)
    return out


def conditionals_at(D, beta):
    """the conditionals of given betas (the device's own), float64"""
    N = D.shape[0]
    C = np.zeros((N, N))
    h = np.zeros(N)
    for i in range(N):
        row = np.delete(D[i], i)
        h[i], _, p, _, _ = entropy(row, beta[i])
        C[i] = np.insert(p, i, 0.0)
    return C, h


def joint(C):
    S = C + C.T
    P = np.maximum(S / max(S.sum(), EPS), EPS)
    np.fill_diagonal(P, 0.0)
    return P


# ---------------------------------------------------------------- one iteration
def pair_sums(Pe, y):
    """from the fp32 y, in double -> dict(Z, a, b (N, 2), g64 the gradient before its rounding, bound (N, 2), q)"""
    y = np.asarray(y, F32).astype(np.float64)
    d = y[:, None, :] - y[None, :, :]
    q = 1.0 / (1.0 + (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]))
    np.fill_diagonal(q, 0.0)
    Z = q.sum()
    pq = Pe * q
    ta, tb = pq[:, :, None] * d, (q * q)[:, :, None] * d
    a, b = ta.sum(1), tb.sum(1)
    N = y.shape[0]
    bound = 4 * E * ((N + 4) * (np.abs(ta).sum(1) + np.abs(tb).sum(1) / Z) + max(N + 4, 64) * np.abs(b) / Z)
    return dict(Z=Z, a=a, b=b, g64=4.0 * (a - b / Z), bound=bound, q=q)


def error(Pe, q, Z):
    off = ~np.eye(Pe.shape[0], dtype=bool)
    return float((Pe[off] * np.log(np.maximum(Pe[off], EPS) / np.maximum(q[off] / Z, EPS))).sum())


def round_margin(g64):
    """distance of a double from the nearest boundary between two fp32 roundings"""
    g32 = g64.astype(F32)
    up = (g32.astype(np.float64) + np.nextafter(g32, F32(np.inf)).astype(np.float64)) / 2
    dn = (g32.astype(np.float64) + np.nextafter(g32, F32(-np.inf)).astype(np.float64)) / 2
    return np.minimum(np.abs(g64 - up), np.abs(g64 - dn))


def update(y, upd, gains, g, momentum, lr):
    """the fp32 state arithmetic, every operation rounded (numpy fp32 never fuses) -> (y, update, gains, g')"""
    y, upd, gains, g = (np.asarray(v, F32) for v in (y, upd, gains, g))
    inc = upd * g < F32(0)
    gains = np.where(inc, gains + F32(0.2), gains * F32(0.8)).astype(F32)
    gains = np.maximum(gains, F32(0.01))
    gp = g * gains
    upd = F32(momentum) * upd - F32(lr) * gp
    return y + upd, upd, gains, gp


def auto_lr(N, ee):
    return float(F32(max(N / ee / 4.0, 50.0)))


# ---------------------------------------------------------------- the loop
def fit(P, y, max_iter, lr, ee=12.0, exag_iter=250, n_iter_check=50, nwp=300, min_grad_norm=1e-7, it0=0, state=None):
    """the contract's loop -> dict(y, kl (2), stat (4), trace (2, max_iter), grad, ug (2, N, 2), prog (4)).  state: (ug, prog) of a
    warm continuation"""
    N = P.shape[0]
    y = np.asarray(y, F32).copy()
    X = min(exag_iter, max_iter)
    if state is None:
        upd, gains = np.zeros((N, 2), F32), np.ones((N, 2), F32)
        best, best_it, phase = np.finfo(np.float64).max, it0, 1 if it0 < exag_iter else 2
    else:
        upd, gains = state[0][0].copy(), state[0][1].copy()
        best, best_it, phase = float(state[1][0]), int(state[1][1]), int(state[1][2])
    trace = np.full((2, max(max_iter, 1)), np.nan)
    kl = [np.nan, np.nan]
    last, how, p1_last, grad = it0 - 1, 0, -1, np.zeros((N, 2), F32)
    Pex = ee * P
    for i in range(it0, max_iter):
        Pe, m, W = (Pex, 0.5, X) if phase == 1 else (P, 0.8, nwp)
        check = (i + 1) % n_iter_check == 0
        comp = check or i == (X - 1 if phase == 1 else max_iter - 1)
        ps = pair_sums(Pe, y)
        grad = ps['g64'].astype(F32)
        err = error(Pe, ps['q'], ps['Z']) if comp else np.nan
        y, upd, gains, gp = update(y, upd, gains, grad, m, lr)
        last = i
        if comp:
            kl[0] = trace[0, i] = err
        if phase == 1:
            p1_last, kl[1] = i, err
        ended = 0
        if check:
            gn = trace[1, i] = float(np.sqrt((gp.astype(np.float64) ** 2).sum()))
            if err < best:
                best, best_it = err, i
            elif i - best_it > W:
                ended = 1
            if not ended and gn <= min_grad_norm:
                ended = 2
        if phase == 1:
            if ended or i == exag_iter - 1:
                phase, best, best_it = 2, np.finfo(np.float64).max, i + 1
                upd, gains = np.zeros((N, 2), F32), np.ones((N, 2), F32)
        elif ended:
            how = ended
            break
    return dict(y=y, kl=np.array(kl), stat=np.array([last, how, p1_last, 0], np.int32), trace=trace[:, :max_iter], grad=grad,
                ug=np.stack([upd, gains]), prog=np.array([best, best_it, phase, 0.0]))


def replay_stop(trace, max_iter, exag_iter, n_iter_check, nwp, min_grad_norm, it0=0):
    """the stop rule over a trace alone -> (last iteration, how phase 2 ended, phase 1's last iteration, kl0, kl1)"""
    X = min(exag_iter, max_iter)
    best, best_it, phase = np.finfo(np.float64).max, it0, 1 if it0 < exag_iter else 2
    last, how, p1_last, kl0, kl1 = it0 - 1, 0, -1, np.nan, np.nan
    for i in range(it0, max_iter):
        W = X if phase == 1 else nwp
        check = (i + 1) % n_iter_check == 0
        comp = check or i == (X - 1 if phase == 1 else max_iter - 1)
        err = trace[0, i]
        assert comp or np.isnan(err), i                                      # no error where the rule computes none
        last = i
        if comp:
            kl0 = err
        if phase == 1:
            p1_last, kl1 = i, err
        ended = 0
        if check:
            if err < best:
                best, best_it = err, i
            elif i - best_it > W:
                ended = 1
            if not ended and trace[1, i] <= min_grad_norm:
                ended = 2
        if phase == 1:
            if ended or i == exag_iter - 1:
                phase, best, best_it = 2, np.finfo(np.float64).max, i + 1
        elif ended:
            how = ended
            break
    return last, how, p1_last, kl0, kl1


def purity_1nn(y, lab):
    y = np.asarray(y, np.float64)
    d = ((y[:, None, :] - y[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(d, np.inf)
    return float((lab[d.argmin(1)] == lab).mean())
