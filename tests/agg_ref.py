"""float64 reference of the aggregate-posterior contract (include/argsim_vae.h, avae_agg_logq / avae_latent_moments) on the fp32
inputs, and the inputs of the tests.

Two input regimes, z always drawn from its own rows (query i is a sample of bank row i):
    peaked  mu ~ N(0, 1), lv ~ U(-6, 1): narrow posteriors far apart -- the own pair holds the sum, and its value is where an
            expanded square would cancel;
    broad   mu ~ N(0, 1) / sqrt(dim), lv ~ U(-0.5, 0.2): posteriors that overlap -- hundreds of bank rows weigh in the
            logsumexp for dim <= 128 (tests/test_agg.py asserts it).
"""
import functools

import numpy as np

REGIMES = ('peaked', 'broad')
# (n, N, dim).  The kernel has ONE tile form: query tiles of 128 rows, bank tiles of 64 rows, dim chunks of 32.
# Query-tile remainders 1 (n 1, 129), tile - 1 (127), tile + 1 (129), 2 (130); bank-tile remainders 1 (N 1, 129, 257, 321),
# tile - 1 (63, 127, 191), tile + 1 (65), 3 (4099); dim 4 .. 1024 with chunk remainders 4, 8, 12, 20 and none.
CASES = [(1, 1, 4), (5, 129, 4), (33, 777, 20), (65, 300, 128), (130, 4099, 128), (3, 127, 512), (7, 257, 1024),
         (4, 63, 8), (3, 65, 36), (127, 191, 20), (129, 321, 12)]
# case: (median over the queries of the largest term's share of the sum <=, mean count of rows weighing > 1e-3 of the largest >=)
BROAD_SPREAD = {(5, 129, 4): (0.15, 100.0), (33, 777, 20): (0.15, 600.0), (65, 300, 128): (0.3, 150.0)}
MOMENT_N = (1, 2, 257, 4099)
MOMENT_DIM = (4, 20, 1024)
AU_THRESHOLD = 0.01


def make_inputs(n, N, dim, regime, seed=0):
    """-> z (n, dim), mu, lv (N, dim) float32; z[i] = mu[i] + exp(lv[i] / 2) eps[i] in float32"""
    assert n <= N and regime in REGIMES
    rng = np.random.default_rng(1000 * seed + 7 * n + 3 * N + dim + (500000 if regime == 'broad' else 0))
    if regime == 'peaked':
        mu = rng.standard_normal((N, dim))
        lv = rng.uniform(-6.0, 1.0, (N, dim))
    else:
        mu = rng.standard_normal((N, dim)) / np.sqrt(dim)
        lv = rng.uniform(-0.5, 0.2, (N, dim))
    mu, lv = mu.astype(np.float32), lv.astype(np.float32)
    eps = rng.standard_normal((n, dim)).astype(np.float32)
    z = (mu[:n] + np.exp(np.float32(0.5) * lv[:n]) * eps).astype(np.float32)
    return z, mu, lv


@functools.lru_cache(maxsize=None)
def case_inputs(case, regime):
    out = make_inputs(*case, regime)
    for a in out:
        a.setflags(write=False)
    return out


def pair_terms64(z, mu, lv):
    """(n, N) float64: t(i, j) = -1/2 sum_d [(z_id - mu_jd)^2 exp(-lv_jd) + lv_jd], query row by query row"""
    z, mu, lv = (np.asarray(x, np.float64) for x in (z, mu, lv))
    with np.errstate(all='ignore'):
        a, c = np.exp(-lv), lv.sum(1)
        t = np.empty((z.shape[0], mu.shape[0]))
        for i in range(z.shape[0]):
            d = z[i][None, :] - mu
            t[i] = -0.5 * ((d * d * a).sum(1) + c)
    return t


def logsumexp64(t):
    """row-wise, the maximum subtracted; a row of -inf gives -inf"""
    with np.errstate(all='ignore'):
        m = np.max(np.where(np.isnan(t), -np.inf, t), axis=1)
        r = np.where(np.isneginf(m), 0.0, m)
        return m + np.log(np.exp(t - r[:, None]).sum(1))


def logq64(z, mu, lv, self_base=-1):
    """-> logq (n,), or (logq, logqx) where self_base >= 0: float64"""
    n, dim, N = z.shape[0], z.shape[1], mu.shape[0]
    t = pair_terms64(z, mu, lv)
    cst = 0.5 * dim * np.log(2.0 * np.pi)
    with np.errstate(all='ignore'):
        logq = logsumexp64(t) - np.log(N) - cst
    if self_base < 0:
        return logq
    return logq, t[np.arange(n), self_base + np.arange(n)] - cst


@functools.lru_cache(maxsize=None)
def case_ref(case, regime):
    out = logq64(*case_inputs(case, regime), self_base=0)
    for a in out:
        a.setflags(write=False)
    return out


def spread(case, regime):
    """per query of a case: (share of the largest term in the sum, bank rows that weigh more than 1e-3 of the largest)"""
    t = pair_terms64(*case_inputs(case, regime))
    w = np.exp(t - t.max(1, keepdims=True))
    return 1.0 / w.sum(1), (w > 1e-3).sum(1)


def rel_err(dev, ref):
    """max |dev - ref| / max(1, |ref|) over the entries, which must be finite"""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    assert dev.shape == ref.shape and np.isfinite(ref).all() and np.isfinite(dev).all(), (dev, ref)
    return float((np.abs(dev - ref) / np.maximum(1.0, np.abs(ref))).max()) if dev.size else 0.0


# ---- moments
def moment_inputs(N, dim, seed=0):
    """mu, lv (N, dim) float32: even dimensions active (mu ~ 0.3 + N(0, 1)), odd ones collapsed (mu ~ 0.05 + 0.01 N(0, 1)); for N = 2
    the two rows of an active dimension are planted 1 apart (variance 0.5: nothing is left to the draw)"""
    rng = np.random.default_rng(77 + 1000 * seed + 5 * N + dim)
    scale = np.where(np.arange(dim) % 2 == 0, 1.0, 0.01)
    shift = np.where(np.arange(dim) % 2 == 0, 0.3, 0.05)
    mu = shift + scale * rng.standard_normal((N, dim))
    if N == 2:
        mu[1] = mu[0] + scale
    lv = rng.uniform(-6.0, 1.0, (N, dim))
    return mu.astype(np.float32), lv.astype(np.float32)


def moments64(mu, lv):
    """(4, dim) float64: mean mu, unbiased variance (0 for N = 1), mean exp(lv), mean 1/2 (mu^2 + exp(lv) - lv - 1)"""
    mu, lv = np.asarray(mu, np.float64), np.asarray(lv, np.float64)
    N = mu.shape[0]
    mean = mu.mean(0)
    var = ((mu - mean) ** 2).sum(0) / (N - 1) if N > 1 else np.zeros(mu.shape[1])
    return np.stack([mean, var, np.exp(lv).mean(0), (0.5 * (mu * mu + np.exp(lv) - lv - 1.0)).mean(0)])


def posterior_stats64(mu, lv, eps, au_threshold=AU_THRESHOLD):
    """the composite of VAE.posterior_stats in float64 from the encoder's fp32 mu, lv (N, R) and eps (samples, N, R)"""
    mu, lv, eps = (np.asarray(x, np.float64) for x in (mu, lv, eps))
    N, R = mu.shape
    mom = moments64(mu, lv)
    z = mu[None] + np.exp(0.5 * lv)[None] * eps
    logq, logqx = (np.stack(x) for x in zip(*(logq64(z[s], mu, lv, self_base=0) for s in range(eps.shape[0]))))
    logp = -0.5 * (z * z).sum(-1) - 0.5 * R * np.log(2.0 * np.pi)
    return dict(kl=float(mom[3].sum()), kl_dim=mom[3], var_mu=mom[1], au=int((mom[1] > au_threshold).sum()),
                mi=float((logqx - logq).mean()), kl_marginal=float((logq - logp).mean()), n=N, logq=logq, logqx=logqx, logp=logp, z=z)
