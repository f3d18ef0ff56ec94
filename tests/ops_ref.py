"""Plain numpy restatements of the small kernels' contracts (argsim_amd/csrc/kernels.h, section "small kernels"): int64 for the
integer kernels, float64 for the float kernels, loops where that is clearest.  Also the input builders the GPU tests share with
tests/test_ops_ref.py, which checks on the CPU the conditions those inputs have to meet (exact-sum class, free-bits gate).

A summing reference returns (sum, terms, abs_sum) per output element: the float64 sum, how many terms went into it and the sum of
their magnitudes -- what the order-independent fp32 bound  (terms - 1) 2^-24 abs_sum + 2^-24 |sum|  is made of (sum_bound)."""
import numpy as np

U = 2.0 ** -24                    # unit roundoff of fp32
LADDER = (1, 31, 32, 33, 64, 65, 1500)      # tokens per id around the 32-row segment; the last spans two 1024-token workgroups
GATE_MARGIN = 2.0 ** -16


def clamp_ids(ids, V):
    return np.clip(np.asarray(ids, np.int64), 0, V - 1)


def sum_bound(s, terms, abs_sum):
    return np.maximum(np.asarray(terms, np.float64) - 1, 0) * U * abs_sum + U * np.abs(s)


# ------------------------------------------------------------------------------------------ ids
def prep_ids(src, tgt, eos, bos, train, keep_mask):
    """-> dict src_tm (Ss, B), lens_src, lens_tgt (B), lead, gold, rank (St + 1, B), cidx (ntok), ntok"""
    src, tgt = np.asarray(src, np.int64), np.asarray(tgt, np.int64)
    B, St = tgt.shape
    ne = tgt != eos
    o = dict(src_tm=src.T.copy(), lens_src=(src != eos).sum(1))
    # the steps that can reach the loss end one behind the LAST non-eos id, wherever other eos ids sit
    o['lens_tgt'] = np.where(ne.any(1), St - np.argmax(ne[:, ::-1], axis=1), 0) if St else np.zeros(B, np.int64)
    o['gold'] = np.concatenate([tgt.T, np.full((1, B), eos, np.int64)], 0)
    fed = tgt.T.copy()
    if train:
        fed[np.asarray(keep_mask).reshape(St, B) == 0] = 0
    o['lead'] = np.concatenate([np.full((1, B), bos, np.int64), fed], 0)
    mask = np.concatenate([np.ones((1, B), bool), ne.T], 0)
    flat = mask.ravel()
    rank = np.full(flat.size, -1, np.int64)
    o['cidx'] = np.flatnonzero(flat)
    rank[o['cidx']] = np.arange(o['cidx'].size)
    o['rank'] = rank.reshape(St + 1, B)
    o['ntok'] = int(o['cidx'].size)
    o['mask'] = mask
    return o


def embed_gather(E, ids, V):
    return np.asarray(E)[clamp_ids(ids, V)]


def id_groups(ids, V):
    """-> rank (V): index among the present ids or -1, uid (nuniq): the present ids ascending, nuniq"""
    present = np.zeros(V, bool)
    for t in clamp_ids(ids, V):
        present[t] = True
    rank, uid = np.full(V, -1, np.int64), []
    for v in range(V):
        if present[v]:
            rank[v] = len(uid)
            uid.append(v)
    return rank, np.asarray(uid, np.int64), len(uid)


def rank_rows(ids, rank, V):
    return np.asarray(rank, np.int64)[clamp_ids(ids, V)]


def rows_gather_ranked(src, ids, rank, V):
    return np.asarray(src)[np.asarray(rank, np.int64)[clamp_ids(ids, V)]]


def scatter_sum(V, ids, rows, base=None):
    """per id the float64 sum of the rows whose id it is (+ base[id]) -> (sum, terms, abs_sum), each (V, D) / (V, 1)"""
    rows = np.asarray(rows, np.float64)
    ids = clamp_ids(ids, V)
    s = np.zeros((V, rows.shape[1])) if base is None else np.asarray(base, np.float64).copy()
    a = np.abs(s)
    terms = np.full((V, 1), 0 if base is None else 1, np.int64)
    np.add.at(s, ids, rows)
    np.add.at(a, ids, np.abs(rows))
    np.add.at(terms, ids, 1)
    return s, terms, a


# ------------------------------------------------------------------------------------------ compaction
def rows_gather(dst, src, idx, n_dev, n_max, map_=None):
    """in place: dst[i] = src[map[idx[i]] or idx[i]] for i < min(n_max, n_dev)"""
    for i in range(max(0, min(n_max, n_dev))):
        dst[i] = src[map_[idx[i]] if map_ is not None else idx[i]]
    return dst


def rows_expand(dst, src, rank, rows, map_=None):
    for r in range(rows):
        dr = map_[r] if map_ is not None else r
        if dr < 0:
            continue
        dst[dr] = src[rank[r]] if rank[r] >= 0 else 0
    return dst


def zero_rows_dyn(X, count, rows_max):
    X[:max(0, min(rows_max, count))] = 0
    return X


# ------------------------------------------------------------------------------------------ ordering
def order_slot(g, T, cpj):
    return ((g % cpj) + (g // cpj // T) * cpj) * T + (g // cpj) % T


def row_order(lens, add, T, cpj, Breal, B, S):
    """-> perm (B), slens (B), steps_sum (sum over the real rows)"""
    steps = [min(max(int(lens[b]) + add, 1), S) if b < Breal else 1 for b in range(B)]
    order = sorted(range(B), key=lambda b: (-steps[b], b))           # descending, stable
    perm, slens = np.full(B, -1, np.int64), np.full(B, -1, np.int64)
    for r, b in enumerate(order):
        slot = order_slot(r >> 4, T, cpj) * 16 + (r & 15)
        assert 0 <= slot < B and perm[slot] < 0, "the slots of a (T, cpj) geometry must be a permutation of the B rows"
        perm[slot], slens[slot] = b, steps[b]
    return perm, slens, int(sum(steps[:Breal]))


def row_map(lens, add, S, B):
    """-> map (S, B), nact (S), count"""
    m, nact, cnt = np.full((S, B), -1, np.int64), np.zeros(S, np.int64), 0
    for t in range(S):
        for b in range(B):
            if t < lens[b] + add:
                m[t, b] = cnt
                cnt += 1
                nact[t] += 1
    return m, nact, cnt


# ------------------------------------------------------------------------------------------ final-state picks
def pick_row(lens, b, B, map_):
    """row of the (positions x B) array that holds row b's last real step, or -1 where it has none"""
    if lens[b] <= 0:
        return -1
    r = (int(lens[b]) - 1) * B + b
    return int(map_[r]) if map_ is not None else r


def pick_last(h, hs, lens, B, map_=None):
    for b in range(B):
        r = pick_row(lens, b, B, map_)
        h[b] = hs[r] if r >= 0 else 0
    return h


def pick_last_add(dhs, d, lens, B, map_=None):
    for b in range(B):
        r = pick_row(lens, b, B, map_)
        if r >= 0:
            dhs[r] = dhs[r] + d[b]
    return dhs


def pick_last_bwd(dh, lens, S, B):
    dhs = np.zeros((S * B,) + dh.shape[1:], dh.dtype)
    for b in range(B):
        if 1 <= lens[b] <= S:
            dhs[(int(lens[b]) - 1) * B + b] = dh[b]
    return dhs


def bf16_bits(x):
    """fp32 array -> (uint16 bf16 bit patterns by truncation, the fp32 values those patterns stand for)"""
    u = np.asarray(x, np.float32).view(np.uint32) & np.uint32(0xffff0000)
    return (u >> np.uint32(16)).astype(np.uint16), u.view(np.float32)


# ------------------------------------------------------------------------------------------ latent
def kl_term(mu, lv):
    mu, lv = np.asarray(mu, np.float64), np.asarray(lv, np.float64)
    return 0.5 * (mu * mu + np.exp(lv) - lv - 1.0)


def kl_scale(mu, lv):
    """the magnitudes the KL term is made of (it cancels near zero)"""
    mu, lv = np.asarray(mu, np.float64), np.asarray(lv, np.float64)
    return mu * mu + np.exp(lv) + np.abs(lv) + 1.0


def latent_fwd(mu, lv, eps, train, free_bits):
    """-> z, kld, sum of max(kld, free_bits); eps: the draw used (ignored unless train)"""
    mu64, lv64 = np.asarray(mu, np.float64), np.asarray(lv, np.float64)
    z = mu64 + np.exp(0.5 * lv64) * np.asarray(eps, np.float64) if train else mu64.copy()
    k = kl_term(mu, lv)
    return z, k, np.maximum(k, float(np.float32(free_bits)))


def latent_bwd(dz, mu, lv, eps, coef, free_bits):
    dz, mu64, lv64 = (np.asarray(a, np.float64) for a in (dz, mu, lv))
    c = np.where(kl_term(mu, lv) >= float(np.float32(free_bits)), float(np.float32(coef)), 0.0)
    dmu = dz + c * mu64
    t1 = dz * np.asarray(eps, np.float64) * 0.5 * np.exp(0.5 * lv64) if eps is not None else np.zeros_like(dz)
    t2 = c * 0.5 * (np.exp(lv64) - 1.0)
    return dmu, t1 + t2, c, t1, t2


def gate_clear(mu, lv, free_bits):
    """no element's KL term within GATE_MARGIN (1 + k) of free_bits: the gate of latent_bwd is discontinuous there"""
    k = kl_term(mu, lv)
    return np.abs(k - float(np.float32(free_bits))) > GATE_MARGIN * (1.0 + k)


# ------------------------------------------------------------------------------------------ sums, losses
def colsum(X, M, N, out, m_dev):
    """-> (sum, terms, abs_sum) of out[n] + sum over the first min(M, m_dev) rows"""
    m = M if m_dev is None else max(0, min(M, m_dev))
    X = np.asarray(X, np.float64)[:m, :N]
    o = np.asarray(out, np.float64)
    return o + X.sum(0), m + 1, np.abs(o) + np.abs(X).sum(0)


def add3(a, b, c):
    s = np.asarray(a, np.float64).copy()
    m = np.abs(s)
    for x in (b, c):
        if x is not None:
            s = s + np.asarray(x, np.float64)
            m = m + np.abs(np.asarray(x, np.float64))
    return s, m


def finalize_losses(loss_samp, n_dev, n_max, kld, free_bits, inv_br, anneal):
    """-> (gen, kl, loss) and their fp32 bounds for any summation order"""
    n = max(0, min(n_max, n_dev))
    ls = np.asarray(loss_samp, np.float64)[:n]
    kt = np.maximum(np.asarray(kld, np.float64), float(np.float32(free_bits)))
    inv_br, anneal = float(np.float32(inv_br)), float(np.float32(anneal))
    sg, sk = ls.sum(), kt.sum()
    gen, kl = sg / max(n, 1), sk * inv_br
    loss = anneal * kl + gen
    # each sum in any order, then one division / product, then a product and a sum
    eg = max(n - 1, 0) * U * np.abs(ls).sum() / max(n, 1) + U * abs(gen)
    ek = max(kt.size - 1, 0) * U * np.abs(kt).sum() * abs(inv_br) + U * abs(kl)
    el = abs(anneal) * ek + eg + U * abs(anneal * kl) + U * abs(loss)
    return np.array([gen, kl, loss]), np.array([eg, ek, el])


# ------------------------------------------------------------------------------------------ Adam
def adam_tf(p, g, m, v, lr_t, b1, b2, eps):
    """one step on fp32 inputs in float64 -> (m, v, p) and their fp32 bounds (see tests/test_gpu_ops.py)"""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1f, b2f = np.float32(b1), np.float32(b2)
    c1, c2 = float(np.float32(1) - b1f), float(np.float32(1) - b2f)          # the kernel's own fp32 1 - b
    b1, b2, lr_t, eps = float(b1f), float(b2f), float(np.float32(lr_t)), float(np.float32(eps))
    m1 = b1 * m + c1 * g
    v1 = b2 * v + c2 * g * g
    den = np.sqrt(v1) + eps
    q = lr_t * m1 / den
    p1 = p - q
    em = U * (np.abs(b1 * m) + np.abs(c1 * g) + np.abs(m1))
    ev = U * (np.abs(b2 * v) + 2 * np.abs(c2 * g * g) + np.abs(v1))
    rel_v = np.divide(ev, v1, out=np.zeros_like(v1), where=v1 > 0)
    eq = lr_t * em / den + np.abs(q) * (0.5 * rel_v + 4 * U)       # sqrt halves v's relative error; sqrt, sum, product, quotient round once each
    ep = eq + U * np.abs(p1)
    return (m1, v1, p1), (em, ev, ep)


# ------------------------------------------------------------------------------------------ layout
def g16_permute(src, D, to_g16):
    """(3D, cols): G16 row ht * 48 + u * 3 + gate <-> natural row gate * D + ht * 16 + u"""
    dst = np.empty_like(src)
    for ht in range(D // 16):
        for u in range(16):
            for gate in range(3):
                g, nat = ht * 48 + u * 3 + gate, gate * D + ht * 16 + u
                if to_g16:
                    dst[g] = src[nat]
                else:
                    dst[nat] = src[g]
    return dst


# ------------------------------------------------------------------------------------------ input builders
INT_MAX_ABS = 8                   # class (a): integers in [-8, 8] times 2^-3


def int_valued(rng, shape):
    """class (a) floats: small integers times a power of two -- every partial sum of fewer than 2^24 / 8 terms is exact in fp32"""
    return (rng.integers(-INT_MAX_ABS, INT_MAX_ABS + 1, shape) * 0.125).astype(np.float32)


def int_sum_is_exact(terms):
    """largest possible partial sum of `terms` class (a) values, in units of 2^-3, stays below 2^24"""
    return int(terms) * INT_MAX_ABS < 2 ** 24


def ladder_ids(rng, V, n, oob=True):
    """n ids in [0, V) (V >= 8) whose per-id counts hold as much of LADDER as fits in n, exactly: ids 0 and V - 1 carry the first two
    steps, the others sit on random ids; what is left of n goes one token at a time to further ids while they last, the rest to one
    more id.  oob: half of id 0's tokens are written as negative ids and half of
    id V - 1's beyond V, which the kernels clamp.  -> (ids as the kernel gets them, counts per clamped id)"""
    assert V >= 8
    others = rng.permutation(np.arange(1, V - 1))
    owners = [0, V - 1] + [int(v) for v in others[:len(LADDER) - 2]]
    rest = [int(v) for v in others[len(LADDER) - 2:]]
    ids, left = [], n
    for v, c in zip(owners, LADDER):
        if c > left:
            break
        ids += [v] * c
        left -= c
    fill = []
    if left:
        k = min(left, max(len(rest) - 1, 0))
        fill = rest[:k] + [rest[-1]] * (left - k)
    ids = np.asarray(ids + fill, np.int64)
    assert ids.size == n
    counts = np.bincount(ids, minlength=V)
    ids = ids[rng.permutation(n)]
    if oob:
        z, t = np.flatnonzero(ids == 0), np.flatnonzero(ids == V - 1)
        ids[z[::2]] = -1 - rng.integers(0, 5, z[::2].size)
        ids[t[::2]] = V + rng.integers(0, 5, t[::2].size)
    return ids.astype(np.int32), counts


def latent_inputs(rng, n, free_bits, clear=True):
    """mu, lv (fp32) around zero -- where the KL term cancels; clear: no element near the free-bits gate (nudged away in mu),
    which the kernels with a discontinuous gate need (latent_fwd's max(k, free_bits) is continuous and takes the raw draw)"""
    mu = (rng.standard_normal(n) * 0.5).astype(np.float32)
    lv = (rng.standard_normal(n) * 0.7).astype(np.float32)
    k = min(n, 8)
    mu[:k] = [0, 0, 1e-3, -1e-3, 2.5, -2.5, 0, 1e-4][:k]
    lv[:k] = [0, 1e-3, 0, -1e-3, 3.0, -6.0, -0.28, 0][:k]
    for _ in range(8 if clear else 0):
        bad = ~gate_clear(mu, lv, free_bits)
        if not bad.any():
            break
        mu[bad] += np.float32(0.25)
    return mu, lv


def adam_inputs(rng, n):
    """p, g, m, v with zeros in g, zeros and tiny values in v"""
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 0.1).astype(np.float32)
    g[np.abs(g) < 1e-4] = 0.0
    g[::5] = 0.0
    m = (rng.standard_normal(n) * 0.05).astype(np.float32)
    v = (rng.random(n) * 1e-2).astype(np.float32)
    v[::3] = 0.0
    v[1::7] = 1e-30
    v[2::11] = 1e-12
    m[0] = 0.0              # element 0: m = v = g = 0, the quotient 0 / eps
    return p, g, m, v
