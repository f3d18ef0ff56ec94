"""The step's small kernels (ops.hip) one by one, through the test hook avae_debug_op, against the plain references of
tests/ops_ref.py on the same input values.  Every output buffer starts as a sentinel and carries guard bytes behind its end; every
comparison covers the whole buffer, so whatever the contract leaves alone must still hold its bits.

Integer kernels and row movers: exact.  Summing kernels, class (a) -- integer-valued floats, every partial sum exact in fp32: exact;
class (b) -- normal draws against the float64 sum: the order-independent bound.  u = 2^-24, the unit roundoff of fp32; expf is
taken at 1 ulp = 2u.  The bounds, each roundoff against the magnitude it applies to (first order, times 1 + 2^-10 for the rest):

    sums (scatter, rows_group_sum, colsum, add3)   (terms - 1) u sum|term| + u |sum|                         largest seen: not measured
    finalize_losses   gen: the sum bound / n + u |gen|;  kl: the sum bound * inv_br + u |kl|;
                      loss: anneal * err(kl) + err(gen) + u |anneal kl| + u |loss|                           not measured
    latent_fwd   z    u (3 |e^(lv/2) eps| + |z|)            expf 2u, product u, sum u                        not measured
                 kld  3u (mu^2 + e^lv + |lv| + 1)           five roundings of at most u M, halved            not measured
                 acc  sum of the kld bounds + n u sum|term|                                                  not measured
    latent_bwd   dmu  u (|c mu| + |dmu|)                                                                     not measured
                 dlv  4u |t1| + c u (e^lv + |e^lv - 1|) + u |dlv|,  t1 = dz eps e^(lv/2) / 2, three products  not measured
                      and expf; t2 = c (e^lv - 1) / 2: expf 2u e^lv, difference u, product u
    adam_tf      m    u (|b1 m| + |c1 g| + |m'|)                                                             not measured
                 v    u (|b2 v| + 2 |c2 g^2| + |v'|)                                                         not measured
                 p    lr err(m) / den + |q| (err(v) / 2v' + 4u) + u |p'|,  q = lr m' / den, den = sqrt v' + eps   not measured
(the fractions: of the bound, on MI355X, at the first run of this file).  No bound was taken from a kernel's output."""
import ctypes as C

import numpy as np
import pytest
import torch

import ops_ref as R

pytestmark = pytest.mark.gpu

U = R.U
SLACK = 1.0 + 2.0 ** -10
SENT_F = np.float32(-1234.5)
SENT_I = np.int32(-7777)
GUARD_BYTE = 0xA5
GUARD = 256               # bytes


@pytest.fixture(scope='module')
def vae():
    from argsim_amd.model import VAE
    m = VAE('train', dim_tgt=64, dim_emb=16, dim_rep=8, rnn_layers=1)
    yield m
    m.close()


class Dev:
    """a device copy of a host array with guard bytes behind its end"""

    def __init__(self, a, dtype=None, lead=0):
        a = np.ascontiguousarray(a, dtype)
        self.shape, self.dtype, self.lead = a.shape, a.dtype, lead
        raw = a.reshape(-1).view(np.uint8)
        self.nbytes = raw.size
        g = np.full(GUARD, GUARD_BYTE, np.uint8)
        self.t = torch.from_numpy(np.concatenate([g[:lead], raw, g])).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr() + self.lead

    def get(self):
        h = self.t.cpu().numpy()
        assert (h[:self.lead] == GUARD_BYTE).all() and (h[self.lead + self.nbytes:] == GUARD_BYTE).all(), 'written outside the buffer'
        return h[self.lead:self.lead + self.nbytes].view(self.dtype).reshape(self.shape).copy()


def f32(shape, fill=SENT_F):
    return np.full(shape, fill, np.float32)


def i32(shape, fill=SENT_I):
    return np.full(shape, fill, np.int32)


def call(m, op, ptrs, ints=(), floats=()):
    """-> None, or the error text where the launcher refused"""
    m._stream()
    raw = [None if x is None else (x.ptr if isinstance(x, Dev) else int(x)) for x in ptrs]
    P = (C.c_void_p * max(len(raw), 1))(*raw)
    I = (C.c_int64 * max(len(ints), 1))(*[int(v) for v in ints])
    F = (C.c_float * max(len(floats), 1))(*[float(v) for v in floats])
    rc = m._l.avae_debug_op(m._h, op.encode(), P, I, F)
    torch.cuda.synchronize()
    return None if rc == 0 else m._l.avae_last_error(m._h).decode()


def run(m, op, ptrs, ints=(), floats=()):
    err = call(m, op, ptrs, ints, floats)
    assert err is None, err


def refused(m, op, ptrs, ints=(), floats=()):
    err = call(m, op, ptrs, ints, floats)
    assert err is not None and 'invalid argument' in err, err


def layout(m, n, V):
    o = (C.c_int64 * 6)()
    assert m._l.avae_debug_op_layout(n, V, o) == 0
    return dict(scatter=o[0], groups=o[1], rank=o[2], uid=o[3], count=o[4], supported=o[5])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8, 8: np.uint64}[a.dtype.itemsize])


def same(got, want, what=''):
    want = np.asarray(want).astype(got.dtype).reshape(got.shape)
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, (what, bad.size, [(int(i), got.ravel()[i], want.ravel()[i]) for i in bad[:5]])


FRAC = {}


def within(name, got, ref, bound):
    """|got - ref| <= bound elementwise (a zero bound: equality); the largest fraction is printed for the record"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.broadcast_to(np.asarray(bound, np.float64) * SLACK, np.shape(ref))
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), name
    frac = float(np.max(np.divide(err, bound, out=np.where(err > 0, np.inf, 0.0), where=bound > 0))) if err.size else 0.0
    FRAC[name] = max(FRAC.get(name, 0.0), frac)
    print('FRAC %s %.4f' % (name, frac))
    assert frac <= 1.0, (name, frac, int(np.argmax(err / np.maximum(bound, 1e-300))))


# ------------------------------------------------------------------------------------------ prep_ids
PREP_SHAPES = ((1, 1, 1), (5, 3, 7), (100, 12, 12), (256, 64, 64), (2048, 8, 1024))
EOS, BOS = 1, 2


def prep_inputs(B, Ss, St, off):
    """row type (b + off) % 5: all eos, eos in the middle of the row, full, two ragged prefixes"""
    rng = np.random.default_rng(B * 131 + St)

    def ids(S):
        x = rng.integers(3, 50, (B, S)).astype(np.int32)
        for b in range(B):
            k = (b + off) % 5
            if k == 0:
                x[b] = EOS
            elif k == 1:
                x[b, S // 2:] = EOS
                x[b, S // 3] = EOS
                if S > 2:
                    x[b, S - 1] = 7          # a real id behind eos ids
            elif k >= 3:
                x[b, rng.integers(0, S + 1):] = EOS
        return x
    return ids(Ss), ids(St), rng.integers(0, 2, (St, B)).astype(np.uint8)


@pytest.mark.parametrize('train', (0, 1))
@pytest.mark.parametrize('shape', PREP_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_prep_ids(vae, shape, train):
    B, Ss, St = shape
    zero2 = (train + PREP_SHAPES.index(shape)) % 2 == 0
    src, tgt, keep = prep_inputs(B, Ss, St, 2 * (1 - train) if B == 1 else 0)
    T = St + 1
    d = dict(src=Dev(src), tgt=Dev(tgt), keep=Dev(keep), src_tm=Dev(i32((Ss, B))), lens_src=Dev(i32(B)), lens_tgt=Dev(i32(B)),
             lead=Dev(i32((T, B))), gold=Dev(i32((T, B))), rank=Dev(i32((T, B))), cidx=Dev(i32(T * B)), ntok=Dev(i32(3)),
             zero2=Dev(f32(6)), chunks=Dev(i32(1024)))
    run(vae, 'prep_ids', [d['src'], d['tgt'], d['keep'], d['src_tm'], d['lens_src'], d['lens_tgt'], d['lead'], d['gold'], d['rank'], d['cidx'],
                          d['ntok'], d['zero2'] if zero2 else None, d['chunks']], [B, Ss, St, EOS, BOS, train, 0], [0.5])
    ref = R.prep_ids(src, tgt, EOS, BOS, train, keep)
    for k in ('src_tm', 'lens_src', 'lens_tgt', 'lead', 'gold', 'rank'):
        same(d[k].get(), ref[k], k)
    n = ref['ntok']
    same(d['ntok'].get(), [n, SENT_I, SENT_I], 'ntok')
    same(d['cidx'].get(), np.concatenate([ref['cidx'], np.full(T * B - n, SENT_I)]), 'cidx')
    same(d['zero2'].get(), [0, 0] + [SENT_F] * 4 if zero2 else [SENT_F] * 6, 'zero2')
    same(d['src'].get(), src), same(d['tgt'].get(), tgt)
    d['chunks'].get()


# ------------------------------------------------------------------------------------------ row_order
GEOMS = ((4, 1), (2, 2), (4, 2), (2, 4))
ORDER_CASES = [(B, g) for B in (16, 64, 128, 256, 1024) for g in GEOMS if (B // 16) % (g[0] * g[1]) == 0]


def order_lens(rng, B, S, kind):
    if kind == 0:
        x = rng.integers(0, 6, B)                    # many ties, zeros
    elif kind == 1:
        x = rng.integers(0, S + 4, B)                # values above S
    else:
        x = np.full(B, 3)                            # one tie over the whole batch
        x[rng.integers(0, B, 3)] = (0, S, S + 9)
    return x.astype(np.int32)


@pytest.mark.parametrize('B,geom', ORDER_CASES, ids=['B%d-T%dc%d' % (B, g[0], g[1]) for B, g in ORDER_CASES])
def test_row_order(vae, B, geom):
    S = 12
    rng = np.random.default_rng(B + 7 * geom[0] + geom[1])
    geoms = [geom] + [g for g in GEOMS if g != geom and (B // 16) % (g[0] * g[1]) == 0]
    for k, Breal in enumerate(sorted({B, B - 1, max(B - 28, 1), 1}, reverse=True)):
        n = 1 + (k + B // 64) % 3
        with_sum = k % 2 == 0
        lens = [Dev(order_lens(rng, B, S, (k + j) % 3)) for j in range(n)]
        adds = [(k + j) % 2 for j in range(n)]
        gs = [geoms[j % len(geoms)] for j in range(n)]
        perm, slens = [Dev(i32(B)) for _ in range(n)], [Dev(i32(B)) for _ in range(n)]
        ssum = Dev(i32(4))
        ptrs = sum(([lens[j], perm[j], slens[j]] for j in range(n)), []) + [ssum if with_sum else None]
        ints = [n, Breal, B, S, 4321] + sum(([adds[j], gs[j][0], gs[j][1]] for j in range(n)), [])
        run(vae, 'row_order', ptrs, ints)
        for j in range(n):
            rp, rs, tot = R.row_order(lens[j].get(), adds[j], gs[j][0], gs[j][1], Breal, B, S)
            got = perm[j].get()
            assert sorted(got.tolist()) == list(range(B)), ('perm is no permutation', Breal, j)
            same(got, rp, ('perm', Breal, j)), same(slens[j].get(), rs, ('slens', Breal, j))
            if j == 0:
                same(ssum.get(), [tot, 4321, SENT_I, SENT_I] if with_sum else [SENT_I] * 4, 'steps_sum')


def test_row_order_refusals(vae):
    x = [Dev(i32(64, 3)) for _ in range(13)]
    g = [0, 4, 1]
    refused(vae, 'row_order', x[:3] + [None], [1, 24, 24, 8, 0] + g)            # B % 16
    refused(vae, 'row_order', x[:12] + [None], [4, 64, 64, 8, 0] + g * 4)       # four orders
    refused(vae, 'row_order', x[:3] + [None], [1, 65, 64, 8, 0] + g)            # B < Breal
    for b in x[:3]:
        same(b.get(), i32(64, 3))


# ------------------------------------------------------------------------------------------ row_map
@pytest.mark.parametrize('add', (0, 1))
@pytest.mark.parametrize('S', (1, 5, 40))
@pytest.mark.parametrize('B', (1, 7, 256, 257, 600))
def test_row_map(vae, B, S, add):
    rng = np.random.default_rng(B * 41 + S)
    ragged = rng.integers(0, S + 1, B).astype(np.int32)
    ragged[rng.integers(0, B)] = 0
    if B > 1:
        ragged[B - 1] = S
    for lens in (ragged, np.zeros(B, np.int32)):
        d = [Dev(lens), Dev(i32((S, B))), Dev(i32(S)), Dev(i32(2))]
        run(vae, 'row_map', d, [add, S, B])
        rm, rn, rc = R.row_map(lens, add, S, B)
        same(d[1].get(), rm, 'map'), same(d[2].get(), rn, 'nact'), same(d[3].get(), [rc, SENT_I], 'count')
    assert add == 1 or rc == 0


# ------------------------------------------------------------------------------------------ token groups
def group_ids(V, n, seed):
    rng = np.random.default_rng(seed + V * 3 + n)
    if V < 8:
        return rng.integers(-3, V + 3, n).astype(np.int32)
    return R.ladder_ids(rng, V, n)[0]


def build_groups(m, ids, V, lists):
    """id_groups_build on a sentinel-filled scratch -> (scratch Dev, layout)"""
    n = ids.size
    lay = layout(m, n, V)
    sc = Dev(i32(lay['groups']))
    run(m, 'id_groups_build', [Dev(ids), sc], [n, V, int(lists)])
    return sc, lay


@pytest.mark.parametrize('lists', (0, 1))
@pytest.mark.parametrize('n', (1, 31, 1024, 1025, 5000))
@pytest.mark.parametrize('V', (1, 8, 1000, 12288))
def test_id_groups_build(vae, V, n, lists):
    for ids in (group_ids(V, n, lists), np.full(n, V // 2, np.int32)):         # the second: every id absent but one
        sc, lay = build_groups(vae, ids, V, lists)
        assert lay['supported'] == 1 and lay['count'] + 1 <= lay['groups']
        s = sc.get()
        rank, uid, nuniq = R.id_groups(ids, V)
        same(s[lay['rank']:lay['rank'] + V], rank, 'rank')
        same(s[lay['count']:lay['count'] + 1], [nuniq], 'nuniq')
        same(s[lay['uid']:lay['uid'] + V], np.concatenate([uid, np.full(V - nuniq, SENT_I)]), 'uid')
    assert nuniq == 1


def test_id_groups_refusals(vae):
    sc, ids = Dev(i32(layout(vae, 8, 12289)['groups'])), Dev(i32(8, 0))
    assert layout(vae, 8, 12289)['supported'] == 0
    refused(vae, 'id_groups_build', [ids, sc], [8, 12289, 1])
    refused(vae, 'id_groups_build', [ids, sc], [0, 100, 1])
    refused(vae, 'rows_group_sum', [sc, ids, sc, sc], [8, 6, 100])             # W & 3
    refused(vae, 'rows_gather_ranked', [sc, sc, ids, ids], [8, 6, 100])        # W & 3
    refused(vae, 'rows_add_indexed', [sc, sc, ids, ids], [8, 6])               # D & 3
    same(sc.get(), i32(sc.shape)), same(ids.get(), i32(8, 0))


@pytest.mark.parametrize('V,n', ((1, 5), (8, 300), (1000, 1025), (12288, 2049)))
def test_rank_rows(vae, V, n):
    rng = np.random.default_rng(V + n)
    ids, rank = rng.integers(-2, V + 2, n).astype(np.int32), rng.integers(-1, 9999, V).astype(np.int32)
    out = Dev(i32(n + 5))
    run(vae, 'rank_rows', [out, Dev(ids), Dev(rank)], [n, V])
    same(out.get(), np.concatenate([R.rank_rows(ids, rank, V), [SENT_I] * 5]))


@pytest.mark.parametrize('W', (4, 256, 260, 1536))
def test_rows_gather_ranked(vae, W):
    V, n = 1000, 1025
    rng = np.random.default_rng(W)
    ids = group_ids(V, n, 5)
    rank, uid, nuniq = R.id_groups(ids, V)
    src = rng.standard_normal((nuniq, W)).astype(np.float32)
    dst = Dev(f32((n + 2, W)))
    run(vae, 'rows_gather_ranked', [dst, Dev(src), Dev(ids), Dev(rank, np.int32)], [n, W, V])
    same(dst.get(), np.concatenate([R.rows_gather_ranked(src, ids, rank, V), f32((2, W))]))


@pytest.mark.parametrize('D', (4, 256, 260, 516))
def test_embed_gather(vae, D):
    V, n = 37, 1030
    rng = np.random.default_rng(D)
    E, ids = rng.standard_normal((V, D)).astype(np.float32), rng.integers(-2, V + 2, n).astype(np.int32)
    out = Dev(f32((n + 2, D)))
    run(vae, 'embed_gather', [Dev(E), Dev(ids), out], [n, D, V])
    same(out.get(), np.concatenate([R.embed_gather(E, ids, V), f32((2, D))]))


@pytest.mark.parametrize('cols', (1, 4, 512))
@pytest.mark.parametrize('D', (16, 32, 64, 128, 256, 512))
def test_g16_permute(vae, D, cols):
    rng = np.random.default_rng(D + cols)
    nat = rng.standard_normal((3 * D, cols)).astype(np.float32)
    g, back = Dev(f32((3 * D, cols))), Dev(f32((3 * D, cols)))
    run(vae, 'g16_permute', [g, Dev(nat)], [D, cols, 1])
    same(g.get(), R.g16_permute(nat, D, True))
    run(vae, 'g16_permute', [back, g], [D, cols, 0])
    same(back.get(), nat)
    same(back.get(), R.g16_permute(R.g16_permute(nat, D, True), D, False))


# ------------------------------------------------------------------------------------------ row movers
@pytest.mark.parametrize('use_map', (0, 1))
@pytest.mark.parametrize('D', (4, 260))
def test_rows_gather(vae, D, use_map):
    n_max, nsrc, nmap = 37, 50, 60
    rng = np.random.default_rng(D + use_map)
    src = rng.standard_normal((nsrc, D)).astype(np.float32)
    idx = rng.integers(0, nmap if use_map else nsrc, n_max + 5).astype(np.int32)
    mp = rng.integers(0, nsrc, nmap).astype(np.int32)
    for n_dev in (0, n_max - 1, n_max, n_max + 5):
        dst = Dev(f32((n_max + 5, D)))
        run(vae, 'rows_gather', [dst, Dev(src), Dev(idx), Dev(np.int32([n_dev])), Dev(mp) if use_map else None], [n_max, D])
        same(dst.get(), R.rows_gather(f32((n_max + 5, D)), src, idx, n_dev, n_max, mp if use_map else None), n_dev)


@pytest.mark.parametrize('use_map', (0, 1))
@pytest.mark.parametrize('D', (4, 260))
def test_rows_expand(vae, D, use_map):
    rows, nsrc = 41, 20
    rng = np.random.default_rng(D + use_map)
    src = rng.standard_normal((nsrc, D)).astype(np.float32)
    rank = rng.integers(-1, nsrc, rows).astype(np.int32)
    rank[[0, 7, rows - 1]] = -1
    mp = rng.permutation(rows).astype(np.int32)
    mp[[3, 7, 30]] = -1                      # (row 7: rank -1 AND no place: stays untouched)
    dst = Dev(f32((rows + 3, D)))
    run(vae, 'rows_expand', [dst, Dev(src), Dev(rank), Dev(mp) if use_map else None], [rows, D])
    same(dst.get(), R.rows_expand(f32((rows + 3, D)), src, rank, rows, mp if use_map else None))


@pytest.mark.parametrize('count', (0, 7, 19, 30))
def test_zero_rows_dyn(vae, count):
    rows_max, W = 19, 12
    X = Dev(f32((rows_max + 11, W)))
    run(vae, 'zero_rows_dyn', [X, Dev(np.int32([count]))], [rows_max, W])
    same(X.get(), R.zero_rows_dyn(f32((rows_max + 11, W)), count, rows_max))


@pytest.mark.parametrize('nbytes,lead', [(b, 0) for b in (0, 4, 12, 16, 20, 4096 + 8)] + [(20, 4)])
def test_zero_fill(vae, nbytes, lead):
    """lead 4: a pointer 4 bytes off the 16-byte grid, which takes the runtime's memset"""
    buf = Dev(i32(nbytes // 4 + 9), lead=lead)
    assert (buf.ptr & 15) == lead
    run(vae, 'zero_fill', [buf], [nbytes])
    want = i32(nbytes // 4 + 9)
    want[:nbytes // 4] = 0
    same(buf.get(), want)


@pytest.mark.parametrize('use_map', (0, 1))
@pytest.mark.parametrize('B', (1, 33))
@pytest.mark.parametrize('W', (4, 64, 1024, 1028))
def test_pick_last(vae, W, B, use_map):
    S = 5
    rng = np.random.default_rng(W + B)
    for lens in ([np.int32([0]), np.int32([1]), np.int32([S])] if B == 1 else [np.resize(np.int32([0, 1, S, 3, 0, 2, S, 1, 4]), B)]):
        mp, _, count = R.row_map(lens, 0, S, B)
        mp = mp.ravel().astype(np.int32)
        rows = count if use_map else S * B
        dmap = Dev(mp) if use_map else None
        hmap = mp if use_map else None
        assert not use_map or all(mp[b] == -1 for b in range(B) if lens[b] == 0)
        hs = rng.standard_normal((rows + 1, W)).astype(np.float32)            # (one spare row: no empty buffer at count 0)
        h16, hs16 = R.bf16_bits(hs)
        d = rng.standard_normal((B, W)).astype(np.float32)
        dl = Dev(lens)
        h = Dev(f32((B + 1, W)))
        run(vae, 'pick_last', [h, Dev(hs), dl, dmap], [B, W])
        same(h.get(), np.concatenate([R.pick_last(f32((B, W)), hs, lens, B, hmap), f32((1, W))]), 'pick_last')
        h = Dev(f32((B + 1, W)))
        run(vae, 'pick_last16', [h, Dev(h16), dl, dmap], [B, W])
        same(h.get(), np.concatenate([R.pick_last(f32((B, W)), hs16, lens, B, hmap), f32((1, W))]), 'pick_last16')
        dhs = Dev(hs)
        run(vae, 'pick_last_add', [dhs, Dev(d), dl, dmap], [B, W])
        same(dhs.get(), R.pick_last_add(hs.copy(), d, lens, B, hmap), 'pick_last_add')
        if not use_map:
            out = Dev(f32((S * B + 1, W)))
            run(vae, 'pick_last_bwd', [out, Dev(d), dl], [S, B, W])
            same(out.get(), np.concatenate([R.pick_last_bwd(d, lens, S, B), f32((1, W))]), 'pick_last_bwd')


# ------------------------------------------------------------------------------------------ summing kernels
def draw(rng, shape, cls):
    return R.int_valued(rng, shape) if cls == 'a' else rng.standard_normal(shape).astype(np.float32)


def check_sum(name, cls, got, s, terms, abs_sum):
    if cls == 'a':
        same(got, s, name)
    else:
        within(name, got, s, R.sum_bound(s, terms, abs_sum))


# (D, V, n0, n1): the D and V edges of the grouped form and its two fallbacks at the whole count ladder, then the token-count edges
SCATTER_CASES = ([(D, 1000, 1400, 1600) for D in (4, 256, 260, 512, 516)] + [(256, V, 3000, 0) for V in (8, 12288, 12289)] + [(512, 12288, 0, 3000)]
                 + [(260, 1000, 1, 0), (260, 1000, 0, 1023), (260, 1000, 1000, 24), (260, 1000, 1025, 0), (260, 1000, 512, 513)])
SCATTER_MAX_TERMS = 3000 + 1


@pytest.mark.parametrize('cls', ('a', 'b'))
@pytest.mark.parametrize('D,V,n0,n1', SCATTER_CASES, ids=['D%d-V%d-%d+%d' % c for c in SCATTER_CASES])
def test_embed_scatter_add2(vae, D, V, n0, n1, cls):
    n = n0 + n1
    rng = np.random.default_rng(D + V + n)
    ids, counts = R.ladder_ids(rng, V, n)
    if n == 3000:
        assert all(c in counts for c in R.LADDER)
    rows, dE = draw(rng, (n, D), cls), draw(rng, (V + 1, D), cls)
    sc = Dev(i32(layout(vae, n, V)['scatter']))
    out, d_ids, d_rows = Dev(dE), Dev(ids), Dev(rows)
    run(vae, 'embed_scatter_add2', [out, d_ids.ptr, d_rows.ptr, d_ids.ptr + 4 * n0, d_rows.ptr + 4 * n0 * D, sc], [n0, n1, D, V])
    s, terms, a = R.scatter_sum(V, ids, rows, dE[:V])
    got = out.get()
    absent = np.flatnonzero(counts == 0)
    same(got[absent], dE[absent], 'absent ids'), same(got[V:], dE[V:], 'behind the table')
    check_sum('scatter', cls, got[:V], s, terms, a)
    sc.get(), same(d_ids.get(), ids), same(d_rows.get(), rows)


GROUP_SUM_CASES = [(W, 1000, 3000) for W in (4, 256, 260, 1536)] + [(260, 8, 3000), (256, 12288, 1025), (4, 1000, 1)]


@pytest.mark.parametrize('cls', ('a', 'b'))
@pytest.mark.parametrize('W,V,n', GROUP_SUM_CASES, ids=['W%d-V%d-n%d' % c for c in GROUP_SUM_CASES])
def test_rows_group_sum(vae, W, V, n, cls):
    rng = np.random.default_rng(W + V + n)
    ids, counts = R.ladder_ids(rng, V, n)
    src = draw(rng, (n, W), cls)
    sc, lay = build_groups(vae, ids, V, 1)
    rank, uid, nuniq = R.id_groups(ids, V)
    dst = Dev(f32((nuniq + 3, W)))
    run(vae, 'rows_group_sum', [dst, Dev(ids), Dev(src), sc], [n, W, V])
    s, terms, a = R.scatter_sum(V, ids, src)
    got = dst.get()
    same(got[nuniq:], f32((3, W)), 'rows at and beyond nuniq')
    check_sum('group_sum', cls, got[:nuniq], s[uid], terms[uid], a[uid])


@pytest.mark.parametrize('nuniq', (0, 20, 29, 30, 45))
def test_rows_add_indexed(vae, nuniq):
    n_max, D, V = 30, 260, 70
    rng = np.random.default_rng(nuniq)
    uid = np.sort(rng.permutation(V)[:n_max + 15]).astype(np.int32)
    src, dst = rng.standard_normal((n_max + 15, D)).astype(np.float32), rng.standard_normal((V, D)).astype(np.float32)
    out = Dev(dst)
    run(vae, 'rows_add_indexed', [out, Dev(src), Dev(uid), Dev(np.int32([nuniq]))], [n_max, D])
    want = dst.copy()
    for r in range(min(n_max, nuniq)):
        want[uid[r]] = dst[uid[r]] + src[r]
    same(out.get(), want)


COLSUM_SHAPES = ((1, 1, 4), (3, 70, 72), (17, 64, 64), (100, 130, 132), (4099, 512, 512))
COLSUM_MAX_TERMS = 4099 + 1


@pytest.mark.parametrize('cls', ('a', 'b'))
@pytest.mark.parametrize('M,N,ldx', COLSUM_SHAPES, ids=lambda v: str(v))
def test_colsum(vae, M, N, ldx, cls):
    rng = np.random.default_rng(M + N)
    X, out0 = draw(rng, (M + 9, ldx), cls), draw(rng, N + 3, cls)
    dX = Dev(X)
    for m_dev in (None, 0, M - 1, M + 9):
        out = Dev(out0)
        run(vae, 'colsum', [dX, out, None if m_dev is None else Dev(np.int32([m_dev]))], [M, N, ldx])
        s, terms, a = R.colsum(X, M, N, out0[:N], m_dev)
        got = out.get()
        same(got[N:], out0[N:], 'behind N')
        check_sum('colsum', cls, got[:N], s, terms, a)
    same(dX.get(), X)


@pytest.mark.parametrize('n', (1, 255, 70000))
def test_add3(vae, n):
    rng = np.random.default_rng(n)
    for cls in ('a', 'b'):
        a, b, c = (draw(rng, n, cls) for _ in range(3))
        for use_b, use_c in ((1, 1), (1, 0), (0, 1), (0, 0)):
            out = Dev(f32(n + 3))
            run(vae, 'add3', [out, Dev(a), Dev(b) if use_b else None, Dev(c) if use_c else None], [n])
            s, mag = R.add3(a, b if use_b else None, c if use_c else None)
            got = out.get()
            same(got[n:], f32(3))
            check_sum('add3', cls, got[:n], s, 1 + use_b + use_c, mag)


FINALIZE_NS = (0, 1, 1023, 1025, 20000)
FINALIZE_NKS = (4, 4096)
FINALIZE_MAX_TERMS = 20000


def finalize_inputs(n_max, nk, free_bits, cls):
    rng = np.random.default_rng(n_max + nk)
    if cls == 'a':
        return np.abs(R.int_valued(rng, n_max + 7)), np.abs(R.int_valued(rng, nk)) + np.float32(0.125)
    mu, lv = R.latent_inputs(rng, nk, free_bits)
    return (rng.random(n_max + 7) * 9).astype(np.float32), R.kl_term(mu, lv).astype(np.float32)


@pytest.mark.parametrize('free_bits', (0.0, 0.02))
@pytest.mark.parametrize('nk', FINALIZE_NKS)
@pytest.mark.parametrize('n', FINALIZE_NS)
def test_finalize_losses(vae, n, nk, free_bits):
    n_max = n
    inv_br, anneal = 1.0 / 64, 0.375
    for cls in ('a', 'b'):
        loss, kld = finalize_inputs(n_max, nk, free_bits, cls)
        for n_dev in (max(n_max - 3, 0), n_max + 5):
            runs = []
            for _ in range(2):
                out = Dev(f32(5))
                run(vae, 'finalize_losses', [out, Dev(loss), Dev(np.int32([n_dev])), Dev(kld)], [n_max, nk], [free_bits, inv_br, anneal])
                runs.append(out.get())
            same(runs[0], runs[1], 'two runs')
            same(runs[0][3:], f32(2))
            ref, bound = R.finalize_losses(loss, n_dev, n_max, kld, free_bits, inv_br, anneal)
            if cls == 'a':          # exact sums; 1/64 and 0.375 exact; the division by n rounds once
                ns = max(min(n_max, n_dev), 1)
                sg = np.float32(loss[:min(n_max, n_dev)].astype(np.float64).sum())
                gen = sg / np.float32(ns)
                kl = np.float32(np.maximum(kld, np.float32(free_bits)).astype(np.float64).sum() * inv_br)
                same(runs[0][:2], [gen, kl], 'exact sums')
            within('finalize', runs[0][:3], ref, bound)


# ------------------------------------------------------------------------------------------ elementwise float kernels
LATENT_N = 70001          # several strides of the 1024 x 256 grid


@pytest.mark.parametrize('outs', (0, 1), ids=('no-kld-acc', 'kld-acc'))
@pytest.mark.parametrize('eps_given', (0, 1))
@pytest.mark.parametrize('train', (0, 1))
def test_latent_fwd(vae, train, eps_given, outs):
    n, fb = LATENT_N, 0.02
    rng = np.random.default_rng(train + 2 * eps_given)
    mu, lv = R.latent_inputs(rng, n, fb, clear=False)
    eps_in = rng.standard_normal(n).astype(np.float32)
    acc0 = np.float32(3.5)
    z, kld, eps_out, acc = Dev(f32(n + 3)), Dev(f32(n + 3)), Dev(f32(n + 3)), Dev(np.float32([acc0, SENT_F]))
    run(vae, 'latent_fwd', [Dev(mu), Dev(lv), Dev(eps_in) if eps_given else None, eps_out, z, kld if outs else None, acc if outs else None],
        [n, train, 12345], [fb])
    e = eps_out.get()
    same(e[n:], f32(3))
    if train:
        if eps_given:
            same(e[:n], eps_in, 'eps echoed')
        else:
            assert np.isfinite(e[:n]).all() and abs(float(e[:n].mean())) < 0.02 and abs(float(e[:n].std()) - 1) < 0.02
        used = e[:n]
    else:
        same(e[:n], f32(n), 'no draw outside training')
        used = np.zeros(n, np.float32)
    rz, rk, rt = R.latent_fwd(mu, lv, used, train, fb)
    gz, gk, ga = z.get(), kld.get(), acc.get()
    same(gz[n:], f32(3)), same(gk[n:], f32(3)), same(ga[1:], [SENT_F])
    if train:
        within('latent_fwd.z', gz[:n], rz, U * (3 * np.abs(rz - mu.astype(np.float64)) + np.abs(rz)))
    else:
        same(gz[:n], mu, 'z = mu')
    kb = 3 * U * R.kl_scale(mu, lv)
    if outs:
        within('latent_fwd.kld', gk[:n], rk, kb)
        within('latent_fwd.acc', ga[:1], [acc0 + rt.sum()], [kb.sum() + n * U * (acc0 + np.abs(rt).sum()) + U * abs(acc0 + rt.sum())])
    else:
        same(gk[:n], f32(n)), same(ga[:1], [acc0])


@pytest.mark.parametrize('free_bits', (0.0, 0.02))
@pytest.mark.parametrize('eps_given', (0, 1))
def test_latent_bwd(vae, eps_given, free_bits):
    B, Rr = 37, 70
    n, coef = B * Rr, 0.37 / 64
    rng = np.random.default_rng(eps_given)
    mu, lv = R.latent_inputs(rng, n, free_bits)
    assert R.gate_clear(mu, lv, free_bits).all()
    dz, eps = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    dmu, dlv = Dev(f32(n + 3)), Dev(f32(n + 3))
    run(vae, 'latent_bwd', [Dev(dz), Dev(mu), Dev(lv), Dev(eps) if eps_given else None, dmu, dlv], [B, Rr], [coef, free_bits])
    rm, rl, c, t1, t2 = R.latent_bwd(dz, mu, lv, eps if eps_given else None, coef, free_bits)
    assert free_bits == 0 or (0 < np.count_nonzero(c) < n)            # both sides of the gate
    gm, gl = dmu.get(), dlv.get()
    same(gm[n:], f32(3)), same(gl[n:], f32(3))
    el = np.exp(lv.astype(np.float64))
    within('latent_bwd.dmu', gm[:n], rm, U * (np.abs(c * mu) + np.abs(rm)))
    within('latent_bwd.dlv', gl[:n], rl, U * (4 * np.abs(t1) + c * (el + np.abs(el - 1)) + np.abs(rl)))


@pytest.mark.parametrize('skip', (None, 0, 1))
@pytest.mark.parametrize('n', (4, 7, 1000003))
def test_adam_tf(vae, n, skip):
    rng = np.random.default_rng(n)
    p, g, m, v = R.adam_inputs(rng, n)
    hp = (1e-3 * 1.7, 0.9, 0.999, 1e-8)
    d = [Dev(np.concatenate([x, f32(3)])) for x in (p, g, m, v)]
    flag = None if skip is None else Dev(np.int32([skip]))
    for step in range(2):
        p0, g0, m0, v0 = (x.get()[:n] for x in d)
        run(vae, 'adam_tf', d + [flag], [n], hp)
        got = [x.get() for x in d]
        for x in got:
            same(x[n:], f32(3), 'behind n')
        same(got[1][:n], g, 'g')
        if skip:
            same(got[0][:n], p, 'p'), same(got[2][:n], m, 'm'), same(got[3][:n], v, 'v')
            continue
        (rm, rv, rp), (em, ev, ep) = R.adam_tf(p0, g0, m0, v0, *hp)
        within('adam.m', got[2][:n], rm, em)
        within('adam.v', got[3][:n], rv, ev)
        within('adam.p', got[0][:n], rp, ep)
