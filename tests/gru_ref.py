"""float64 numpy restatement of the GRU launch contract (argsim_amd/csrc/kernels.h, section GRU; gru_dev.h "Padding skipped"), the cases of
tests/test_gpu_gru.py, and the comparison both test files share.  No GPU, no model: what one gru_forward / gru_backward call reads and writes.

Layout.  G16 column c' = ht * 48 + u * 3 + gate = unit * 3 + gate: the three gates of a unit side by side (checked against
ops_ref.g16_permute in tests/test_gru_ref.py).  Step p of a row of length len touches position pos_map(p, len, reverse).  Every per-position
array is time-major, row pos * B + b, or, with a row map, the row the map gives (compact layout; -1: nothing read or written).

Method.  A forward launch is checked by induction, not against a second recurrence: (a) the saved h_prev of step p is, bit for
bit, h0 (step 0) or the h the launch stored for step p - 1; (b) h and the saved gates of step p agree with step_fwd applied to the launch's OWN
h_prev of that step.  A backward launch takes drawn sv / hp / dh_out and is compared with the float64 recurrence over step_bwd (bf16 forms: the
recurrence takes dgh of step p + 1 from the launch's own output, rounded as the kernel rounds it).

Tolerance.  The yardstick of an output array is the largest error of the float32 restatement of the same single step (this file's step
functions with dtype = float32) against float64 on the same inputs, floored at 4 * 2^-24 * max |reference|; a launch may use MARGIN = 8 of
it (other summation order over K, 1-ulp exp / rcp), times the number of steps behind a position in the backward, whose error grows linearly
through dgh R and the carry dH u.  Bias sums: ops_ref.sum_bound.

16-bit outputs are widened exactly and get half a bf16 ulp of the reference on top, half_ulp_bf16(): 2^(floor(log2 |x|) - 8).  That is NOT
2^-9 |x| everywhere: bf16 keeps 8 significant bits, so half an ulp is 2^-9 |x| only at the top of a binade and 2^-8 |x| at its bottom (1 + 2^-8
+ 2^-20 rounds to 1 + 2^-7: an error of 0.996 * 2^-8 |x|); a correctly rounded value misses 2^-9 |x| for about half of all inputs
(tests/test_gru_ref.py test_half_ulp_of_bf16).  The stronger statement is checked beside it: a 16-bit array is, bit for bit, the
round-to-nearest-even bf16 of the fp32 array the same launch gives without it.

16-bit inputs (Case.in16): the backward's drawn sv / hp are rounded to bf16 and packed as uint16 beside the fp32 arrays of the same values, NAN16
wherever no step reads (read_mask); the launch that reads them must give the bits of the launch that reads the fp32 arrays."""
import dataclasses

import numpy as np

import ops_ref
from ops_ref import U

SENT = np.int32(0x7FC5A5A5)       # a quiet NaN with a payload no arithmetic produces: "nobody wrote here"
SENT16 = np.uint16(0x7FC5)
GUARD_ROWS = 3
MARGIN = 8.0
TABLE_ROWS, TABLE_V = 17, 40     # a table-fed layer: ids of a vocabulary of TABLE_V, TABLE_ROWS of them present
FORMS = ('stepwise', 'persistent', 'item', 'team', 'team_rs')          # GruForm, in its order


# ------------------------------------------------------------------------------------------ number formats, layout
def bf16_rne(x):
    """fp32 values -> (bf16 bit patterns, the fp32 values they stand for), round to nearest even as pack_bf16 converts"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32)
    return ops_ref.bf16_bits(r.view(np.float32))          # (exact on values that are bf16 already)


def half_ulp_bf16(x):
    """half a unit in the last place of bf16 (8 significant bits) at |x|: 2^(floor(log2 |x|) - 8), between 2^-9 |x| and 2^-8 |x|; 0 at 0"""
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(x)
    return np.where(x > 0, np.ldexp(1.0, e - 9), 0.0)


def widen16(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def g16_col(unit, gate):
    return unit * 3 + gate


def pos_map(p, length, reverse):
    return length - 1 - p if (reverse and p < length) else p


def pos_table(S, plen, reverse, pm=pos_map):
    """(S, B): position of step p of row b"""
    return np.array([[pm(p, int(l), reverse) for l in plen] for p in range(S)], np.int64).reshape(S, len(plen))


def team_steps(slens, T, cpj, S):
    """steps per SLOT of a (T, cpj) team geometry: the maximum of slens over a team's 16 slots, then the suffix maximum over the row blocks
    slot, slot + cpj, ... of a workgroup (gru_dev.h team_steps and the nst0..3 chain of the team kernels)"""
    slens = np.asarray(slens, np.int64)
    Bg, RB = slens.size, 16 * T
    nrb = (Bg // RB) // cpj
    out = np.zeros(Bg, np.int64)
    for slot in range(cpj):
        for team in range(T):
            nst = 0
            for r in range(nrb - 1, -1, -1):
                row0 = (slot + r * cpj) * RB + team * 16
                nst = max(nst, min(S, int(slens[row0:row0 + 16].max())))
                out[row0:row0 + 16] = nst
    return out


# ------------------------------------------------------------------------------------------ one step
def _sig(x):
    return 1 / (1 + np.exp(-x))


def step_fwd(gi_p, h_prev, R, bR, bf16, dtype=np.float64, swap_ru=False, a_rows=None):
    """one cell update from a given h_prev: gi_p (B, 3D), R (3D, D), bR (3D) in G16 order -> h, r, u, n, hn (B, D).  bf16: both operands of
    h R' are rounded to bf16 first, everything else stays unrounded.  dtype float32: the restatement the yardstick is measured with.
    (swap_ru, a_rows: the defects of tests/test_gru_ref.py -- a_rows: the rows whose h_prev enters the product)"""
    B, D = h_prev.shape
    a, w = np.asarray(h_prev), np.asarray(R)
    if bf16:
        a, w = bf16_rne(a)[1], bf16_rne(w)[1]
    if a_rows is not None:
        a = a[a_rows]
    a, w = a.astype(dtype), w.astype(dtype)
    gh = (a @ w.T + np.asarray(bR, dtype)).reshape(B, D, 3)
    g = np.asarray(gi_p, dtype).reshape(B, D, 3)
    one = dtype(1)
    r, u = _sig(g[..., 0] + gh[..., 0]), _sig(g[..., 1] + gh[..., 1])
    if swap_ru:
        r, u = u, r
    n = np.tanh(g[..., 2] + r * gh[..., 2])
    h = (one - u) * n + u * np.asarray(h_prev, dtype)
    return h, r, u, n, gh[..., 2]


def step_bwd(dh_out_p, carry, dgh_next, R, sv_p, hp_p, bf16, dtype=np.float64):
    """one BPTT step: dH = dh_out_p + carry + dgh_next R, carry = dH u of step p + 1 (zeros at the last step), dgh_next (B, 3D) or None.
    sv_p (B, D, 4) = r, u, n, hn -> dgi, dgh (B, 3D), the carry this step hands on, dH"""
    B, D = hp_p.shape
    dH = np.asarray(dh_out_p, dtype) + np.asarray(carry, dtype)
    if dgh_next is not None:
        dH = dH + bf_prod(dgh_next, R, bf16, dtype)
    s = np.asarray(sv_p, dtype)
    r, u, n, hn = s[..., 0], s[..., 1], s[..., 2], s[..., 3]
    one = dtype(1)
    dn = dH * (one - u) * (one - n * n)
    du = dH * (np.asarray(hp_p, dtype) - n) * u * (one - u)
    dr = dn * hn * r * (one - r)
    dgi = np.stack([dr, du, dn], -1).reshape(B, 3 * D)
    dgh = np.stack([dr, du, dn * r], -1).reshape(B, 3 * D)
    return dgi, dgh, dH * u, dH


# ------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    fwd: bool
    njobs: int
    S: int
    B: int
    D: int
    persistent: int = 1
    reach: tuple = ('persistent', 0, 0, 0)          # form, T, C, pipe: what avae_debug_gru_plan must answer for the case
    G: int = 0                      # 0: as the model chooses (gru_geometry)
    rpg: int = 0
    ldh_pad: int = 0                # floats beyond njobs * D in a row of hs / dh_out
    ldg_pad: int = 0
    h0: bool = False                # h0 given (forward) / dh0 wanted (backward)
    save: bool = True               # forward: sv and hp wanted
    item: int = 0                   # GruArgs::item_pipeline
    xbuf: bool = False
    bf16: int = 0
    bwd_rs: int = 0
    stagger: int = 0
    force_slow: int = 0
    spec: int = 0
    skip: str = ''                  # '': no slens / perm; 'sorted': row_order; 'unsorted': any permutation
    cmp: bool = False               # rowmap: compact external arrays
    Breal: int = 0                  # > 0: phantom slots, B slots hold Breal rows (needs cmp)
    out16: bool = False             # bf16 team forms: forward hs16 + hp16 + sv16, backward dgi16 + dgh16 INSTEAD of the fp32 arrays
    dgh16_only: bool = False        # backward: dgh16 alone, dgi stays fp32 (a table-fed layer)
    table: bool = False             # forward: gi is a per-id table of TABLE_ROWS rows read through gi_rows
    by_pos: bool = False            # backward, with cmp: dgi keeps the padded (pos * B + row) layout, zeros at padding (dgi_by_pos)
    in16: str = ''                  # backward, bf16 team forms: 'sv' the saved gates (GruArgs::sv16), 'hp' h_prev (GruJob::hp16) or 'sv+hp' are READ as bf16, as
                                    # the bf16 forward leaves them; the drawn sv / hp are rounded to bf16 on the host, so the fp32 arrays hold the same values
    seed: int = 0

    @property
    def id(self):
        return '%s-%s-j%d-S%d-B%d-D%d' % (self.name, 'fwd' if self.fwd else 'bwd', self.njobs, self.S, self.B, self.D)

    @property
    def rows(self):                 # rows per position of every external array
        return self.Breal or self.B

    @property
    def ldh(self):
        return self.njobs * self.D + self.ldh_pad

    @property
    def ldg(self):
        return self.njobs * 3 * self.D + self.ldg_pad

    def xbuf_floats(self, rs_floats=0):
        if not self.xbuf:
            return 0
        return max(self.njobs * self.S * self.B * self.D * (1 if self.fwd else 3), rs_floats if self.bwd_rs else 0)

    def shape_ints(self, rs_floats=0):
        """the shape fields avae_debug_gru_plan / avae_debug_gru take, in their order"""
        return [self.njobs, self.S, self.rows, self.D, self.ldg, self.ldh, self.B if self.Breal else 0, self.G, self.rpg, 0, self.S, self.item,
                self.bf16, self.bwd_rs, self.xbuf_floats(rs_floats)]


def ragged_lens(rng, S, B):
    """one full row, one row of length 1, two different lengths inside one 16-row team (rows 0..3), the rest random"""
    lens = rng.integers(1, S + 1, B)
    fixed = [S, 1, max(S - 2, 1), min(2, S)][:B]
    lens[:len(fixed)] = fixed
    return lens.astype(np.int32)


@dataclasses.dataclass
class Rows:
    """who sits where: what the case's row order and row map make of (step, row)"""
    lens: np.ndarray            # (rows) int32
    plen: np.ndarray            # (rows): the length pos_map is taken with (slens of the row's slot under a row order)
    steps: np.ndarray           # (rows): steps the launch computes for the row
    rowmap: np.ndarray          # (S, rows): row of the external arrays, -1 none
    nrows: int                  # rows of the external arrays
    perm: np.ndarray = None     # (B slots) or None
    slens: np.ndarray = None
    map_dev: np.ndarray = None  # (S, rows) the row map as the launch takes it, or None (padded layout)


def make_rows(c, T=0, cpj=0):
    rng = np.random.default_rng(1000 + c.seed)
    n = c.rows
    lens = ragged_lens(rng, c.S, n)
    plen, steps, perm, slens = lens.astype(np.int64), np.full(n, c.S, np.int64), None, None
    if c.skip:
        assert T and cpj
        if c.skip == 'sorted':
            perm, slens, _ = ops_ref.row_order(lens, 0, T, cpj, n, c.B, c.S)
        else:
            perm = rng.permutation(c.B)
            slens = np.array([min(max(int(lens[b]), 1), c.S) if b < n else 1 for b in perm], np.int64)
        by_slot = team_steps(slens, T, cpj, c.S)
        for slot, b in enumerate(perm):
            if b < n:
                plen[b], steps[b] = slens[slot], by_slot[slot]
    rowmap = np.arange(c.S * n, dtype=np.int64).reshape(c.S, n)
    nrows, map_dev = c.S * n, None
    if c.cmp:
        rowmap, _, nrows = ops_ref.row_map(lens, 0, c.S, n)
        map_dev = rowmap
    return Rows(lens, plen, steps, rowmap, nrows, perm, slens, map_dev)


NAN16 = np.uint16(0x7FC1)         # a bf16 NaN: what a 16-bit INPUT holds wherever no launch may read


def read_mask(c, rows, reverse):
    """(S, rows): the positions whose saved state a backward launch reads -- position pos_map(p) of every step p the row's team runs, where it has a row"""
    pos = pos_table(c.S, rows.plen, reverse)
    read = np.zeros((c.S, c.rows), bool)
    for p in range(c.S):
        sel = np.flatnonzero(rows.steps > p)
        read[pos[p, sel], sel] = True
    return read & (rows.rowmap >= 0)


def nan32(shape):
    return np.full(shape, np.nan, np.float32)


def sentinel(shape):
    return np.full(shape, SENT, np.int32).view(np.float32)


def sentinel16(shape):
    return np.full(shape, SENT16, np.uint16)


def make_inputs(c, rows):
    """-> dict of the physical input buffers (fp32, NaN in everything no launch may read) and, under 'log', the logical per-job arrays"""
    rng = np.random.default_rng(c.seed)
    S, B, D, n = c.S, c.rows, c.D, rows.nrows
    real = rows.rowmap >= 0
    b = {'log': []}
    lim = (6.0 / (2 * D)) ** 0.5
    if c.fwd and c.table:
        ids = rng.integers(0, TABLE_ROWS, (S, B))
        ids.ravel()[:TABLE_ROWS] = np.arange(TABLE_ROWS)             # every row of the table is somebody's
        present = np.sort(rng.choice(TABLE_V, TABLE_ROWS, replace=False))
        b['gi'] = nan32((TABLE_ROWS + GUARD_ROWS, c.ldg))
        b['tok'], b['gi_rows'] = present[ids].ravel().astype(np.int32), ids.ravel().astype(np.int32)      # (gi_rows: what rank_rows makes of tok)
        b['rank'] = ops_ref.id_groups(b['tok'], TABLE_V)[0].astype(np.int32)
    elif c.fwd:
        b['gi'] = nan32((n + GUARD_ROWS, c.ldg))
    else:
        b['dh_out'] = nan32((n + GUARD_ROWS, c.ldh))
    for k in range(c.njobs):
        L = {'R': rng.uniform(-lim, lim, (3 * D, D)).astype(np.float32)}
        b['R%d' % k] = np.concatenate([L['R'], nan32((GUARD_ROWS, D))])
        if c.fwd:
            L['bR'] = (0.1 * rng.standard_normal(3 * D)).astype(np.float32)
            if c.table:
                L['table'] = rng.standard_normal((TABLE_ROWS, 3 * D)).astype(np.float32)
                L['gi'] = L['table'][ids]
            else:
                L['gi'] = rng.standard_normal((S, B, 3 * D)).astype(np.float32)
            L['h0'] = rng.uniform(-1, 1, (B, D)).astype(np.float32) if c.h0 else None
            b['bR%d' % k] = np.concatenate([L['bR'], nan32(GUARD_ROWS)])
            if c.table:
                b['gi'][:TABLE_ROWS, k * 3 * D:(k + 1) * 3 * D] = L['table']
            else:
                b['gi'][rows.rowmap[real], k * 3 * D:(k + 1) * 3 * D] = L['gi'][real]
            if c.h0:
                b['h0%d' % k] = np.concatenate([L['h0'], nan32((GUARD_ROWS, D))])
        else:
            sv = np.empty((S, B, D, 4), np.float32)
            sv[..., 0:2] = rng.uniform(0.02, 0.98, (S, B, D, 2))
            sv[..., 2] = rng.uniform(-0.98, 0.98, (S, B, D))
            sv[..., 3] = 0.5 * rng.standard_normal((S, B, D))
            L['sv'] = sv
            L['hp'] = rng.uniform(-1, 1, (S, B, D)).astype(np.float32)
            if c.in16:
                L['sv'], L['hp'] = bf16_rne(L['sv'])[1], bf16_rne(L['hp'])[1]
                # the 16-bit arrays: NAN16 wherever no step of the launch reads -- guard rows, and in the padded layout the positions behind a row's steps
                read = read_mask(c, rows, k == 1)
                for nm, w in (('sv', 4 * D), ('hp', D)):
                    b['%s16_%d' % (nm, k)] = np.full((n + GUARD_ROWS, w), NAN16, np.uint16)
                    b['%s16_%d' % (nm, k)][rows.rowmap[read]] = bf16_rne(L[nm].reshape(S, B, w)[read])[0]
                sv = L['sv']
            L['dh_out'] = rng.standard_normal((S, B, D)).astype(np.float32)
            L['dh_out'][np.arange(S)[:, None] >= rows.lens[None, :]] = 0          # zero at padding, as the model guarantees
            L['dbW0'] = rng.standard_normal(3 * D).astype(np.float32)
            L['dbR0'] = rng.standard_normal(3 * D).astype(np.float32)
            b['sv%d' % k] = nan32((n + GUARD_ROWS, 4 * D))
            b['sv%d' % k][rows.rowmap[real]] = sv.reshape(S, B, 4 * D)[real]
            b['hp%d' % k] = nan32((n + GUARD_ROWS, D))
            b['hp%d' % k][rows.rowmap[real]] = L['hp'][real]
            b['dh_out'][rows.rowmap[real], k * D:(k + 1) * D] = L['dh_out'][real]
        b['log'].append(L)
    return b


def make_outputs(c, rows, inp):
    """-> the output buffers as the launch gets them: the sentinel everywhere but the bias sums' logical part, which is pre-filled"""
    D, n = c.D, rows.nrows
    o = {}
    if c.fwd:
        o['hs'] = sentinel((n + GUARD_ROWS, c.ldh)).copy()
        if c.out16:
            o['hs16'] = sentinel16((n + GUARD_ROWS, c.ldh))
        for k in range(c.njobs):
            if c.save and c.out16:          # (sv itself holds bf16 under GruArgs::sv16; hp is not given)
                o['sv%d' % k], o['hp16_%d' % k] = sentinel16((n + GUARD_ROWS, 4 * D)), sentinel16((n + GUARD_ROWS, D))
            elif c.save:
                o['sv%d' % k] = sentinel((n + GUARD_ROWS, 4 * D)).copy()
                o['hp%d' % k] = sentinel((n + GUARD_ROWS, D)).copy()
    else:
        o['dgi'] = sentinel(((c.S * c.rows if c.by_pos else n) + GUARD_ROWS, c.ldg)).copy()
        o['dgh'] = sentinel((n + GUARD_ROWS, c.ldg)).copy()
        if c.out16:
            o['dgi16'] = sentinel16((n + GUARD_ROWS, c.ldg))
        if c.out16 or c.dgh16_only:
            o['dgh16'] = sentinel16((n + GUARD_ROWS, c.ldg))
        for k in range(c.njobs):
            for nm in ('dbW', 'dbR'):
                o['%s%d' % (nm, k)] = sentinel(3 * D + GUARD_ROWS).copy()
                o['%s%d' % (nm, k)][:3 * D] = inp['log'][k][nm + '0']
            if c.h0:
                o['dh0%d' % k] = sentinel((c.rows + GUARD_ROWS, D)).copy()
    return o


def written_masks(c, rows):
    """per output buffer the elements a correct launch writes: every position of every row in the padded layout (a row order's skipped
    positions are zero-filled), the mapped rows in the compact layout; never a padding column, a guard row or another job's columns"""
    D, n = c.D, rows.nrows
    live = np.zeros(n + GUARD_ROWS, bool)
    live[rows.rowmap[rows.rowmap >= 0]] = True
    m = {}

    def cols(ld, w):
        x = np.zeros((n + GUARD_ROWS, ld), bool)
        x[live, :c.njobs * w] = True
        return x
    never = lambda ld: np.zeros((n + GUARD_ROWS, ld), bool)
    if c.fwd:
        m['hs'] = never(c.ldh) if c.out16 else cols(c.ldh, D)
        if c.out16:
            m['hs16'] = cols(c.ldh, D)
        for k in range(c.njobs):
            if c.save:
                ran = np.zeros(n + GUARD_ROWS, bool)          # (the saved gates of a skipped position are not written at all)
                sel = (rows.rowmap >= 0) & (np.arange(c.S)[:, None] < rows.steps[None, :])
                ran[rows.rowmap[sel]] = True
                m['sv%d' % k], m['hp16_%d' % k if c.out16 else 'hp%d' % k] = np.repeat(ran[:, None], 4 * D, 1), np.repeat(live[:, None], D, 1)
    else:
        m['dgi'], m['dgh'] = never(c.ldg) if c.out16 else cols(c.ldg, 3 * D), never(c.ldg) if (c.out16 or c.dgh16_only) else cols(c.ldg, 3 * D)
        if c.by_pos:            # every position of every row, in the padded order
            m['dgi'] = np.zeros((c.S * c.rows + GUARD_ROWS, c.ldg), bool)
            m['dgi'][:c.S * c.rows, :c.njobs * 3 * D] = True
        if c.out16:
            m['dgi16'] = cols(c.ldg, 3 * D)
        if c.out16 or c.dgh16_only:
            m['dgh16'] = cols(c.ldg, 3 * D)
        for k in range(c.njobs):
            for nm in ('dbW', 'dbR'):
                m['%s%d' % (nm, k)] = np.arange(3 * D + GUARD_ROWS) < 3 * D
            if c.h0:
                m['dh0%d' % k] = np.repeat((np.arange(c.rows + GUARD_ROWS) < c.rows)[:, None], D, 1)
    return m


# ------------------------------------------------------------------------------------------ float32 restatement of a whole launch
def run_forward(c, rows, inp, out, dtype=np.float32, defect=''):
    """the launch contract played out with step_fwd in `dtype`, written into `out` as a kernel would.  defect: one deliberate fault
    (tests/test_gru_ref.py "the comparison has teeth")"""
    S, B, D = c.S, c.rows, c.D
    for k in range(c.njobs):
        L, rev = inp['log'][k], k == 1
        pm = (lambda p, l, r: l - 1 - p if (r and p <= l) else p) if defect == 'pos_map' else pos_map
        pos = pos_table(S, rows.plen, rev, pm)
        h = L['h0'].copy() if L['h0'] is not None else np.zeros((B, D), np.float32)
        if c.skip and not c.cmp:
            for bi in range(B):
                for p in range(int(rows.steps[bi]), S):
                    out['hs'][rows.rowmap[p, bi], k * D:(k + 1) * D] = 0
                    if c.save:
                        out['hp%d' % k][rows.rowmap[p, bi]] = 0
        for p in range(S):
            a_rows = None
            if defect == 'neighbour' and p == 2:
                a_rows = np.arange(B)
                a_rows[1] = 0
            hn, r, u, n, ghn = step_fwd(L['gi'][pos[p], np.arange(B)], h, L['R'], L['bR'], c.bf16, dtype, swap_ru=defect == 'swap_ru', a_rows=a_rows)
            for bi in range(B):
                if p >= rows.steps[bi]:
                    continue
                row = rows.rowmap[pos[p, bi] % S, bi]
                if row < 0:
                    continue
                out['hs'][row, k * D:(k + 1) * D] = hn[bi]
                if c.save:
                    out['sv%d' % k][row] = np.stack([r[bi], u[bi], n[bi], ghn[bi]], -1).reshape(-1)
                    out['hp%d' % k][row] = h[bi]
            h = hn.astype(np.float32)
    if defect == 'padding':
        bi = int(np.argmin(rows.steps))
        assert rows.steps[bi] < S, 'the padding defect needs a case whose row order skips a position'
        out['hs'][rows.rowmap[S - 1, bi], 3] = 0.25
    if defect == 'ld':
        out['hs'][1, c.njobs * D] = 0.25
    return out


def run_backward(c, rows, inp, out, dtype=np.float32, defect=''):
    S, B, D = c.S, c.rows, c.D
    real = rows.rowmap >= 0
    for k in range(c.njobs):
        L, rev = inp['log'][k], k == 1
        pos = pos_table(S, rows.plen, rev)
        carry, dgh_next = np.zeros((B, D), dtype), None
        cols = slice(k * 3 * D, (k + 1) * 3 * D)
        sums = [np.zeros(3 * D, np.float64), np.zeros(3 * D, np.float64)]
        if c.skip and not c.cmp:
            for bi in range(B):
                for p in range(int(rows.steps[bi]), S):
                    out['dgi'][rows.rowmap[p, bi], cols] = 0
                    out['dgh'][rows.rowmap[p, bi], cols] = 0
        Lsv, Lhp = L['sv'], L['hp']
        if c.in16:
            # the saved state as a kernel gets it: out of the 16-bit buffers, widened.  Defects: 'sv16_index' -- the gates fetched at the fp32
            # element index (twice the halfword offset; beyond the buffer a buffer load gives zeros); 'hp16_next' -- h_prev of position p from p + 1
            flat = widen16(inp['sv16_%d' % k]).ravel()
            at = (np.arange(flat.size) * (2 if defect == 'sv16_index' else 1))
            sv_rows = np.where(at < flat.size, flat[np.minimum(at, flat.size - 1)], 0).astype(np.float32).reshape(-1, 4 * D)
            Lsv = logical(sv_rows, rows, 0, 4 * D).reshape(S, B, D, 4)
            Lhp = logical(inp['hp16_%d' % k], rows, 0, D)
            if defect == 'hp16_next':
                Lhp = Lhp[np.minimum(np.arange(S) + 1, S - 1)]
        for p in range(S - 1, -2, -1):
            act = rows.steps > max(p, 0)
            nxt = rows.steps > p + 1
            q = pos[max(p, 0)], np.arange(B)
            ok = real[q] & act
            sv, hp, do = (np.where(ok.reshape((B,) + (1,) * (x.ndim - 2)), x[q], 0) for x in (Lsv, Lhp, L['dh_out']))
            cin = np.where(nxt[:, None], carry, 0)
            if defect == 'carry':
                cin = cin * 0
            gnx = None if dgh_next is None else np.where(nxt[:, None], dgh_next, 0)
            if p < 0:
                if c.h0:
                    dH = cin + (0 if gnx is None else bf_prod(gnx, L['R'], c.bf16, dtype))
                    out['dh0%d' % k][:B] = np.where(rows.steps[:, None] > 0, dH, 0)
                break
            dgi, dgh, cout, _ = step_bwd(do, cin, gnx, L['R'], sv, hp, c.bf16, dtype)
            for bi in np.flatnonzero(ok):
                row = rows.rowmap[q[0][bi], bi]
                out['dgi'][row, cols], out['dgh'][row, cols] = dgi[bi], dgh[bi]
            sums[0] += np.where(act[:, None], dgi, 0).sum(0)
            sums[1] += np.where(act[:, None], dgh, 0).sum(0)
            carry = np.where(act[:, None], cout, carry).astype(dtype)
            dgh_next = np.where(act[:, None], dgh, 0 if dgh_next is None else dgh_next).astype(np.float32)
        for nm, s in zip(('dbW', 'dbR'), sums):
            out['%s%d' % (nm, k)][:3 * D] = (0 if defect == 'bias' else L[nm + '0']) + s.astype(np.float32)
    return out


def bf_prod(a, R, bf16, dtype):
    """a R in dtype; bf16: both operands rounded to bf16 first"""
    if bf16:
        a, R = bf16_rne(np.asarray(a, np.float32))[1], bf16_rne(R)[1]
    return np.asarray(a, dtype) @ np.asarray(R, dtype)


# ------------------------------------------------------------------------------------------ the comparison
def untouched(name, got, before, mask):
    """(row, column) of every element outside `mask` whose bits changed"""
    bits = np.int32 if got.dtype == np.float32 else got.dtype
    g, w = got.view(bits), before.view(bits)
    bad = np.argwhere((g != w) & ~mask)
    assert bad.size == 0, ('%s: written outside what the launch may write, first at' % name, bad[:5].tolist())


class Worst:
    """per output array: the largest error beyond its allowance, in units of the yardstick, and the yardstick's ingredients"""
    def __init__(self):
        self.err, self.yard, self.ref = {}, {}, {}

    def see(self, name, got, ref64, ref32, sel, scale=1.0, extra=False):
        """got / ref64 / ref32 (B, ...) of one step, sel (B) the rows that count; scale: the steps the error may have grown over (B);
        extra: the output is 16-bit: half a bf16 ulp of the reference comes on top"""
        if not sel.any():
            return
        g, r, f = np.asarray(got, np.float64)[sel], np.asarray(ref64, np.float64)[sel], np.asarray(ref32, np.float64)[sel]
        assert np.isfinite(g).all(), '%s: not finite (or never written) where the launch computes a value' % name
        sc = np.asarray(scale, np.float64)
        if sc.ndim:
            sc = sc[sel].reshape((-1,) + (1,) * (g.ndim - 1))
        e = np.maximum(np.abs(g - r) - (half_ulp_bf16(r) if extra else 0.0), 0) / sc
        self.err[name] = max(self.err.get(name, 0.0), float(e.max()))
        self.yard[name] = max(self.yard.get(name, 0.0), float(np.abs(f - r).max()))
        self.ref[name] = max(self.ref.get(name, 0.0), float(np.abs(r).max()))

    def ratios(self):
        return {k: self.err[k] / max(self.yard[k], 4 * U * self.ref[k], 1e-300) for k in self.err}

    def check(self, cid):
        r = self.ratios()
        print('RATIO %s %s' % (cid, ' '.join('%s=%.3f' % (k, v) for k, v in sorted(r.items()))))
        bad = {k: v for k, v in r.items() if not v <= MARGIN}
        assert not bad, (cid, 'error / yardstick beyond the margin of %g' % MARGIN, bad)
        return r


def logical(buf, rows, lo, hi, padded=False):
    """(S, rows, hi - lo) view of a physical per-position buffer through the row map (padded: in the order pos * B + row whatever the
    map): NaN where the map has no row; a 16-bit buffer is widened"""
    S, B = rows.rowmap.shape
    rowmap = np.arange(S * B).reshape(S, B) if padded else rows.rowmap
    out = np.full((S, B, hi - lo), np.nan, buf.dtype if buf.dtype != np.uint16 else np.float32)
    real = rowmap >= 0
    src = buf[rowmap[real], lo:hi]
    out[real] = widen16(src) if buf.dtype == np.uint16 else src
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


def check_forward(c, rows, inp, before, got, companion=None):
    """before / got: the output buffers as the launch got them and as it left them -> {array: error / yardstick}.  16-bit outputs
    (c.out16): companion = the fp32 outputs of the same launch without the 16-bit arrays (checked on its own): the fp32 state is not an
    output of such a launch, so the step check takes the companion's h_prev -- after holding the 16-bit arrays, bit for bit, to the
    round-to-nearest-even bf16 of the companion's"""
    S, B, D = c.S, c.rows, c.D
    for nm, m in written_masks(c, rows).items():
        untouched(nm, got[nm], before[nm], m)
    real = rows.rowmap >= 0
    w = Worst()
    ar = np.arange(B)
    for k in range(c.njobs):
        L, rev = inp['log'][k], k == 1
        pos = pos_table(S, rows.plen, rev)
        hs = logical(got['hs16' if c.out16 else 'hs'], rows, k * D, (k + 1) * D)
        sv = logical(got['sv%d' % k], rows, 0, 4 * D).reshape(S, B, D, 4) if c.save else None
        hp = logical(got[('hp16_%d' if c.out16 else 'hp%d') % k], rows, 0, D) if c.save else None
        extra = c.out16
        if c.out16:
            assert c.save and companion is not None
            chp = logical(companion['hp%d' % k], rows, 0, D)
            ran = real & (np.arange(S)[:, None] < rows.steps[None, :])          # (positions: a skipped one is beyond its row's plen too)
            for nm, a16, a32 in (('hs16', hs, logical(companion['hs'], rows, k * D, (k + 1) * D)), ('hp16', hp, chp),
                                 ('sv16', sv.reshape(S, B, 4 * D), logical(companion['sv%d' % k], rows, 0, 4 * D))):
                assert same_bits(a16[ran], bf16_rne(a32[ran])[1]), (c.id, 'job %d: %s is not the bf16 rounding of the fp32 output of the same launch' % (k, nm))
        for p in range(S):
            q = pos[p], ar
            sel = (rows.steps > p) & real[q]
            first = L['h0'] if L['h0'] is not None else np.zeros((B, D), np.float32)
            if c.out16:
                first = bf16_rne(first)[1]
            chain = first if p == 0 else hs[pos[p - 1], ar]
            if p > 0:
                assert real[pos[p - 1], ar][sel].all(), 'a real step behind a step without a row'
            if c.save:
                # (a) the chain identity, bit for bit
                bad = [int(bi) for bi in np.flatnonzero(sel) if not same_bits(hp[q][bi], chain[bi])]
                assert not bad, (c.id, 'job %d step %d: the saved h_prev is not the h of the step before (h0 at step 0), rows' % (k, p), bad[:8])
            h_prev = np.where(sel[:, None], chp[q] if c.out16 else (hp[q] if c.save else chain), 0).astype(np.float32)
            # (b) one step from the launch's own h_prev
            ref = step_fwd(L['gi'][q], h_prev, L['R'], L['bR'], c.bf16)
            r32 = step_fwd(L['gi'][q], h_prev, L['R'], L['bR'], c.bf16, np.float32)
            w.see('h', hs[q], ref[0], r32[0], sel, extra=extra)
            if c.save:
                for i, nm in enumerate(('r', 'u', 'n', 'hn')):
                    w.see(nm, sv[q][..., i], ref[1 + i], r32[1 + i], sel, extra=extra)
            # positions a row order skips: exact zeros in the padded layout
            if c.skip and not c.cmp:
                z = rows.steps <= p
                for nm, arr in (('hs', hs[p]),) + ((('hp', hp[p]),) if c.save else ()):
                    assert same_bits(arr[z], np.zeros_like(arr[z])), (c.id, 'job %d: %s at skipped position %d is not an exact zero' % (k, nm, p))
    return w.check(c.id)


def check_backward(c, rows, inp, before, got):
    S, B, D = c.S, c.rows, c.D
    for nm, m in written_masks(c, rows).items():
        untouched(nm, got[nm], before[nm], m)
    real = rows.rowmap >= 0
    w = Worst()
    ar = np.arange(B)
    for k in range(c.njobs):
        L, rev = inp['log'][k], k == 1
        pos = pos_table(S, rows.plen, rev)
        cols = (k * 3 * D, (k + 1) * 3 * D)
        dgi = logical(got['dgi16'], rows, *cols) if c.out16 else logical(got['dgi'], rows, *cols, padded=c.by_pos)
        dgh = logical(got['dgh16' if (c.out16 or c.dgh16_only) else 'dgh'], rows, *cols)
        xi, xh = c.out16, c.out16 or c.dgh16_only
        if c.by_pos:
            assert same_bits(dgi[~real], np.zeros_like(dgi[~real])), (c.id, 'job %d: dgi by position is not an exact zero at a padding position' % k)
        carry = np.zeros((B, D))
        ref_next = None
        for p in range(S - 1, -2, -1):
            act, nxt = rows.steps > max(p, 0), rows.steps > p + 1
            q = pos[max(p, 0)], ar
            ok = real[q] & act
            sv, hp, do = (np.where(ok.reshape((B,) + (1,) * (x.ndim - 2)), x[q], 0) for x in (L['sv'], L['hp'], L['dh_out']))
            cin = np.where(nxt[:, None], carry, 0)
            gnx = None
            if p + 1 < S:
                # fp32 forms: the recurrence's own dgh; bf16 forms: the launch's, which step_bwd rounds as the kernel does (a position
                # without a row took part in the exchange with the value the formulas give from zero inputs: zero)
                src = np.nan_to_num(dgh[pos[p + 1], ar], nan=0.0) if c.bf16 else ref_next
                gnx = np.where(nxt[:, None], src, 0)
            behind = np.maximum(rows.steps - max(p, 0), 1)
            if p < 0:
                if c.h0:
                    ref = cin + bf_prod(gnx, L['R'], c.bf16, np.float64)
                    r32 = cin.astype(np.float32) + bf_prod(gnx, L['R'], c.bf16, np.float32)
                    w.see('dh0', got['dh0%d' % k][:B], ref, r32, rows.steps > 0, scale=behind + 1)
                break
            ref = step_bwd(do, cin, gnx, L['R'], sv, hp, c.bf16)
            r32 = step_bwd(do, cin, gnx, L['R'], sv, hp, c.bf16, np.float32)
            w.see('dgi', dgi[q], ref[0], r32[0], ok, scale=behind, extra=xi)
            w.see('dgh', dgh[q], ref[1], r32[1], ok, scale=behind, extra=xh)
            carry = np.where(act[:, None], ref[2], carry)
            ref_next = np.where(act[:, None], ref[1], 0 if ref_next is None else ref_next)
            if c.skip and not c.cmp:
                z = rows.steps <= p
                for nm, arr in (('dgi', dgi[p]), ('dgh', dgh[p])):
                    assert same_bits(arr[z], np.zeros_like(arr[z])), (c.id, 'job %d: %s at skipped position %d is not an exact zero' % (k, nm, p))
        # bias sums: the pre-filled value plus the float64 column sums of the launch's OWN gate gradients, in any fp32 order
        for nm, arr, x16 in (('dbW', dgi, xi), ('dbR', dgh, xh)):
            x = arr[real].astype(np.float64)
            s, a = L[nm + '0'] + x.sum(0), np.abs(L[nm + '0']) + np.abs(x).sum(0)
            bound = ops_ref.sum_bound(s, x.shape[0] + 1, a) + (2.0 ** -8 * a if x16 else 0.0)      # (the kernel sums the fp32 values, the test their bf16 roundings: half an ulp each)
            e = np.abs(got['%s%d' % (nm, k)][:3 * D].astype(np.float64) - s)
            assert (e <= bound).all(), (c.id, 'job %d: %s is not its value before the launch plus the column sums' % (k, nm), float((e / bound).max()))
    return w.check(c.id)


# ------------------------------------------------------------------------------------------ the cases of tests/test_gpu_gru.py
PERSISTENT, STEPWISE, ITEM = ('persistent', 0, 0, 0), ('stepwise', 0, 0, 0), ('item', 0, 0, 0)
# team geometries: (njobs, slots) -> T, C, pipe (gru.hip team_rows; tests/test_gru_ref.py holds every case's reach against the plan hook)
TEAM = {(1, 32): (2, 1, 0), (1, 64): (2, 2, 0), (2, 32): (2, 2, 0), (2, 64): (4, 2, 0), (2, 128): (2, 8, 0), (2, 256): (4, 8, 0),
        (2, 384): (2, 8, 1), (2, 512): (4, 8, 1), (1, 1024): (4, 8, 1), (1, 128): (2, 4, 0)}
SMALL_TEAM = ((1, 32), (2, 64), (2, 384), (2, 512))
LARGE_TEAM = ((1, 64), (2, 32), (2, 128), (2, 256), (1, 1024))


def _reg(name, fwd, njobs, B, D, S=6, **kw):
    kw.setdefault('reach', PERSISTENT if kw.get('persistent', 1) and (not fwd or S >= 2) else STEPWISE)
    return Case(name, fwd, njobs, S, B, D, h0=njobs == 1, seed=B + D + njobs, **kw)


def register_cases():
    o = []
    for fwd in (True, False):
        for njobs in (1, 2):                       # 1: h0 / dh0 (a decoder layer); 2: both directions with lens (an encoder layer)
            for D in (16, 32, 64, 512):            # 16, 32: scalar operand path; 64, 512: vector path
                o.append(_reg('reg', fwd, njobs, 5, D))                          # rows clamped to B - 1
                o.append(_reg('reg', fwd, njobs, 16, D, S=5))
                o.append(_reg('reg-2sc', fwd, njobs, 40, D, S=7, G=1, rpg=48))       # two super-chunks, the second chunk of the last absent
                o.append(_reg('reg-3g', fwd, njobs, 40, D, G=3, rpg=16))
                o.append(_reg('step', fwd, njobs, 5, D, persistent=0))
                o.append(_reg('step-2sc', fwd, njobs, 40, D, S=5, G=1, rpg=48, persistent=0))
            o.append(_reg('reg', fwd, njobs, 16, 128 if njobs == 1 else 256))
        o.append(_reg('reg-bf16', fwd, 2, 16, 64, bf16=1))                       # bf16 operands in the register forms (opnd)
        o.append(_reg('reg-ldh', fwd, 2, 16, 64, ldh_pad=8, ldg_pad=12))         # the 2-D sentinel fill: padding columns survive
        o.append(_reg('reg-S1', fwd, 1, 16, 64, S=1))                           # forward: stepwise; backward: persistent with the dh0 tail
        o.append(_reg('reg-S1', fwd, 2, 5, 32, S=1))
    return o


def item_cases():
    return [Case('item', True, 1, 6, B, 512, G=B // 32, rpg=32, item=1, h0=h0, reach=ITEM, seed=B) for B, h0 in ((32, True), (64, False))]


def _team(name, fwd, njobs, B, S=6, **kw):
    T, C, pipe = TEAM[(njobs, B)]
    form = 'team_rs' if kw.get('bwd_rs') and not fwd else 'team'
    return Case(name, fwd, njobs, S, B, 512, item=2, xbuf=True, h0=njobs == 1, reach=(form, T, C, pipe), seed=B + njobs, **kw)


def team_cases():
    o = []
    for fwd in (True, False):
        for njobs, B in SMALL_TEAM:
            S = 5 if B >= 384 else 6
            o.append(_team('team', fwd, njobs, B, S))
            o.append(_team('team-skip', fwd, njobs, B, S, skip='sorted'))
            o.append(_team('team-cmp', fwd, njobs, B, S, skip='sorted', cmp=True))
            o.append(_team('team-bf16', fwd, njobs, B, S, bf16=1))
            o.append(_team('team-bf16-cmp', fwd, njobs, B, S, bf16=1, skip='sorted', cmp=True))
            if fwd:
                o.append(_team('team-table', fwd, njobs, B, S, table=True))
            else:
                o.append(_team('team-bypos', fwd, njobs, B, S, skip='sorted', cmp=True, by_pos=True))
                o.append(_team('team-rs', fwd, njobs, B, S, bwd_rs=1))
                o.append(_team('team-rs-cmp', fwd, njobs, B, S, bwd_rs=1, skip='sorted', cmp=True))
        o.append(_team('team-table-cmp', fwd, 2, 64, skip='sorted', cmp=True, table=True) if fwd else
                 _team('team-bypos-phantom', fwd, 1, 32, skip='sorted', cmp=True, by_pos=True, Breal=20))
        o.append(_team('team-anyperm', fwd, 2, 64, skip='unsorted'))
        o.append(_team('team-phantom', fwd, 1, 32, skip='sorted', cmp=True, Breal=20))
        o.append(_team('team-phantom', fwd, 1, 128, skip='sorted', cmp=True, Breal=100))
        o.append(_team('team-phantom', fwd, 2, 128, skip='sorted', cmp=True, Breal=100))
        for njobs, B in LARGE_TEAM:
            o.append(_team('team', fwd, njobs, B, 5))
            o.append(_team('team-cmp', fwd, njobs, B, 5, skip='sorted', cmp=True))
            o.append(_team('team-bf16', fwd, njobs, B, 5, bf16=1))
    return o


def team16_cases():
    """bf16 team forms with 16-bit outputs; each runs beside its fp32-output companion (the same case with out16 / dgh16_only off)"""
    o = []
    for fwd in (True, False):
        for njobs, B in SMALL_TEAM:
            S = 5 if B >= 384 else 6
            o.append(_team('team-16', fwd, njobs, B, S, bf16=1, out16=True))
            if not fwd:
                o.append(_team('team-dgh16', fwd, njobs, B, S, bf16=1, dgh16_only=True))
        o.append(_team('team-16-cmp', fwd, 2, 64, bf16=1, out16=True, skip='sorted', cmp=True))
        o.append(_team('team-16-skip', fwd, 2, 512, 5, bf16=1, out16=True, skip='sorted'))
    return o


def team_in16_cases():
    """backward launches of the bf16 team forms READING their saved gates / h_prev as bf16 (the default bf16 configuration of a step: bf16_sv, bf16_act):
    T = 2 / 4, with and without PIPE, one and two jobs; then the layouts and outputs that change the load's row index or what the step writes; then
    each 16-bit input without the other (a table-fed layer keeps h_prev fp32; bf16_sv = 0 keeps the gates fp32)"""
    o = []
    for njobs, B in SMALL_TEAM:
        o.append(_team('team-in16', False, njobs, B, 5 if B >= 384 else 6, bf16=1, in16='sv+hp'))
    o.append(_team('team-in16-skip', False, 2, 64, bf16=1, in16='sv+hp', skip='sorted'))
    o.append(_team('team-in16-cmp', False, 2, 64, bf16=1, in16='sv+hp', skip='sorted', cmp=True))
    o.append(_team('team-in16-phantom', False, 1, 32, bf16=1, in16='sv+hp', skip='sorted', cmp=True, Breal=20))
    o.append(_team('team-in16-dgh16', False, 2, 64, bf16=1, in16='sv+hp', dgh16_only=True))
    o.append(_team('team-in16-16', False, 2, 512, 5, bf16=1, in16='sv+hp', out16=True))
    o.append(_team('team-in16-16-cmp', False, 2, 64, bf16=1, in16='sv+hp', out16=True, skip='sorted', cmp=True))
    for njobs, B in ((1, 32), (2, 512)):
        o.append(_team('team-in16-sv', False, njobs, B, 5, bf16=1, in16='sv'))
        o.append(_team('team-in16-hp', False, njobs, B, 5, bf16=1, in16='hp'))
    return o


# every form gru_plan can give a backward launch that asks for bf16 operands (GruArgs::bf16) or is handed 16-bit inputs, and what check_operands
# (gru.hip) does with sv16 / hp16 there: only the bf16 team kernels read them; everything else refuses the launch -- none ignores them
IN16_TABLE = [
    (_team('in16', False, 2, 64, bf16=1), 'reached'),
    (_team('in16-pipe', False, 2, 512, 5, bf16=1), 'reached'),
    (_team('in16-fp32', False, 2, 64), 'refused'),                           # the fp32 team kernels
    (_team('in16-rs', False, 2, 64, bwd_rs=1), 'refused'),                   # the reduce-scatter kernel: fp32 only (bf16 = 1 plans the team form instead)
    (_reg('in16-reg', False, 2, 16, 64, bf16=1), 'refused'),                 # register forms take bf16 OPERANDS of the recurrent product, no 16-bit arrays
    (_reg('in16-step', False, 2, 16, 64, bf16=1, persistent=0), 'refused'),
]


def all_cases():
    return register_cases() + item_cases() + team_cases() + team16_cases() + team_in16_cases()
