"""Every GRU kernel form on its own: ONE gru_forward / gru_backward call per case through avae_debug_gru (plan, operand check, residency check and
exchange preparation as in the product) on caller buffers, against tests/gru_ref.py.  Every buffer is larger than its logical extent: NaN in
everything of an input no launch may read, a NaN-payload sentinel in everything of an output no launch may write (padding columns of ldg / ldh,
guard rows, the exchange scratch beyond xbuf_floats), compared through an int32 view afterwards.

Forward launches are checked by induction -- the saved h_prev of a step is bit for bit the h of the step before, and every step agrees with the
float64 cell applied to the launch's own h_prev --, backward launches against the float64 recurrence from drawn sv / hp / dh_out; the tolerance is
MARGIN = 8 yardsticks, a yardstick being the error of a float32 numpy restatement of the same single step (gru_ref.py).

Which kernel a case reaches: Case.reach = (form, T, C, pipe) is what gru_plan -- the function the launchers themselves call -- answers for the
case; tests/test_gru_ref.py holds the whole table against avae_debug_gru_plan without a GPU, and every launch here compares the plan it ran.

Largest error / yardstick seen on MI355X per kernel form (the RATIO lines these tests print; the margin is 8), forward / backward:
    register forms, persistent (gru_fwd_kernel / gru_bwd_kernel, D = 16 .. 512)     0.98 (h) / 0.38 (dgh)
    register forms, one launch per step                                           0.93 (n) / 0.24 (dgh)
    item-pipelined forward (gru_fwd_item_kernel)                                  0.99 (n)
    team T = 2, fp32 / bf16 operands / bf16 with 16-bit outputs                   0.65, 1.04, 1.03 (h, n) / 0.34, 0.30, 0.21 (dgh, dgi)
    team T = 4, likewise                                                          0.82, 1.16, 0.96 (h) / 0.25, 0.23, 0.21
    team T = 2 PIPE, likewise                                                     0.58, 1.02, 1.02 (u, n) / 0.32, 0.32, 0.23 (dgh)
    team T = 4 PIPE, likewise                                                     0.77, 0.99, 0.99 (h) / 0.33, 0.33, 0.33 (dgh)
    reduce-scatter backward (gru_rs.hip), T = 2 / 4 / 2 PIPE / 4 PIPE             0.22 / 0.27 / 0.32 / 0.33 (dgh)
    one-step kernels (gru_first_step_fwd / bwd)                                   0.89 (n) / 0.42 (dgi)
(the compact layout, phantom rows, a table-fed gi, dgi by position, spec, stagger and the slow path change no figure beyond the second digit.)
Every 16-bit output was, bit for bit, the round-to-nearest-even bf16 of the fp32 output of the same launch.
    team backward READING sv16 / hp16 (Case.in16), T = 2 / 4 / 2 PIPE / 4 PIPE               0.20 / 0.15 / 0.20 / 0.19 (dgh, dgi)
Every such launch gave, bit for bit, the dgi / dgh / dh0 (dgi16 / dgh16) of the launch reading the same bf16 values as fp32 arrays; the fp32 team,
reduce-scatter and register forms refuse the 16-bit inputs (gru_ref.IN16_TABLE) and leave every buffer as it was.

Not reached by these hooks and left to the whole-step tests: njobs = 3, partial persistent launches (p_begin > 0), the ablation / stamp
instantiations of the diagnostic build, and the GRU cell inside decode.hip.

Safety: one handle for the module, one launch per hook call; the kernels' spins are bounded (2 s) and the hook reports a time-out as a non-zero
return.  The first unexpected non-zero return or failed synchronise sets a module latch, and every later case fails at once without launching."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import gru_ref as G
import ops_ref

pytestmark = pytest.mark.gpu

XGUARD = 1024                    # sentinel floats behind the exchange scratch
_LATCH = []


@pytest.fixture(scope='module')
def gpu():
    from argsim_amd import lib
    l = lib.load()
    cfg = lib.AvaeConfig(32, 16, 8, 1, 1e-4, 1e-3, 2, 1, 0, 0, 1.0, 0.0, 0)
    h = C.c_void_p()
    assert l.avae_create(C.byref(cfg), 0, C.byref(h)) == 0
    yield l, h
    l.avae_destroy(h)


def guard():
    if _LATCH:
        pytest.fail('not run after an earlier GPU failure: %s' % _LATCH[0])


def trip(what):
    _LATCH.append(what)
    pytest.fail(what)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sync(what):
    import torch
    try:
        torch.cuda.synchronize()
    except Exception as e:          # noqa: BLE001 -- whatever the runtime raises: nothing more is launched
        trip('%s: synchronise failed: %s' % (what, e))


def plan_of(l, c):
    rs = (C.c_int64 * 10)()
    assert l.avae_debug_gru_plan((C.c_int64 * 15)(*c.shape_ints()), int(c.fwd), c.persistent, rs) == 0
    out = (C.c_int64 * 10)()
    assert l.avae_debug_gru_plan((C.c_int64 * 15)(*c.shape_ints(int(rs[8]))), int(c.fwd), c.persistent, out) == 0
    return out


def debug_op(l, h, op, ptrs, ints):
    P = (C.c_void_p * len(ptrs))(*[None if t is None else t.data_ptr() for t in ptrs])
    rc = l.avae_debug_op(h, op.encode(), P, (C.c_int64 * len(ints))(*ints), (C.c_float * 1)(0.0))
    if rc != 0:
        trip('%s: %s' % (op, (l.avae_last_error(h) or b'').decode()))
    sync(op)


def device_rows(gpu, c, rows, inp, T, cpj):
    """perm / slens / the row map / a table-fed layer's gi_rows as the product makes them (row_order, row_map, rank_rows on the device), held
    against ops_ref through gru_ref.make_rows / make_inputs"""
    import torch
    l, h = gpu
    d = {'lens': dev(rows.lens.astype(np.int32))}
    if c.fwd and c.table:
        n = c.S * c.rows
        d['gi_rows'], tok, rank = torch.full((n,), -7, dtype=torch.int32).cuda(), dev(inp['tok']), dev(inp['rank'])
        debug_op(l, h, 'rank_rows', [d['gi_rows'], tok, rank], [n, G.TABLE_V])
        want = ops_ref.rank_rows(inp['tok'], inp['rank'], G.TABLE_V)
        assert np.array_equal(d['gi_rows'].cpu().numpy(), want) and np.array_equal(want, inp['gi_rows']), (c.id, 'rank_rows')
    if c.skip == 'sorted':
        d['perm'], d['slens'] = torch.full((c.B,), -7, dtype=torch.int32).cuda(), torch.full((c.B,), -7, dtype=torch.int32).cuda()
        debug_op(l, h, 'row_order', [d['lens'], d['perm'], d['slens'], None], [1, c.rows, c.B, c.S, 0, 0, T, cpj])
        assert np.array_equal(d['perm'].cpu().numpy(), rows.perm) and np.array_equal(d['slens'].cpu().numpy(), rows.slens), (c.id, 'row_order')
    elif c.skip:
        d['perm'], d['slens'] = dev(rows.perm.astype(np.int32)), dev(rows.slens.astype(np.int32))
    if c.cmp:
        d['map'] = torch.full((c.S * c.rows,), -7, dtype=torch.int32).cuda()
        nact, count = torch.zeros(c.S, dtype=torch.int32).cuda(), torch.zeros(2, dtype=torch.int32).cuda()
        debug_op(l, h, 'row_map', [d['lens'], d['map'], nact, count], [0, c.S, c.rows])
        assert np.array_equal(d['map'].cpu().numpy().reshape(c.S, c.rows), rows.map_dev) and int(count[0]) == rows.nrows, (c.id, 'row_map')
    return d


class Launch:
    """a case's buffers on the device; run() is one hook call"""
    def __init__(self, gpu, c):
        guard()
        self.gpu, self.c = gpu, c
        l, _ = gpu
        p = plan_of(l, c)
        self.rs_floats = int(p[8])
        self.rows = G.make_rows(c, int(p[1]), int(p[3]))
        self.inp = G.make_inputs(c, self.rows)
        self.before = G.make_outputs(c, self.rows, self.inp)
        self.din = {k: dev(v) for k, v in self.inp.items() if k != 'log'}
        self.drows = device_rows(gpu, c, self.rows, self.inp, int(p[1]), int(p[3]))

    def run(self, expect_refusal=False, **edit):
        """-> the output buffers as the launch left them (the scratch buffers are checked here: nothing written behind their extent).  edit: Case
        fields changed for this launch alone; raw = {(kind, index): value} replaces an int / a job pointer / a shared pointer of the hook's
        arguments (the refusals)"""
        guard()
        l, h = self.gpu
        raw = edit.pop('raw', {})
        c = dataclasses.replace(self.c, **edit)
        D, fb = c.D, 4
        assert (c.out16, c.dgh16_only, c.table, c.by_pos) == (self.c.out16, self.c.dgh16_only, self.c.table, self.c.by_pos), 'these change the buffers'
        out = {k: dev(v) for k, v in self.before.items() if c.save or not (k.startswith('sv') or k.startswith('hp'))}
        scratch = {}
        if not c.fwd:
            scratch['carry'] = dev(G.sentinel((c.B + G.GUARD_ROWS, D)))
        nx = c.xbuf_floats(self.rs_floats)
        if c.xbuf:
            scratch['xbuf'] = dev(G.sentinel(nx + XGUARD))
        jobs = []
        for k in range(c.njobs):
            j = [None] * 19
            j[2] = self.din['R%d' % k].data_ptr()
            if c.fwd:
                j[0] = self.din['gi'].data_ptr() + k * 3 * D * fb
                j[3] = self.din['bR%d' % k].data_ptr()
                j[4] = self.din['h0%d' % k].data_ptr() if c.h0 else None
                j[5] = out['hs'].data_ptr() + k * D * fb
                j[1] = self.drows['gi_rows'].data_ptr() if c.table else None
                if c.out16:
                    j[8] = out['hs16'].data_ptr() + k * D * 2
                if c.save and c.out16:
                    j[6], j[9] = out['sv%d' % k].data_ptr(), out['hp16_%d' % k].data_ptr()
                elif c.save:
                    j[6], j[7] = out['sv%d' % k].data_ptr(), out['hp%d' % k].data_ptr()
            else:
                j[6], j[7] = self.din['sv%d' % k].data_ptr(), self.din['hp%d' % k].data_ptr()
                if 'sv' in c.in16:              # (GruArgs::sv16: the sv pointer itself holds bf16)
                    j[6] = self.din['sv16_%d' % k].data_ptr()
                if 'hp' in c.in16:              # the fp32 h_prev: not given (one job) or all NaN, to come back as it went (two jobs)
                    j[9] = self.din['hp16_%d' % k].data_ptr()
                    if c.njobs == 2:
                        scratch['hp-nan%d' % k] = dev(G.nan32((self.rows.nrows + G.GUARD_ROWS, D)))
                    j[7] = scratch['hp-nan%d' % k].data_ptr() if c.njobs == 2 else None
                j[10] = self.din['dh_out'].data_ptr() + k * D * fb
                j[11], j[12] = out['dgi'].data_ptr() + k * 3 * D * fb, out['dgh'].data_ptr() + k * 3 * D * fb
                j[13] = out['dgi16'].data_ptr() + k * 3 * D * 2 if c.out16 else None
                j[14] = out['dgh16'].data_ptr() + k * 3 * D * 2 if (c.out16 or c.dgh16_only) else None
                j[15] = out['dh0%d' % k].data_ptr() if c.h0 else None
                j[16] = scratch['carry'].data_ptr()
                j[17], j[18] = out['dbW%d' % k].data_ptr(), out['dbR%d' % k].data_ptr()
            jobs += j
        if not c.fwd and c.njobs == 2:          # (a carry scratch per job)
            scratch['carry1'] = dev(G.sentinel((c.B + G.GUARD_ROWS, D)))
            jobs[19 + 16] = scratch['carry1'].data_ptr()
        r = self.drows
        shared = [r['lens'].data_ptr(), r['slens'].data_ptr() if c.skip else None, r['perm'].data_ptr() if c.skip else None,
                  r['map'].data_ptr() if c.cmp else None, scratch['xbuf'].data_ptr() if c.xbuf else None]
        ints = c.shape_ints(self.rs_floats) + [c.stagger, c.force_slow, int((c.fwd and c.out16 and c.save) or (not c.fwd and 'sv' in c.in16)), c.spec]
        ints += [v for k in range(c.njobs) for v in (int(k == 1), int(c.by_pos))]
        for k, v in raw.items():
            kind, idx = k
            if kind == 'int':
                ints[idx] = v
            elif kind == 'job':
                jobs[idx] = v(self, out) if callable(v) else v
            else:
                shared[idx] = v(self, out) if callable(v) else v
        plan = (C.c_int64 * 10)()
        rc = l.avae_debug_gru(h, int(c.fwd), c.persistent, (C.c_int64 * len(ints))(*ints), (C.c_void_p * len(jobs))(*jobs),
                              (C.c_void_p * 5)(*shared), plan)
        err = (l.avae_last_error(h) or b'').decode()
        if expect_refusal:
            if rc == 0 or 'invalid argument' not in err:
                trip('%s: expected the operand check to refuse, got %d %r' % (c.id, rc, err))
        elif rc != 0:
            trip('%s: avae_debug_gru returned %d: %s' % (c.id, rc, err))
        sync(c.id)
        if not expect_refusal:
            assert (G.FORMS[plan[0]], int(plan[1]), int(plan[2]), int(plan[5])) == c.reach, (c.id, list(plan))
        got = {k: v.cpu().numpy() for k, v in out.items()}
        left = {k: v.cpu().numpy() for k, v in scratch.items()}
        for k, v in left.items():           # scratch: whatever the launch leaves inside, nothing behind it
            if k.startswith('hp-nan'):
                assert np.array_equal(v.view(np.int32), G.nan32(v.shape).view(np.int32)), (c.id, '%s: an input was written' % k)
                continue
            tail = v[nx:] if k == 'xbuf' else v[c.B:]
            assert (tail.view(np.int32) == G.SENT).all(), (c.id, '%s: written beyond its extent' % k)
        return got

    def check(self, got, c=None, **kw):
        c = c or self.c
        return (G.check_forward if c.fwd else G.check_backward)(c, self.rows, self.inp, self.before, got, **kw)


def bits_equal(a, b, names=None):
    """-> the arrays that differ in a bit.  The bias sums are left out: every kernel form adds its rows' partial sums with LDS float atomics, whose
    order is free, so two runs of ONE launch already differ in their last bits (they are held to their bound by check_backward)"""
    return [k for k in (names or a) if not k.startswith('db') and not np.array_equal(a[k].view(np.int32), b[k].view(np.int32))]


_ids = lambda c: c.id


# ------------------------------------------------------------------------------------------ register forms
@pytest.mark.parametrize('c', G.register_cases(), ids=_ids)
def test_register_forms(gpu, c):
    L = Launch(gpu, c)
    L.check(L.run())


@pytest.mark.parametrize('fwd', [True, False], ids=['fwd', 'bwd'])
def test_stagger_and_slow_path_change_no_bit(gpu, fwd):
    """stagger (the second half of the grid delayed) and force_slow (write-through stores) are speed only.  D = 128, one group per job:
    blocks 8..15 are the staggered half"""
    c = G.Case('reg-speed', fwd, 2, 6, 16, 128, G=1, rpg=16, reach=G.PERSISTENT, seed=3)
    L = Launch(gpu, c)
    plain = L.run()
    L.check(plain)
    for edit in (dict(stagger=1), dict(force_slow=1)):
        assert not bits_equal(plain, L.run(**edit)), edit


@pytest.mark.parametrize('c', [G._reg('reg', True, 2, 40, 64, G=3, rpg=16), G._team('team', True, 2, 64), G._team('team-bf16', True, 1, 32, bf16=1),
                               G._team('team-pipe', True, 2, 384, 5)], ids=_ids)
def test_inference_launch_gives_the_same_h(gpu, c):
    """without sv / hp (no gradient wanted) hs is bit for bit the hs of the launch that saves them"""
    L = Launch(gpu, c)
    full = L.run()
    L.check(full)
    bare = L.run(save=False)
    assert not bits_equal(full, bare, ['hs'])
    L.check(bare, dataclasses.replace(c, save=False))


# ------------------------------------------------------------------------------------------ item form
@pytest.mark.parametrize('c', G.item_cases(), ids=_ids)
def test_item_form(gpu, c):
    L = Launch(gpu, c)
    got = L.run()
    L.check(got)
    reg = L.run(item=0, reach=G.PERSISTENT)
    assert not bits_equal(got, reg), 'the item-pipelined forward and the register form differ'


# ------------------------------------------------------------------------------------------ team forms
@pytest.mark.parametrize('c', G.team_cases(), ids=_ids)
def test_team_forms(gpu, c):
    L = Launch(gpu, c)
    L.check(L.run())


@pytest.mark.parametrize('c', G.team16_cases(), ids=_ids)
def test_team_forms_16bit_outputs(gpu, c):
    """hs16 / hp16 / sv16, dgi16 / dgh16 INSTEAD of the fp32 arrays (which stay untouched): the bf16, bit for bit, of what the same launch
    gives as fp32, and inside the fp32 tolerance plus half a bf16 ulp of the reference"""
    Lc = Launch(gpu, dataclasses.replace(c, out16=False, dgh16_only=False))
    comp = Lc.run()
    Lc.check(comp)
    L = Launch(gpu, c)
    got = L.run()
    if c.fwd:
        L.check(got, companion=comp)
    else:
        L.check(got)
        for nm in ('dgi', 'dgh') if c.out16 else ('dgh',):
            m = G.written_masks(c, L.rows)[nm + '16']
            assert np.array_equal(got[nm + '16'][m], G.bf16_rne(comp[nm][m])[0]), (c.id, '%s16 is not the bf16 rounding of the fp32 output' % nm)
        if c.dgh16_only:
            assert not bits_equal(got, comp, ['dgi'])


@pytest.mark.parametrize('c', G.team_in16_cases(), ids=_ids)
def test_team_backward_reads_16bit_saved_state(gpu, c):
    """sv16 / hp16 as INPUTS (gru_team.hip: the 8-byte gate load at the halfword index, the 2-byte h_prev load).  Against the float64 recurrence on the
    rounded values at the usual margin, and bit for bit the launch that gets the same values as fp32 arrays: widening bf16 is a shift, so everything
    behind the load is the same arithmetic (the bias sums keep their bound: their LDS atomic order is free)"""
    L = Launch(gpu, c)
    got = L.run()
    L.check(got)
    plain = L.run(in16='')
    L.check(plain, dataclasses.replace(c, in16=''))
    assert not bits_equal(got, plain), (c.id, 'the launch reading bf16 sv / hp and the one reading the same values as fp32 differ in', bits_equal(got, plain))


@pytest.mark.parametrize('in16', ['sv', 'hp'])
@pytest.mark.parametrize('c,what', G.IN16_TABLE, ids=lambda v: v.id if isinstance(v, G.Case) else v)
def test_which_backward_forms_take_16bit_saved_state(gpu, c, what, in16):
    """every form a backward plan can have (gru_ref.IN16_TABLE): the bf16 team kernels read the 16-bit arrays, every other form refuses the launch and
    leaves every buffer as it was -- none runs on and ignores them"""
    L = Launch(gpu, dataclasses.replace(c, in16='sv+hp'))
    if what == 'reached':
        L.check(L.run(in16=in16), dataclasses.replace(c, in16=in16))
    else:
        got = L.run(expect_refusal=True, in16=in16)
        assert not bits_equal(got, {k: L.before[k] for k in got}), (c.id, in16)
        assert not [k for k in got if k.startswith('db') and not np.array_equal(got[k].view(np.int32), L.before[k].view(np.int32))], (c.id, in16)


@pytest.mark.parametrize('fwd', [True, False], ids=['fwd', 'bwd'])
@pytest.mark.parametrize('njobs,B', G.SMALL_TEAM)
def test_spec_changes_no_bit(gpu, njobs, B, fwd):
    """GruArgs::spec (the operand loaded without a probe in front) is speed only"""
    c = G._team('team-spec', fwd, njobs, B, 5, skip='sorted', cmp=True)
    L = Launch(gpu, c)
    plain = L.run()
    spec = L.run(spec=1)
    L.check(spec)
    assert not bits_equal(plain, spec)


# ------------------------------------------------------------------------------------------ refusals
def _rowmap(L, out):
    import torch
    L.keep = torch.zeros(L.c.S * L.c.rows, dtype=torch.int32).cuda()
    return L.keep.data_ptr()


REFUSALS = {
    'sv16 without bf16': (G._team('team', True, 2, 64), {('int', 17): 1}),
    'rowmap on a register form': (G._reg('reg', True, 2, 16, 64), {('shared', 3): _rowmap}),
    'Bx > B without slens / perm / rowmap': (G._team('team', True, 1, 32), {('int', 2): 20, ('int', 6): 32}),
    'gi_rows on a register form': (G._reg('reg', True, 1, 16, 64), {('job', 1): _rowmap}),
    'hs16 in fp32 mode': (G._team('team', True, 2, 64), {('job', 8): lambda L, out: out['hs'].data_ptr()}),
}


@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_refusals(gpu, what):
    """check_operands answers hipErrorInvalidValue: nothing is launched and every buffer stays as it was"""
    c, raw = REFUSALS[what]
    L = Launch(gpu, c)
    got = L.run(expect_refusal=True, raw=raw)
    assert not bits_equal(got, {k: L.before[k] for k in got}), what


def test_hook_takes_whole_sequences_only(gpu):
    L = Launch(gpu, G._reg('reg', True, 1, 16, 64))
    l, h = gpu
    ints = L.c.shape_ints() + [0, 0, 0, 0, 0, 0]
    ints[9] = 1
    rc = l.avae_debug_gru(h, 1, 1, (C.c_int64 * len(ints))(*ints), (C.c_void_p * 19)(), (C.c_void_p * 5)(), (C.c_int64 * 10)())
    assert rc != 0 and b'whole-sequence' in l.avae_last_error(h)


# ------------------------------------------------------------------------------------------ one-step kernels
@pytest.mark.parametrize('with_sv', [True, False], ids=['sv', 'nosv'])
@pytest.mark.parametrize('D', [16, 512])
@pytest.mark.parametrize('B', [1, 20])
def test_first_step_kernels(gpu, B, D, with_sv):
    """gru_first_step_fwd / bwd: one step from a zero state into a 2 D wide array at a column offset; a row of length 0 gives h = 0 and zero
    gate gradients"""
    guard()
    l, h = gpu
    rng = np.random.default_rng(B * 7 + D)
    lens = rng.integers(0, 4, B).astype(np.int32)
    lens[0] = 0
    if B > 1:
        lens[1] = 3
    gi = np.concatenate([rng.standard_normal((B, 3 * D)).astype(np.float32), G.nan32((G.GUARD_ROWS, 3 * D))])
    bR = np.concatenate([(0.5 * rng.standard_normal(3 * D)).astype(np.float32), G.nan32(G.GUARD_ROWS)])
    live = (lens > 0)[:, None]
    zero = np.zeros((B, D), np.float32)
    ref = G.step_fwd(gi[:B], zero, np.zeros((3 * D, D), np.float32), bR[:3 * D], 0)
    r32 = G.step_fwd(gi[:B], zero, np.zeros((3 * D, D), np.float32), bR[:3 * D], 0, np.float32)
    hout, sv = dev(G.sentinel((B + G.GUARD_ROWS, 2 * D))), dev(G.sentinel((B + G.GUARD_ROWS, 4 * D)))
    dl = dev(lens)
    keep = [dev(gi), dev(bR)]
    P = (C.c_void_p * 5)(keep[0].data_ptr(), keep[1].data_ptr(), hout.data_ptr() + D * 4, sv.data_ptr() if with_sv else None, dl.data_ptr())
    rc = l.avae_debug_op(h, b'gru_first_step_fwd', P, (C.c_int64 * 3)(2 * D, B, D), (C.c_float * 1)(0.0))
    if rc != 0:
        trip('gru_first_step_fwd: %s' % l.avae_last_error(h).decode())
    sync('gru_first_step_fwd')
    hg, sg = hout.cpu().numpy(), sv.cpu().numpy()
    mask = np.zeros(hg.shape, bool)
    mask[:B, D:] = True
    G.untouched('h_out', hg, G.sentinel(hg.shape), mask)
    smask = np.zeros(sg.shape, bool)
    smask[:B] = with_sv
    G.untouched('sv', sg, G.sentinel(sg.shape), smask)
    w = G.Worst()
    every = np.ones(B, bool)
    w.see('h', hg[:B, D:], np.where(live, ref[0], 0), np.where(live, r32[0], 0), every)
    assert (hg[:B, D:][lens == 0] == 0).all()
    if with_sv:
        for i, nm in enumerate(('r', 'u', 'n')):
            w.see(nm, sg[:B].reshape(B, D, 4)[..., i], ref[1 + i], r32[1 + i], every)
        assert np.array_equal(sg[:B].reshape(B, D, 4)[..., 3], bR[:3 * D].reshape(D, 3)[None, :, 2].repeat(B, 0))      # hn = bR_n, the bits
    w.check('first-step-fwd-B%d-D%d' % (B, D))
    # backward from drawn gates
    svb = np.empty((B + G.GUARD_ROWS, D, 4), np.float32)
    svb[:] = np.nan
    svb[:B, :, 0:2] = rng.uniform(0.02, 0.98, (B, D, 2))
    svb[:B, :, 2] = rng.uniform(-0.98, 0.98, (B, D))
    svb[:B, :, 3] = 0.5 * rng.standard_normal((B, D))
    dh = G.nan32((B + G.GUARD_ROWS, 2 * D))
    dh[:B, D:] = rng.standard_normal((B, D))
    dgi, dgh = dev(G.sentinel((B + G.GUARD_ROWS, 3 * D))), dev(G.sentinel((B + G.GUARD_ROWS, 3 * D)))
    keep += [dev(dh), dev(svb)]
    P = (C.c_void_p * 5)(keep[2].data_ptr() + D * 4, keep[3].data_ptr(), dgi.data_ptr(), dgh.data_ptr(), dl.data_ptr())
    rc = l.avae_debug_op(h, b'gru_first_step_bwd', P, (C.c_int64 * 3)(2 * D, B, D), (C.c_float * 1)(0.0))
    if rc != 0:
        trip('gru_first_step_bwd: %s' % l.avae_last_error(h).decode())
    sync('gru_first_step_bwd')
    do = np.where(live, dh[:B, D:], 0)
    ref = G.step_bwd(do, zero, None, None, svb[:B], zero, 0)
    r32 = G.step_bwd(do, zero, None, None, svb[:B], zero, 0, np.float32)
    w = G.Worst()
    for nm, t, i in (('dgi', dgi, 0), ('dgh', dgh, 1)):
        g = t.cpu().numpy()
        m = np.zeros(g.shape, bool)
        m[:B] = True
        G.untouched(nm, g, G.sentinel(g.shape), m)
        w.see(nm, g[:B], ref[i], r32[i], every)
        assert (g[:B][lens == 0] == 0).all()
    w.check('first-step-bwd-B%d-D%d' % (B, D))
