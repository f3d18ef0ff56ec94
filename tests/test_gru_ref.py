"""tests/gru_ref.py on the CPU: the reference against the oracles, the layouts against naive loops, the comparison against float32
restatements with one defect each (every defect must fail, the clean restatement must pass), and every case of tests/test_gpu_gru.py against
the plan the library itself makes for it (avae_debug_gru_plan: host arithmetic, no GPU) -- a case can never quietly test another kernel."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import gru_ref as G
import ops_ref


def plan(c, fwd=None):
    from argsim_amd import lib
    l = lib.load()
    out = (C.c_int64 * 10)()
    rs = (C.c_int64 * 10)()
    ints = c.shape_ints()
    assert l.avae_debug_gru_plan((C.c_int64 * 15)(*ints), int(c.fwd), c.persistent, rs) == 0
    ints = c.shape_ints(int(rs[8]))
    assert l.avae_debug_gru_plan((C.c_int64 * 15)(*ints), int(c.fwd if fwd is None else fwd), c.persistent, out) == 0
    return dict(form=G.FORMS[out[0]], T=int(out[1]), C=int(out[2]), cpj=int(out[3]), Bg=int(out[4]), pipe=int(out[5]), G=int(out[6]), rpg=int(out[7]),
                rs_floats=int(out[8]))


def rows_of(c):
    p = plan(c)
    return G.make_rows(c, p['T'], p['cpj'])


# ------------------------------------------------------------------------------------------ the plan table
@pytest.mark.parametrize('c', G.all_cases(), ids=lambda c: c.id)
def test_case_reaches_the_kernel_it_claims(c):
    p = plan(c)
    assert (p['form'], p['T'], p['C'], p['pipe']) == c.reach, (c.id, p)
    assert p['Bg'] == c.B and p['rpg'] % 16 == 0 and p['G'] * p['rpg'] >= c.rows
    if c.skip:
        assert p['form'] in ('team', 'team_rs')
    assert 5 <= c.S <= 7 or c.name.endswith('S1')


def test_ids_are_unique():
    ids = [c.id for c in G.all_cases()]
    assert len(ids) == len(set(ids))


def test_plan_hook_geometry_and_scratch():
    """G = 0: the model's own choice (gru_geometry); the reduce-scatter scratch: 4 * 8192 floats per job and slot"""
    p = plan(G.Case('x', False, 2, 6, 64, 512, item=2, xbuf=True, bwd_rs=1))
    assert p['form'] == 'team_rs' and p['rs_floats'] == 2 * 64 * 4 * 8192 and (p['G'], p['rpg']) == (4, 16)
    p = plan(G.Case('x', True, 1, 6, 40, 16))
    assert (p['form'], p['G'], p['rpg']) == ('persistent', 3, 16)
    # too little scratch, no scratch, the item switch off: register forms
    from argsim_amd import lib
    l = lib.load()
    c = G.Case('x', True, 2, 6, 64, 512, item=2, xbuf=True)
    for edit, form in (({14: c.xbuf_floats() - 1}, 'persistent'), ({11: 0}, 'persistent'), ({}, 'team')):
        ints = c.shape_ints()
        for k, v in edit.items():
            ints[k] = v
        out = (C.c_int64 * 10)()
        assert l.avae_debug_gru_plan((C.c_int64 * 15)(*ints), 1, 1, out) == 0
        assert G.FORMS[out[0]] == form, (edit, list(out))


# ------------------------------------------------------------------------------------------ layouts
def test_g16_is_unit_major():
    D = 48
    nat = np.arange(3 * D).reshape(3 * D, 1)
    g16 = ops_ref.g16_permute(nat, D, True)[:, 0]
    for unit in range(D):
        for gate in range(3):
            assert g16[G.g16_col(unit, gate)] == gate * D + unit


def test_pos_map_is_reverse_sequence():
    from oracle.vae_numpy import reverse_sequence
    S, lens = 7, [7, 1, 4, 0, 2]
    x = np.arange(S * len(lens)).reshape(S, len(lens))
    y = reverse_sequence(x, lens)
    pos = G.pos_table(S, lens, 1)
    for b in range(len(lens)):
        assert sorted(pos[:, b]) == list(range(S))
        for p in range(S):
            assert y[p, b] == x[pos[p, b], b]
    assert (G.pos_table(S, lens, 0) == np.arange(S)[:, None]).all()


def test_team_steps_against_a_naive_loop():
    rng = np.random.default_rng(0)
    for T, cpj, Bg in ((2, 1, 32), (4, 1, 64), (2, 4, 384), (4, 4, 512), (4, 8, 1024)):
        slens = rng.integers(1, 8, Bg)
        got = G.team_steps(slens, T, cpj, 6)
        RB = 16 * T
        for slot in range(Bg):
            blk, team = slot // RB, (slot % RB) // 16
            later = [b for b in range(blk, Bg // RB, cpj)]
            want = max(min(6, int(slens[b * RB + team * 16:b * RB + team * 16 + 16].max())) for b in later)
            assert got[slot] == want, (T, cpj, slot)


def test_rows_and_buffers_round_trip():
    """sv, the row map and the row order: what make_inputs packs, logical() unpacks; a skipped row has fewer steps than S only under a row order"""
    for c in (G._team('t', False, 2, 64, skip='sorted', cmp=True), G._team('t', False, 1, 32, skip='sorted', cmp=True, Breal=20),
              G._reg('r', False, 2, 5, 16, ldh_pad=8)):
        rows = rows_of(c)
        inp = G.make_inputs(c, rows)
        S, B, D = c.S, c.rows, c.D
        cnt = 0
        for p in range(S):
            for b in range(B):
                real = p < rows.lens[b] if c.cmp else True
                assert (rows.rowmap[p, b] >= 0) == real
                if real:
                    assert rows.rowmap[p, b] == (cnt if c.cmp else p * B + b)
                    cnt += 1
                    for k in range(c.njobs):
                        L = inp['log'][k]
                        assert np.array_equal(inp['sv%d' % k][rows.rowmap[p, b]].reshape(D // 16, 16, 4), L['sv'][p, b].reshape(D // 16, 16, 4))
                        assert np.array_equal(inp['dh_out'][rows.rowmap[p, b], k * D:(k + 1) * D], L['dh_out'][p, b])
        assert rows.nrows == cnt
        for k in range(c.njobs):
            back = G.logical(inp['hp%d' % k], rows, 0, D)
            real = rows.rowmap >= 0
            assert np.array_equal(back[real], inp['log'][k]['hp'][real]) and np.isnan(back[~real]).all()
        assert np.isnan(inp['dh_out'][:, c.njobs * D:]).all() and np.isnan(inp['dh_out'][rows.nrows:]).all()
        if c.skip:
            assert sorted(rows.perm) == list(range(c.B)) and (rows.steps >= np.minimum(np.maximum(rows.lens, 1), S)).all() and (rows.steps < S).any()


def test_bf16_rne():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-5, 0.3333333], np.float32)      # 1 + 2^-8: a tie, to even; 1 + 3 * 2^-8: a tie, up
    bits, vals = G.bf16_rne(x)
    assert vals[0] == 1.0 and vals[1] == 1.0 and vals[2] == np.float32(1.015625) and vals[3] == -1.0
    import torch
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(vals, want) and np.array_equal(G.widen16(bits), want)


def test_half_ulp_of_bf16():
    """the allowance of a 16-bit output: a correctly rounded value always meets half an ulp, and misses 2^-9 |x| about every other time"""
    x = np.random.default_rng(5).uniform(-2, 2, 100000).astype(np.float32)
    err = np.abs(G.bf16_rne(x)[1].astype(np.float64) - x)
    assert (err <= G.half_ulp_bf16(x)).all()
    assert (G.half_ulp_bf16(x) <= 2.0 ** -8 * np.abs(x)).all() and (G.half_ulp_bf16(x) > 2.0 ** -9 * np.abs(x) * (1 - 1e-12)).all()
    assert 0.2 < (err > 2.0 ** -9 * np.abs(x)).mean() < 0.5
    assert G.half_ulp_bf16(np.array([0.0, 1.0, 1.5, 2.0, -0.75])).tolist() == [0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9]


# ------------------------------------------------------------------------------------------ the reference against the oracles
def natural(x16, D):
    """(..., 3D) G16 columns -> natural gate-major columns"""
    return np.moveaxis(ops_ref.g16_permute(np.moveaxis(x16, -1, 0).reshape(3 * D, -1), D, False).reshape((3 * D,) + x16.shape[:-1]), 0, -1)


def recurrence(c, rows, inp, k):
    """the float64 launch by step_fwd alone -> hs (S, B, D) by position"""
    L = inp['log'][k]
    S, B, D = c.S, c.rows, c.D
    pos = G.pos_table(S, rows.plen, k == 1)
    h = L['h0'].astype(np.float64) if L['h0'] is not None else np.zeros((B, D))
    hs = np.zeros((S, B, D))
    for p in range(S):
        h = G.step_fwd(L['gi'][pos[p], np.arange(B)], h, L['R'], L['bR'], 0)[0]
        hs[pos[p], np.arange(B)] = h
    return hs


@pytest.mark.parametrize('njobs', [1, 2])
def test_forward_against_numpy_oracle_and_torch(njobs):
    import torch
    from oracle import vae_numpy as vn
    c = G._reg('o', True, njobs, 5, 16, S=7)
    rows = rows_of(c)
    inp = G.make_inputs(c, rows)
    S, B, D = c.S, c.B, c.D
    for k in range(njobs):
        L = inp['log'][k]
        hs = recurrence(c, rows, inp, k)
        R, bR = ops_ref.g16_permute(L['R'].astype(np.float64), D, False), ops_ref.g16_permute(L['bR'].astype(np.float64).reshape(-1, 1), D, False)[:, 0]
        x = natural(L['gi'].astype(np.float64), D)
        if k == 1:          # the reversed direction: the oracle runs forward over the reversed input and reverses the output back
            x = vn.reverse_sequence(x, rows.lens)
        W = np.eye(3 * D)
        want, _ = vn.gru(x, W, R, np.zeros(3 * D), bR, L['h0'])
        if k == 1:
            want = vn.reverse_sequence(want, rows.lens)
        # (beyond a row's length the reversed direction goes on in step order: the same positions in both orders)
        assert np.abs(hs - want).max() < 1e-13
        g = torch.nn.GRU(3 * D, D).double()
        with torch.no_grad():
            g.weight_ih_l0.copy_(torch.eye(3 * D, dtype=torch.float64))
            g.weight_hh_l0.copy_(torch.from_numpy(R))
            g.bias_ih_l0.zero_()
            g.bias_hh_l0.copy_(torch.from_numpy(bR))
            h0 = torch.from_numpy(L['h0'].astype(np.float64))[None] if L['h0'] is not None else torch.zeros(1, B, D, dtype=torch.float64)
            got, _ = g(torch.from_numpy(x), h0)
        got = got.numpy()
        if k == 1:
            got = vn.reverse_sequence(got, rows.lens)
        assert np.abs(hs - got).max() < 1e-13


@pytest.mark.parametrize('njobs', [1, 2])
def test_backward_against_autograd(njobs):
    """dgi = d / d gi, dgh = d / d (R h + bR), dh0, through a float64 torch restatement of the cell; sv and hp come from the forward"""
    import torch
    cf = G._reg('o', True, njobs, 5, 16, S=7)
    rows = rows_of(cf)
    fin = G.make_inputs(cf, rows)
    S, B, D = cf.S, cf.B, cf.D
    cb = dataclasses.replace(cf, fwd=False)
    binp = G.make_inputs(cb, rows)
    ar = np.arange(B)
    for k in range(njobs):
        L = fin['log'][k]
        pos = G.pos_table(S, rows.plen, k == 1)
        gi = torch.tensor(L['gi'].astype(np.float64), requires_grad=True)
        R, bR = torch.tensor(L['R'].astype(np.float64)), torch.tensor(L['bR'].astype(np.float64))
        h0 = torch.tensor((L['h0'] if L['h0'] is not None else np.zeros((B, D))).astype(np.float64), requires_grad=True)
        h, ghs, outs = h0, [], []
        sv, hp = np.zeros((S, B, D, 4)), np.zeros((S, B, D))
        for p in range(S):
            gh = h @ R.T + bR
            gh.retain_grad()
            g3, h3 = gi[pos[p], ar].reshape(B, D, 3), gh.reshape(B, D, 3)
            r, u = torch.sigmoid(g3[..., 0] + h3[..., 0]), torch.sigmoid(g3[..., 1] + h3[..., 1])
            n = torch.tanh(g3[..., 2] + r * h3[..., 2])
            hp[pos[p], ar] = h.detach().numpy()
            sv[pos[p], ar] = torch.stack([r, u, n, h3[..., 2]], -1).detach().numpy()
            h = (1 - u) * n + u * h
            ghs.append(gh)
            outs.append(h)
        dh_out = binp['log'][k]['dh_out'].astype(np.float64)
        loss = sum((outs[p] * torch.tensor(dh_out[pos[p], ar])).sum() for p in range(S))
        loss.backward()
        # the same by step_bwd
        carry, nxt = np.zeros((B, D)), None
        for p in range(S - 1, -1, -1):
            dgi, dgh, carry, _ = G.step_bwd(dh_out[pos[p], ar], carry, nxt, L['R'].astype(np.float64), sv[pos[p], ar], hp[pos[p], ar], 0)
            nxt = dgh
            assert np.abs(dgi - gi.grad.numpy()[pos[p], ar]).max() < 1e-12
            assert np.abs(dgh - ghs[p].grad.numpy()).max() < 1e-12
        dh0 = carry + G.bf_prod(nxt, L['R'], 0, np.float64)
        assert np.abs(dh0 - h0.grad.numpy()).max() < 1e-12


# ------------------------------------------------------------------------------------------ the comparison has teeth
TEETH_FWD = [('', 'reg'), ('swap_ru', 'reg'), ('pos_map', 'reg'), ('neighbour', 'reg'), ('ld', 'reg'), ('padding', 'skip')]
TEETH_BWD = [('', 'reg'), ('carry', 'reg'), ('bias', 'reg'), ('', 'skip')]


def teeth_case(kind, fwd, bf16=0):
    if kind == 'reg':
        return G._reg('teeth', fwd, 2, 5, 16, S=7, ldh_pad=8, ldg_pad=12, bf16=bf16)
    return G._team('teeth', fwd, 2, 64, skip='sorted', bf16=bf16)


@pytest.mark.parametrize('bf16', [0, 1])
@pytest.mark.parametrize('defect,kind', TEETH_FWD)
def test_forward_comparison_has_teeth(defect, kind, bf16):
    c = teeth_case(kind, True, bf16)
    if kind == 'skip':
        c = dataclasses.replace(c, D=16, reach=None)         # (the comparison does not look at the width; the plan does: the geometry of D = 512)
        rows = G.make_rows(c, 4, 1)
    else:
        rows = rows_of(c)
    inp = G.make_inputs(c, rows)
    before = G.make_outputs(c, rows, inp)
    got = G.run_forward(c, rows, inp, {k: v.copy() for k, v in before.items()}, defect=defect)
    if not defect:
        r = G.check_forward(c, rows, inp, before, got)
        assert max(r.values()) <= 1.0 + 1e-9          # the float32 restatement IS the yardstick
    else:
        with pytest.raises(AssertionError):
            G.check_forward(c, rows, inp, before, got)


@pytest.mark.parametrize('cmp', [False, True], ids=['padded', 'compact'])
@pytest.mark.parametrize('defect', ['', 'sv16_index', 'hp16_next'])
def test_backward_comparison_has_teeth_for_16bit_inputs(defect, cmp):
    """Case.in16: the restatement reads its saved gates / h_prev out of the 16-bit buffers.  Clean, it passes and gives the bits of the same restatement on
    the fp32 arrays (which hold the same rounded values); the gates fetched at the fp32 index, or h_prev of position p taken from p + 1, must fail"""
    c = dataclasses.replace(G._team('teeth', False, 2, 64, skip='sorted', cmp=cmp, bf16=1, in16='sv+hp'), D=16, reach=None)
    rows = G.make_rows(c, 4, 1)
    inp = G.make_inputs(c, rows)
    for k in range(c.njobs):
        L = inp['log'][k]
        assert np.array_equal(G.bf16_rne(L['sv'])[1], L['sv']) and np.array_equal(G.bf16_rne(L['hp'])[1], L['hp'])
        read = G.read_mask(c, rows, k == 1)
        for nm, w in (('sv', 4 * c.D), ('hp', c.D)):
            buf = inp['%s16_%d' % (nm, k)]
            assert np.array_equal(G.widen16(buf[rows.rowmap[read]]), L[nm].reshape(c.S, c.rows, w)[read])
            assert (buf == G.NAN16).sum() == buf.size - int(read.sum()) * w            # NaN in the guard rows and wherever no step reads
        assert cmp or not read.all()                    # the padded layout under a row order has positions no step reads
    before = G.make_outputs(c, rows, inp)
    got = G.run_backward(c, rows, inp, {k: v.copy() for k, v in before.items()}, defect=defect)
    if not defect:
        G.check_backward(c, rows, inp, before, got)
        plain = G.run_backward(dataclasses.replace(c, in16=''), rows, inp, {k: v.copy() for k, v in before.items()})
        assert all(G.same_bits(got[k], plain[k]) for k in got)
    else:
        with pytest.raises(AssertionError):
            G.check_backward(c, rows, inp, before, got)


def test_which_backward_forms_take_16bit_inputs():
    """IN16_TABLE against the plan: 'reached' is the bf16 team form and nothing else (check_operands: the 16-bit operands need a team form that asked for
    bf16); tests/test_gpu_gru.py launches every row of the table and holds the refused ones to 'nothing written'"""
    seen = set()
    for c, what in G.IN16_TABLE:
        p = plan(c)
        assert (p['form'], p['T'], p['C'], p['pipe']) == c.reach, (c.id, p)
        assert (what == 'reached') == (p['form'] == 'team' and c.bf16 == 1), (c.id, p['form'])
        seen.add((p['form'], c.bf16))
    # every (form, bf16) a backward plan can have: team_rs is fp32 only (bf16 plans the team form), the item form is forward only
    assert seen == {('team', 1), ('team', 0), ('team_rs', 0), ('persistent', 1), ('stepwise', 1)}
    assert plan(dataclasses.replace(G._team('x', False, 2, 64, bwd_rs=1), bf16=1))['form'] == 'team'
    for c in G.team_in16_cases():
        assert c.bf16 == 1 and not c.fwd and c.reach[0] == 'team' and c.in16 in ('sv', 'hp', 'sv+hp')


@pytest.mark.parametrize('bf16', [0, 1])
@pytest.mark.parametrize('defect,kind', TEETH_BWD)
def test_backward_comparison_has_teeth(defect, kind, bf16):
    c = teeth_case(kind, False, bf16)
    if kind == 'skip':
        c = dataclasses.replace(c, D=16, reach=None)
        rows = G.make_rows(c, 4, 1)
    else:
        rows = rows_of(c)
    inp = G.make_inputs(c, rows)
    before = G.make_outputs(c, rows, inp)
    got = G.run_backward(c, rows, inp, {k: v.copy() for k, v in before.items()}, defect=defect)
    if not defect:
        G.check_backward(c, rows, inp, before, got)
    else:
        with pytest.raises(AssertionError):
            G.check_backward(c, rows, inp, before, got)
