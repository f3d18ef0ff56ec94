"""The case table of tests/test_gpu_step_routes.py: whole training steps at dim_emb = 512, the one width the GRU team kernels have a geometry
for (gru.hip team_geometry), one case per route model.cpp can take there -- table-fed first layers, the compact row map, phantom rows, the
one-step top encoder layer, the 16-bit panels of bf16 mode, the two BPTT forms, and the kernel forms behind the options.

A batch is the smallest that reaches its route (BATCHES); a case is a batch, a dtype, the options it forces and the route it must take, as
VAE.step_route() reports it (Case.route: the expectation lives HERE, as gru_ref.Case.reach does for single launches).
tests/test_step_routes.py holds the GRU plans of the table against avae_debug_gru_plan and Bx against avae_debug_team_batch without a GPU;
every GPU case compares step_route() with its entry before it compares a number.

No case HERE relies on the fill hint (the asynchronous copy that decides compact = 2, bwd_rs = 2 and gru_spec = 2): every case forces those
three, "default" to what the hint gives once it has arrived (the batch's own fill), except AUTO, which leaves compact and bwd_rs at 2, runs
twice and is asserted on what the second call took.  What the hint of ANOTHER batch does to a step -- the three options left at their
defaults, one handle over many shapes -- is tests/step_history.py and tests/test_gpu_step_history.py.

check_step is what a step is held to against the float64 oracle, in both GPU files."""
import dataclasses

import numpy as np

import helpers
from helpers import grad_blocks_ratio, grads_bad, rel_l2

D, R, STEP = 512, 32, 20000

# name: (V, L, B, S, variant) -- what each reaches:
#   b64    384 and 448 tokens >= V: both first layers table-fed; own team geometry (4-team encoder pair, 2-team decoder); S = 6 wraps the
#          4-slot exchange ring
#   b64x   b64 with source != target and an eos id in the middle of a source row and of a target row: the compact map with steps behind an eos
#   b64v   fewer tokens than vocabulary entries: no table, hence no compact layout -- the team kernels over padded arrays with skip_pad
#   b64L1  no one-step top form: pick_last sits directly on the table-fed layer;  b64L3  a middle layer that is neither table-fed nor top
#   b20    32 slots, 12 phantom rows; table-fed because tokens >= V
#   b100   128 slots; 1100 tokens >= 1024 but < V: the "table-fed below the vocabulary size" clause of use_table
#   bpipe  the smallest batch whose encoder-pair AND decoder launches are row-block pipelined (GruPlan::pipe): 1024 rows (at 512 the
#          one-job launches still have one row block per workgroup)
#   b256   the smallest batch whose encoder pair has gru_geometry's 8 groups of 32 rows: with gru_item = 1 the item-pipelined forward
BATCHES = {
    'b64':   (256, 2, 64, 6, ''),
    'b64x':  (256, 2, 64, 6, 'eos'),
    'b64v':  (1024, 2, 64, 6, ''),
    'b64L1': (256, 1, 64, 6, ''),
    'b64L3': (256, 3, 64, 6, ''),
    'b20':   (256, 2, 20, 14, ''),
    'b100':  (2048, 2, 100, 11, ''),
    'bpipe': (512, 2, 1024, 4, ''),
    'b256':  (256, 2, 256, 6, ''),
}


def make(name):
    """-> cfg, P, src, tgt, keep, eps: helpers.make_batch's ragged batch (rows 0 and B / 2 full, row 1 of length 1, the rest in [2, S], ids
    from [3, V), parameters exactly representable in fp32); 'eos': source != target as in test_eos_in_the_middle_of_a_row"""
    V, L, B, S, variant = BATCHES[name]
    cfg, P, ids, keep, eps = helpers.make_batch(dict(dim_tgt=V, dim_emb=D, dim_rep=R, rnn_layers=L), B, S, 'ragged')
    src, tgt = ids.copy(), ids.copy()
    if variant == 'eos':            # rows 0 and B / 2 are full: every other row keeps its length, no source row is all eos
        src[0, 3] = cfg['eos']
        tgt[B // 2, 4] = cfg['eos']
        tgt[B // 2, 1] = cfg['eos']
    return cfg, P, src, tgt, keep, eps


def fill(name):
    """real source positions / padded source positions of the batch: what the fill hint reports once it has arrived"""
    cfg, _, src, _, _, _ = make(name)
    lens = (src != cfg['eos']).sum(1)
    return float(lens.sum()) / float(lens.max() * len(lens))


# GruForm (kernels.h)
STEPWISE, PERSISTENT, ITEM, TEAM, TEAM_RS = range(5)
# the options a case forces, in the order they are set; compact / bwd_rs / gru_spec: see default_options
OPTIONS = dict(persistent=1, gru_item=2, gru_ring=1, skip_pad=1, enc_top1=1, table_l1=1, compact=1, bwd_rs=0, gru_spec=0,
               bf16_act=1, bf16_sv=1, bf16_tn=1, logits16=1)
# fill of each batch (fill(), held by tests/test_step_routes.py): the hint's thresholds are 0.92 (compact), 0.40 (bwd_rs), 0.60 (gru_spec), so
# "default" is compact 1 and bwd_rs 0 everywhere, gru_spec 1 on b20 and b100
FILL = {'b64': 0.648, 'b64x': 0.646, 'b64v': 0.648, 'b64L1': 0.648, 'b64L3': 0.648, 'b20': 0.496, 'b100': 0.576, 'bpipe': 0.742, 'b256': 0.650}
SPEC = {'b20': 1, 'b100': 1}


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    batch: str
    dtype: str
    options: tuple          # ((key, value), ...): every option of OPTIONS
    route: tuple            # step_route() as sorted items
    calls: int = 1          # AUTO: 2

    def opt(self, key):
        return dict(self.options)[key]

    def want(self):
        return dict(self.route)


def _team(T, C, pipe=0, ring=4, form=TEAM):
    return (form, T, C, pipe, 0 if form == TEAM_RS else ring)


REG = (PERSISTENT, 0, 0, 0, 0)
STEP1 = (STEPWISE, 0, 0, 0, 0)


def _route(table=(1, 1), compact=(1, 1), Bx=64, bwd_rs=0, top1=1, pair=_team(4, 2), one=_team(2, 2), pair_bwd=None, one_bwd=None, top=True):
    """pair: the two-direction encoder launches, one: the one-job launches (top encoder layer where top, decoder); *_bwd: where the backward
    differs from the forward"""
    pair_bwd, one_bwd = pair_bwd or pair, one_bwd or one
    return tuple(sorted(dict(table=table, compact=compact, Bx=Bx, bwd_rs=bwd_rs, top1=top1, enc_fwd=pair, enc_bwd=pair_bwd,
                             top_fwd=one if top else None, top_bwd=one_bwd if top else None, dec_fwd=one, dec_bwd=one_bwd).items()))


def _rs(g):
    return _team(g[1], g[2], g[3], form=TEAM_RS)


def _case(cid, batch, dtype='f32', route=None, calls=1, **opts):
    o = dict(OPTIONS, gru_spec=SPEC.get(batch, 0))
    assert not set(opts) - set(o), opts
    o.update(opts)
    return Case(cid, batch, dtype, tuple(o.items()), route, calls)


def cases():
    o = []
    P4, P2 = _team(4, 2), _team(2, 2)
    # ---- b64, fp32: the options one by one
    o.append(_case('b64-default', 'b64', route=_route()))
    o.append(_case('b64-compact1-skip1', 'b64', route=_route(), compact=1, skip_pad=1))
    o.append(_case('b64-compact0-skip1', 'b64', route=_route(compact=(0, 0)), compact=0, skip_pad=1))
    o.append(_case('b64-compact0-skip0', 'b64', route=_route(compact=(0, 0)), compact=0, skip_pad=0))
    o.append(_case('b64-enc_top1=0', 'b64', route=_route(top1=0, top=False), enc_top1=0))
    o.append(_case('b64-bwd_rs=0', 'b64', route=_route(), bwd_rs=0))
    o.append(_case('b64-bwd_rs=1', 'b64', route=_route(bwd_rs=1, pair_bwd=_rs(P4), one_bwd=_rs(P2)), bwd_rs=1))
    o.append(_case('b64-gru_ring=0', 'b64', route=_route(pair=_team(4, 2, ring=0), one=_team(2, 2, ring=0)), gru_ring=0))
    # (at 64 rows gru_geometry gives 4 groups of 16: gru_item = 1 takes the register-form persistent kernels both ways, as gru_item = 0 does;
    #  the item-pipelined forward needs groups of 32 rows: b256 below)
    o.append(_case('b64-gru_item=1', 'b64', route=_route(compact=(0, 0), pair=REG, one=REG), gru_item=1))
    o.append(_case('b64-gru_item=0', 'b64', route=_route(compact=(0, 0), pair=REG, one=REG), gru_item=0))
    o.append(_case('b64-persistent=0', 'b64', route=_route(compact=(0, 0), pair=STEP1, one=STEP1), persistent=0))
    o.append(_case('b64-table_l1=0', 'b64', route=_route(table=(0, 0), compact=(0, 0)), table_l1=0))
    # ---- b64, the other dtypes (bf16: no exchange ring, gru.hip gru_plan)
    B4, B2 = _team(4, 2, ring=0), _team(2, 2, ring=0)
    o.append(_case('b64-f32s', 'b64', 'f32s', route=_route()))
    o.append(_case('b64-bf16', 'b64', 'bf16', route=_route(pair=B4, one=B2)))
    for k in ('bf16_act', 'bf16_sv', 'bf16_tn', 'logits16'):
        o.append(_case('b64-bf16-%s=0' % k, 'b64', 'bf16', route=_route(pair=B4, one=B2), **{k: 0}))
    # ---- the other 64-row batches
    o.append(_case('b64x-default', 'b64x', route=_route()))
    o.append(_case('b64v-default', 'b64v', route=_route(table=(0, 0), compact=(0, 0))))
    o.append(_case('b64L1-default', 'b64L1', route=_route(top1=0, top=False)))
    o.append(_case('b64L3-default', 'b64L3', route=_route()))
    # ---- phantom rows and the pipelined forms: default, the reduce-scatter BPTT, bf16
    for b, Bx, pair, one in (('b20', 32, _team(2, 2), _team(2, 1)), ('b100', 128, _team(2, 8), _team(2, 4)),
                             ('bpipe', 1024, _team(4, 8, 1, ring=0), _team(4, 8, 1, ring=0))):
        nr = lambda g: _team(g[1], g[2], g[3], ring=0)
        o.append(_case(b + '-default', b, route=_route(Bx=Bx, pair=pair, one=one)))
        o.append(_case(b + '-bwd_rs=1', b, route=_route(Bx=Bx, bwd_rs=1, pair=pair, one=one, pair_bwd=_rs(pair), one_bwd=_rs(one)), bwd_rs=1))
        o.append(_case(b + '-bf16', b, 'bf16', route=_route(Bx=Bx, pair=nr(pair), one=nr(one))))
    # (gemm_plan gives a product of up to 512 rows the thin tiles, which stay on the exact-fp32 kernel in f32s mode: at b64 the f32s step runs
    #  the fp32 step's GEMMs.  bpipe's 4096 and 5120 rows reach gemm_f32s.)
    o.append(_case('bpipe-f32s', 'bpipe', 'f32s', route=_route(Bx=1024, pair=_team(4, 8, 1, ring=0), one=_team(4, 8, 1, ring=0))))
    # ---- the automatic choices: a phantom batch takes the compact layout whatever the hint says; its fill of 0.50 is not below 0.40, so the
    #      second call (the first call's hint has arrived: losses() synchronised) keeps the gather form of the BPTT
    o.append(_case('b20-AUTO', 'b20', route=_route(Bx=32, pair=_team(2, 2), one=_team(2, 1)), calls=2, compact=2, bwd_rs=2))
    # ---- the item-pipelined forward (encoder pair: 8 groups of 32 rows) in front of the register-form persistent backward
    o.append(_case('b256-gru_item=1', 'b256', route=_route(compact=(0, 0), Bx=256, pair=(ITEM, 0, 0, 0, 0), pair_bwd=REG, one=REG), gru_item=1))
    return o


CASES = cases()


def launches(c):
    """what the GPU-less test asks avae_debug_gru_plan: (kind, fwd, njobs, steps) of every GRU launch kind the case expects"""
    _, _, _, S, _ = BATCHES[c.batch]
    return [(k, fwd, njobs, steps) for k, fwd, njobs, steps in
            (('enc_fwd', 1, 2, S), ('enc_bwd', 0, 2, S), ('top_fwd', 1, 1, S), ('top_bwd', 0, 1, S), ('dec_fwd', 1, 1, S + 1), ('dec_bwd', 0, 1, S + 1))
            if c.want()[k] is not None]


# ------------------------------------------------------------------------------------------ what a step is held to
#        losses rel, mu / lv abs, CE abs, gradients
TOLS = {'f32': (2e-5, 2e-5, 1e-4, 2e-4), 'f32s': (2e-5, 2e-5, 1e-4, 2e-4), 'bf16': (1e-2, 3e-2, 6e-2, 5e-2)}


def block_ratios(got, want, tol):
    """{variable: worst block error over its bound}; the embedding: the worse of its 16-row blocks and its single rows"""
    r = {k: grad_blocks_ratio(got[k], want[k], tol) for k in want}
    r['embed/embedding'] = max(r['embed/embedding'], grad_blocks_ratio(got['embed/embedding'], want['embed/embedding'], tol, rows=1))
    return r


def check_step(tag, dtype, t, losses, ce, got, mu, lv, head=None):
    """One training step against the float64 oracle of its batch.  t: the batch's truth (cfg, outs, grads of vt.loss_and_grads in float64, f32:
    {tolerance: block_ratios of the float32 oracle}); losses, ce (float64), got, mu, lv: losses(), train_ce(), get_grads() and encode() of the
    step.  Prints a RATIO line per variable and one line that starts with `head` (default: the ROUTE line), then asserts with TOLS[dtype]."""
    tl, tz, tc, tg = TOLS[dtype]
    outs, grads = t['outs'], t['grads']
    ratios = block_ratios(got, grads, tg)
    for k in grads:
        print('RATIO %s %s %s block %.4f (float32 oracle %.2g) rel_l2 %.3g' % (tag, dtype, k, ratios[k], t['f32'][tg][k], rel_l2(got[k], grads[k])))
    worst = max(ratios, key=ratios.get)
    if head is None:
        head = 'ROUTE %s %s worst block ratio %.4f %s' % (tag, dtype, ratios[worst], worst)
    else:
        head = '%s worst block ratio %.4f (float32 oracle %.2g) %s' % (head, ratios[worst], t['f32'][tg][worst], worst)
    print('%s; CE %.3g mu %.3g lv %.3g' % (
        head, np.abs(ce - outs['loss_gen_samp']).max() if ce.shape == outs['loss_gen_samp'].shape else -1.0,
        np.abs(mu - outs['mu']).max(), np.abs(lv - outs['lv']).max()))

    for got_l, key in zip(losses, ('loss_gen', 'loss_kld', 'loss')):
        assert abs(got_l - outs[key]) <= tl * abs(outs[key]), (tag, key, got_l, float(outs[key]))
    assert np.abs(mu - outs['mu']).max() <= tz and np.abs(lv - outs['lv']).max() <= tz, tag
    assert ce.shape == outs['loss_gen_samp'].shape, (tag, ce.shape)
    assert np.abs(ce - outs['loss_gen_samp']).max() <= tc, (tag, float(np.abs(ce - outs['loss_gen_samp']).max()))
    zeros = [k for k in grads if not grads[k].any()]
    assert zeros == ['encode/rnn%d/bwd/R' % t['cfg']['rnn_layers']], zeros      # (the top layer's backward direction is read at its first step alone, from h = 0)
    for k in zeros:
        assert not got[k].any(), (tag, k)
    bad = {k: rel_l2(got[k], grads[k]) for k in grads if not rel_l2(got[k], grads[k]) <= tg}
    assert not bad, (tag, bad)
    bad = grads_bad(got, grads, tg)
    assert not bad, (tag, bad)
    return ratios[worst], worst
