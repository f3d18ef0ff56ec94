"""The exchange ring of the fp32 team kernels (gru_dev.h "exchange ring"): the value a team produces in its iteration q lives in
slot q % 4 of a scratch of min(S, 4) slots per job, and the producers re-arm the slots themselves.  No bit of any result may change.

Every case is ONE avae_debug_gru call on caller buffers (the Launch of tests/test_gpu_gru.py: NaN / sentinel guards around everything), checked
(i) like every kernel form -- forward by the float64 single-step induction, backward against the float64 recurrence, yardstick and margin of
gru_ref.py -- and (ii) bit for bit against the same launch with option gru_ring = 0 (one slot per position): hs, hp, the saved gates, dgi, dgh and
dh0.  The bias sums are left to their summation bound in (i): their atomic order is free, two runs of one launch already differ.

Geometries: the smallest the team kernels have -- (1 job, 32 rows): 2 teams of 8 waves, one chain group; (2 jobs, 64 rows): 4 teams of 4 waves,
both directions, the second job reversed over ragged lengths (gru_ref.ragged_lens: a full row, a row of length 1 and two more lengths inside
one 16-row team, so rows end before their team does).  S = 1 .. 4: no slot is used twice; 5: the first wrap (one re-arm); 9, 13: two and three.
A forward launch of one step is a stepwise launch (gru_plan) and takes no exchange at all: it is kept for the option's sake."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import gru_ref as G
import test_gpu_gru as TG
from test_gpu_gru import gpu          # noqa: F401 -- the module-scoped handle fixture

pytestmark = pytest.mark.gpu

GEOM = ((1, 32), (2, 64))
LENGTHS = (1, 2, 3, 4, 5, 9, 13)
RING = 4


def case(name, fwd, njobs, B, S, **kw):
    c = G._team(name, fwd, njobs, B, S, **kw)
    return dataclasses.replace(c, reach=G.STEPWISE) if fwd and S < 2 else c


def ring_slots_floats(c):
    """floats of the scratch a launch with the ring on may touch: min(S, 4) slots per job at the front"""
    return c.njobs * min(c.S, RING) * c.B * c.D * (1 if c.fwd else 3)


@pytest.fixture
def ring_option(gpu):
    """-> set(v): option gru_ring of the module's handle; back to its default (1) afterwards, whatever happened"""
    l, h = gpu

    def set_(v):
        assert l.avae_set_option(h, b'gru_ring', int(v)) == 0
    yield set_
    set_(1)


def own_scratch(c, floats=None):
    """an exchange scratch of the test's own (to look into afterwards, or to share between launches), sentinel everywhere"""
    return TG.dev(G.sentinel((floats or c.xbuf_floats()) + TG.XGUARD))


def on_and_off(L, ring_option, c=None, **edit):
    """-> the outputs of the launch with the ring on, after holding them bit for bit to those of the same launch with the ring off"""
    c = c or L.c
    ring_option(1)
    on = L.run(**edit)
    ring_option(0)
    off = L.run(**edit)
    ring_option(1)
    diff = TG.bits_equal(on, off)
    assert not diff, (c.id, 'ring on / off differ in', diff)
    return on


def planned_ring(gpu, c):
    return int(TG.plan_of(gpu[0], c)[9])


# ------------------------------------------------------------------------------------------ every length, both geometries
@pytest.mark.parametrize('S', LENGTHS)
@pytest.mark.parametrize('njobs,B', GEOM)
@pytest.mark.parametrize('fwd', [True, False], ids=['fwd', 'bwd'])
def test_ring_lengths(gpu, ring_option, fwd, njobs, B, S):
    c = case('ring', fwd, njobs, B, S)
    assert planned_ring(gpu, c) == (0 if fwd and S < 2 else RING), c.id
    L = TG.Launch(gpu, c)
    L.check(on_and_off(L, ring_option))


# ------------------------------------------------------------------------------------------ the whole chip
# the geometries of the flagship step: 8 chain groups x 32 workgroups, every CU taken (both encoder directions in 4 teams; a decoder layer in 2)
FULL_CHIP = {(2, 256): (4, 8, 0), (1, 256): (2, 8, 0)}


@pytest.mark.parametrize('njobs,B', sorted(FULL_CHIP))
@pytest.mark.parametrize('fwd', [True, False], ids=['fwd', 'bwd'])
def test_ring_full_chip(gpu, ring_option, fwd, njobs, B):
    c = G.Case('ring-chip', fwd, njobs, 13, B, 512, item=2, xbuf=True, h0=njobs == 1, reach=('team',) + FULL_CHIP[(njobs, B)], seed=B + njobs)
    assert planned_ring(gpu, c) == RING, c.id
    L = TG.Launch(gpu, c)
    L.check(on_and_off(L, ring_option))


# ------------------------------------------------------------------------------------------ variants at S = 9
VARIANTS = {
    'row-order': dict(skip='sorted'),                                # slens / perm: teams run their own step counts
    'any-order': dict(skip='unsorted'),                              # rows of any length in one team: most end before the team does
    'compact': dict(skip='sorted', cmp=True),
    'phantom': dict(skip='sorted', cmp=True, phantom=True),          # B 20 on 32 slots / 48 on 64
    'slow-path': dict(force_slow=1),                                 # sc1 stores: data and re-arm
    'stagger': dict(stagger=1),
    'spec': dict(skip='sorted', cmp=True, spec=1),
}


@pytest.mark.parametrize('what', sorted(VARIANTS))
@pytest.mark.parametrize('njobs,B', GEOM)
@pytest.mark.parametrize('fwd', [True, False], ids=['fwd', 'bwd'])
def test_ring_variants(gpu, ring_option, fwd, njobs, B, what):
    kw = dict(VARIANTS[what])
    if kw.pop('phantom', False):
        kw['Breal'] = 20 if B == 32 else 48
    c = case('ring-' + what, fwd, njobs, B, 9, **kw)
    assert planned_ring(gpu, c) == RING, c.id
    L = TG.Launch(gpu, c)
    L.check(on_and_off(L, ring_option))


# ------------------------------------------------------------------------------------------ one scratch, two launches
@pytest.mark.parametrize('order', [(13, 5), (5, 13)], ids=['13-then-5', '5-then-13'])
@pytest.mark.parametrize('njobs,B', GEOM)
@pytest.mark.parametrize('fwd', [True, False], ids=['fwd', 'bwd'])
def test_ring_back_to_back(gpu, ring_option, fwd, njobs, B, order):
    """two launches with different inputs on ONE scratch: the second gives what it gives on a fresh scratch -- nothing an earlier launch left
    in a slot is ever taken for a fresh value"""
    ring_option(1)
    first = TG.Launch(gpu, dataclasses.replace(case('ring-b2b', fwd, njobs, B, order[0]), seed=71))
    second = TG.Launch(gpu, dataclasses.replace(case('ring-b2b', fwd, njobs, B, order[1]), seed=72))
    fresh = second.run()
    second.check(fresh)
    X = own_scratch(first.c, max(first.c.xbuf_floats(), second.c.xbuf_floats()))
    first.check(first.run(raw={('shared', 4): X.data_ptr()}))
    again = second.run(raw={('shared', 4): X.data_ptr()})
    diff = TG.bits_equal(fresh, again)
    assert not diff, (second.c.id, 'after a launch of S = %d on the same scratch' % order[0], diff)
    second.check(again)


# ------------------------------------------------------------------------------------------ the ring stays inside its slots
@pytest.mark.parametrize('S', [3, 9])
@pytest.mark.parametrize('njobs,B', GEOM)
@pytest.mark.parametrize('fwd', [True, False], ids=['fwd', 'bwd'])
def test_ring_touches_its_slots_only(gpu, ring_option, fwd, njobs, B, S):
    """with the ring on nothing behind njobs x min(S, 4) slots of the scratch is written (fill, data, re-arm); with it off the launcher's
    fill covers all S slots of every job, so the option is seen to switch"""
    c = case('ring-guard', fwd, njobs, B, S)
    L = TG.Launch(gpu, c)
    n, inside = c.xbuf_floats(), ring_slots_floats(c)
    for ring in (1, 0):
        ring_option(ring)
        X = own_scratch(c)
        L.run(raw={('shared', 4): X.data_ptr()})
        x = X.cpu().numpy().view(np.int32)
        assert (x[n:] == G.SENT).all(), (c.id, ring, 'written behind the scratch')
        if ring:
            assert (x[inside:n] == G.SENT).all(), (c.id, 'written behind the ring: first at float %d of %d' % (inside + int(np.argmax(x[inside:n] != G.SENT)), n))
            assert (x[:inside] != G.SENT).all(), (c.id, 'a word of the ring neither filled nor stored')
        else:
            assert (x[:n] != G.SENT).all(), (c.id, 'gru_ring = 0 did not fill the full-length exchange')
