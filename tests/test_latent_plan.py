"""knn_plan, agg_plan and probe_plan (knn.hip, agg.hip, probe.hip: since this change their constants + one row_parts call, row_parts.h)
against the plans of the commit in which each still carried its own copy of the part arithmetic.

tests/golden/latent_plan_parent.npz was recorded from that commit (its hash is in the `parent` field), never from the code under test,
by tests/golden/make_latent_plan_golden.py: the parent's three functions compiled as a host program.  `inputs` rows are (kind, n, N,
k or P, dim, chunk_opt), kind 0 knn / 1 agg / 2 probe; `plan` rows every field of the plan (qrows or ptiles, qtiles or Ppad, LD or 0,
parts, chunk).  No GPU: host arithmetic of the library, through avae_debug_latent_plan."""
import ctypes as C
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'latent_plan_parent.npz')
CLAMP = 0x7fffff80
NMAX = (1 << 31) - 256
TILE = {0: 128, 1: 64, 2: 128}


def _plan(inputs):
    from argsim_amd import lib
    fn = lib.load().avae_debug_latent_plan
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
    out = np.full((len(inputs), 5), -1, dtype=np.int32)
    for r, o in zip(inputs.tolist(), out):
        assert fn(r[0], r[1], r[2], r[3], r[4], r[5], o.ctypes.data_as(C.POINTER(C.c_int32))) == 0, r
    return out


def _max_parts(kind, k):
    return min(512, 48 * 1024 // (12 * k) - 1) if kind == 0 else (1024, 256)[kind - 1]


def test_plans_equal_the_parents():
    g = np.load(GOLDEN)
    assert str(g['parent']) == 'b7888ab'
    inputs, want = g['inputs'], g['plan']
    assert inputs.dtype == np.int64 and want.dtype == np.int32 and inputs.shape[1] == 6 == len(g['fields']) and want.shape == (len(inputs), 5)
    got = _plan(inputs)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, [(dict(zip(map(str, g['fields']), inputs[i].tolist())), got[i].tolist(), want[i].tolist()) for i in bad[:5]]


def test_plan_table_covers_what_it_claims():
    """the table itself: every n, k and chunk option, both knn tile heights, the thresholds from both sides, the part limit's
    correction taken and not taken for each planner, the clamp, and 2^31 - 256 rows"""
    g = np.load(GOLDEN)
    inputs, plan = g['inputs'], g['plan']
    kind, n, N, kp, dim, opt = inputs.T
    assert 2000 <= len(inputs) <= 4000 and set(kind) == {0, 1, 2}
    assert set(plan[kind == 0, 0]) == {32, 128}
    for kd in (0, 1):
        assert set(n[kind == kd]) == {1, 32, 64, 65, 128, 129, 4096}
    assert set(kp[kind == 0]) == {1, 2, 16, 31, 32}
    assert {_max_parts(0, int(k)) for k in kp[kind == 0]} >= {512, 127}
    assert (N[kind == 0] == 0).any() and (plan[(kind == 0) & (N == 0), 3:] == 0).all()
    for kd in (0, 1, 2):
        rows = kind == kd
        assert set(opt[rows]) == {0, 1, 50, 127, 128, 129, 1 << 30, (1 << 31) - 1}
        assert {1, NMAX} <= set(N[rows])
        parts, chunk = plan[rows, 3].astype(np.int64), plan[rows, 4].astype(np.int64)
        Nk, ok, limit = N[rows], opt[rows], np.array([_max_parts(kd, int(k)) for k in kp[rows]])
        live = Nk > 0
        assert (parts[live] <= limit[live]).all() and (parts[live] == -(-Nk[live] // chunk[live])).all()
        given = live & (ok > 0)
        assert (given & (chunk == ok)).any()                                              # the option as it stands
        raised = given & (chunk > ok)                                                     # the part limit raised it: to a tile multiple
        assert raised.any() and (chunk[raised] % TILE[kd] == 0).all() and (-(-Nk[raised] // ok[raised]) > limit[raised]).all()
        assert (given & (chunk == CLAMP) & (ok > CLAMP)).any()                            # the clamp
        own = live & (ok == 0)
        # the plan's own chunk: a tile multiple; one tile up to tile x want rows, two tiles one row later
        assert (chunk[own] % TILE[kd] == 0).all() and {TILE[kd], 2 * TILE[kd]} <= set(chunk[own].tolist())
        one = own & (chunk == TILE[kd])
        assert ((Nk + 1)[one][:, None] == Nk[own & (chunk == 2 * TILE[kd])][None, :]).any()
