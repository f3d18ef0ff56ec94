"""gemm_plan() (argsim_amd/csrc/gemm_plan.cpp) against the launch decisions of the commit that still made them inline in model.cpp.

tests/golden/gemm_plan_parent.npz was recorded from that commit (its hash is in the `parent` field), never from the code under test: its
gemm(), gemm_tn_grad(), grad_split() and dyn_expected() compiled as a host program with recorders in place of the launcher and the two
clearing kernels.  `inputs` holds GemmShape's fields in their order (names in `fields`), `plan` the launches the parent made -- count,
then per launch first row, rows, tile form, K slices, accumulate, what was cleared (0 nothing / 1 all / 2 the first *dyn rows), whether
the device-side count applied -- and `parent_return` which of the parent's return statements produced the row (informational).
Rows: every product of a training step at D 512, V 8192, R 128, L 3 for each compute_dtype (256 x 64 full and ragged at fill 0.44,
100 x 12, 1024 x 128, the decode step at 1 and 16 rows), every return of the parent three times or more, each option switched off
where that changes the plan, and the shapes one step either side of every threshold.  No GPU: host arithmetic of the library."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gemm_plan_parent.npz')


def _plan(inputs):
    from argsim_amd import lib
    l = lib.load()
    inputs = np.ascontiguousarray(inputs, dtype=np.int32)
    out = np.full((len(inputs), 15), -1, dtype=np.int32)
    assert l.avae_debug_gemm_plan(inputs.ctypes.data, len(inputs), out.ctypes.data) == 0
    return out


def test_gemm_plan_equals_the_parents_decisions():
    g = np.load(GOLDEN)
    assert str(g['parent']) == '9b102c2'
    inputs, want = g['inputs'], g['plan']
    assert inputs.dtype == np.int32 and want.dtype == np.int32 and inputs.shape[1] == 19 == len(g['fields']) and want.shape == (len(inputs), 15)
    got = _plan(inputs)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, [(dict(zip(map(str, g['fields']), inputs[i].tolist())), got[i].tolist(), want[i].tolist()) for i in bad[:5]]


def test_gemm_plan_table_covers_what_it_claims():
    """the table itself: every return of the parent at least three times, both two-launch tails, each clearing form, each option"""
    g = np.load(GOLDEN)
    f = {str(n): i for i, n in enumerate(g['fields'])}
    inputs, plan, ret = g['inputs'], g['plan'], g['parent_return']
    assert 2000 <= len(inputs) <= 4200
    assert ret.max() == 13 and np.bincount(ret, minlength=14)[1:].min() >= 3
    two = plan[:, 0] == 2
    assert two.any() and (plan[two, 1 + 7 + 5] == 1).any() and (plan[two, 1 + 7 + 5] == 0).any()      # the tail: cleared + split, or a thin form
    assert set(np.unique(plan[:, 1 + 5])) == {0, 1, 2}
    assert set(np.unique(inputs[:, f['compute_dtype']])) == {0, 1, 2}
    head = (inputs[:, f['M']] == 16640) & (inputs[:, f['N']] == 8192) & (inputs[:, f['K']] == 512)      # the headline's logits
    assert head.any() and (plan[head, 0] == 2).all()
    for opt in ('skinny', 'dyn_split', 'dyn_thin'):
        rows = {tuple(r): p for r, p in zip(inputs.tolist(), plan.tolist())}
        changed = 0
        for r, p in rows.items():
            if r[f[opt]] == 0:
                on = list(r)
                on[f[opt]] = 1
                changed += tuple(on) in rows and rows[tuple(on)] != p
        assert changed >= 3, opt
