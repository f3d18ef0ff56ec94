"""The case table of tests/decode_geom.py against the library's own decision (avae_debug_decode_plan: decode_route, decode_mode and decode_plan,
the functions decode_loop and the launchers of csrc/decode.hip themselves go by) at G = 256 workgroups and 160 KB of LDS -- the proof that the
geometries of tests/test_gpu_decode_geom.py reach the branches they are meant to reach.  Host arithmetic only: no GPU."""
import ctypes as C

import pytest

import decode_geom as dg


def _lib():
    from argsim_amd import lib
    return lib, lib.load()


def plan(l, c, mode, b=17, **kw):
    return dg.ask(l, dg.hook_ints(c, mode, b, **kw))


def test_the_hook_is_exported_and_typed_and_not_public():
    lib, l = _lib()
    assert 'avae_debug_decode_plan' in lib.SIGNATURES and hasattr(l, 'avae_debug_decode_plan')
    assert lib.SIGNATURES['avae_debug_decode_plan'] == (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int64)])
    assert 'avae_debug_decode_plan' not in open(lib.CSRC + '/../../include/argsim_vae.h').read()
    out = (C.c_int64 * 9)()
    assert l.avae_debug_decode_plan(None, out) != 0
    for bad in ((1, 0, 32, 3), (1, 16, 0, 3), (1, 16, 32, 0), (1, 16, 32, 3, 0), (1, 16, 32, 3, 4, -1)):      # D, V, L, b < 1; top_k < 0
        ints = dg.hook_ints((16, 3, 32), 'topk', 4)
        for i, v in enumerate(bad[1:], 1):
            ints[i] = v
        assert l.avae_debug_decode_plan((C.c_int64 * 10)(*ints), out) != 0, bad


def test_the_table_is_well_formed():
    assert len({c.name for c in dg.CASES}) == len(dg.CASES)
    for c in dg.CASES:
        assert set(c.reach) == set(dg.MODE_NAMES) and 17 in c.batches and max(c.batches) <= 32, c.name
        assert c.V % 4 == 0 and c.D in (32, 128, 256, 512) and 1 <= c.L <= 8, c.name        # what avae_create takes
    assert sum(c.eos_lean != 0.0 for c in dg.CASES) == 1
    assert dg.BY_NAME['nocache'].batches == (1, 17, 32)


@pytest.mark.parametrize("c", dg.CASES, ids=lambda c: c.name)
def test_every_case_reaches_the_form_it_claims(c):
    lib, l = _lib()
    for mode in dg.MODE_NAMES:
        for b in c.batches:
            p = plan(l, c, mode, b)
            assert (p['route'], p['nu'], p['vp'], p['cache_e']) == c.reach[mode], (c.name, mode, b, p)
            assert p['kmode'] == dg.kmode(c, mode), (c.name, mode, p)
            assert (p['G'], p['lds_max']) == (dg.G_REF, dg.LDS_REF)
            # the budget, restated from the comment on decode_plan
            ok, nu, vp, cache_e, lds = dg.budget(p['kmode'], c.D, c.V, c.L)
            assert (p['ok'], p['nu'], p['vp'], p['cache_e'], p['lds_bytes']) == (ok, nu, vp, cache_e, lds), (c.name, mode, p)
            assert p['route'] == (0 if ok else 2) and (not ok or lds <= dg.LDS_REF)
    # the vocabulary blocks the table speaks of
    vp = -(-c.V // dg.G_REF)
    first_empty = -(-c.V // vp)
    assert (first_empty, c.V - (first_empty - 1) * vp) == c.blocks, c.name


def test_what_the_cases_are_there_for():
    """one assertion per line of the table's `what`"""
    lib, l = _lib()
    R = lambda name, mode: dg.BY_NAME[name].reach[mode]
    assert all(R('nocache', m) == (0, 2, 32, 0) for m in dg.MODE_NAMES)
    assert [R('cache-by-mode', m)[3] for m in dg.MODE_NAMES] == [1, 1, 0, 0, 0] and R('cache-by-mode', 'topk')[2] % 8 == 5
    assert all(R('deep', m)[0] == 0 and R('deep', m)[3] == 0 for m in dg.MODE_NAMES)
    assert all(R('refused', m)[0] == 2 for m in dg.MODE_NAMES)
    assert [R('bigv', m)[0] for m in dg.MODE_NAMES] == [0, 0, 2, 2, 2] and R('bigv', 'sampled') == (0, 2, 48, 0)
    assert R('d256', 'greedy')[1] == 1 and dg.BY_NAME['d256'].D == dg.G_REF and dg.BY_NAME['d256'].L == 8
    assert dg.BY_NAME['d256-ragged'].L == 1 and R('d256-ragged', 'greedy')[2] == 4 and dg.BY_NAME['d256-ragged'].blocks[0] == 250
    assert dg.BY_NAME['d128'].D * 2 == dg.G_REF and dg.BY_NAME['d128'].blocks == (150, 2)
    c = dg.BY_NAME['d32']
    assert c.V < dg.G_REF and dg.MODES['topk-nucleus']['k'] >= c.V and dg.MODES['topk']['k'] < c.V
    ints = dg.hook_ints(c, 'topk-nucleus', 17)
    ints[6] = 0                                          # top_k 40 alone: every logit is kept, kMode 1
    assert dg.ask(l, ints)['kmode'] == 1
    # every form of the launch is run by some case: (nu, cache_e) per kMode, an odd vp, empty blocks, every accepted extreme of L
    seen = {(dg.kmode(c, m),) + c.reach[m][1:] for c in dg.CASES for m in dg.MODE_NAMES if c.reach[m][0] == 0}
    for k in range(4):           # (two units with the cache and a select scratch is the production geometry of the older tests)
        assert {(nu, ce) for (km, nu, vp, ce) in seen if km == k} >= ({(1, 1), (2, 1), (2, 0)} if k < 2 else {(1, 1), (2, 0)}), k
    assert {c.L for c in dg.CASES if c.reach['greedy'][0] == 0} >= {1, 2, 3, 4, 6, 8}


def test_the_boundaries_around_the_cases():
    lib, l = _lib()
    for mode in dg.MODE_NAMES:
        # D = 512: six layers launch, seven do not (at any vocabulary: the weights alone)
        for V in (512, 8192):
            assert plan(l, (512, 6, V), mode)['route'] == 0 and plan(l, (512, 7, V), mode)['route'] == 2
            assert plan(l, (512, 7, V), mode)['ok'] == 0 and plan(l, (512, 7, V), mode)['lds_bytes'] > dg.LDS_REF
        assert plan(l, (256, 8, 8192), mode)['route'] == 0
        # V = 7168 is 28 rows per workgroup, four more ids make it 29
        assert plan(l, (512, 4, 7168), mode)['vp'] == 28 and plan(l, (512, 4, 7172), mode)['vp'] == 29
        # the batch limit and the option come first, whatever the geometry
        for c in dg.CASES:
            assert plan(l, c, mode, 32)['route'] == c.reach[mode][0]
            assert plan(l, c, mode, 33)['route'] == 1 and plan(l, c, mode, 17, persistent=0)['route'] == 1
    # the cache flips between V = 7168 and 7172 only where the select scratch is there ... and with the fifth layer in every mode
    assert [plan(l, (512, 4, 7168), m)['cache_e'] for m in dg.MODE_NAMES] == [1, 1, 1, 0, 0]
    assert [plan(l, (512, 3, 8192), m)['cache_e'] for m in dg.MODE_NAMES] == [1] * 5
    assert [plan(l, (512, 4, 8192), m)['cache_e'] for m in dg.MODE_NAMES] == [0] * 5
    # 8192 ids is the most a row's owner holds; one more block of four refuses top-k and the nucleus, not the other two
    assert [plan(l, (512, 3, 8196), m)['route'] for m in dg.MODE_NAMES] == [0, 0, 2, 2, 2]
    assert [plan(l, (512, 3, 8192), m)['route'] for m in dg.MODE_NAMES] == [0] * 5
    # a device with fewer CUs: more than two units per workgroup is refused; a smaller LDS loses the cache first, then the launch
    assert plan(l, (512, 3, 8192), 'greedy', G=255)['route'] == 2 and plan(l, (512, 3, 8192), 'greedy', G=256)['nu'] == 2
    p = plan(l, (512, 3, 8192), 'greedy', lds_max=128 * 1024)
    assert (p['route'], p['cache_e']) == (0, 0)
    assert plan(l, (512, 3, 8192), 'greedy', lds_max=64 * 1024)['route'] == 2


def test_the_older_geometries_all_cache_the_embedding():
    """what test_gpu_sampling, test_gpu_nucleus, test_gpu_beam, test_gpu_round2 and test_gpu_parity cover of this kernel: cache_e = 1, whole blocks, L = 3"""
    lib, l = _lib()
    for name, (D, L, V) in dg.OLD.items():
        for mode in dg.MODE_NAMES:
            for b in (1, 4, 5, 8, 32):
                p = plan(l, (D, L, V), mode, b)
                assert (p['route'], p['cache_e']) == (0, 1) and L == 3, (name, mode, b, p)
                assert V < dg.G_REF or V % dg.G_REF == 0
