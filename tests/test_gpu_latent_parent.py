"""the latent-row entries (avae_probe_fit, avae_probe_fit_l1, avae_probe_decision, avae_knn, avae_agg_logq, avae_latent_moments) give
the bits they gave before their host code and the shared pieces of probe.hip were folded into one part planner, one workspace placer
and one probe loop.

tests/golden/latent_parent_bits.npz holds the SHA-256 of every output array's bytes, recorded on an MI355X from a build of the
commit BEFORE that change (its hash is in the `parent` field), never from the code under test, by
tests/golden/make_latent_parent_bits.py, which runs digests() below.  Inputs: the case generators of probe_ref, probe_l1_ref, knn_ref
and agg_ref as they stand; every case once with the default plan and once with the family's chunk option at 50 (several parts, none a
multiple of the tile).  `input_names` / `input_digests` hold the same hash of every input array, so that a platform whose numpy
draws other inputs is told apart from a change of the device arithmetic.  Ward and affinity are held by their own exact-result tests.

A later change that alters this arithmetic ON PURPOSE re-records the file with that script from a build it has verified against its
own parent (every entry it did not mean to change still equal), stores that build's hash and names in its message what changed."""
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'latent_parent_bits.npz')
PARENT = 'b7888ab'
FAMILIES = ('probe', 'probe_l1', 'decision', 'knn', 'agg', 'moments')
CHUNK = 50


def _sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.dtype.str.encode() + repr(a.shape).encode() + a.tobytes()).hexdigest()


def _Plans(model, option):
    """the two plans of a case: the default one, then `option` at CHUNK on the model that runs the case"""
    yield 'default'
    model.set_option(option, CHUNK)
    try:
        yield 'chunk%d' % CHUNK
    finally:
        model.set_option(option, 0)


def _probe(out, inp):
    import probe_ref as pr
    import test_gpu_probe as tp
    for case, cid in zip(pr.CASES, pr.CASE_IDS):
        x, s = pr.case_inputs(case)
        inp['probe/%s/x' % cid], inp['probe/%s/s' % cid] = _sha(x), _sha(s)
        for plan in _Plans(tp._model(), 'probe_chunk'):
            w, st = tp._fit(x, s)
            out['probe/%s/%s/w' % (cid, plan)], out['probe/%s/%s/stats' % (cid, plan)] = _sha(w), _sha(st)


def _probe_l1(out, inp):
    import probe_l1_ref as pl
    import test_gpu_probe_l1 as tl
    for case in pl.GPU_CASES:
        cid = pl.CASE_ID(case)
        x, s = pl.case_inputs(case)
        inp['probe_l1/%s/x' % cid], inp['probe_l1/%s/s' % cid] = _sha(x), _sha(s)
        for plan in _Plans(tl._model(), 'probe_chunk'):
            w, st = tl._fit(x, s)
            out['probe_l1/%s/%s/w' % (cid, plan)], out['probe_l1/%s/%s/stats' % (cid, plan)] = _sha(w), _sha(st)


def _decision(out, inp):
    import probe_ref as pr
    import test_gpu_probe as tp
    for case, cid in zip(pr.CASES, pr.CASE_IDS):
        x, _ = pr.case_inputs(case)
        N, P, dim = case
        w = np.random.default_rng(4000 + dim).standard_normal((P, dim + 1)).astype(np.float32)      # (drawn, not fitted: the same on every host)
        inp['decision/%s/x' % cid], inp['decision/%s/w' % cid] = _sha(x), _sha(w)
        for plan in _Plans(tp._model(), 'probe_chunk'):
            out['decision/%s/%s/out' % (cid, plan)] = _sha(tp._decision(x, w))


def _knn(out, inp):
    import knn_ref as kr
    import test_gpu_knn as tk
    for case in kr.CASES:
        n, N, dim, k = case
        cid = 'n%d-N%d-d%d-k%d' % case
        q, bank = kr.case_inputs(case)
        inp['knn/%s/q' % cid], inp['knn/%s/bank' % cid] = _sha(q), _sha(bank)
        cut = N // 3 + 5
        for plan in _Plans(tk._model(), 'knn_chunk'):
            for metric in kr.METRICS:
                runs = {'plain': tk._knn(q, bank, k, metric), 'self': tk._knn(q, bank, k, metric, self_base=1)}
                first = tk._knn(q, bank[:cut], k, metric, self_base=1)
                runs['carry-self'] = tk._knn(q, bank[cut:], k, metric, idx_base=cut, self_base=1, carry=first)
                for name, (idx, sc) in runs.items():
                    out['knn/%s/%s/%s/%s/idx' % (cid, plan, metric, name)] = _sha(idx)
                    out['knn/%s/%s/%s/%s/score' % (cid, plan, metric, name)] = _sha(sc)


def _agg(out, inp):
    import agg_ref as ar
    import test_gpu_agg as ta
    for case in ar.CASES:
        for regime in ar.REGIMES:
            cid = 'n%d-N%d-d%d-%s' % (case + (regime,))
            z, mu, lv = ar.case_inputs(case, regime)
            inp['agg/%s/z' % cid], inp['agg/%s/mu' % cid], inp['agg/%s/lv' % cid] = _sha(z), _sha(mu), _sha(lv)
            for plan in _Plans(ta._model(), 'agg_chunk'):
                logq, logqx = ta._logq(z, mu, lv, self_base=0)
                out['agg/%s/%s/logq' % (cid, plan)], out['agg/%s/%s/logqx' % (cid, plan)] = _sha(logq), _sha(logqx)


def _moments(out, inp):
    import agg_ref as ar
    import test_gpu_agg as ta
    m = ta._model()
    for N in ar.MOMENT_N:
        for dim in ar.MOMENT_DIM:
            mu, lv = ar.moment_inputs(N, dim)
            inp['moments/N%d-d%d/mu' % (N, dim)], inp['moments/N%d-d%d/lv' % (N, dim)] = _sha(mu), _sha(lv)
            got = m.latent_moments(mu, lv)             # (avae_latent_moments has no plan option: one run)
            for key in ('mean', 'var', 'sigma2', 'kl_dim'):
                out['moments/N%d-d%d/%s' % (N, dim, key)] = _sha(got[key])


_RUN = {'probe': _probe, 'probe_l1': _probe_l1, 'decision': _decision, 'knn': _knn, 'agg': _agg, 'moments': _moments}


def digests(family):
    """-> (outputs, inputs): name -> SHA-256 of the array (dtype, shape and bytes) for one family of entries"""
    out, inp = {}, {}
    _RUN[family](out, inp)
    return out, inp


def _table(g, names, values, family):
    return {str(n): str(v) for n, v in zip(g[names], g[values]) if str(n).startswith(family + '/')}


@pytest.mark.parametrize('family', FAMILIES)
def test_outputs_equal_the_parents_bit_for_bit(family):
    g = np.load(GOLDEN)
    assert str(g['parent']) == PARENT
    out, inp = digests(family)
    want_in, want = _table(g, 'input_names', 'input_digests', family), _table(g, 'names', 'digests', family)
    assert inp == want_in, "the INPUTS differ from the recorded ones (numpy draws, not the device): %s" % sorted(k for k in set(inp) | set(want_in) if inp.get(k) != want_in.get(k))[:8]
    assert sorted(out) == sorted(want) and len(want) > 0
    bad = sorted(k for k in want if out[k] != want[k])
    assert not bad, "%d of %d outputs differ from the parent's: %s" % (len(bad), len(want), bad[:8])
