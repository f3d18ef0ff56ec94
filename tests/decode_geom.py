"""The geometries of the one-launch decoding kernel (csrc/decode.hip) that tests/test_gpu_decode_geom.py runs, and what each of them reaches.

decode_plan (csrc/decode.hip) chooses per launch: nu = ceil(D / G) hidden units and vp = ceil(V / G) vocabulary rows per workgroup, cache_e =
the workgroup's embedding rows lie in LDS behind the weights (else the logits phase reads E from global memory), and refuses where the weights
alone exceed the LDS; decode_route (csrc/generate.cpp) puts the option "persistent", the batch limit and that refusal in front of it.  The three
geometries of the older decoding tests (OLD below) all take cache_e = 1, V below G or a multiple of it, and L = 3.  Every Case here claims a `reach`
per mode, (route, nu, vp, cache_e) at G = 256 workgroups and 160 KB of LDS; tests/test_decode_plan.py holds the claims against
avae_debug_decode_plan -- the functions the library itself decides with -- without a GPU, tests/test_gpu_decode_geom.py asks again for the device
it runs on.  route: 0 one launch, 1 one launch sequence per token by option or batch, 2 the same because the geometry is refused.

Parameters are built as tests/test_gpu_sampling.py builds them: oracle.vae_numpy.init_params rounded through fp32, decode/out/kernel and
decode/out/bias scaled so that the first step's max |logit| is 8; eos_lean adds that much of the unit eos embedding to the out bias, so that rows
end early.  numpy only: no GPU is needed to import this module or to call params()."""
import dataclasses

import numpy as np

from oracle import vae_numpy as vn

G_REF, LDS_REF = 256, 160 * 1024          # an MI355X: 256 CUs, one workgroup may own the CU's 160 KB
STEPS = 12
DIM_REP = 64
ROWS = 33                                 # latent rows per case: b = 33 is the first batch the per-token loop takes

# name -> sampled (0: avae_decode_greedy), temperature, top_k, top_p, and the kMode of the launch where top_k < V <= 8192
MODES = {
    'greedy': dict(sampled=0, T=0.0, k=0, p=0.0, kmode=0),
    'sampled': dict(sampled=1, T=0.7, k=0, p=0.0, kmode=1),
    'topk': dict(sampled=1, T=1.0, k=8, p=0.0, kmode=2),
    'nucleus': dict(sampled=1, T=1.0, k=0, p=0.9, kmode=3),
    'topk-nucleus': dict(sampled=1, T=1.0, k=40, p=0.9, kmode=3),
}
MODE_NAMES = tuple(MODES)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    D: int
    L: int
    V: int
    reach: dict                           # mode -> (route, nu, vp, cache_e) at G_REF, LDS_REF, persistent, b <= 32
    blocks: tuple                         # (first empty vocabulary block or G_REF, rows of the last non-empty block)
    batches: tuple = (17,)                # 17: the first batch at which a wave takes a second row pass (16 waves), mostly idle
    eos_lean: float = 0.0
    pseed: int = 4                        # parameters
    zseed: int = 11                       # latent rows
    seed: int = 1                         # the sampler's
    what: str = ''


def _all(r):
    return {m: r for m in MODE_NAMES}


def _by(plain, select):
    """greedy and sampled reach `plain`, the three modes with a select scratch `select`"""
    return {m: (plain if MODES[m]['kmode'] < 2 else select) for m in MODE_NAMES}


CASES = [
    Case('nocache', 512, 4, 8192, _all((0, 2, 32, 0)), (256, 32), batches=(1, 17, 32),
         what='the embedding block does not fit behind four layers of weights: every mode reads E from global memory, sel lies straight behind Kl'),
    Case('cache-by-mode', 512, 4, 7172, _by((0, 2, 29, 1), (0, 2, 29, 0)), (248, 9), eos_lean=6.0,
         what='vp = 29 is no multiple of 8; the select scratch of top-k and nucleus pushes the embedding block out; block 247 holds 9 rows, 248.. none'),
    Case('deep', 512, 6, 8192, _all((0, 2, 32, 0)), (256, 32),
         what='the largest L that launches at D = 512: 148 KB of weights'),
    Case('refused', 512, 7, 512, _all((2, 2, 2, 0)), (256, 2),
         what='the weights alone exceed the LDS: the per-token loop in every mode'),
    Case('bigv', 512, 3, 12288, _by((0, 2, 48, 0), (2, 0, 0, 0)), (256, 48),
         what='greedy and sampled in one launch without the cache; the row owner of top-k / nucleus holds 8192 ids at most: per token'),
    Case('d256', 256, 8, 8192, _all((0, 1, 32, 1)), (256, 32),
         what='nu = 1 with every workgroup owning a unit, the largest L'),
    Case('d256-ragged', 256, 1, 1000, _all((0, 1, 4, 1)), (250, 4),
         what='L = 1, vp = 4: half an eight-row pass, blocks 250.. empty'),
    Case('d128', 128, 2, 300, _all((0, 1, 2, 1)), (150, 2),
         what='half the workgroups own no unit, lanes 32.. idle in every dot product, blocks 150.. empty'),
    Case('d32', 32, 1, 20, _all((0, 1, 1, 1)), (20, 1),
         what='V < G; top_k 40 >= V keeps everything: the nucleus runs over all of V (alone, top_k 40 would be kMode 1)'),
]
BY_NAME = {c.name: c for c in CASES}
# the geometries of test_gpu_sampling / test_gpu_nucleus / test_gpu_beam / test_gpu_round2 / test_gpu_parity: (D, L, V)
OLD = {'tiny': (16, 3, 32), 'mid': (64, 3, 256), 'production': (512, 3, 8192)}


def kmode(c, mode):
    """the kMode decode_mode answers for the case: -1 where top-k or the nucleus meet more than 8192 ids, top_k >= V keeps everything"""
    m = MODES[mode]
    if not m['sampled']:
        return 0
    if m['p'] > 0.0:
        return -1 if c.V > 8192 else 3
    if m['k'] == 0 or m['k'] >= c.V:
        return 1
    return -1 if c.V > 8192 else 2


def budget(mode_k, D, V, L, G=G_REF, lds_max=LDS_REF):
    """the LDS budget of a launch, restated from the comment on decode_plan (csrc/decode.hip) -> (ok, nu, vp, cache_e, lds_bytes):
    4 bytes x (L x nu x 6 x D gate rows + nu x D columns of the out affine), 64 bytes to spare, 2048 / 3584 bytes of select scratch in
    kMode 2 / 3; the vp x D embedding rows join them where 1 KB of the LDS stays free with them"""
    if mode_k < 0:
        return (0, 0, 0, 0, 0)
    nu, vp = -(-D // G), -(-V // G)
    if nu > 2 or L > 8 or D % 4 or D > 512:
        return (0, nu, vp, 0, 0)
    weights = 4 * (L * nu * 6 * D + nu * D)
    fixed = 64 + {0: 0, 1: 0, 2: 2048, 3: 3584}[mode_k]
    cache_e = int(weights + 4 * vp * D + fixed <= lds_max - 1024)
    lds = weights + fixed + (4 * vp * D if cache_e else 0)
    return (int(lds <= lds_max), nu, vp, cache_e, lds)


def hook_ints(c, mode, b, persistent=1, G=G_REF, lds_max=LDS_REF):
    """avae_debug_decode_plan's ten inputs for a case (a Case or a (D, L, V) triple); G = lds_max = 0 asks the current device"""
    D, L, V = (c.D, c.L, c.V) if isinstance(c, Case) else c
    m = MODES[mode]
    return [m['sampled'], D, V, L, b, m['k'], int(m['p'] > 0.0), persistent, G, lds_max]


PLAN_FIELDS = ('route', 'kmode', 'ok', 'nu', 'vp', 'cache_e', 'lds_bytes', 'G', 'lds_max')


def ask(l, ints):
    """avae_debug_decode_plan -> dict of PLAN_FIELDS"""
    import ctypes as C
    out = (C.c_int64 * 9)()
    rc = l.avae_debug_decode_plan((C.c_int64 * 10)(*ints), out)
    assert rc == 0, (rc, ints)
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


DECODER_KEYS = ('embed/embedding', 'latent/ex/kernel', 'latent/ex/bias', 'decode/out/kernel', 'decode/out/bias')
_PARAMS = {}


def first_logits(P, cfg, z):
    D, L = cfg['dim_emb'], cfg['rnn_layers']
    E = P['embed/embedding']
    h0 = np.asarray(z, np.float64) @ P['latent/ex/kernel'] + P['latent/ex/bias']
    hd, _ = vn.decoder_rnn(P, cfg, E[np.full((1, len(z)), cfg['bos'], np.int32)], np.stack([h0] * L))
    hd = hd.reshape(-1, D) @ P['decode/out/kernel'] + P['decode/out/bias']
    return hd @ ((D ** -0.5) * E.T)


def params(c):
    """(cfg, P, z (ROWS, DIM_REP) float32) of a case; P holds what decoding reads (the embedding, latent/ex, decode/*) as float64 values
    that are exact in fp32"""
    if c.name not in _PARAMS:
        cfg = vn.make_cfg(dim_tgt=c.V, dim_emb=c.D, dim_rep=DIM_REP, rnn_layers=c.L)
        P = {k: v.astype(np.float32).astype(np.float64) for k, v in vn.init_params(cfg, c.pseed, bias_scale=0.1).items()
             if k in DECODER_KEYS or k.startswith('decode/rnn/')}
        z = np.random.default_rng(c.zseed).standard_normal((ROWS, DIM_REP)).astype(np.float32)
        f = 8.0 / float(np.abs(first_logits(P, cfg, z)).max())
        for k in ('decode/out/kernel', 'decode/out/bias'):
            P[k] = (P[k] * f).astype(np.float32).astype(np.float64)
        if c.eos_lean:
            e = P['embed/embedding'][cfg['eos']]
            P['decode/out/bias'] = (P['decode/out/bias'] + c.eos_lean * np.sqrt(c.D) * e / (e @ e)).astype(np.float32).astype(np.float64)
        _PARAMS[c.name] = (cfg, P, z)
    return _PARAMS[c.name]
