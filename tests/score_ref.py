"""float64 reference of the importance-weighted sentence likelihood (include/argsim_vae.h, avae_score / avae_score_z): numpy only.

The generator (stream 4 of the counter generator: mix64, the 24-bit uniform, Box-Muller) is restated in uint64 / float64
arithmetic; the model pieces are oracle.vae_numpy's encoder, decoder_rnn and the decoder mask of prep_decoder_io without a
keep mask."""
import numpy as np

import sampling_ref as sr
from oracle import vae_numpy as vn

M64 = sr.M64
STREAM = 4 * 0xD6E8FEB86659FD93 & M64


def uniforms(seed, r, k, R):
    """(u1, u2) (R,) of row r, draw k: ((x >> 40) + 0.5) 2^-24 of the 64-bit draws at 2 idx and 2 idx + 1 -- exact in float64"""
    assert 0 <= k < 1 << 20 and R <= 1 << 20
    key = sr.mix64(np.array([(int(seed) ^ STREAM) & M64], np.uint64))
    idx = np.uint64((((int(r) << 20) + int(k)) << 20) & M64) + np.arange(R, dtype=np.uint64)
    with np.errstate(over='ignore'):
        x1, x2 = sr.mix64(key + np.uint64(2) * idx), sr.mix64(key + np.uint64(2) * idx + np.uint64(1))
    u = lambda x: ((x >> np.uint64(40)).astype(np.float64) + 0.5) * 2.0 ** -24
    return u(x1), u(x2)


def eps(seed, r, k, R):
    """the R standard normal draws of row r, draw k: sqrt(-2 log u1) cos(2 pi u2) in float64.  The device rounds u to fp32 first
    ((x >> 40) + 0.5 is no fp32 number above 2^23): so does this."""
    u1, u2 = uniforms(seed, r, k, R)
    u1, u2 = u1.astype(np.float32).astype(np.float64), u2.astype(np.float32).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def eps_all(seed, k, B, R):
    return np.stack([np.stack([eps(seed, r, kk, R) for r in range(B)]) for kk in range(k)])


def encode(P, cfg, src):
    """valid-mode mu, lv (B, R) of src (B, S') eos-padded"""
    src_tm, _, len_src = vn.trim(np.asarray(src).T, cfg['eos'])
    _, h = vn.encoder(P, cfg, src_tm, len_src)
    return h @ P['latent/mu/kernel'] + P['latent/mu/bias'], h @ P['latent/lv/kernel'] + P['latent/lv/bias']


def score_z(P, cfg, z, tgt):
    """teacher-forced log p(tgt row | z row): (logpx (b,), ntok (b,)).  lead = [bos] + tgt, no word dropout; the positions the
    decoder mask keeps: position 0 and every position whose preceding target id is not eos"""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    D, L = cfg['dim_emb'], cfg['rnn_layers']
    tgt = np.asarray(tgt)
    tgt_tm = tgt.T
    not_eos = tgt_tm != cfg['eos']
    lead, gold, msk = vn.prep_decoder_io(tgt_tm, not_eos, cfg, None)
    E = P['embed/embedding']
    h0 = np.asarray(z, np.float64) @ P['latent/ex/kernel'] + P['latent/ex/bias']
    hd, _ = vn.decoder_rnn(P, cfg, E[lead], np.stack([h0] * L))
    T, b = lead.shape
    hd = hd.reshape(-1, D) @ P['decode/out/kernel'] + P['decode/out/bias']
    logits = hd @ ((D ** -0.5) * E.T)
    mx = logits.max(-1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(logits - mx).sum(-1))
    ce = (lse - logits[np.arange(T * b), gold.reshape(-1)]).reshape(T, b)
    return -(ce * msk).sum(0), msk.sum(0).astype(np.int32)


def latent_term(mu, lv, e):
    """1/2 sum_j (z^2 - eps^2 - lv) for e (k, B, R): -(log p(z) - log q(z | x)), the log 2 pi terms cancelled"""
    z = mu[None] + np.exp(0.5 * lv)[None] * e
    return 0.5 * (z * z - e * e - lv[None]).sum(-1)


def log_mean_exp(logw):
    """over axis 0, the maximum subtracted"""
    logw = np.asarray(logw, np.float64)
    m = logw.max(0)
    return m + np.log(np.exp(logw - m).sum(0)) - np.log(logw.shape[0])


def score(P, cfg, src, tgt, e):
    """e (k, B, R) -> dict logpx (k, B), logw (k, B), bound (B,), ntok (B,), mu, lv"""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    e = np.asarray(e, np.float64)
    k, B, R = e.shape
    mu, lv = encode(P, cfg, src)
    z = mu[None] + np.exp(0.5 * lv)[None] * e
    # the k draws as rows of one decoder batch
    logpx, ntok = score_z(P, cfg, z.reshape(k * B, R), np.tile(np.asarray(tgt), (k, 1)))
    logpx, ntok = logpx.reshape(k, B), ntok.reshape(k, B)[0]
    logw = logpx - latent_term(mu, lv, e)
    return dict(logpx=logpx, logw=logw, bound=log_mean_exp(logw), ntok=ntok, mu=mu, lv=lv)
