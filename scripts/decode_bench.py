"""greedy decoding, steps = 512 (explore_centroids.py:40): persistent launch vs one launch sequence per token.
--sample adds sampled decoding (temperature 1, top_k 0 and 40, then the nucleus top_p 0.9 alone and after top_k 40) at the same batch
sizes on both paths.
--beam instead: beam search at (b, width) = (1, 4), (16, 4), (1, 16) against the launch-per-token greedy loop (persistent = 0) at
b * width rows -- the same decoder work without select and gather -- in us per step, HIP events, three runs each (median, min - max)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from argsim_amd.model import VAE
m = VAE('infer', seed=2, dim_tgt=8192, dim_emb=512, dim_rep=128, rnn_layers=3)
steps = 512


def beam_table():
    import ctypes as C
    from argsim_amd import lib

    def timed(call):
        call()                                              # warm-up: workspace and scratch grow here
        ms, n = [], 0
        for _ in range(3):
            a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(torch.cuda.current_stream(m.device))
            n = call()
            b_.record(torch.cuda.current_stream(m.device))
            b_.synchronize()
            ms.append(a.elapsed_time(b_))
        us = sorted(1e3 * t / max(n, 1) for t in ms)
        return n, us

    m.set_option('persistent', 0)
    for b, W in ((1, 4), (16, 4), (1, 16)):
        z = torch.as_tensor(np.random.default_rng(b).standard_normal((b * W, 128)).astype(np.float32)).to(m.device)
        out = torch.empty((b * W, steps), dtype=torch.int32, device=m.device)
        n = C.c_int32()
        bc = lib.AvaeBeamConfig(W, 0.0)
        m._stream()

        def greedy():
            m._ck(m._l.avae_decode_greedy(m._h, C.c_void_p(z.data_ptr()), b * W, steps, C.c_void_p(out.data_ptr()), C.byref(n)))
            return steps if n.value == steps else min(steps, (n.value // 16 + 1) * 16)      # steps LAUNCHED: the loop checks every 16 tokens

        def beam():
            m._ck(m._l.avae_decode_beam(m._h, C.c_void_p(z.data_ptr()), b, steps, C.byref(bc), C.c_void_p(out.data_ptr()),
                                        None, None, None, None, None, None, C.byref(n)))
            return min(steps, -(-n.value // 16) * 16)
        ng, g = timed(greedy)
        nb, w = timed(beam)
        print('b %3d width %2d (%4d rows)  greedy per-token %.1f us/step (%.1f - %.1f, %d steps)  beam %.1f us/step (%.1f - %.1f, %d steps)  ratio %.2f' %
              (b, W, b * W, g[1], g[0], g[2], ng, w[1], w[0], w[2], nb, w[1] / g[1]), flush=True)


if '--beam' in sys.argv[1:]:
    beam_table()
    sys.exit(0)
legs = [('greedy', lambda z: m.decode(z, steps=steps))]
if '--sample' in sys.argv[1:]:
    for k in (0, 40):
        legs.append(('sample k=%d' % k, lambda z, k=k: m.sample(z, steps=steps, temperature=1.0, top_k=k, seed=1)))
    for k in (0, 40):
        legs.append(('k=%d p=0.9' % k, lambda z, k=k: m.sample(z, steps=steps, temperature=1.0, top_k=k, seed=1, top_p=0.9)))
for b in (1, 16, 64, 128):
    z = np.random.default_rng(b).standard_normal((b, 128)).astype(np.float32)
    for mode in (1, 0):
        m.set_option('persistent', mode)
        for name, run in legs:
            y = run(z)
            t0 = time.perf_counter()
            y = run(z)
            dt = time.perf_counter() - t0
            print('b %4d  %-10s %-11s tokens kept %4d  %.1f ms  %.1f us/token-step  %.0f tokens/s' %
                  (b, 'persistent' if mode else 'stepwise', name, y.shape[1], dt * 1e3, dt * 1e6 / max(y.shape[1], 1), b * y.shape[1] / dt), flush=True)
