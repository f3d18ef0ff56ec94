#!/usr/bin/env python3
"""avae_agg_logq against torch restatements on the same device, in the same process.

n = N samples, one per encoded row (self_base 0), inputs of the peaked regime of tests/agg_ref.py (mu ~ N(0, 1), lv ~ U(-6, 1),
z drawn from its own row).  Two yardsticks:
    direct    the same arithmetic in torch, query rows in chunks whose (chunk, N, dim) panel is 256 MB:
              logsumexp(-1/2 (((z[:, None] - mu) ** 2 * a).sum(-1) + c))
    expanded  the two-GEMM form (z * z) @ a.T - 2 z @ (mu a).T + sum(mu^2 a), query rows in chunks whose (chunk, N) panel is
              256 MB -- the form the library does NOT use; its error is printed beside its time
HIP events around `iters` back-to-back calls, `warmup` calls first, `runs` such measurements: the median and the spread (min ..
max).  "floor" is the vector-ALU floor of the direct form, 3 packed fp32 instructions per pair and 2 dims at the fp32 vector
peak of 157.3 TFLOP/s (4 flops per lane of a packed fma): n N dim x 1.5 / 39.3e12 s.  err = max |x - float64| / max(1, |float64|)
over logq and logqx of the first 256 queries.

    python scripts/agg_bench.py [--runs 3] > profiles/agg_bench.txt
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_PK_LANES = 157.3e12 / 4.0


def timed(fn, warmup, iters, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return float(np.median(ms)), min(ms), max(ms)


def torch_direct(z, mu, lv, budget=256 << 20):
    N, dim = mu.shape
    a, c = torch.exp(-lv), lv.sum(1)
    step = max(1, budget // (4 * N * dim))
    cst = 0.5 * dim * math.log(2.0 * math.pi)
    logq, logqx = torch.empty(z.shape[0], device=z.device, dtype=z.dtype), torch.empty(z.shape[0], device=z.device, dtype=z.dtype)
    for i in range(0, z.shape[0], step):
        d = z[i:i + step, None, :] - mu[None]
        t = -0.5 * ((d * d * a[None]).sum(-1) + c[None])
        logq[i:i + step] = torch.logsumexp(t, 1) - math.log(N) - cst
        logqx[i:i + step] = t[torch.arange(t.shape[0]), torch.arange(i, i + t.shape[0])] - cst
    return logq, logqx


def torch_expanded(z, mu, lv, budget=256 << 20):
    N, dim = mu.shape
    a = torch.exp(-lv)
    ma, c = mu * a, lv.sum(1) + (mu * mu * a).sum(1)
    step = max(1, budget // (4 * N))
    cst = 0.5 * dim * math.log(2.0 * math.pi)
    logq, logqx = torch.empty(z.shape[0], device=z.device, dtype=z.dtype), torch.empty(z.shape[0], device=z.device, dtype=z.dtype)
    for i in range(0, z.shape[0], step):
        zc = z[i:i + step]
        t = -0.5 * ((zc * zc) @ a.T - 2.0 * (zc @ ma.T) + c[None])
        logq[i:i + step] = torch.logsumexp(t, 1) - math.log(N) - cst
        logqx[i:i + step] = t[torch.arange(t.shape[0]), torch.arange(i, i + t.shape[0])] - cst
    return logq, logqx


def err(got, ref):
    e = 0.0
    for g, r in zip(got, ref):
        g, r = g[:r.shape[0]].double(), r.double()
        e = max(e, float(((g - r).abs() / r.abs().clamp(min=1.0)).max()))
    return e


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--runs', type=int, default=3)
    A = ap.parse_args(argv)
    from argsim_amd.model import VAE
    m = VAE('infer', dim_tgt=32, dim_emb=16, dim_rep=8, rnn_layers=1)
    torch.backends.cuda.matmul.allow_tf32 = False
    print("# avae_agg_logq (n = N, self_base 0, logq and logqx) vs torch on the same device; peaked inputs; %d warm-up, %d x %d calls "
          "(torch direct: 1 x 1 at most); ms = median (min .. max)" % (A.warmup, A.runs, A.iters))
    print("# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    g = torch.Generator(device='cuda').manual_seed(0)
    for N, dim in ((8192, 128), (32768, 128), (8192, 1024)):
        mu = torch.randn((N, dim), device='cuda', generator=g)
        lv = torch.rand((N, dim), device='cuda', generator=g) * 7.0 - 6.0
        z = mu + torch.exp(0.5 * lv) * torch.randn((N, dim), device='cuda', generator=g)
        ours = timed(lambda: m.log_q(z, mu, lv, self_index=0), A.warmup, A.iters, A.runs)
        mom = timed(lambda: m.latent_moments(mu, lv), A.warmup, A.iters, A.runs)
        exp_t = timed(lambda: torch_expanded(z, mu, lv), A.warmup, A.iters, A.runs)
        big = N * N * dim > 1 << 35
        dir_t = timed(lambda: torch_direct(z, mu, lv), 1, 1, 1 if big else min(A.runs, 2))
        ref = torch_direct(z[:256].double(), mu.double(), lv.double(), budget=512 << 20)
        e_ours, e_dir, e_exp = err(m.log_q(z, mu, lv, self_index=0), ref), err(torch_direct(z[:256], mu, lv), ref), err(torch_expanded(z[:256], mu, lv), ref)
        floor = N * N * dim * 1.5 / PEAK_PK_LANES * 1e3
        print("N %5d dim %4d | agg_logq %8.3f ms (%.3f .. %.3f)  floor %.3f ms = %.1f %% of it  err %.2e | torch direct %9.3f ms (%.3f .. %.3f) x%.1f "
              "err %.2e | torch expanded %8.3f ms (%.3f .. %.3f) x%.2f err %.2e | latent_moments %.3f ms (%.3f .. %.3f) %.0f GB/s"
              % (N, dim, ours[0], ours[1], ours[2], floor, 100.0 * floor / ours[0], e_ours, dir_t[0], dir_t[1], dir_t[2], dir_t[0] / ours[0], e_dir,
                 exp_t[0], exp_t[1], exp_t[2], exp_t[0] / ours[0], e_exp, mom[0], mom[1], mom[2], 3 * N * dim * 4 / (mom[0] * 1e-3) / 1e9))
        sys.stdout.flush()
        del mu, lv, z, ref
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
