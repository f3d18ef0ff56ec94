#!/usr/bin/env python3
"""avae_knn against torch.topk(q @ bank.T, k) on the same device, in the same process.

Rows are pre-normalised, so the yardstick's dot product IS the cosine; avae_knn runs metric cos and its time includes the
norms pass over the bank.  HIP events around `iters` back-to-back calls, `warmup` calls first, `runs` such measurements per
geometry: the median and the spread (min .. max) are printed, with the bank bytes streamed per second and the TFLOP/s of
2 n N dim.  The yardstick materialises the (n, N) panel.

    python scripts/knn_bench.py [--logN 20] [--runs 5] > profiles/knn_bench.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--logN', type=int, default=20)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--runs', type=int, default=5)
    A = ap.parse_args(argv)
    from argsim_amd.model import VAE
    m = VAE('infer', dim_tgt=32, dim_emb=16, dim_rep=8, rnn_layers=1)
    N, k = 1 << A.logN, A.k
    print("# avae_knn (metric cos, norms pass included) vs torch.topk(q @ bank.T, k); N = 2^%d = %d, k = %d; %d warm-up, %d x %d calls; "
          "ms = median (min .. max)" % (A.logN, N, k, A.warmup, A.runs, A.iters))
    print("# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    g = torch.Generator(device='cuda').manual_seed(0)
    for dim in (128, 1024):
        bank = torch.randn((N, dim), device='cuda', generator=g)
        bank /= bank.norm(dim=1, keepdim=True)
        for n in (1, 16, 256):
            q = torch.randn((n, dim), device='cuda', generator=g)
            q /= q.norm(dim=1, keepdim=True)
            ours = timed(lambda: m.neighbors(q, bank, k=k, metric='cos'), A.warmup, A.iters, A.runs)
            ref = timed(lambda: torch.topk(q @ bank.T, k), A.warmup, A.iters, A.runs)
            idx, sc = m.neighbors(q, bank, k=k, metric='cos')
            tv, ti = torch.topk(q @ bank.T, k)
            agree = float((idx == ti).float().mean())
            gbs = N * dim * 4 / (ours[0] * 1e-3) / 1e9
            tf = 2.0 * n * N * dim / (ours[0] * 1e-3) / 1e12
            print("dim %4d n %3d | knn %8.3f ms (%.3f .. %.3f)  bank %7.1f GB/s  %6.2f TFLOP/s | topk(q @ bank.T) %8.3f ms (%.3f .. %.3f) | "
                  "x%.2f | same indices %.4f" % (dim, n, ours[0], ours[1], ours[2], gbs, tf, ref[0], ref[1], ref[2], ref[0] / ours[0], agree))
            sys.stdout.flush()
        del bank
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
