#!/usr/bin/env python3
"""avae_dbscan: the time of a call on device-resident rows, beside scikit-learn's DBSCAN(algorithm='brute') on the host.

    TIME     one call (row norms for the cosine, the pair pass into the bit matrix, the rounds of hook and jump, verify, numbering, labels,
             statistics), HIP events after a warm-up call, median (min .. max) of `runs` calls, at
               test set   3000 x 128     (the reference's scale)
               bank       65536 x 128
               bank       131072 x 128   (the largest N: a 2 GiB bit matrix)
             euclidean, min_samples 5.  Rows: N / 512 Gaussian blobs (at least 6) and a tenth of uniform rows.  eps is read off the knee of
             the 4-distance curve (VAE.kdist): the point of the ascending curve farthest below the chord between its ends.  Beside it the
             plan, the rounds used and the bound of the pair arithmetic: N^2 dim pairs of (subtract, fused multiply-add) at 64
             double-precision vector instructions per CU and clock (256 CUs, 2.4 GHz).
    HOST     sklearn.cluster.DBSCAN(eps, min_samples=5, algorithm='brute', n_jobs=16) on the same rows as float64, wall clock on this
             machine's cores; the number of rows whose label differs is printed with it.  A host run estimated (from the shape before,
             quadratically) to take more than --host-limit seconds is left out and said so.
    The split between db_pairs and the rest comes from a run of its own under rocprofv3 --kernel-trace --stats (--runs 2 --skip-host).

    python scripts/dbscan_bench.py [--runs 5] > profiles/dbscan_bench.txt
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FMA_PER_S = 256 * 64 * 2.4e9      # double-precision vector instructions per second


def timed(fn, runs):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def rows(n, dim, seed):
    r = np.random.default_rng(seed)
    k = max(6, n // 512)
    x = r.standard_normal((n, dim)) + 3.0 * r.standard_normal((k, dim))[r.integers(0, k, n)]
    far = r.random(n) < 0.1
    x[far] = r.uniform(-8.0, 8.0, (int(far.sum()), dim))
    return x.astype(np.float32)


def knee(curve):
    """the point of an ascending curve farthest below the chord between its ends"""
    t = np.linspace(0.0, 1.0, len(curve))
    chord = curve[0] + (curve[-1] - curve[0]) * t
    return float(curve[int(np.argmax(chord - curve))])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--shapes', default='3000,65536,131072')
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--host-limit', type=float, default=240.0)
    A = ap.parse_args(argv)
    from argsim_amd import lib
    from argsim_amd.model import VAE
    m = VAE('infer', dim_tgt=32, dim_emb=16, dim_rep=8, rnn_layers=1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("# avae_dbscan on %s (%d CUs), torch %s, %s; host baseline on %d threads"
          % (torch.cuda.get_device_name(0), cus, torch.__version__, time.strftime('%Y-%m-%d'),
             int(os.environ.get('OMP_NUM_THREADS', len(os.sched_getaffinity(0))))))
    dim, ms = 128, 5
    last = None                                                 # (n, seconds) of the last host run
    for n in [int(v) for v in A.shapes.split(',')]:
        x = rows(n, dim, 3)
        dx = torch.as_tensor(x).cuda()
        t0 = time.perf_counter()
        eps = knee(m.kdist(dx, ms - 1))
        t_kd = (time.perf_counter() - t0) * 1e3
        label = torch.zeros(n, dtype=torch.int32, device='cuda')
        count = torch.zeros(n, dtype=torch.int32, device='cuda')
        stat = torch.zeros(8, dtype=torch.int32, device='cuda')
        cfg = lib.AvaeDbscanConfig(metric=0, min_samples=ms, max_rounds=0, reserved=0, eps=eps)
        p = lambda t: C.c_void_p(t.data_ptr())

        def call():
            m._stream()
            m._ck(m._l.avae_dbscan(m._h, p(dx), n, dim, C.byref(cfg), p(label), p(count), p(stat)))
        t = timed(call, A.runs)
        st = stat.cpu().numpy()
        plan = np.zeros(9, np.int32)
        m._l.avae_debug_dbscan_plan(n, dim, 0, cus, plan.ctypes.data_as(C.POINTER(C.c_int32)))
        bound = 2.0 * n * n * dim / FMA_PER_S * 1e3
        ws = (int(plan[7]) & 0xffffffff) | (int(plan[8]) << 32)
        print("%7d x %d eps %.4g (knee of the 4-distance curve, %.0f ms with the upload) | call %9.2f ms (%.2f .. %.2f) | TI %d, %d x %d workgroups, "
              "workspace %.1f MiB, pair bound %.3f ms: %.1f %% | clusters %d core %d border %d noise %d, rounds %d of %d enqueued, verify %d"
              % (n, dim, eps, t_kd, t[0], t[1], t[2], plan[0], plan[1], plan[2], ws / 2.0 ** 20, bound, 100 * bound / t[0], st[0], st[1], st[2], st[3],
                 st[4], plan[6], st[5]))
        sys.stdout.flush()
        if not A.skip_host:
            try:
                from sklearn.cluster import DBSCAN
            except ImportError:
                print("         host: scikit-learn is not installed on this machine; the device times stand alone")
                A.skip_host = True
                continue
            est = last[1] * (n / last[0]) ** 2 if last else 0.0
            if est > A.host_limit:
                print("         host: left out, estimated %.0f s from the shape before (limit %.0f s)" % (est, A.host_limit))
            else:
                X = x.astype(np.float64)
                t0 = time.perf_counter()
                sk = DBSCAN(eps=eps, min_samples=ms, algorithm='brute', n_jobs=16).fit(X)
                ht = time.perf_counter() - t0
                last = (n, ht)
                diff = int((sk.labels_ != label.cpu().numpy()).sum())
                print("         host, the same rows: sklearn DBSCAN(algorithm='brute', n_jobs=16) %9.2f ms; rows whose label differs %d; device / host time 1 : %.0f"
                      % (ht * 1e3, diff, ht * 1e3 / t[0]))
            sys.stdout.flush()
        del dx, label, count, stat
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
