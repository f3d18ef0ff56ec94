#!/usr/bin/env python3
"""avae_affinity: the time of a call and of one iteration beside scikit-learn's AffinityPropagation on the host.

    TIME     one call (similarities, median, every enqueued round, labels), HIP events after a warm-up call, median (min .. max) of
             `runs` calls, at
               test set   1900 x 1024, euclidean and cosine   (the reference's test set: src/eval_clustering_explorative.py:83-103)
               corpus     8192 x 128, euclidean
             Rows: Gaussian noise around planted centres.  The call enqueues 3 launches per round for all max_iter = 200 rounds;
             after the stop a launch returns at once.
    ITER     (time of a call with max_iter = 60 - time with max_iter = 20) / 40, convergence_iter = max_iter so that neither stops
             early: the time of one live iteration, three kernel boundaries included
    SETUP    the call with max_iter = 1: similarities, median select, diagonal, labels
    BYTES    per live iteration the kernels read or write 8 matrices of 4 N^2 bytes (rows: A, S; S, R, R'; availabilities: R, A, A')
    HOST     sklearn.cluster.AffinityPropagation(affinity='precomputed', max_iter=200, random_state=0) on the SAME S, wall clock on
             this machine's cores; where sklearn does not import, the fp32 numpy emulation of tests/ap_ref.py

    python scripts/affinity_bench.py [--runs 5] > profiles/affinity_bench.txt
"""
import argparse
import ctypes as C
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dev_affinity(m, x, out, **kw):
    """the C entry on device tensors; nothing copied"""
    from argsim_amd import lib
    cfg = lib.AvaeAffinityConfig(metric=kw.get('metric', 0), max_iter=kw.get('max_iter', 200), convergence_iter=kw.get('convergence_iter', 15),
                                 use_preference=0, noise=kw.get('noise', 1), warm=0, damping=0.5, preference=0.0, seed=0)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    m._stream()
    m._ck(m._l.avae_affinity(m._h, p(x), x.shape[0], x.shape[1], C.byref(cfg), p(out['label']), p(out['stat']), p(out.get('s')), None, None))


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


def rows(n, dim, k, seed):
    r = np.random.default_rng(seed)
    return (r.standard_normal((n, dim)) + 1.5 * r.standard_normal((k, dim))[r.integers(0, k, n)]).astype(np.float32)


def fmt(t):
    return "%9.2f ms (%.2f .. %.2f)" % t


def host(S, runs):
    try:
        from sklearn.cluster import AffinityPropagation
        name = 'sklearn AffinityPropagation'

        def fn():
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                ap = AffinityPropagation(affinity='precomputed', max_iter=200, random_state=0).fit(S.astype(np.float64))
            return ap.n_iter_, len(ap.cluster_centers_indices_)
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import ap_ref
        name = 'fp32 numpy (tests/ap_ref.py)'

        def fn():
            res = ap_ref.run(S, one=ap_ref.step_fp32)
            return res['n_iter'], res['K']
    s = []
    for _ in range(runs):
        t = time.perf_counter()
        it, K = fn()
        s.append((time.perf_counter() - t) * 1e3)
    return name, (float(np.median(s)), min(s), max(s)), it, K


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--host-runs', type=int, default=1)
    ap.add_argument('--skip-host', action='store_true')
    A = ap.parse_args(argv)
    from argsim_amd.model import VAE
    m = VAE('infer', dim_tgt=32, dim_emb=16, dim_rep=8, rnn_layers=1)
    print("# avae_affinity on %s, torch %s; host baseline on %d cores" % (torch.cuda.get_device_name(0), torch.__version__, len(os.sched_getaffinity(0))))
    for name, n, dim, metric in (('test set', 1900, 1024, 0), ('test set', 1900, 1024, 1), ('corpus', 8192, 128, 0)):
        dx = torch.as_tensor(rows(n, dim, 40, 3)).cuda()
        out = dict(label=torch.zeros(n, dtype=torch.int32, device='cuda'), stat=torch.zeros(4, dtype=torch.int32, device='cuda'),
                   s=torch.zeros((n, n), dtype=torch.float32, device='cuda'))
        call = timed(lambda: dev_affinity(m, dx, out, metric=metric), A.runs)
        stat = out['stat'].cpu().numpy()
        t60 = timed(lambda: dev_affinity(m, dx, out, metric=metric, max_iter=60, convergence_iter=60), A.runs)
        t20 = timed(lambda: dev_affinity(m, dx, out, metric=metric, max_iter=20, convergence_iter=20), A.runs)
        t1 = timed(lambda: dev_affinity(m, dx, out, metric=metric, max_iter=1, convergence_iter=1), A.runs)
        per = (t60[0] - t20[0]) / 40
        nbytes = 8 * 4 * n * n
        print("%-8s %5d x %4d %-9s | call %s: %d iterations, K %d, converged %d, %d launches enqueued | live iteration %.3f ms (%.1f MB: %.2f TB/s) | "
              "setup + labels %s" % (name, n, dim, ('euclidean', 'cosine')[metric], fmt(call), stat[0], stat[2], stat[1], 3 * 200 + 14, per,
                                     nbytes / 1e6, nbytes / per / 1e9, fmt(t1)))
        if not A.skip_host:
            dev_affinity(m, dx, out, metric=metric, max_iter=1, convergence_iter=1)
            S = out['s'].cpu().numpy()
            hname, ht, it, K = host(S, A.host_runs)
            print("         host, the same S: %s %s: %d iterations, K %d" % (hname, fmt(ht), it, K))
        sys.stdout.flush()
        del dx, out
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
