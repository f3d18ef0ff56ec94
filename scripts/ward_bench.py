#!/usr/bin/env python3
"""avae_ward: the time of a call in both kernel forms beside scipy and scikit-learn on the host, and whether the planner's threshold
between the forms (kWardOneWgMax = 128 rows in the largest group) is where the measurements put it.

    TIME     one call (init + every merge), HIP events after a warm-up call, median (min .. max) of `runs` calls, at
               topics     4 groups x 1250 x 1024   (the reference's test set by topic)
               whole      1 x 5000 x 1024
               corpus     1 x 16384 x 128
               stances    8 x 600 x 1024
             in the one-workgroup form (ward_form 1) and the launch-per-merge form (ward_form 2); the one-workgroup form is not
             run beyond --max-onewg rows (one workgroup would hold a CU for many seconds).  Rows: Gaussian noise around 10 planted
             centres per group.  Both forms must return the same bits.
    HOST     scipy.cluster.hierarchy.linkage(x, 'ward') and sklearn.cluster.AgglomerativeClustering(n_clusters=10).fit(x) per
             group, one after the other, wall clock on this machine's cores (median of `runs`; one run from 16384 rows on)
    SWEEP    1 and 64 groups of n rows, dim 1024 and 36, n = 16 .. 1024 (.. 4096 for one group), both forms: where they cross

    python scripts/ward_bench.py [--runs 3] > profiles/ward_bench.txt
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

THRESHOLD = 128       # kWardOneWgMax (argsim_amd/csrc/kernels.h)


def dev_ward(m, x, off, out, form):
    """the C entry on device tensors; nothing copied"""
    from argsim_amd import lib
    G = len(off) - 1
    wc = lib.AvaeWardConfig()
    m.set_option('ward_form', form)
    m._stream()
    try:
        m._ck(m._l.avae_ward(m._h, C.c_void_p(x.data_ptr()), x.shape[1], (C.c_int32 * (G + 1))(*off), G, C.byref(wc), C.c_void_p(out[0].data_ptr()),
                             C.c_void_p(out[1].data_ptr()), C.c_void_p(out[2].data_ptr())))
    finally:
        m.set_option('ward_form', 0)


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


def wall(fn, runs):
    s = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        s.append((time.perf_counter() - t) * 1e3)
    return float(np.median(s)), min(s), max(s)


def rows(G, n, dim, seed):
    r = np.random.default_rng(seed)
    return np.concatenate([(r.standard_normal((n, dim)) + 1.5 * r.standard_normal((10, dim))[r.integers(0, 10, n)]) for _ in range(G)]).astype(np.float32)


def outputs(N, G):
    return (torch.zeros((N - G, 2), dtype=torch.int32, device='cuda'), torch.zeros(N - G, dtype=torch.float32, device='cuda'),
            torch.zeros(N - G, dtype=torch.int32, device='cuda'))


def fmt(t):
    return "%10.2f ms (%.2f .. %.2f)" % t if t else "      not run"


def both_forms(m, x, off, runs, max_onewg):
    G, n = len(off) - 1, max(off[i + 1] - off[i] for i in range(len(off) - 1))
    dx = torch.as_tensor(x).cuda()
    res, bits = {}, {}
    for form in (1, 2):
        if form == 1 and n > max_onewg:
            res[form] = None
            continue
        out = outputs(x.shape[0], G)
        res[form] = timed(lambda: dev_ward(m, dx, off, out, form), runs)
        bits[form] = [o.cpu().numpy() for o in out]
    same = len(bits) < 2 or all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(bits[1], bits[2]))
    return res, same


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--max-onewg', type=int, default=5000)
    ap.add_argument('--skip-host', action='store_true')
    A = ap.parse_args(argv)
    from scipy.cluster.hierarchy import linkage
    from sklearn.cluster import AgglomerativeClustering
    from argsim_amd.model import VAE
    m = VAE('infer', dim_tgt=32, dim_emb=16, dim_rep=8, rnn_layers=1)
    print("# avae_ward on %s, torch %s; planner: one-workgroup form up to %d rows in the largest group; host baselines on %d cores"
          % (torch.cuda.get_device_name(0), torch.__version__, THRESHOLD, len(os.sched_getaffinity(0))))
    supports = []
    for name, G, n, dim in (('topics', 4, 1250, 1024), ('whole', 1, 5000, 1024), ('corpus', 1, 16384, 128), ('stances', 8, 600, 1024)):
        x = rows(G, n, dim, 3)
        off = [g * n for g in range(G + 1)]
        res, same = both_forms(m, x, off, A.runs, A.max_onewg)
        plan = 1 if n <= THRESHOLD else 2
        line = "%-8s %d x %5d x %4d | one-workgroup %s | launch-per-merge %s | planner: %s | same bits: %s" % (
            name, G, n, dim, fmt(res[1]), fmt(res[2]), 'one-workgroup' if plan == 1 else 'launch-per-merge', same)
        if res[1] and res[2]:
            supports.append((name, n, plan, 1 if res[1][0] <= res[2][0] else 2))
        if not A.skip_host:
            hr = 1 if n >= 16384 else A.runs
            xs = [x[off[g]:off[g + 1]].astype(np.float64) for g in range(G)]
            sp = wall(lambda: [linkage(v, 'ward') for v in xs], hr)
            sk = wall(lambda: [AgglomerativeClustering(n_clusters=10).fit(v) for v in xs], hr)
            line += " | scipy linkage %s | sklearn AgglomerativeClustering %s" % (fmt(sp), fmt(sk))
        print(line)
        sys.stdout.flush()
        torch.cuda.empty_cache()
    for G, dim in ((1, 1024), (1, 36), (64, 1024), (64, 36)):
        print("# sweep: %d group%s of n x %d" % (G, 's' if G > 1 else '', dim))
        for n in (16, 32, 64, 128, 256, 512, 1024) + ((2048, 4096) if G == 1 else ()):
            res, same = both_forms(m, rows(G, n, dim, 5), [g * n for g in range(G + 1)], A.runs, A.max_onewg)
            supports.append(('sweep %d x n x %d' % (G, dim), n, 1 if n <= THRESHOLD else 2, 1 if res[1][0] <= res[2][0] else 2))
            print("n %5d | one-workgroup %s | launch-per-merge %s | same bits: %s" % (n, fmt(res[1]), fmt(res[2]), same))
            sys.stdout.flush()
    wrong = [(name, n) for name, n, plan, best in supports if plan != best]
    print("THRESHOLD %d: the planner's form is the faster one at %d of %d measured geometries%s" % (
        THRESHOLD, len(supports) - len(wrong), len(supports), '' if not wrong else '; not at ' + ', '.join('%s n=%d' % w for w in wrong)))


if __name__ == '__main__':
    main()
