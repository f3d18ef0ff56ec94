#!/usr/bin/env python3
"""avae_kmeans: the time of a call and of one live iteration beside scikit-learn's KMeans on the host.

    TIME     one call (k-means++ seeding, every enqueued iteration, inertias, copy-out), HIP events after a warm-up call, median
             (min .. max) of `runs` calls, at
               test set   5000 x 1024, k = 300, n_init 10, euclidean and cosine   (the reference's scale)
               bank       131072 x 128, k = 1024, n_init 4, euclidean             (beyond the quadratic methods)
             Rows: Gaussian noise around planted centres.  max_iter 30, tol 1e-4 (every iteration is seven enqueued launches whether
             or not a restart has stopped).
    ITER     (time of a call with max_iter = 9 - time with max_iter = 3) / 6 from given random-row centres with tol 0 on unstructured
             Gaussian rows, where no restart stops that early: the time of one live iteration of all restarts, seven kernel
             boundaries included.  Beside it the bound of the distance kernel: N k dim n_init pairs of (subtract, fused multiply-add)
             at 64 double-precision vector instructions per CU and clock (256 CUs, 2.4 GHz: the 78.6 TFLOP/s of the data sheet).
    SEED     the call with max_iter = 1, less one live iteration: the seeding
    HOST     sklearn.cluster.KMeans(k, n_init, max_iter, tol, algorithm='lloyd', random_state=0) on the same rows as float32, wall clock
             on this machine's cores (16 threads); the best inertia of both, on the rows as the metric takes them.  For the cosine sklearn
             runs on the unit rows and its labels are scored by the spherical objective (the members' mean projected on the sphere)

    python scripts/kmeans_bench.py [--runs 5] > profiles/kmeans_bench.txt
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


def dev_kmeans(m, x, out, k, n_init, cin=None, **kw):
    """the C entry on device tensors; nothing copied"""
    from argsim_amd import lib
    cfg = lib.AvaeKmeansConfig(k=k, n_init=n_init, max_iter=kw.get('max_iter', 30), metric=kw.get('metric', 0), init=0 if cin is None else 1,
                               reserved=0, tol=kw.get('tol', 1e-4), seed=kw.get('seed', 0))
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    m._stream()
    m._ck(m._l.avae_kmeans(m._h, p(x), x.shape[0], x.shape[1], C.byref(cfg), p(cin), p(out['label']), p(out['centers']), p(out['stat']),
                           p(out['inertia']), None, None, p(out['stat_all'])))


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


def host(x, k, n_init, max_iter, tol, metric, runs):
    from sklearn.cluster import KMeans
    z = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30) if metric else x
    s, best = [], None
    for _ in range(runs):
        t = time.perf_counter()
        km = KMeans(n_clusters=k, n_init=n_init, max_iter=max_iter, tol=tol, algorithm='lloyd', random_state=0).fit(z)
        s.append((time.perf_counter() - t) * 1e3)
        best = (float(km.inertia_), int(km.n_iter_))
    if metric:          # sklearn's inertia is measured to the members' means; the spherical objective to the means projected on the sphere
        z64 = z.astype(np.float64)
        S = np.zeros((k, z.shape[1]))
        np.add.at(S, km.labels_, z64)
        S /= np.maximum(np.linalg.norm(S, axis=1, keepdims=True), 1e-300)
        best = (float(((z64 - S[km.labels_]) ** 2).sum()), best[1])
    return (float(np.median(s)), min(s), max(s)), best


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--host-runs', type=int, default=1)
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--max-iter', type=int, default=30)
    A = ap.parse_args(argv)
    from argsim_amd.model import VAE
    m = VAE('infer', dim_tgt=32, dim_emb=16, dim_rep=8, rnn_layers=1)
    print("# avae_kmeans on %s, torch %s; host baseline on %d threads" % (torch.cuda.get_device_name(0), torch.__version__, int(os.environ.get('OMP_NUM_THREADS', len(os.sched_getaffinity(0))))))
    for name, n, dim, k, R, metric in (('test set', 5000, 1024, 300, 10, 0), ('test set', 5000, 1024, 300, 10, 1), ('bank', 1 << 17, 128, 1024, 4, 0)):
        x = rows(n, dim, k, 3)
        dx = torch.as_tensor(x).cuda()
        out = dict(label=torch.zeros(n, dtype=torch.int32, device='cuda'), centers=torch.zeros((k, dim), dtype=torch.float32, device='cuda'),
                   stat=torch.zeros(4, dtype=torch.int32, device='cuda'), inertia=torch.zeros(R, dtype=torch.float64, device='cuda'),
                   stat_all=torch.zeros((R, 4), dtype=torch.int32, device='cuda'))
        call = timed(lambda: dev_kmeans(m, dx, out, k, R, metric=metric, max_iter=A.max_iter), A.runs)
        stat, ine, sa = out['stat'].cpu().numpy(), out['inertia'].cpu().numpy(), out['stat_all'].cpu().numpy()
        noise = torch.as_tensor(np.random.default_rng(5).standard_normal((n, dim)).astype(np.float32)).cuda()
        pick = np.random.default_rng(6).integers(0, n, (R, k))
        cin = noise[torch.as_tensor(pick.ravel()).cuda()].reshape(R, k, dim).contiguous()
        if metric:                                                        # given centres are taken as they are: unit rows for the cosine
            cin = cin / cin.norm(dim=2, keepdim=True)
        t9 = timed(lambda: dev_kmeans(m, noise, out, k, R, cin, metric=metric, max_iter=9, tol=0.0), A.runs)
        alive = int(out['stat_all'].cpu().numpy()[:, 0].min())
        t3 = timed(lambda: dev_kmeans(m, noise, out, k, R, cin, metric=metric, max_iter=3, tol=0.0), A.runs)
        t1 = timed(lambda: dev_kmeans(m, dx, out, k, R, metric=metric, max_iter=1), A.runs)
        per = (t9[0] - t3[0]) / 6
        bound = 2.0 * n * k * dim * R / FMA_PER_S * 1e3
        print("%-8s %6d x %4d k %4d n_init %2d %-9s | call %s: best restart %d, %d iterations (%s; all: %s), inertia %.6g | live iteration "
              "%.3f ms (fewest iterations in the 9-iteration call: %d), distance bound %.3f ms: %.1f %% | seeding %.2f ms"
              % (name, n, dim, k, R, ('euclidean', 'cosine')[metric], fmt(call), stat[0], stat[1], ('converged', 'tol', 'max_iter')[stat[2]],
                 sa[:, 0].tolist(), ine[stat[0]], per, alive, bound, 100 * bound / per, t1[0] - per))
        if not A.skip_host:
            ht, (hi, hn) = host(x, k, R, A.max_iter, 1e-4, metric, A.host_runs)
            print("         host, the same rows: sklearn KMeans %s: %d iterations in its best restart, inertia %.6g; inertia device / host %.6f"
                  % (fmt(ht), hn, hi, ine[stat[0]] / hi))
        sys.stdout.flush()
        del dx, out, noise, cin
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
