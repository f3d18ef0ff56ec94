#!/usr/bin/env python3
"""avae_silhouette: the time of a call for one labeling and for 32 labelings of the same rows, beside scikit-learn on the host
(DESIGN 4.3n).

    TIME     one call (row norms, counts, the pair passes, score, CH and DB; every optional output asked for), HIP events after a warm-up
             call, median (min .. max) of `runs` calls, at
               test set   3000 x 128    (the reference's scale)
               bank       65536 x 128
             with L = 1 (k-means-like labels into 16 clusters) and L = 32 (k = 2 .. 33: a k sweep), euclidean; the test set also cosine.
             Rows: Gaussian noise around planted centres; the labels are the nearest of k random rows (what matters to the time is K, not
             the quality of the partition).  Beside it the plan (TI, passes) and the bound of the distance arithmetic: passes x N^2 dim
             pairs of (subtract, fused multiply-add) at 64 double-precision vector instructions per CU and clock (256 CUs, 2.4 GHz).
    RATIO    time(L = 32) / time(L = 1): 32 labelings share every pair distance of a pass; 32 separate calls would cost 32 times L = 1.
    HOST     sklearn.metrics.silhouette_samples (+ calinski_harabasz_score + davies_bouldin_score) per labeling on the same rows as float64,
             wall clock on this machine's cores (16 threads); the numpy reference of tests/sil_ref.py where sklearn is missing.  The
             largest |device - host| silhouette score of the labelings is printed with it.  (The host is timed for one labeling at the
             bank and scaled by L: its labelings share nothing.)

    python scripts/silhouette_bench.py [--runs 5] > profiles/silhouette_bench.txt
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


def dev_call(m, x, label, K, out, metric):
    """the C entry on device tensors; nothing copied but K, which the host holds"""
    from argsim_amd import lib
    cfg = lib.AvaeSilhouetteConfig(metric=metric, L=label.shape[0], reserved=0, reserved2=0)
    p = lambda t: C.c_void_p(t.data_ptr())
    m._stream()
    m._ck(m._l.avae_silhouette(m._h, p(x), x.shape[0], x.shape[1], C.byref(cfg), p(label), K.ctypes.data_as(C.POINTER(C.c_int32)),
                               p(out['score']), p(out['sil']), p(out['ab']), p(out['nearest']), p(out['count']), p(out['cluster_mean']),
                               p(out['index'])))


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


def nearest_of(x, k, seed):
    """labels in [0, k): the nearest of k random rows, every cluster with its own row as a member"""
    c = x[np.random.default_rng(seed).choice(x.shape[0], k, replace=False)].astype(np.float64)
    out = np.empty(x.shape[0], np.int32)
    for a in range(0, x.shape[0], 8192):
        z = x[a:a + 8192].astype(np.float64)
        out[a:a + 8192] = ((z * z).sum(1)[:, None] - 2 * z @ c.T + (c * c).sum(1)[None, :]).argmin(1)
    return out


def fmt(t):
    return "%9.2f ms (%.2f .. %.2f)" % t


def host(x, labels, metric, scale=1):
    """wall clock of the host's scores for the labelings given (x scale where only the first was run) -> (ms, scores)"""
    X = x.astype(np.float64)
    if metric:
        X /= np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1e-300)
    scores = []
    try:
        from sklearn import metrics
        metrics.silhouette_samples(X[:64], np.arange(64) % 2)      # (imports and thread pools are not the host's time)
        t = time.perf_counter()
        for lab in labels:
            scores.append(float(metrics.silhouette_samples(X, lab, metric='cosine' if metric else 'euclidean').mean()))
            metrics.calinski_harabasz_score(X, lab)
            metrics.davies_bouldin_score(X, lab)
        what = 'sklearn'
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import sil_ref
        t = time.perf_counter()
        for lab in labels:
            scores.append(float(sil_ref.one(x, metric, lab, int(lab.max()) + 1)['score']))
        what = 'numpy reference'
    return (time.perf_counter() - t) * 1e3 * scale, scores, what


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--skip-bank', action='store_true')
    A = ap.parse_args(argv)
    from argsim_amd.model import VAE
    m = VAE('infer', dim_tgt=32, dim_emb=16, dim_rep=8, rnn_layers=1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("# avae_silhouette on %s (%d CUs), torch %s, %s; host baseline on %d threads"
          % (torch.cuda.get_device_name(0), cus, torch.__version__, time.strftime('%Y-%m-%d'),
             int(os.environ.get('OMP_NUM_THREADS', len(os.sched_getaffinity(0))))))
    shapes = [('test set', 3000, 128, 0), ('test set', 3000, 128, 1)] + ([] if A.skip_bank else [('bank', 1 << 16, 128, 0)])
    for name, n, dim, metric in shapes:
        x = rows(n, dim, 16, 3)
        dx = torch.as_tensor(x).cuda()
        t1 = None
        for L, ks in ((1, [16]), (32, list(range(2, 34)))):
            labels = np.stack([nearest_of(x, k, 10 + k) for k in ks])
            K = np.array(ks, np.int32)
            dl = torch.as_tensor(labels).cuda()
            kmax = int(K.max())
            out = dict(score=torch.zeros(L, dtype=torch.float64, device='cuda'), sil=torch.zeros((L, n), dtype=torch.float64, device='cuda'),
                       ab=torch.zeros((L, n, 2), dtype=torch.float64, device='cuda'), nearest=torch.zeros((L, n), dtype=torch.int32, device='cuda'),
                       count=torch.zeros((L, kmax), dtype=torch.int32, device='cuda'),
                       cluster_mean=torch.zeros((L, kmax), dtype=torch.float64, device='cuda'),
                       index=torch.zeros((L, 2), dtype=torch.float64, device='cuda'))
            t = timed(lambda: dev_call(m, dx, dl, K, out, metric), A.runs)
            plan = np.zeros(2 * L + 5, np.int32)
            m._l.avae_debug_sil_plan(n, dim, L, K.ctypes.data_as(C.POINTER(C.c_int32)), 0, cus, plan.ctypes.data_as(C.POINTER(C.c_int32)))
            bound = 2.0 * plan[2] * n * n * dim / FMA_PER_S * 1e3
            score = out['score'].cpu().numpy()
            line = "%-8s %6d x %4d L %2d (sum K %3d) %-9s | call %s | TI %2d, %d pass(es), distance bound %.3f ms: %.1f %%" % (
                name, n, dim, L, int(K.sum()), ('euclidean', 'cosine')[metric], fmt(t), plan[0], plan[2], bound, 100 * bound / t[0])
            if t1 is None:
                t1 = t[0]
            else:
                line += " | L = 32 : L = 1 = %.2f (32 separate calls: 32.00)" % (t[0] / t1)
            print(line)
            if not A.skip_host:
                part = labels if n <= 4096 else labels[:1]
                ht, hs, what = host(x, part, metric, len(labels) / len(part))
                print("         host, the same rows: %s %9.2f ms%s; largest |device - host| score %.3g; device / host time 1 : %.0f"
                      % (what, ht, '' if len(part) == len(labels) else ' (one labeling timed, x %d)' % len(labels),
                         max(abs(a - b) for a, b in zip(score, hs)), ht / t[0]))
            sys.stdout.flush()
            del dl, out
        del dx
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
