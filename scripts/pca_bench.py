#!/usr/bin/env python3
"""avae_pca_fit / avae_pca_transform: the time of a call on device-resident rows, beside scikit-learn's PCA on the host.

    FIT        one call (column sums, mean, covariance tiles, their merge, the Jacobi solve, order / sign / copy-out), HIP events after a
               warm-up call, median (min .. max) of `runs` calls, at
                 test set   3000 x 128      (the reference's scale; the resident solve)
                 bank       65536 x 128     (the resident solve)
                 bank       131072 x 1024   (the launched solve: one launch per round)
               Rows: dim / 8 strong directions over Gaussian noise, an offset of 2.  Beside it the plan, the sweeps used and the bound of
               the covariance arithmetic: N dreal (dreal + 64) / 2 fused multiply-adds at 64 double-precision vector instructions per CU
               and clock (256 CUs, 2.4 GHz).
    SOLVE      the eigen-solve on its own: a second fit of the FIRST 2 dreal rows only (the same dreal, so the same solve kernels and launch
               counts, a covariance that costs next to nothing); the sweeps it took are printed with it.
    TRANSFORM  avae_pca_transform of all rows onto the leading k = 32 components and onto all of them.
    HOST       sklearn.decomposition.PCA(svd_solver='covariance_eigh') and 'full' fitted on the same rows (float32, as scikit-learn takes
               them), wall clock on this machine's cores (OMP_NUM_THREADS); a host run estimated to take more than --host-limit seconds is
               left out and said so.  The largest difference of the explained variances, relative to the largest, is printed with it.

    python scripts/pca_bench.py [--runs 5] > profiles/pca_bench.txt
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
    g = torch.Generator(device='cuda').manual_seed(seed)
    k = dim // 8
    load = torch.randn((k, dim), generator=g, device='cuda') * torch.linspace(3.0, 0.5, k, device='cuda')[:, None]
    x = torch.randn((n, k), generator=g, device='cuda') @ load + 0.3 * torch.randn((n, dim), generator=g, device='cuda') + 2.0
    return x.float().contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--shapes', default='3000x128,65536x128,131072x1024')
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--host-limit', type=float, default=120.0)
    A = ap.parse_args(argv)
    from argsim_amd import lib
    from argsim_amd.model import VAE
    m = VAE('infer', dim_tgt=32, dim_emb=16, dim_rep=8, rnn_layers=1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("# avae_pca_fit / avae_pca_transform on %s (%d CUs), torch %s, %s; host baseline on %d threads"
          % (torch.cuda.get_device_name(0), cus, torch.__version__, time.strftime('%Y-%m-%d'),
             int(os.environ.get('OMP_NUM_THREADS', len(os.sched_getaffinity(0))))))
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    for shape in A.shapes.split(','):
        n, dim = (int(v) for v in shape.split('x'))
        dx = rows(n, dim, 3)
        mean = torch.zeros(dim, dtype=torch.float64, device='cuda')
        var = torch.zeros(dim, dtype=torch.float64, device='cuda')
        comp = torch.zeros((dim, dim), dtype=torch.float64, device='cuda')
        stat = torch.zeros(8, dtype=torch.int32, device='cuda')
        cfg = lib.AvaePcaConfig(pad=0, max_sweeps=0, reserved=0, reserved2=0)

        def fit(rows_used):
            m._stream()
            m._ck(m._l.avae_pca_fit(m._h, p(dx), rows_used, dim, C.byref(cfg), p(mean), p(var), p(comp), p(stat)))
        small = min(n, 2 * dim)
        ts = timed(lambda: fit(small), A.runs)
        st_small = stat.cpu().numpy().copy()
        t = timed(lambda: fit(n), A.runs)
        st = stat.cpu().numpy().copy()
        plan = np.zeros(13, np.int32)
        m._l.avae_debug_pca_plan(n, dim, 0, 0, 0, cus, plan.ctypes.data_as(C.POINTER(C.c_int32)))
        ws = (int(plan[11]) & 0xffffffff) | (int(plan[12]) << 32)
        bound = n * plan[2] * 4096.0 / FMA_PER_S * 1e3
        print("%7d x %-4d fit %9.2f ms (%.2f .. %.2f) | %d tile pairs x %d chunks of %d rows, %s solve, %d launches enqueued, workspace %.1f MiB, "
              "covariance bound %.3f ms | sweeps %d of %d, converged %d, rotations %d, rank %d"
              % (n, dim, t[0], t[1], t[2], plan[2], plan[4], plan[3], 'resident' if plan[5] == 1 else 'launched', plan[8], ws / 2.0 ** 20, bound,
                 st[0], plan[7], st[1], st[2], st[3]))
        print("         solve alone (a fit of the first %d rows): %9.2f ms (%.2f .. %.2f), sweeps %d; covariance and the rest of the full fit: %.2f ms"
              % (small, ts[0], ts[1], ts[2], st_small[0], t[0] - ts[0]))
        for k in sorted({min(32, dim), dim}):
            y = torch.zeros((n, k), dtype=torch.float32, device='cuda')

            def tr():
                m._stream()
                m._ck(m._l.avae_pca_transform(m._h, p(dx), n, dim, p(mean), p(comp), None, k, p(y)))
            tt = timed(tr, A.runs)
            print("         transform onto %4d components %9.2f ms (%.2f .. %.2f); bound %.3f ms" % (k, tt[0], tt[1], tt[2], n * dim * k / FMA_PER_S * 1e3))
            del y
        sys.stdout.flush()
        if not A.skip_host:
            try:
                from sklearn.decomposition import PCA
            except ImportError:
                print("         host: scikit-learn is not installed on this machine; the device times stand alone")
                A.skip_host = True
                continue
            X = dx.cpu().numpy()
            dv = var.cpu().numpy()
            for solver in ('covariance_eigh', 'full'):
                est = 4.0 * n * dim * dim / 2e10 if solver == 'full' else 0.0
                if est > A.host_limit:
                    print("         host %s: left out, estimated %.0f s (limit %.0f s)" % (solver, est, A.host_limit))
                    continue
                try:
                    t0 = time.perf_counter()
                    sk = PCA(svd_solver=solver).fit(X)
                    ht = (time.perf_counter() - t0) * 1e3
                except ValueError as e:
                    print("         host %s: %s" % (solver, e))
                    continue
                k = len(sk.explained_variance_)
                print("         host, the same rows: sklearn PCA(svd_solver='%s') fit %9.2f ms; variances differ by %.2g of the largest; device / host time 1 : %.2f"
                      % (solver, ht, np.abs(sk.explained_variance_ - dv[:k]).max() / dv[0], ht / t[0]))
                sys.stdout.flush()
        del dx, mean, var, comp, stat
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
