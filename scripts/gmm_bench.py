#!/usr/bin/env python3
"""avae_gmm_fit: the time of a call and of one live iteration beside scikit-learn's GaussianMixture on the host.

    TIME     one call (the start from labels, every enqueued iteration, the pick, the final E-step, copy-out), HIP events after a warm-up
             call, median (min .. max) of `runs` calls, at
               test set   5000 x 1024, k = 32, n_init 4      (the reference's scale)
               bank       131072 x 128, k = 64, n_init 4
             both with 'diag' and 'spherical' covariances.  Rows: Gaussian noise around planted centres; the start: random labels, another
             draw per restart.  max_iter 30, tol 1e-3 (every iteration is five enqueued launches whether or not a restart has stopped).
    ITER     (time of a call with max_iter = 9 - time with max_iter = 3) / 6 with tol 0, where no restart stops: the time of one live
             iteration of all restarts, five kernel boundaries included.  Beside it the derived arithmetic bound: per row, component and
             column 3 double operations for the E-step's q_ic, 3 for forming it again in the M-step and 4 for the two weighted sums, at
             the data sheet's 78.6 TFLOP/s of double-precision vector arithmetic.
    HOST     sklearn.mixture.GaussianMixture(k, covariance_type, tol, reg_covar, max_iter) on the same rows as float64 from the SAME start
             parameters (the device's, read back from a max_iter = 0 call), one fit per restart, wall clock summed, on this machine's
             cores (16 threads); the ratio of the best final lower bounds.

    python scripts/gmm_bench.py [--runs 3] > profiles/gmm_bench.txt
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

FLOPS = 78.6e12
OUTS = ('weights', 'means', 'covars', 'label', 'stat', 'lower', 'logp', 'resp', 'weights_all', 'means_all', 'covars_all', 'stat_all', 'trace')


def dev_gmm(m, x, lab, out, k, n_init, covariance, max_iter, tol):
    """the C entry on device tensors; nothing copied"""
    from argsim_amd import lib
    cfg = lib.AvaeGmmConfig(k=k, n_init=n_init, max_iter=max_iter, covariance=covariance, init=0, reserved=0, tol=tol, reg_covar=1e-6)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    m._stream()
    m._ck(m._l.avae_gmm_fit(m._h, p(x), x.shape[0], x.shape[1], C.byref(cfg), p(lab), None, None, None, *[p(out.get(n)) for n in OUTS]))


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


def host(x, k, covariance, starts, max_iter, tol):
    from sklearn.mixture import GaussianMixture
    X = x.astype(np.float64)
    total, best = 0.0, (-np.inf, 0)
    for w, mu, cov in zip(*starts):
        g = GaussianMixture(k, covariance_type=('diag', 'spherical')[covariance], tol=tol, reg_covar=1e-6, max_iter=max_iter, weights_init=w / w.sum(),
                            means_init=mu, precisions_init=1.0 / cov if covariance == 0 else 1.0 / cov[:, 0])
        t = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            g.fit(X)
        total += (time.perf_counter() - t) * 1e3
        if g.lower_bound_ > best[0]:
            best = (float(g.lower_bound_), int(g.n_iter_))
    return total, best


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--max-iter', type=int, default=30)
    A = ap.parse_args(argv)
    from argsim_amd.model import VAE
    m = VAE('infer', dim_tgt=32, dim_emb=16, dim_rep=8, rnn_layers=1)
    print("# avae_gmm_fit on %s, torch %s; host baseline on %d threads" % (torch.cuda.get_device_name(0), torch.__version__, int(os.environ.get('OMP_NUM_THREADS', len(os.sched_getaffinity(0))))))
    for name, n, dim, k, R in (('test set', 5000, 1024, 32, 4), ('bank', 1 << 17, 128, 64, 4)):
        x = rows(n, dim, k, 3)
        dx = torch.as_tensor(x).cuda()
        lab = torch.as_tensor(np.random.default_rng(5).integers(0, k, (R, n)).astype(np.int32)).cuda()
        f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device='cuda')
        out = dict(weights=f64(k), means=f64(k, dim), covars=f64(k, dim), label=torch.zeros(n, dtype=torch.int32, device='cuda'),
                   stat=torch.zeros(4, dtype=torch.int32, device='cuda'), lower=f64(R), logp=f64(n), weights_all=f64(R, k), means_all=f64(R, k, dim),
                   covars_all=f64(R, k, dim), stat_all=torch.zeros((R, 4), dtype=torch.int32, device='cuda'))
        for cov in (0, 1):
            dev_gmm(m, dx, lab, out, k, R, cov, 0, 1e-3)
            starts = [out[q].cpu().numpy().copy() for q in ('weights_all', 'means_all', 'covars_all')]
            call = timed(lambda: dev_gmm(m, dx, lab, out, k, R, cov, A.max_iter, 1e-3), A.runs)
            stat, low, sa = out['stat'].cpu().numpy(), out['lower'].cpu().numpy(), out['stat_all'].cpu().numpy()
            t9 = timed(lambda: dev_gmm(m, dx, lab, out, k, R, cov, 9, 0.0), A.runs)
            alive = int(out['stat_all'].cpu().numpy()[:, 0].min())
            t3 = timed(lambda: dev_gmm(m, dx, lab, out, k, R, cov, 3, 0.0), A.runs)
            per = (t9[0] - t3[0]) / 6
            bound = 10.0 * n * k * dim * R / FLOPS * 1e3
            print("%-8s %6d x %4d k %3d n_init %d %-9s | call %s: best restart %d, %d iterations (%s; all: %s), lower bound %.6f | live iteration "
                  "%.3f ms (fewest iterations in the 9-iteration call: %d), arithmetic bound %.3f ms: %.1f %%"
                  % (name, n, dim, k, R, ('diag', 'spherical')[cov], fmt(call), stat[0], stat[1], ('converged', 'max_iter', 'degenerate')[stat[2]],
                     sa[:, 0].tolist(), low[stat[0]], per, alive, bound, 100 * bound / per))
            if not A.skip_host:
                ht, (hl, hn) = host(x, k, cov, starts, A.max_iter, 1e-3)
                print("         host, the same rows and starts: sklearn GaussianMixture %9.2f ms for the %d fits: %d iterations in its best, lower bound "
                      "%.6f; lower bound device / host %.9f" % (ht, R, hn, hl, low[stat[0]] / hl))
            sys.stdout.flush()
        del dx, out, lab
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
