#!/usr/bin/env python3
"""avae_probe_fit_l1: how low a tol it reaches, how truthful its stop rule is, and its time beside the same proximal Newton in torch
(DESIGN 4.3j).

    LADDER   tol 1e-4, 1e-5, 1e-6, 1e-7 over every case of tests/probe_l1_ref.py (max_newton 50, max_inner 50): the problems that do
             not end with status 0, the most outer iterations, and the worst float64 |v(w_dev)|_1 / (tol |v(0)|_1) (the GPU test
             demands <= 2 at 1e-4).  FLOOR is the smallest tol down to which every problem still converges.
    TIME     one fit, HIP events after a warm-up call, median (min .. max) of `runs` calls, tol 1e-4, C = 0.1, no class weights, at
               reference  N 1901 (the posts of the reference's docs/results_iac/clustering.csv), dim 1024, P = 8 (topic, stance) classes
               corpus     N 2^18, dim 128, P 32
             rows around class centres planted on two columns per class (3 apart from the rest) with unit noise, beside
             torch_fit_l1 below: the same method in lockstep written with torch matmuls on the same device (masked updates, a
             synchronisation wherever the loop wants to know whether to go on), whose outer iterations and Hessian products are
             printed; and, once, scikit-learn's liblinear on the host at its default tol, as context (where scikit-learn is installed).

    python scripts/probe_l1_bench.py [--runs 3] > profiles/probe_l1_bench.txt
    python scripts/probe_l1_bench.py --trace reference      one warm-up and one fit of that geometry and nothing else (for rocprofv3)
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from probe_bench import _softplus, timed  # noqa: E402


def dev_fit(m, x, s, tol, max_newton=50, max_inner=50):
    """the C entry on device tensors -> (w, stats) device tensors; nothing copied"""
    from argsim_amd import lib
    (N, dim), P = x.shape, s.shape[0]
    w = torch.empty((P, dim + 1), dtype=torch.float32, device=x.device)
    st = torch.empty((P, 4), dtype=torch.float32, device=x.device)
    pc = lib.AvaeProbeL1Config(max_newton, max_inner, tol, 0)
    m._stream()
    m._ck(m._l.avae_probe_fit_l1(m._h, C.c_void_p(x.data_ptr()), N, dim, C.c_void_p(s.data_ptr()), P, C.byref(pc), C.c_void_p(w.data_ptr()),
                                 C.c_void_p(st.data_ptr())))
    return w, st


def _soft(a, t):
    return torch.sign(a) * torch.clamp(a.abs() - t, min=0)


def _vnorm(g, w):
    return torch.where(w != 0, g + torch.sign(w), torch.sign(g) * torch.clamp(g.abs() - 1, min=0)).abs().sum(1)


def torch_fit_l1(x, s, tol, max_newton=50, max_inner=50):
    """the yardstick: x (N, dim), s (P, N) on the device -> (w (P, dim + 1), outer iterations, Hessian products)"""
    N, dim = x.shape
    P = s.shape[0]
    xt = torch.cat([x, torch.ones((N, 1), device=x.device)], 1)
    x2 = xt * xt
    sT = s.T.contiguous()
    y, c = torch.sign(sT), sT.abs()
    w = torch.zeros((P, dim + 1), device=x.device)
    alive = torch.ones(P, dtype=torch.bool, device=x.device)
    v0, rho, hv = None, torch.zeros(P, device=x.device), 0
    for it in range(max_newton + 1):
        z = xt @ w.T
        sig = torch.sigmoid(y * z)
        g = (-(sT * (1 - sig))).T @ xt
        vn = _vnorm(g, w)
        v0 = vn if v0 is None else v0
        alive &= vn > tol * v0
        if it == max_newton or not bool(alive.any()):
            break
        D = c * sig * (1 - sig)
        mx = (D.T @ x2).max(1).values
        L = torch.where(rho > 2, mx * 0.5 * rho, mx).clamp(min=1e-30)
        d, Hd, yy, Hy = (torch.zeros_like(w) for _ in range(4))
        t, run = torch.ones(P, device=x.device), alive.clone()
        for _ in range(max_inner):
            iL = (1 / L)[:, None]
            cand = _soft(w + yy - (g + Hy) * iL, iL) - w
            Hc = (D * (xt @ cand.T)).T @ xt
            hv += 1
            delta = cand - yy
            acc = (delta * (Hc - Hy)).sum(1) <= L * (delta * delta).sum(1)
            restart = ((yy - cand) * (cand - d)).sum(1) > 0
            tn = torch.where(restart | ~acc, torch.ones_like(t), 0.5 * (1 + torch.sqrt(1 + 4 * t * t)))
            beta = torch.where(restart, torch.zeros_like(t), (t - 1) / tn)[:, None]
            up, rej = (run & acc)[:, None], (run & ~acc)[:, None]
            yy = torch.where(up, cand + beta * (cand - d), torch.where(rej, d, yy))
            Hy = torch.where(up, Hc + beta * (Hc - Hd), torch.where(rej, Hd, Hy))
            d, Hd = torch.where(up, cand, d), torch.where(up, Hc, Hd)
            L = torch.where(run & ~acc, 2 * L, L)
            t = torch.where(run, tn, t)
            run &= ~(acc & (_vnorm(g + Hd, w + d) <= 0.1 * vn))
            if not bool(run.any()):
                break
        rho = torch.where(alive, L / mx.clamp(min=1e-30), rho)
        u = xt @ d.T
        zd, ud, cd, yd, wd, dd = z.double(), u.double(), c.double(), y.double(), w.double(), d.double()
        f0, w1 = (cd * _softplus(-yd * zd)).sum(0), wd.abs().sum(1)
        delta = (g.double() * dd).sum(1) + (wd + dd).abs().sum(1) - w1
        step, todo, a = torch.zeros(P, device=x.device), alive.clone(), 1.0
        for _ in range(21):
            f = (cd * _softplus(-yd * (zd + a * ud))).sum(0)
            ok = todo & ((f - f0) + ((wd + a * dd).abs().sum(1) - w1) <= 0.01 * a * delta)
            step = torch.where(ok, torch.full_like(step, a), step)
            todo &= ~ok
            if not bool(todo.any()):
                break
            a *= 0.5
        w = w + step[:, None] * d
    return w, it, hv


def geometry(N, dim, K, seed):
    """rows and the one-vs-rest L1 costs of their K classes (argsim_amd.probe.l1_costs) -> x, s on the device, labels"""
    from argsim_amd import probe
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, K, N)
    centres = np.zeros((K, dim), np.float32)
    for k in range(K):
        centres[k, 2 * k] = centres[k, 2 * k + 1] = 3.0
    x = torch.as_tensor(centres[cls]).cuda() + torch.randn((N, dim), device='cuda', generator=torch.Generator('cuda').manual_seed(seed))
    _, costs = probe.l1_costs(cls)
    return x.contiguous(), torch.as_tensor(costs).cuda(), cls


SHAPES = {'reference': (1901, 1024, 8), 'corpus': (1 << 18, 128, 32)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--skip-corpus', action='store_true')
    ap.add_argument('--trace', choices=tuple(SHAPES), default=None)
    A = ap.parse_args(argv)
    import probe_l1_ref as pl
    from argsim_amd.model import VAE
    m = VAE('infer', dim_tgt=32, dim_emb=16, dim_rep=8, rnn_layers=1)
    torch.backends.cuda.matmul.allow_tf32 = False
    if A.trace:
        x, s, _ = geometry(*SHAPES[A.trace], 3)
        for _ in range(2):
            dev_fit(m, x, s, 1e-4)
            torch.cuda.synchronize()
        return
    print("# avae_probe_fit_l1 on %s, torch %s; max_newton 50, max_inner 50" % (torch.cuda.get_device_name(0), torch.__version__))
    floor, unbroken = None, True
    for tol in (1e-4, 1e-5, 1e-6, 1e-7):
        bad, worst, its = 0, 0.0, 0
        for case in pl.GPU_CASES + pl.SK_CASES:
            x, s = pl.case_inputs(case)
            w, st = dev_fit(m, torch.as_tensor(np.array(x)).cuda(), torch.as_tensor(np.array(s)).cuda(), tol)
            w, st = w.cpu().numpy(), st.cpu().numpy()
            v0 = pl.v0_64(x, s)
            bad += int((st[:, 3] != 0).sum())
            its = max(its, int(st[:, 2].max()))
            for p in range(s.shape[0]):
                if v0[p] > 0 and st[p, 3] == 0:
                    worst = max(worst, float(np.abs(pl.v64(x, s[p], w[p])).sum()) / (tol * v0[p]))
        print("tol %.0e: %3d problems not converged, most outer iterations %2d, worst |v|_1_64 / (tol |v(0)|_1) of the converged = %.3f" % (tol, bad, its, worst))
        sys.stdout.flush()
        if bad:
            unbroken = False
        elif unbroken:
            floor = tol
    print("FLOOR = %s" % ('%.0e' % floor if floor else 'above 1e-4'))
    for name in ['reference'] + ([] if A.skip_corpus else ['corpus']):
        N, dim, K = SHAPES[name]
        x, s, cls = geometry(N, dim, K, 3)
        ours = timed(lambda: dev_fit(m, x, s, 1e-4), A.runs)
        theirs = timed(lambda: torch_fit_l1(x, s, 1e-4), A.runs)
        w, st = dev_fit(m, x, s, 1e-4)
        wt, it_t, hv_t = torch_fit_l1(x, s, 1e-4)
        print("%-9s N %7d dim %4d P %3d | avae_probe_fit_l1 %9.2f ms (%.2f .. %.2f), outer iterations %d, not converged %d, columns kept %d | torch proximal "
              "Newton %9.2f ms (%.2f .. %.2f), outer iterations %d, Hessian products %d, x%.2f | max |w - w_torch| %.2e, supports differ in %d places"
              % (name, N, dim, s.shape[0], ours[0], ours[1], ours[2], int(st[:, 2].max()), int((st[:, 3] != 0).sum()), int((w[:, :-1] != 0).any(0).sum()),
                 theirs[0], theirs[1], theirs[2], it_t, hv_t, theirs[0] / ours[0], float((w - wt).abs().max()), int(((w != 0) != (wt != 0)).sum())))
        sys.stdout.flush()
        if name == 'reference':
            try:
                from sklearn.linear_model import LogisticRegression
                xh = x.cpu().numpy().astype(np.float64)
                t0 = time.perf_counter()
                models = [LogisticRegression(penalty='l1', C=0.1, solver='liblinear').fit(xh, (cls == k).astype(int)) for k in range(K)]
                t1 = time.perf_counter()
                coef = np.concatenate([mod.coef_ for mod in models])
                print("%-9s scikit-learn liblinear on the host, one-vs-rest, default tol: %.0f ms, columns kept %d (context, not a comparison)"
                      % (name, 1e3 * (t1 - t0), int((coef != 0).any(0).sum())))
            except ImportError:
                print("%-9s scikit-learn is not installed: no host figure" % name)
        del x, s, w, wt
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
