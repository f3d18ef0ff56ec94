#!/usr/bin/env python3
"""avae_probe_fit: how low a tol it reaches, how truthful its stop rule is, and its time beside the same Newton-CG in torch.

    FLOOR    the smallest tol of the ladder 1e-4, 5e-5, 2.5e-5, 1e-5 .. 1e-7 down to which every problem of every case of
             tests/probe_ref.py still ends with status 0 (max_newton 50, max_cg 30)
    RATIO    the worst float64 |grad f(w_dev)| / (tol g0) over those problems at tol = 1e-4 (the GPU test demands <= 2)
    TIME     one fit, HIP events after a warm-up call, median (min .. max) of `runs` calls, at
               reference  N 5000, dim 1024, P = 4 topics x 5 folds x 10 classes = 200 (a cross-validation of eval_classification.py)
               corpus     N 2^20, dim 128, P 64 (16 classes x 4 folds over one corpus)
             rows around class centres 3 apart with unit noise, C = 0.001, balanced weights, tol 1e-4, max_cg 30,
             beside torch_fit below: the same truncated Newton-CG in lockstep written with torch matmuls on the same device, the way
             one writes it in torch (masked updates, a synchronisation wherever the loop wants to know whether to go on).

    python scripts/probe_bench.py [--runs 3] > profiles/probe_bench.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def dev_fit(m, x, s, tol, max_newton=50, max_cg=30):
    """the C entry on device tensors -> (w, stats) device tensors; nothing copied"""
    from argsim_amd import lib
    (N, dim), P = x.shape, s.shape[0]
    w = torch.empty((P, dim + 1), dtype=torch.float32, device=x.device)
    st = torch.empty((P, 4), dtype=torch.float32, device=x.device)
    pc = lib.AvaeProbeConfig(max_newton, max_cg, tol, 0)
    m._stream()
    m._ck(m._l.avae_probe_fit(m._h, C.c_void_p(x.data_ptr()), N, dim, C.c_void_p(s.data_ptr()), P, C.byref(pc), C.c_void_p(w.data_ptr()),
                              C.c_void_p(st.data_ptr())))
    return w, st


def _softplus(t):
    return torch.clamp(t, min=0) + torch.log1p(torch.exp(-t.abs()))


def torch_fit(x, s, tol, max_newton=50, max_cg=30):
    """the yardstick: x (N, dim), s (P, N) on the device -> (w (P, dim + 1), Newton iterations)"""
    N, dim = x.shape
    P = s.shape[0]
    xt = torch.cat([x, torch.ones((N, 1), device=x.device)], 1)
    sT = s.T.contiguous()
    y, c = torch.sign(sT), sT.abs()
    w = torch.zeros((P, dim + 1), device=x.device)
    alive = torch.ones(P, dtype=torch.bool, device=x.device)
    g0 = None
    for it in range(max_newton + 1):
        z = xt @ w.T
        m = y * z
        sig = torch.sigmoid(m)
        g = w + (-(sT * (1 - sig))).T @ xt
        gn = g.norm(dim=1)
        g0 = gn if g0 is None else g0
        alive &= gn > tol * g0
        if it == max_newton or not bool(alive.any()):
            break
        D = c * sig * (1 - sig)
        p, r = torch.zeros_like(w), -g
        d, rr, cg = r.clone(), gn * gn, alive.clone()
        for _ in range(max_cg):
            hd = d + (D * (xt @ d.T)).T @ xt
            a = torch.where(cg, rr / (d * hd).sum(1), torch.zeros_like(rr))
            p += a[:, None] * d
            r -= a[:, None] * hd
            rrn = (r * r).sum(1)
            cg &= rrn.sqrt() > 0.1 * gn
            if not bool(cg.any()):
                break
            d = torch.where(cg[:, None], r + (rrn / rr)[:, None] * d, d)
            rr = torch.where(cg, rrn, rr)
        u = xt @ p.T
        zd, ud, cd, yd = z.double(), u.double(), c.double(), y.double()
        f0 = (cd * _softplus(-yd * zd)).sum(0)
        gtp, wtp, pp = (g.double() * p.double()).sum(1), (w.double() * p.double()).sum(1), (p.double() ** 2).sum(1)
        step, todo, a = torch.zeros(P, device=x.device), alive.clone(), 1.0
        for _ in range(21):
            f = (cd * _softplus(-yd * (zd + a * ud))).sum(0)
            ok = todo & ((f - f0) + a * wtp + 0.5 * a * a * pp <= 1e-4 * a * gtp)
            step = torch.where(ok, torch.full_like(step, a), step)
            todo &= ~ok
            if not bool(todo.any()):
                break
            a *= 0.5
        w = w + step[:, None] * p
    return w, it


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


def geometry(N, dim, topics, folds, classes, seed):
    """rows, and the costs of every topic x fold x class problem (argsim_amd.probe.cv_problems) -> x, s on the device"""
    from argsim_amd import probe
    rng = np.random.default_rng(seed)
    topic, cls, fold = rng.integers(0, topics, N), rng.integers(0, classes, N), rng.integers(0, folds, N)
    centres = rng.standard_normal((topics, classes, dim))
    centres *= (3.0 / np.sqrt(2.0)) / np.linalg.norm(centres, axis=2, keepdims=True)
    x = torch.as_tensor(centres[topic, cls].astype(np.float32)).cuda() + torch.randn((N, dim), device='cuda', generator=torch.Generator('cuda').manual_seed(seed))
    _, costs = probe.cv_problems(cls, fold, topic, 0.001, 'balanced')
    return x.contiguous(), torch.as_tensor(costs).cuda()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--skip-corpus', action='store_true')
    A = ap.parse_args(argv)
    import probe_ref as pr
    from argsim_amd.model import VAE
    m = VAE('infer', dim_tgt=32, dim_emb=16, dim_rep=8, rnn_layers=1)
    torch.backends.cuda.matmul.allow_tf32 = False
    print("# avae_probe_fit on %s, torch %s; max_newton 50, max_cg 30" % (torch.cuda.get_device_name(0), torch.__version__))
    floor, ladder = None, (1e-4, 5e-5, 2.5e-5, 1e-5, 5e-6, 2.5e-6, 1e-6, 5e-7, 2.5e-7, 1e-7)
    for tol in ladder:
        bad, worst, its = 0, 0.0, 0
        for case in pr.CASES:
            x, s = pr.case_inputs(case)
            w, st = dev_fit(m, torch.as_tensor(np.array(x)).cuda(), torch.as_tensor(np.array(s)).cuda(), tol)
            w, st = w.cpu().numpy(), st.cpu().numpy()
            g0 = pr.g0_64(x, s)
            bad += int((st[:, 3] != 0).sum())
            its = max(its, int(st[:, 2].max()))
            for p in range(s.shape[0]):
                if g0[p] > 0:
                    worst = max(worst, float(np.linalg.norm(pr.grad64(x, s[p], w[p]))) / (tol * g0[p]))
        print("tol %.1e: %3d problems not converged, most Newton iterations %2d, worst |grad f|_64 / (tol g0) = %.3f" % (tol, bad, its, worst))
        sys.stdout.flush()
        if bad:
            break
        floor = tol
    print("FLOOR = %s" % ('%.1e' % floor if floor else 'above 1e-4'))
    shapes = [('reference', 5000, 1024, 4, 5, 10)] + ([] if A.skip_corpus else [('corpus', 1 << 20, 128, 1, 4, 16)])
    for name, N, dim, topics, folds, classes in shapes:
        x, s = geometry(N, dim, topics, folds, classes, 3)
        ours = timed(lambda: dev_fit(m, x, s, 1e-4), A.runs)
        theirs = timed(lambda: torch_fit(x, s, 1e-4), A.runs)
        w, st = dev_fit(m, x, s, 1e-4)
        wt, it_t = torch_fit(x, s, 1e-4)
        print("%-9s N %7d dim %4d P %3d | avae_probe_fit %9.2f ms (%.2f .. %.2f), Newton iterations %d, not converged %d | torch Newton-CG %9.2f ms "
              "(%.2f .. %.2f), Newton iterations %d, x%.2f | max |w - w_torch| %.2e"
              % (name, N, dim, s.shape[0], ours[0], ours[1], ours[2], int(st[:, 2].max()), int((st[:, 3] != 0).sum()), theirs[0], theirs[1], theirs[2], it_t,
                 theirs[0] / ours[0], float((w - wt).abs().max())))
        sys.stdout.flush()
        del x, s, w, wt
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
