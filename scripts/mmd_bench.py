#!/usr/bin/env python3
"""avae_mmd: the time of a call with P = 999 relabelings beside the same computation in numpy float64 on the host.

    TIME     one call (counts, the pair passes and their reductions, the statistic; sums and ull asked for, no witness), HIP events after
             a warm-up call, median (min .. max) of `runs` calls, at
               test set   3000 x 128, G = 1    (the reference's scale)
               bank       65536 x 128, G = 1
               topics     65536 x 128, G = 8   (rows sorted by topic, 8192 each: one comparison per topic, the others' rows left out)
             with the rbf kernel at one bandwidth, euclidean; the test set also with the energy kernel.  The masks come from
             avae_mmd_relabel, timed on its own.  Beside it the plan (TI, relabelings per pass, passes) and the least time the
             double-precision vector units could take for the call's arithmetic: per pass pairs x dim x (subtract, fused multiply-add) for
             the distances and pairs x slots additions for the sums, pairs = the unordered pairs of rows valid in the same comparison, at
             64 double-precision vector instructions per CU and clock (256 CUs, 2.4 GHz).  It is a share of the whole call, launches and
             reductions included, not of a kernel.
    HOST     numpy float64 on this machine's cores (16 threads): the kernel values of a block of rows against all rows, two matrix
             products with the 0 / 1 indicators of A and B for all relabelings at once, U = (sum - diagonal) / 2; block-wise, since the
             (N, N) matrix does not fit comfortably.  At 65536 rows `--host-rows` rows are timed and scaled to N (the blocks cost the
             same).  The largest |device - host| statistic over the relabelings is printed where the host ran in full.

    python scripts/mmd_bench.py [--runs 5] > profiles/mmd_bench.txt
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


def fmt(t):
    return "%9.2f ms (%.2f .. %.2f)" % t


def host(x, valid, inA, kernel, gamma, rows, block=1024):
    """U_AA, U_BB (Q,), U_LL over ordered pairs of the first `rows` rows against all rows of ONE comparison -> (seconds, sums or None)"""
    X = x.astype(np.float64)
    sq = (X * X).sum(1)
    v = valid.astype(np.float64)
    A = (inA & valid).astype(np.float64).T.copy()             # (N, Q)
    B = (~inA & valid).astype(np.float64).T.copy()
    Q = A.shape[1]
    uaa, ubb, ull = np.zeros(Q), np.zeros(Q), 0.0
    t = time.perf_counter()
    for r0 in range(0, rows, block):
        r1 = min(rows, r0 + block)
        D = np.maximum(sq[r0:r1, None] - 2.0 * (X[r0:r1] @ X.T) + sq[None, :], 0.0)
        K = -np.sqrt(D) if kernel == 1 else np.exp(-gamma * D)
        K[np.arange(r1 - r0), np.arange(r0, r1)] = 0.0        # the diagonal
        K *= v[r0:r1, None] * v[None, :]
        uaa += (A[r0:r1] * (K @ A)).sum(0)
        ubb += (B[r0:r1] * (K @ B)).sum(0)
        ull += K.sum()
    sec = time.perf_counter() - t
    return sec, (uaa / 2, ubb / 2, ull / 2) if rows == len(X) else None


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--perm', type=int, default=999)
    ap.add_argument('--host-rows', type=int, default=2048)
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--skip-bank', action='store_true')
    A = ap.parse_args(argv)
    from argsim_amd import lib
    from argsim_amd.mmd import pack_bits
    from argsim_amd.model import VAE
    m = VAE('infer', dim_tgt=32, dim_emb=16, dim_rep=8, rnn_layers=1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("# avae_mmd on %s (%d CUs), torch %s, %s; P = %d; host baseline on %d threads"
          % (torch.cuda.get_device_name(0), cus, torch.__version__, time.strftime('%Y-%m-%d'), A.perm,
             int(os.environ.get('OMP_NUM_THREADS', len(os.sched_getaffinity(0))))))
    shapes = [('test set', 3000, 128, 1, 0), ('test set', 3000, 128, 1, 1)]
    shapes += [] if A.skip_bank else [('bank', 1 << 16, 128, 1, 0), ('topics', 1 << 16, 128, 8, 0)]
    P = A.perm
    p = lambda t: C.c_void_p(t.data_ptr())
    for name, n, dim, G, kernel in shapes:
        r = np.random.default_rng(3)
        x = r.standard_normal((n, dim)).astype(np.float32)
        topic = np.arange(n) * G // n
        x += (0.5 * r.standard_normal((G, dim))).astype(np.float32)[topic]
        side = r.random(n) < 0.5
        x[side] += np.float32(0.02)
        valid = topic[None, :] == np.arange(G)[:, None]
        a0 = valid & side[None, :]
        gamma = 1.0 / (2.0 * dim)
        W = (n + 63) // 64
        dx = torch.as_tensor(x).cuda()
        dv = torch.from_numpy(pack_bits(valid).view(np.int64)).cuda()
        din = torch.zeros((G, 1 + P, W), dtype=torch.int64, device='cuda')
        din[:, 0] = torch.from_numpy(pack_bits(a0).view(np.int64)).cuda()
        m._stream()
        t_rel = timed(lambda: m._ck(m._l.avae_mmd_relabel(m._h, n, G, P, p(dv), p(din), C.c_uint64(1))), A.runs)
        cfg = lib.AvaeMmdConfig(kernel=kernel, metric=0, G=G, P=P, nbw=1, reserved=0)
        cfg.gamma[0] = gamma
        out = dict(stat=torch.zeros((G, 1 + P), dtype=torch.float64, device='cuda'), pvalue=torch.zeros(G, dtype=torch.float64, device='cuda'),
                   counts=torch.zeros((G, 2), dtype=torch.int32, device='cuda'), sums=torch.zeros((G, 1 + P, 2), dtype=torch.float64, device='cuda'),
                   ull=torch.zeros(G, dtype=torch.float64, device='cuda'), stat_out=torch.zeros(1, dtype=torch.int32, device='cuda'))
        call = lambda: m._ck(m._l.avae_mmd(m._h, p(dx), n, dim, C.byref(cfg), p(dv), p(din), p(out['stat']), p(out['pvalue']), p(out['counts']),
                                           p(out['sums']), p(out['ull']), None, p(out['stat_out'])))
        t = timed(call, A.runs)
        plan = np.zeros(7, np.int32)
        m._l.avae_debug_mmd_plan(n, dim, G, P, 0, cus, plan.ctypes.data_as(C.POINTER(C.c_int32)), 0)
        per = n // G
        pairs = G * per * (per - 1) / 2.0
        slots = (1 + P) + 1                                    # of one comparison: its relabelings and its valid rows
        passes_per_cmp = max(1.0, plan[2] / G)
        bound = (2.0 * passes_per_cmp * pairs * dim + pairs * slots) / FMA_PER_S * 1e3
        pv = out['pvalue'].cpu().numpy()
        print("%-8s %6d x %4d G %d P %d %-6s | call %s | relabel %s | TI %2d, %d relabelings per pass, %d pass(es) | arithmetic bound %.2f ms: "
              "%.1f %% of the call | p %s" % (name, n, dim, G, P, ('rbf', 'energy')[kernel], fmt(t), fmt(t_rel), plan[0], plan[1], plan[2], bound,
                                              100 * bound / t[0], np.array2string(pv, precision=3)))
        assert int(out['stat_out'].cpu()[0]) == 0
        if not A.skip_host:
            masks = np.unpackbits(din[0].cpu().numpy().view(np.uint8).reshape(1 + P, -1), axis=-1, bitorder='little')[:, :n].astype(bool)
            rows = per if per <= 4096 else min(A.host_rows, per)
            on = valid[0]                                      # the host takes a comparison's own rows only
            sec, sums = host(x[on], np.ones(per, bool), masks[:, on], kernel, gamma, rows)
            if sums is None:                                   # a block of rows of comparison 0 costs what every block of every comparison costs
                total = sec * (per / rows) * G
                print("         host, numpy float64: %9.2f s for %d of the %d rows of a comparison -> %9.1f s for the call; host / device time %.0f : 1"
                      % (sec, rows, per, total, total * 1e3 / t[0]))
            else:
                c = out['counts'].cpu().numpy()[0].astype(np.float64)
                uab = sums[2] - sums[0] - sums[1]
                hs = 2 * sums[0] / (c[0] * (c[0] - 1)) + 2 * sums[1] / (c[1] * (c[1] - 1)) - 2 * uab / (c[0] * c[1])
                err = float(np.abs(out['stat'].cpu().numpy()[0] - hs).max())
                print("         host, numpy float64: %9.2f s; largest |device - host| statistic %.3g; host / device time %.0f : 1"
                      % (sec, err, sec * 1e3 / t[0]))
        sys.stdout.flush()
        del dx, dv, din, out
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
