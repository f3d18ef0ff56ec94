#!/usr/bin/env python3
"""records tests/golden/latent_plan_parent.npz: knn_plan, agg_plan and probe_plan of a checkout of the PARENT commit, compiled as a
host program (no GPU: the three functions are host arithmetic), over the inputs built below.

    git worktree add /tmp/parent <hash>
    python tests/golden/make_latent_plan_golden.py --tree /tmp/parent --parent <hash> [--out FILE]

Never run it on the code under test.  `inputs` rows are (kind, n, N, k or P, dim, chunk_opt) with kind 0 knn, 1 agg, 2 probe; `plan`
rows are every field of the parent's plan: (qrows or ptiles, qtiles or Ppad, LD or 0, parts, chunk), agg's first field 0.

The inputs (tests/test_latent_plan.py checks that they hold what is claimed here): n in 1, 32, 64, 65, 128, 129, 4096 (both knn tile
heights; n is not an input of probe_plan); k in 1, 2, 16, 31, 32 (the merge's LDS limit moves knn's part limit from 512 down to 127);
P in 1, 32, 33; N in 0 (knn alone), 1, one step either side of tile x want and of max_parts x tile of each planner, 2^31 - 256;
chunk_opt in 0, 1, 50, 127, 128, 129, 2^30 and 2^31 - 1 (the only way to the 0x7fffff80 clamp: no plan of <= 2^31 - 256 rows gets there)."""
import argparse
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NS = (1, 32, 64, 65, 128, 129, 4096)
KS = (1, 2, 16, 31, 32)
PS = (1, 32, 33)
CHUNKS = (0, 1, 50, 127, 128, 129, 1 << 30, (1 << 31) - 1)
NMAX = (1 << 31) - 256

MAIN = r"""
#include "kernels.h"
#include <cstdio>
int main()
{
    long long kind, n, N, kp, dim, chunk;
    while (std::scanf("%lld %lld %lld %lld %lld %lld", &kind, &n, &N, &kp, &dim, &chunk) == 6) {
        if (kind == 0) { const avae::KnnPlan p = avae::knn_plan((int)n, (int)N, (int)kp, (int)chunk); std::printf("%d %d 0 %d %d\n", p.qrows, p.qtiles, p.parts, p.chunk); }
        else if (kind == 1) { const avae::AggPlan p = avae::agg_plan((int)n, (int)N, (int)dim, (int)chunk); std::printf("0 %d 0 %d %d\n", p.qtiles, p.parts, p.chunk); }
        else { const avae::ProbePlan p = avae::probe_plan((int)N, (int)kp, (int)dim, (int)chunk); std::printf("%d %d %d %d %d\n", p.ptiles, p.Ppad, p.LD, p.parts, p.chunk); }
    }
    return 0;
}
"""


def around(*centres):
    return sorted({c + d for c in centres for d in (-1, 0, 1) if 1 <= c + d <= NMAX} | {1, NMAX})


def build_inputs():
    rows = []
    for n in NS:
        for k in KS:                                    # knn: tile 128
            max_parts = min(512, 48 * 1024 // (12 * k) - 1)
            qrows = 32 if n <= 64 else 128
            qtiles = -(-n // qrows)
            want = min(max_parts, -(-(256 * (4 if qrows == 32 else 1)) // qtiles))
            for N in [0] + around(128 * want, 128 * max_parts):
                rows += [(0, n, N, k, 128, c) for c in CHUNKS]
        qtiles = -(-n // 128)                           # agg: tile 64, at most 1024 parts
        want = min(1024, -(-1024 // qtiles))
        for N in around(64 * want, 64 * 1024):
            rows += [(1, n, N, 0, 128, c) for c in CHUNKS]
    for P in PS:                                        # probe: tile 128, want 256 = the part limit
        for N in around(128 * 256):
            rows += [(2, 0, N, P, 36, c) for c in CHUNKS]
    return np.array(sorted(set(rows)), dtype=np.int64)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', required=True, help='a checkout of the parent commit')
    ap.add_argument('--parent', required=True, help="the parent's abbreviated hash, stored in the file")
    ap.add_argument('--out', default=os.path.join(HERE, 'latent_plan_parent.npz'))
    A = ap.parse_args(argv)
    csrc = os.path.join(os.path.abspath(A.tree), 'argsim_amd', 'csrc')
    inputs = build_inputs()
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, 'main.hip'), 'w') as f:
            f.write(MAIN)
        prog = os.path.join(tmp, 'plans')
        subprocess.run(['hipcc', '-O1', '-std=c++17', '--offload-arch=gfx950', '-I', csrc, os.path.join(tmp, 'main.hip')]
                       + [os.path.join(csrc, f) for f in ('knn.hip', 'agg.hip', 'probe.hip')] + ['-o', prog], check=True)
        text = '\n'.join(' '.join(str(v) for v in r) for r in inputs.tolist()) + '\n'
        out = subprocess.run([prog], input=text, capture_output=True, text=True, check=True).stdout
    plan = np.array([[int(v) for v in line.split()] for line in out.strip().split('\n')], dtype=np.int32)
    assert plan.shape == (len(inputs), 5), plan.shape
    np.savez(A.out, parent=np.array(A.parent), fields=np.array(['kind', 'n', 'N', 'k_or_P', 'dim', 'chunk_opt']), inputs=inputs, plan=plan)
    print("wrote %s: %d rows" % (A.out, len(inputs)))


if __name__ == '__main__':
    main()
