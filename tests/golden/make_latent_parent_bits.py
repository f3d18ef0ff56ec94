#!/usr/bin/env python3
"""records tests/golden/latent_parent_bits.npz: the SHA-256 of every output of tests/test_gpu_latent_parent.py's cases, from a BUILT
checkout of the parent commit, on an MI355X.

    git worktree add /tmp/parent <hash> && make -C /tmp/parent/argsim_amd/csrc -j16
    python tests/golden/make_latent_parent_bits.py --tree /tmp/parent --parent <hash> [--out FILE]

The package, the case generators and the test helpers are the parent tree's; only the list of cases (test_gpu_latent_parent.digests)
comes from this tree.  Never run it on the code under test: see that file's docstring for when the table may be recorded again."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', required=True, help='a built checkout of the parent commit')
    ap.add_argument('--parent', required=True, help="the parent's abbreviated hash, stored in the file")
    ap.add_argument('--out', default=os.path.join(HERE, 'latent_parent_bits.npz'))
    A = ap.parse_args(argv)
    tree = os.path.abspath(A.tree)
    sys.path[:0] = [tree, os.path.join(tree, 'tests')]
    sys.path.append(os.path.dirname(HERE))
    import argsim_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(argsim_amd.__file__))) == tree, argsim_amd.__file__
    import test_gpu_latent_parent as t
    out, inp = {}, {}
    for family in t.FAMILIES:
        o, i = t.digests(family)
        again, _ = t.digests(family)
        assert o == again, "%s: two runs of the parent differ" % family
        print("%-9s %4d outputs, %3d inputs" % (family, len(o), len(i)), flush=True)
        out.update(o)
        inp.update(i)
    names, inames = sorted(out), sorted(inp)
    np.savez(A.out, parent=np.array(A.parent), names=np.array(names), digests=np.array([out[k] for k in names]),
             input_names=np.array(inames), input_digests=np.array([inp[k] for k in inames]))
    print("wrote %s: %d outputs" % (A.out, len(names)))


if __name__ == '__main__':
    main()
