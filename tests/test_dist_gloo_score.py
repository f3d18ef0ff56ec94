"""summ_iw under data parallelism on the host: two gloo ranks validate their share of the chunks and add the three sums, the way
tests/test_dist_gloo.py exercises summ."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _ScoreStub:
    """VAE.score on the host: values that depend only on the ids"""
    def score(self, src, tgt=None, k=1, seed=0, eps=None, return_parts=False):
        ntok = ((src != 1).sum(1) + 1).astype(np.int32)
        r = np.random.default_rng(int(src.sum()) + k + seed)
        return dict(bound=(-3.0 * ntok * (1 + r.random(len(src)))).astype(np.float32), ntok=ntok)


def _valid():
    rng = np.random.default_rng(5)
    ids = np.ones((48, 10), np.int32)
    for b in range(48):
        n = int(rng.integers(1, 11)); ids[b, :n] = rng.integers(3, 50, n)
    return ids


def _worker(rank, world, port, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    sys.path.insert(0, ROOT)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    host = dist.new_group(backend='gloo')
    from argsim_amd.train import summ_iw
    mine = summ_iw(_ScoreStub(), _valid(), 5, 4, 3, rank, world, host)
    torch.save({'iw': mine}, out + str(rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_report_the_sums_of_one_process(tmp_path):
    out = str(tmp_path / 'iw.pt')
    port = 33500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    from argsim_amd.train import summ_iw
    one = summ_iw(_ScoreStub(), _valid(), 5, 4, 3)
    for rank in range(2):
        got = torch.load(out + str(rank), weights_only=True)['iw']
        assert np.allclose(got, one, rtol=1e-12, atol=0), (rank, got, one)
