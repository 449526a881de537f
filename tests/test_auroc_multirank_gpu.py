"""Distributed compute() of torchrec_amd.metrics: two ranks on ONE GPU over gloo (the set-up of tests/test_multirank_gpu.py),
unequal sample counts per rank, a rank with no samples at all.  Every rank must return the value of the concatenated
data — exactly the host model's float (tests/_auroc_ref.py)."""
import datetime
import os
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _paths  # noqa: F401
import _auroc_ref as ref
from _results import ResultStore
from test_sharded_gloo import _free_port

pytestmark = pytest.mark.gpu

COUNTS = [(1000, 37), (1000, 0)]  # samples of (rank 0, rank 1) in round 0 and round 1
THRESHOLD = 0.4
SPAWN_TIMEOUT_S = 120


def _data(rnd, rank):
    rng = np.random.default_rng(100 * rnd + rank)
    n = COUNTS[rnd][rank]
    x = (rng.integers(0, 50, size=n) / 50).astype(np.float32)  # ties within and across the ranks
    y = (rng.random(n) < 0.2 + 0.6 * x).astype(np.int64)
    return x, y


def _worker(rank, W, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=W, timeout=datetime.timedelta(seconds=SPAWN_TIMEOUT_S))
    try:
        from torchrec_amd.metrics import AUROC, Accuracy

        auroc = AUROC(compute_on_step=False).to(dev)
        accuracy = Accuracy(threshold=THRESHOLD, process_group=dist.group.WORLD).to(dev)
        out = []
        for rnd in range(len(COUNTS)):
            auroc.reset()
            accuracy.reset()
            x, y = _data(rnd, rank)
            if x.size:  # a rank without samples never calls update
                for part in np.array_split(np.arange(x.size), 3):
                    # float targets on one rank, integer ones on the other: the gather must not care
                    t = torch.from_numpy(y[part]).to(dev)
                    auroc(torch.from_numpy(x[part]).to(dev), t.float() if rank == 0 else t)
                    accuracy(torch.from_numpy(x[part]).to(dev), t)
            out.append((auroc.compute().item(), accuracy.compute().item()))
        ret[rank] = out
    finally:
        dist.destroy_process_group()


def test_compute_over_two_ranks_equals_the_model_on_the_concatenation():
    W = 2
    ret = ResultStore()
    ctx = mp.spawn(_worker, args=(W, _free_port(), ret), nprocs=W, join=False)
    deadline = time.monotonic() + SPAWN_TIMEOUT_S
    while not ctx.join(timeout=5):  # returns as soon as a worker ends; raises if one failed
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"the two ranks did not finish within {SPAWN_TIMEOUT_S} s (a collective that not every rank entered?)")
    for rnd in range(len(COUNTS)):
        parts = [_data(rnd, r) for r in range(W)]
        x, y = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        want = (ref.auroc(ref.counts(x, y)), ref.accuracy(ref.counts(x, y, THRESHOLD)))
        for r in range(W):
            assert ret[r][rnd] == want, (rnd, r, ret[r][rnd], want)
