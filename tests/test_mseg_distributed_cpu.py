"""MultiClassScores.all_reduce under gloo: two spawned ranks, each with its own images, end with the one-rank sums (the
spawn pattern of tests/test_distributed_cpu.py)."""
import os
import socket

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

from conceptattention_amd.distributed import shard_items
from conceptattention_amd.segmentation import MultiClassScores

NCLASS, N_ITEMS, IGNORE = 21, 5, 255


def _item(i):
    rng = np.random.default_rng(900 + i)
    pred = rng.integers(0, NCLASS, size=(12, 10))
    lab = np.where(rng.random((12, 10)) < 0.6, pred, rng.integers(0, NCLASS, size=(12, 10)))
    lab[0] = 255
    return pred, lab


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    scores = MultiClassScores(NCLASS)
    for i in shard_items(N_ITEMS, rank, world):
        scores.update(*_item(i), ignore_index=IGNORE)
    local_n = scores.n
    scores.all_reduce()
    q.put((rank, local_n, scores.correct, scores.labelled, scores.n, scores.inter.tolist(), scores.union.tolist(),
           scores.result()["mIoU"]))
    dist.destroy_process_group()


def test_all_reduce_gloo_world2_equals_the_one_rank_sum():
    one = MultiClassScores(NCLASS)
    for i in range(N_ITEMS):
        one.update(*_item(i), ignore_index=IGNORE)
    assert one.all_reduce() is one and one.n == N_ITEMS          # no process group: a no-op
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
    assert sorted(r[1] for r in res) == [2, 3]
    for _, _, correct, labelled, n, inter, union, miou in res:
        assert (correct, labelled, n) == (one.correct, one.labelled, one.n)
        assert inter == one.inter.tolist() and union == one.union.tolist()
        assert miou == one.result()["mIoU"]
