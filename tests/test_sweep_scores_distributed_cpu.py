"""SweepScores on the CPU: update against SegmentationScores cell by cell, add_records against update's counters, rows() in
CSV order, and all_reduce under gloo: two spawned ranks, each with its own images, end with the one-rank tables (the spawn
pattern of tests/test_distributed_cpu.py)."""
import os
import socket

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

from conceptattention_amd.distributed import shard_items
from conceptattention_amd.segmentation import SEG_RECORD, SWEEP_SPACES, SegmentationScores, SweepScores

LEVELS, COLUMNS, N_ITEMS, SIDE = 3, 4, 5, 12
FIELDS = ("correct", "labelled", "inter", "union", "ap_sum", "n")


def _item(i, space, level, column):
    """(mask, coefficients, labels) at the label resolution for one cell of one image's sweep."""
    rng = np.random.default_rng(((700 + i) * 7 + SWEEP_SPACES.index(space)) * 100 + level * 10 + column)
    c = rng.random((SIDE, SIDE), dtype=np.float32)
    labels = (c + 0.3 * rng.standard_normal((SIDE, SIDE)) > 0.5)
    return c > c.mean(), c, labels


def _fill(scores, items):
    for i in items:
        for space in SWEEP_SPACES:
            for lv in range(LEVELS):
                for col in range(COLUMNS):
                    scores.update(space, lv, col, *_item(i, space, lv, col))
    return scores


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    scores = _fill(SweepScores(LEVELS, COLUMNS), shard_items(N_ITEMS, rank, world))
    local_n = int(scores.tables["output"]["n"][0, 0])
    scores.all_reduce()
    q.put((rank, local_n, {s: {k: np.asarray(v).tolist() for k, v in scores.tables[s].items()} for s in SWEEP_SPACES},
           list(scores.rows("cross_attention"))))
    dist.destroy_process_group()


def test_update_is_segmentation_scores_per_cell_and_rows_come_in_csv_order():
    scores = _fill(SweepScores(LEVELS, COLUMNS), range(N_ITEMS))
    for space in SWEEP_SPACES:
        res = scores.result(space)
        for lv in range(LEVELS):
            for col in range(COLUMNS):
                one = SegmentationScores()
                for i in range(N_ITEMS):
                    one.update(*_item(i, space, lv, col))
                t = scores.tables[space]
                assert (t["correct"][lv, col], t["labelled"][lv, col], t["n"][lv, col]) == (one.correct, one.labelled, one.n)
                assert np.array_equal(t["inter"][lv, col], one.inter) and np.array_equal(t["union"][lv, col], one.union)
                want = one.result()
                assert abs(t["ap_sum"][lv, col] - one.ap_sum) <= 1e-12
                assert res["pixAcc"][lv, col] == want["pixAcc"] and res["mIoU"][lv, col] == want["mIoU"]
                assert abs(res["mAP"][lv, col] - want["mAP"]) <= 1e-12
        rows = list(scores.rows(space))
        assert [(lv, col) for lv, col, *_ in rows] == [(lv, col) for lv in range(LEVELS) for col in range(COLUMNS)]
        assert all(r[2:] == (res["pixAcc"][r[0], r[1]], res["mIoU"][r[0], r[1]], res["mAP"][r[0], r[1]]) for r in rows)


def test_add_records_counts_what_update_counts():
    """A record's n11 / n00 give update's counters through the (1 - m, m) double counting; a subset of columns lands in
    those columns alone."""
    scores, want = SweepScores(LEVELS, COLUMNS), SweepScores(LEVELS, COLUMNS)
    cols = [1, 3]
    rec = np.zeros((LEVELS, len(cols)), dtype=SEG_RECORD)
    for lv in range(LEVELS):
        for j, col in enumerate(cols):
            m, c, y = _item(0, "output", lv, col)
            out = want.update("output", lv, col, m, c, y)
            rec[lv, j]["n11"], rec[lv, j]["n00"] = int((m & y).sum()), int((~m & ~y).sum())
            rec[lv, j]["n10"], rec[lv, j]["n01"] = int((m & ~y).sum()), int((~m & y).sum())
            rec[lv, j]["ap"] = out["ap"]
    scores.add_records("output", rec, SIDE * SIDE, cols)
    for k in FIELDS:
        assert np.array_equal(scores.tables["output"][k], want.tables["output"][k]), k
        assert not np.asarray(scores.tables["cross_attention"][k]).any()
    assert (scores.tables["output"]["n"][:, [0, 2]] == 0).all()


def test_all_reduce_gloo_world2_equals_the_one_rank_tables():
    one = _fill(SweepScores(LEVELS, COLUMNS), range(N_ITEMS))
    assert one.all_reduce() is one and (one.tables["output"]["n"] == N_ITEMS).all()       # no process group: a no-op
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
    for _, _, tables, rows in res:
        for s in SWEEP_SPACES:
            for k in ("correct", "labelled", "inter", "union", "n"):
                assert tables[s][k] == np.asarray(one.tables[s][k]).tolist(), (s, k)
            assert np.abs(np.asarray(tables[s]["ap_sum"]) - one.tables[s]["ap_sum"]).max() <= 1e-12
        for got, want in zip(rows, one.rows("cross_attention")):
            assert got[:4] == want[:4] and abs(got[4] - want[4]) <= 1e-12
