"""The three Device*Scores classes on ``device="cpu"``: one growable row buffer behind all of them (earlier rows survive
growth, one download until new rows are reserved, ``to_host`` equals feeding the host class the same rows), ``all_reduce``
without a process group changes nothing, and the encoding methods reject an unknown keyword with one text."""
import numpy as np
import pytest
import torch

from conceptattention_amd import segmentation as S

CHUNK = 4


def _records(n, seed) -> np.ndarray:
    """n seeded records of SEG_RECORD (plausible counts of a 7 x 7 label)."""
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, dtype=S.SEG_RECORD)
    for k in ("n11", "n10", "n01", "n00"):
        rec[k] = rng.integers(0, 13, size=n)
    rec["ap"] = rng.random(n)
    rec["mean"], rec["lo"], rec["hi"] = rng.random(n), -rng.random(n), 1 + rng.random(n)
    rec["thresholds"] = rng.integers(1, 99, size=n)
    return rec


def _fill(view: torch.Tensor, rows: np.ndarray) -> None:
    view.copy_(torch.from_numpy(rows.view(np.uint8).reshape(len(rows), -1) if rows.dtype == S.SEG_RECORD else rows))


@pytest.fixture
def downloads(monkeypatch):
    """Counts Tensor.cpu() calls: the download of a Device*Scores."""
    calls = []
    real = torch.Tensor.cpu

    def cpu(self, *a, **k):
        calls.append(tuple(self.shape))
        return real(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "cpu", cpu)
    return calls


def _same(a: dict, b: dict) -> None:
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def test_segmentation_scores_grow_keep_their_rows_and_download_once(downloads):
    dev = S.DeviceSegmentationScores("cpu", chunk=CHUNK)
    assert (dev.n, dev.chunk, dev.device, dev._pixels) == (0, CHUNK, torch.device("cpu"), [])
    rec = _records(2 * CHUNK + 3, 1)
    _fill(dev.reserve(3, 49), rec[:3])
    first = dev.records().copy()
    _fill(dev.reserve(CHUNK, 49), rec[3:3 + CHUNK])              # across the chunk boundary
    _fill(dev.reserve(CHUNK, 64), rec[3 + CHUNK:])               # and across the next one
    assert dev.n == len(rec) and dev._pixels == [49] * (3 + CHUNK) + [64] * CHUNK
    assert first.tobytes() == rec[:3].tobytes() and dev.records().tobytes() == rec.tobytes()
    before = len(downloads)
    dev.records(), dev.to_host(), dev.result()
    assert len(downloads) == before, "a second download without a new reserve"
    _fill(dev.reserve(1, 64), rec[:1])
    assert dev.records()[-1].tobytes() == rec[0].tobytes() and len(downloads) == before + 1
    host = S.SegmentationScores()
    for r, n_px in zip(np.concatenate([rec, rec[:1]]), dev._pixels):
        agree = int(r["n11"]) + int(r["n00"])
        host.correct, host.labelled = host.correct + 2 * agree, host.labelled + 2 * n_px
        host.inter, host.union = host.inter + agree, host.union + (2 * n_px - agree)
        host.ap_sum, host.n = host.ap_sum + float(r["ap"]), host.n + 1
    _same(dev.to_host().result(), host.result())
    _same(dev.result(), host.result())


def test_sweep_scores_grow_keep_their_rows_and_download_once(downloads):
    levels, layers = 3, 2
    dev = S.DeviceSweepScores(levels, layers + 1, "cpu", chunk=CHUNK)
    assert (dev.n, dev.chunk, dev.device, dev.n_levels, dev.n_columns) == (0, CHUNK, torch.device("cpu"), levels, layers + 1)
    with pytest.raises(ValueError, match="space"):
        dev.reserve("nowhere", 49)
    calls = [("output", list(range(layers)), 49), ("output", [layers], 49), ("cross_attention", list(range(layers)), 64)]
    rows = [_records(levels * len(cols), 10 + i) for i, (_, cols, _) in enumerate(calls)]
    host = S.SweepScores(levels, layers + 1)
    for (space, cols, n_px), rec in zip(calls, rows):             # 6 + 3 + 6 records: two growths of 4
        _fill(dev.reserve(space, n_px, cols), rec)
        host.add_records(space, rec, n_px, cols)
    assert dev.n == sum(len(r) for r in rows)
    got = dev.records()
    assert [(s, c) for s, c, _ in got] == [(s, c) for s, c, _ in calls]
    for (_, cols, rec), want in zip(got, rows):
        assert rec.shape == (levels, len(cols)) and rec.tobytes() == want.tobytes()
    before = len(downloads)
    dev.records(), dev.to_host(), dev.result("output"), list(dev.rows("cross_attention"))
    assert len(downloads) == before, "a second download without a new reserve"
    for space in S.SWEEP_SPACES:
        _same(dev.result(space), host.result(space))
    _fill(dev.reserve("output", 49, [0]), rows[1])
    assert dev.records()[-1][2].tobytes() == rows[1].tobytes() and len(downloads) == before + 1


def test_multi_class_scores_grow_keep_their_rows_and_download_once(downloads):
    nclass = 5
    dev = S.DeviceMultiClassScores(nclass, "cpu", chunk=CHUNK)
    assert (dev.n, dev.chunk, dev.device, dev.nclass, dev.width, dev.ids) == (0, CHUNK, torch.device("cpu"), nclass, 12, [])
    counts = np.random.default_rng(3).integers(0, 1000, size=(2 * CHUNK + 1, 12)).astype(np.int32)
    _fill(dev.reserve(3), counts[:3])
    _fill(dev.reserve(CHUNK, ids=[9, 8, 7, 6]), counts[3:3 + CHUNK])
    _fill(dev.reserve(CHUNK - 2), counts[3 + CHUNK:])
    assert dev.n == len(counts) and dev.ids == [0, 1, 2, 9, 8, 7, 6, 7, 8]
    assert dev.records().dtype == np.int32 and np.array_equal(dev.records(), counts)
    before = len(downloads)
    dev.records(), dev.to_host(), dev.result()
    assert len(downloads) == before, "a second download without a new reserve"
    host = S.MultiClassScores(nclass)
    for row in counts:
        host.add_counts(row)
    _same(dev.result(), host.result())
    dev.reserve(1).fill_(2)
    assert (dev.records()[-1] == 2).all() and len(downloads) == before + 1


def test_all_reduce_without_a_process_group_changes_nothing():
    assert S._all_reduce_vector(torch.arange(4, dtype=torch.float64)) is None
    seg = S.DeviceSegmentationScores("cpu", chunk=CHUNK)
    _fill(seg.reserve(3, 49), _records(3, 4))
    one = seg.to_host()
    want = one.result()
    assert one.all_reduce() is one
    _same(one.result(), want)
    _same(seg.all_reduce().result(), want)
    sweep = S.SweepScores(2, 2).add_records("output", _records(4, 5), 49)
    want = {s: sweep.result(s) for s in S.SWEEP_SPACES}
    assert sweep.all_reduce() is sweep and sweep.tables["output"]["n"].dtype == np.int64
    for s in S.SWEEP_SPACES:
        _same(sweep.result(s), want[s])
    multi = S.MultiClassScores(3).add_counts(np.arange(8))
    want = multi.result()
    assert multi.all_reduce() is multi and multi.inter.dtype == np.int64
    _same(multi.result(), want)


def test_the_encoding_methods_reject_an_unknown_keyword_with_one_text():
    model = S.ConceptAttentionSegmentationModel(pipeline=None)     # (the arguments are checked before the pipeline is used)
    label = np.zeros((8, 8), dtype=np.uint8)
    with pytest.raises(TypeError, match=r"^score_images: unexpected arguments \['layer', 'steps'\]$"):
        model.score_images(["image"], ["cat"], ["cat", "sky"], ["a cat"], [label], None, size=8, steps=4, layer=1, seed=0)
    with pytest.raises(TypeError, match=r"^score_multiclass_images: unexpected arguments \['layer', 'steps'\]$"):
        model.score_multiclass_images(["image"], ["a cat"], ["sky"], [["cat"]], ["background", "cat"], [label], None,
                                      steps=4, layer=1, seed=0)
    with pytest.raises(TypeError, match=r"^segment_multiclass: unexpected arguments \['layer', 'steps'\]$"):
        model.segment_multiclass(["image"], ["a cat"], ["sky"], [["cat"]], steps=4, layer=1, seed=0)
    assert S._ENCODE_KEYS == {"layers", "num_samples", "num_steps", "noise_timestep", "seed", "height", "width", "batch",
                              "joint_attention_kwargs", "noise", "vae_noise", "attention_norm", "softmax"}
