"""ca_segtab_score on the GPU against its numpy restatement (tests/segtab_cases.py): the four counts, thresholds, mean, lo
and hi bit for bit (a NaN as a NaN: its sign and payload are the adder's own), the AP within 1e-12 (derived in
tests/seg_cases.py); without RAW the same against what ops.seg_score writes for the same (map, label).  The unscored
concept planes are NaN, the map table, the records and the workspace are followed by guard elements, and the workspace
starts as garbage: none of it may show."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import placement  # noqa: E402
import segtab_cases as T  # noqa: E402
import stream_gate  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
AP_TOL = 1e-12
GUARD = 64                        # guard elements behind the map table, the records (bytes) and the workspace
RECORD = np.dtype([("n11", "<i4"), ("n10", "<i4"), ("n01", "<i4"), ("n00", "<i4"), ("ap", "<f8"), ("mean", "<f4"),
                   ("lo", "<f4"), ("hi", "<f4"), ("thresholds", "<i4")])
assert RECORD.itemsize == ctypes.sizeof(L.SegRecord) == 40
MAP_GUARD, REC_GUARD, CELL_GUARD = 7.25e30, 0xAB, 0x5A5A5A5A


def table_buffer(maps, C, target) -> np.ndarray:
    """fp32 [n C h w + GUARD]: plane ``target`` of every map holds the map, the other planes NaN, guard elements behind."""
    n, h, w = maps.shape
    full = np.full((n, C, h, w), np.nan, dtype=np.float32)
    full[:, target] = maps
    return np.concatenate([full.reshape(-1), np.full(GUARD, MAP_GUARD, dtype=np.float32)])


def launch(maps, label, C=1, target=0, alloc=None, cells_fill=CELL_GUARD, **flags):
    """The records of one ops.segtab_score call as a RECORD array [n]; checks the inputs and every guard element."""
    n, h, w = maps.shape
    hw4 = (h * w + 3) & ~3
    al = alloc or placement.Plain(DEV)
    tab = table_buffer(maps, C, target)
    md = al.to(torch.from_numpy(tab), {"maps": None})
    ld = al.to(torch.from_numpy(label), {"label": None})
    res = al.full((n * 40 + GUARD,), REC_GUARD, torch.uint8, {"records": None})
    cells = al.full((4 * hw4 + GUARD,), cells_fill, torch.int32, {"cells": None})
    ops.segtab_score(md[:n * C * h * w].view(n, C, h, w) if C > 1 else md[:n * h * w].view(n, h, w), target, ld,
                     res[:n * 40].view(n, 40), cells[:4 * hw4].view(4, hw4),
                     mean_value_threshold=flags.get("mean_value_threshold", True),
                     downscale_for_eval=flags.get("downscale_for_eval", False),
                     blur_weights=ops.seg_blur_weights() if flags.get("apply_blur") else None,
                     normalize=flags.get("normalize", True))
    torch.cuda.synchronize()
    assert np.array_equal(md.cpu().numpy().view(np.uint32), tab.view(np.uint32)), "the map table changed"
    assert np.array_equal(ld.cpu().numpy(), label), "the label changed"
    out = res.cpu().numpy()
    assert (out[n * 40:] == REC_GUARD).all(), "bytes behind the records were written"
    ws = cells.cpu().numpy()
    assert (ws[4 * hw4:] == cells_fill).all(), "words behind the workspace were written"
    return out[:n * 40].copy().view(RECORD).reshape(n), ws[:4 * hw4].reshape(4, hw4)


def same_f32(a, b) -> bool:
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


def check(rec, ref, what, ap_of=None):
    for k in ("n11", "n10", "n01", "n00", "thresholds"):
        assert int(rec[k]) == int(ref[k]), (what, k, int(rec[k]), int(ref[k]))
    for k in ("mean", "lo", "hi"):
        assert same_f32(rec[k], ref[k]), (what, k, rec[k], ref[k])
    diff = abs(float(rec["ap"]) - float(ref["ap"]))
    assert diff <= AP_TOL, (what, float(rec["ap"]), float(ref["ap"]), diff)
    return diff


def seg_score_records(maps, label, **flags) -> np.ndarray:
    """What ops.seg_score writes for the same maps, each against the same label."""
    n = len(maps)
    md = torch.from_numpy(np.ascontiguousarray(maps)).to(DEV)
    ld = torch.from_numpy(label).to(DEV)
    res = torch.zeros(n, 40, dtype=torch.uint8, device=DEV)
    ops.seg_score(list(md), [ld] * n, res, mean_value_threshold=flags.get("mean_value_threshold", True),
                  downscale_for_eval=flags.get("downscale_for_eval", False),
                  blur_weights=ops.seg_blur_weights() if flags.get("apply_blur") else None)
    return res.cpu().numpy().view(RECORD).reshape(n)


def run_case(case, alloc=None):
    maps, label = case.inputs()
    refs = case.references(maps, label)
    rec, ws = launch(maps, label, case.C, case.target, alloc=alloc, **case.flags)
    worst = max(check(rec[m], refs[m], (case.name, m)) for m in range(case.n_maps))
    print(case.name, "maps", case.n_maps, "worst |ap - restatement|", worst)
    tab = T.tables(case.h, case.w, label, case.flags["downscale_for_eval"])
    assert np.array_equal(ws[:, :case.h * case.w].astype(np.int64), tab), "the workspace after the label pass"
    assert (ws[:, case.h * case.w:] == 0).all()
    return rec, ws, maps, label


@pytest.mark.parametrize("case", T.CASES, ids=repr)
def test_every_case_equals_the_restatement_and_seg_score(case):
    rec, ws, maps, label = run_case(case)
    if case.flags["normalize"]:
        k = min(case.n_maps, 32)                                      # (two launches of ca_seg_score at the most)
        flags = {f: v for f, v in case.flags.items() if f != "normalize"}
        one = seg_score_records(maps[:k], label, **flags)
        worst = max(check(rec[m], one[m], (case.name, m, "seg_score")) for m in range(k))
        print(case.name, "worst |ap - seg_score|", worst)


def test_a_record_does_not_depend_on_its_position_the_launch_or_the_workspace():
    h, w, Hl, Wl = 16, 16, 224, 224
    maps = T.table_maps(h, w, 301, seed=40)
    maps[300] = maps[0]
    label = T.seeded_label(h, w, Hl, Wl, 40)
    a, ws_a = launch(maps, label, C=4, target=3)
    assert a[0].tobytes() == a[300].tobytes(), "one map at position 0 and at position 300"
    b, ws_b = launch(maps, label, C=4, target=3)
    assert a.tobytes() == b.tobytes() and np.array_equal(ws_a, ws_b), "two launches of one input differ"
    c, ws_c = launch(maps, label, C=4, target=3, cells_fill=-1)       # another garbage in the workspace
    assert a.tobytes() == c.tobytes() and np.array_equal(ws_a, ws_c), "the workspace's old contents show"
    d, _ = launch(maps[:1], label)                                    # alone, at stride h w
    assert a[0].tobytes() == d[0].tobytes()
    check(a[0], T.reference(maps[0], label), "position 0")


def test_any_nonzero_label_byte_is_positive_and_a_non_default_stream_works():
    h, w = 16, 16
    maps = T.table_maps(h, w, 6, seed=50)
    label = T.seeded_label(h, w, 64, 64, 50)
    refs = [T.reference(m, label) for m in maps]
    bytes_ = (label * np.random.default_rng(0).integers(1, 256, size=label.shape)).astype(np.uint8)
    stream = torch.cuda.Stream()
    # (behind a gate, tests/stream_gate.py: a launch on another stream would read poison instead of these inputs)
    warm = stream_gate.Recording(DEV)
    launch(maps, bytes_, C=4, target=1, alloc=warm)
    with torch.cuda.stream(stream):
        rec, _ = launch(maps, bytes_, C=4, target=1, alloc=stream_gate.Gated(warm, stream_gate.Gate()))
    stream.synchronize()
    for m in range(6):
        check(rec[m], refs[m], ("label bytes 1..255 on a side stream", m))


def test_the_wrapper_rejects_what_the_kernel_cannot_take():
    res = torch.zeros(2, 40, device=DEV, dtype=torch.uint8)
    lab = torch.zeros(8, 8, device=DEV, dtype=torch.uint8)
    ok = torch.zeros(2, 3, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="4096"):
        ops.segtab_score(torch.zeros(2, 65, 64, device=DEV), 0, lab, res)
    with pytest.raises(ValueError):
        ops.segtab_score(ok.double(), 0, lab, res)
    with pytest.raises(ValueError):
        ops.segtab_score(ok, 3, lab, res)                              # no such concept plane
    with pytest.raises(ValueError):
        ops.segtab_score(ok[:, :, :, :4], 0, lab, res)                 # not contiguous
    with pytest.raises(ValueError):
        ops.segtab_score(ok, 0, lab.bool(), res)
    with pytest.raises(ValueError):
        ops.segtab_score(ok, 0, lab, res[:1])
    with pytest.raises(ValueError):
        ops.segtab_score(ok, 0, lab, res, cells=torch.zeros(4, 60, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match=">= 2"):
        ops.segtab_score(torch.zeros(2, 1, 8, device=DEV), 0, lab, res, blur_weights=ops.seg_blur_weights())
    ops.segtab_score(ok, 2, lab, res)                                  # and the call itself is fine
    torch.cuda.synchronize()
