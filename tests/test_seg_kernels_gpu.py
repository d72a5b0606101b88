"""ca_seg_score on the GPU against its numpy restatement (tests/seg_cases.py): the four counts, thresholds, mean, lo, hi,
the mask and the coefficient bit for bit (NaN positions as NaN), the AP within 1e-12 and the same bits every launch."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import placement  # noqa: E402
import seg_cases as T  # noqa: E402
import stream_gate  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
AP_TOL = 1e-12
RECORD = np.dtype([("n11", "<i4"), ("n10", "<i4"), ("n01", "<i4"), ("n00", "<i4"), ("ap", "<f8"), ("mean", "<f4"),
                   ("lo", "<f4"), ("hi", "<f4"), ("thresholds", "<i4")])
assert RECORD.itemsize == ctypes.sizeof(L.SegRecord) == 40


def _launch(maps, labels, mean_value_threshold=True, downscale_for_eval=False, apply_blur=False, outputs=True, alloc=None):
    """(records, masks, coefficients) of one ops.seg_score call; poisoned outputs show what nobody wrote.  ``alloc``: an
    allocator of tests/placement.py for the five operand roles (one item)."""
    n, (h, w) = len(maps), maps[0].shape
    al = alloc or placement.Plain(DEV)
    assert alloc is None or n == 1
    md = [al.to(torch.from_numpy(m), {"map": None}) for m in maps]
    ld = [al.to(torch.from_numpy(l), {"label": None}) for l in labels]
    res = al.full((n, 40), 0xAB, torch.uint8, {"result": None})
    mask = al.full((n, h, w), 77, torch.uint8, {"mask_out": None}) if outputs else None
    coeff = al.full((n, h, w), -3.0, torch.float32, {"coeff_out": None}) if outputs else None
    ops.seg_score(md, ld, res, mean_value_threshold=mean_value_threshold, downscale_for_eval=downscale_for_eval,
                  blur_weights=ops.seg_blur_weights() if apply_blur else None, mask_out=mask, coeff_out=coeff)
    torch.cuda.synchronize()
    for d, t in list(zip(md, maps)) + list(zip(ld, labels)):
        assert np.array_equal(d.cpu().numpy(), t), "an input changed"
    rec = res.cpu().numpy().view(RECORD).reshape(n)
    return rec, (mask.cpu().numpy() if outputs else None), (coeff.cpu().numpy() if outputs else None)


def _check(rec, mask, coeff, ref, what):
    for k in ("n11", "n10", "n01", "n00", "thresholds"):
        assert int(rec[k]) == ref[k], (what, k, int(rec[k]), ref[k])
    for k in ("mean", "lo", "hi"):
        assert np.float32(rec[k]).tobytes() == np.float32(ref[k]).tobytes(), (what, k, rec[k], ref[k])
    print(what, "ap", float(rec["ap"]), "restatement", ref["ap"], "diff", abs(float(rec["ap"]) - ref["ap"]))
    assert abs(float(rec["ap"]) - ref["ap"]) <= AP_TOL, (what, float(rec["ap"]), ref["ap"])
    if mask is not None:
        assert np.array_equal(mask, ref["mask"]), what
        nan = np.isnan(ref["coeff"])
        assert np.array_equal(np.isnan(coeff), nan), what
        assert np.array_equal(coeff[~nan].view(np.uint32), ref["coeff"][~nan].view(np.uint32)), what


@pytest.mark.parametrize("case", T.CASES, ids=repr)
def test_every_case_equals_the_restatement(case):
    run_case(case)


def run_case(case, alloc=None):
    """One case of seg_cases.CASES, its five buffers from an optional allocator, checked against the restatement;
    returns the record, the mask and the coefficient as tensors of bytes."""
    amap, label = case.inputs()
    ref = T.reference(amap, label, **case.flags)
    rec, mask, coeff = _launch([amap], [label], alloc=alloc, **case.flags)
    _check(rec[0], mask[0], coeff[0], ref, case.name)
    if alloc is not None:
        return {"result": torch.from_numpy(rec[:1].copy().view(np.uint8)), "mask_out": torch.from_numpy(mask.copy()),
                "coeff_out": torch.from_numpy(coeff.copy())}
    again, _, _ = _launch([amap], [label], outputs=False, **case.flags)     # (and without the optional outputs)
    assert rec[0].tobytes() == again[0].tobytes(), "two launches of one input differ"


def test_a_launch_of_the_cap_equals_the_single_launches():
    maps, labels = T.cap_launch_inputs()
    assert len(maps) == L.SEG_MAX_PROBLEMS == T.MAX_PROBLEMS
    rec, mask, coeff = _launch(maps, labels)
    for i in range(len(maps)):
        one, m1, c1 = _launch([maps[i]], [labels[i]])
        assert rec[i].tobytes() == one[0].tobytes(), i
        assert np.array_equal(mask[i], m1[0]) and np.array_equal(coeff[i].view(np.uint32), c1[0].view(np.uint32)), i
    _check(rec[5], mask[5], coeff[5], T.reference(maps[5], labels[5]), "item 5 of 16")
    # more items than the cap go in several launches
    more, _, _ = _launch(maps + maps[:3], labels + labels[:3], outputs=False)
    assert more[:16].tobytes() == rec.tobytes() and more[16:].tobytes() == rec[:3].tobytes()


def test_any_nonzero_label_byte_is_positive_and_a_non_default_stream_works():
    case = next(c for c in T.CASES if c.name == "map16x16-label64x64")
    amap, label = case.inputs()
    ref = T.reference(amap, label)
    bytes_ = (label * np.random.default_rng(0).integers(1, 256, size=label.shape)).astype(np.uint8)
    stream = torch.cuda.Stream()
    # (behind a gate, tests/stream_gate.py: a launch on another stream would read poison instead of these inputs)
    warm = stream_gate.Recording(DEV)
    _launch([amap], [bytes_], alloc=warm)
    with torch.cuda.stream(stream):
        rec, mask, coeff = _launch([amap], [bytes_], alloc=stream_gate.Gated(warm, stream_gate.Gate()))
    stream.synchronize()
    _check(rec[0], mask[0], coeff[0], ref, "label bytes 1..255 on a side stream")


def test_the_wrapper_rejects_what_the_kernel_cannot_take():
    res = torch.zeros(1, 40, device=DEV, dtype=torch.uint8)
    lab = torch.zeros(8, 8, device=DEV, dtype=torch.uint8)
    with pytest.raises(ValueError, match="4096"):
        ops.seg_score([torch.zeros(65, 64, device=DEV)], [lab], res)
    with pytest.raises(ValueError):
        ops.seg_score([torch.zeros(8, 8, device=DEV, dtype=torch.float64)], [lab], res)
    with pytest.raises(ValueError):
        ops.seg_score([torch.zeros(8, 8, device=DEV)], [lab.bool()], res)
    with pytest.raises(ValueError):
        ops.seg_score([torch.zeros(8, 8, device=DEV)], [lab], res[:, :39])
    with pytest.raises(ValueError, match=">= 2"):
        ops.seg_score([torch.zeros(1, 8, device=DEV)], [lab], res, blur_weights=ops.seg_blur_weights())
