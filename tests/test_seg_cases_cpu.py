"""The numpy restatement of ca_seg_score (tests/seg_cases.py) against the host scoring path it replaces
(conceptattention_amd.segmentation): integer counters equal, AP within 1e-12 (the bound is derived in seg_cases.py).
This pins the restatement, and through tests/test_seg_kernels_gpu.py the kernel's definition."""
import os

import numpy as np
import pytest
import torch

import seg_cases as T
from conceptattention_amd import segmentation as S

AP_TOL = 1e-12


def _host(case, ref, label):
    """target_mask + prepare_for_scoring + SegmentationScores.update on the restatement's own (blurred) map."""
    x = torch.from_numpy(ref["x"])
    mask = S.target_mask(x[None], 0, case.mvt)
    if case.Hl == case.Wl:
        c, m = S.prepare_for_scoring(x.numpy(), mask.numpy(), size=case.Hl, downscale_for_eval=case.down)
    else:   # prepare_for_scoring resizes to a square; its three steps with the rectangular size
        c = (x - x.min()) / (x.max() - x.min())
        if case.down:
            c = S._resize_nearest(c, (14, 14))
        c = S._resize_nearest(c, (case.Hl, case.Wl))
        m = S._resize_nearest(mask.float(), (case.Hl, case.Wl))
    scores = S.SegmentationScores()
    return mask.numpy(), scores.update(m, c, label.astype(bool)), scores


@pytest.mark.parametrize("case", T.CASES, ids=repr)
def test_restatement_equals_the_host_scoring_path(case):
    amap, label = case.inputs()
    assert amap.shape == (case.h, case.w) and label.shape == (case.Hl, case.Wl) and amap.size <= T.MAX_CELLS
    ref = T.reference(amap, label, **case.flags)
    if case.kind != "const":   # (a constant map's mean is exact in both precisions)
        margin = T.mask_margin_ulps(ref["x"], ref["mean"])
        assert margin >= 4.0, f"a cell lies {margin} fp32 ulps from the mean: the fp32 and fp64 means may disagree on it"
    mask, out, scores = _host(case, ref, label)
    assert np.array_equal(mask.astype(np.uint8), ref["mask"])
    want = T.host_counters(ref, case.Hl * case.Wl)
    assert int(out["correct"]) == want["correct"] and int(out["labelled"]) == want["labelled"]
    assert [int(v) for v in out["inter"]] == want["inter"] and [int(v) for v in out["union"]] == want["union"]
    assert ref["n11"] + ref["n10"] + ref["n01"] + ref["n00"] == case.Hl * case.Wl
    print(case, "ap", ref["ap"], "host", out["ap"], "diff", abs(ref["ap"] - out["ap"]), "thresholds", ref["thresholds"])
    assert abs(ref["ap"] - out["ap"]) <= AP_TOL
    assert 1 <= ref["thresholds"] <= 2 * case.h * case.w


@pytest.mark.parametrize("i", [1, 2])
def test_restatement_equals_the_reference_goldens(i):
    g = np.load(T.GOLD)
    case = next(c for c in T.CASES if c.gold == i)
    amap, label = case.inputs()
    ref = T.reference(amap, label, **case.flags)
    assert np.array_equal(ref["mask"], g[f"mask{i}"].astype(np.uint8))
    want = T.host_counters(ref, label.size)
    assert [want["correct"], want["labelled"]] == [int(v) for v in g[f"pix{i}"]]
    assert want["inter"] == [int(v) for v in g[f"inter{i}"]] and want["union"] == [int(v) for v in g[f"union{i}"]]
    assert abs(ref["ap"] - float(np.asarray(g[f"ap{i}"]).reshape(-1)[0])) <= AP_TOL


def test_special_cases_are_what_their_names_say():
    by = {c.name: c for c in T.CASES}
    ref = T.reference(*by["constant-map"].inputs())
    assert np.isnan(ref["coeff"]).all() and ref["mask"].sum() == 0 and ref["thresholds"] == 1
    ref = T.reference(*by["full-sort-4096-distinct"].inputs())
    assert ref["thresholds"] == 2 * 4096 - 2     # all distinct but (c = 1, 1 - c = 1) and (c = 0, 1 - c = 0)
    for name in ("ties-16-to-64", "ties-64-to-224"):
        assert T.reference(*by[name].inputs())["thresholds"] <= 12
    ref = T.reference(*by["three-cells"].inputs())
    assert ref["thresholds"] <= 6
    assert T.reference(*by["labels-all-negative"].inputs())["n11"] == 0
    amap, _ = by["signed-zero-threshold"].inputs()
    assert (amap < 0).any() and (amap > 0).any()
    assert len(T.cap_launch_inputs()[0]) == T.MAX_PROBLEMS


def test_large_labels_and_the_lds_limit_boundary_are_cases():
    by = {c.name: c for c in T.CASES}
    for name, cells, pixels in (("map64x64-label1024x1024", 4096, 1 << 20), ("map48x64-label375x500", 3072, 187500),
                                ("map32x64-label224x224", 2048, 50176), ("map3x683-label224x224", 2049, 50176),
                                ("map2x2-label4096x4096", 4, 1 << 24)):
        assert by[name].h * by[name].w == cells and by[name].Hl * by[name].Wl == pixels, name
    # the request crosses the default limit between 2048 and 2049 cells, where the padded sort doubles
    assert T.lds_bytes(2048) == 57856 <= T.LDS_DEFAULT_LIMIT < T.lds_bytes(2049) == 90672
    assert T.lds_bytes(48 * 48) > T.LDS_DEFAULT_LIMIT and T.lds_bytes(T.MAX_CELLS) == 115200
    assert 2 * 3072 < 8192                                     # the rectangular map sorts more slots than it has entries
    ref = T.reference(*by["map2x2-label4096x4096"].inputs())   # the entry point's limit: 2^24 pixels, counts up to 2^24
    assert ref["n11"] + ref["n10"] + ref["n01"] + ref["n00"] == 1 << 24 == T.MAX_LABEL_PIXELS
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "conceptattention_amd", "csrc")
    src = open(os.path.join(csrc, "ca_seg_core.h")).read()     # (where both map kernels' request is formed)
    size = "(size_t)npad * 8 + (size_t)((hw + 3) & ~3) * 12 + SEG_SCRATCH_BYTES"
    assert size in src and "if (lds > 64 * 1024)" in src
    assert "48 x 48" not in src
    units = [open(os.path.join(csrc, f)).read() for f in ("ca_seg.hip", "ca_segtab.hip")]
    assert sum(t.count(size) for t in units + [src]) == 1, "the LDS size expression exists once"


def test_mean_tree_is_the_rounded_fp64_mean():
    """The fixed tree is one of the fp64 summation orders: its fp32 result is the exactly rounded mean on every case."""
    import math
    for case in T.CASES:
        amap, _ = case.inputs()
        exact = np.float32(math.fsum(float(v) for v in amap.reshape(-1)) / amap.size)
        assert T.mean_tree(amap) == exact, case


@pytest.mark.parametrize("h,w", [(2, 2), (16, 16), (17, 9)])
def test_blur_restatement_against_gaussian_blur3(h, w):
    x = T.seeded_map(h, w, 4, "signed")
    got = T.blur3(x, T.blur_weights())
    want = S.gaussian_blur3(torch.from_numpy(x)[None])[0].numpy()
    bound = 9 * 2.0 ** -24 * T.blur3(np.abs(x), T.blur_weights()).astype(np.float64)   # 9 roundings of sum |w x|
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= bound).all()
