"""The numpy restatement of ca_segtab_score (tests/segtab_cases.py) pinned on the CPU: normalised it is
seg_cases.reference, raw (``normalize=False``) it equals the host scoring functions of conceptattention_amd.segmentation on
the raw map (counters equal, AP within 1e-12, the bound derived in seg_cases.py), and the counts summed over the cell
tables equal the per-pixel counts for every flag combination."""
import numpy as np
import pytest
import torch

import seg_cases as SC
import segtab_cases as T
from conceptattention_amd import segmentation as S

AP_TOL = 1e-12
COUNTS = ("n11", "n10", "n01", "n00", "thresholds")
# (h, w, Hl, Wl, seed, kind): seeded maps for the raw variant; every one is asserted to keep its cells >= 4 fp32 ulps from
# its mean, so that torch's fp32 mean and the restatement's fp64 mean give one mask
RAW_MAPS = [(5, 5, 7, 7, 1, "heat"), (16, 16, 64, 64, 2, "heat"), (16, 16, 64, 64, 3, "signed"), (64, 64, 224, 224, 4, "heat"),
            (17, 9, 8, 30, 5, "signed"), (16, 16, 7, 7, 6, "heat"), (31, 31, 224, 224, 7, "ties"), (64, 64, 224, 224, 8, "distinct")]


def _host_raw(x, label, mvt, down, special=False):
    """The per-layer script's scoring of a raw map: the mean-threshold mask, the raw coefficients, both resized with
    nearest (through 14 x 14 under downscale_for_eval), SegmentationScores.update."""
    Hl, Wl = label.shape
    xt = torch.from_numpy(x)
    mask = S.target_mask(xt[None], 0, mvt)
    c = xt
    if down:
        c = S._resize_nearest(c, (14, 14))
    c = S._resize_nearest(c, (Hl, Wl))
    m = S._resize_nearest(mask.float(), (Hl, Wl))
    return mask.numpy(), S.SegmentationScores().update(m, c, label.astype(bool))


def _assert_host(ref, out, n_pixels, what):
    want = SC.host_counters(ref, n_pixels)
    assert int(out["correct"]) == want["correct"] and int(out["labelled"]) == want["labelled"], what
    assert [int(v) for v in out["inter"]] == want["inter"] and [int(v) for v in out["union"]] == want["union"], what
    print(what, "ap", ref["ap"], "host", out["ap"], "diff", abs(ref["ap"] - out["ap"]), "thresholds", ref["thresholds"])
    assert abs(ref["ap"] - out["ap"]) <= AP_TOL, what


@pytest.mark.parametrize("h,w,Hl,Wl,seed,kind", RAW_MAPS)
@pytest.mark.parametrize("mvt,down,blur", [(True, False, False), (False, False, False), (True, True, False),
                                           (True, False, True), (False, True, True)])
def test_the_raw_variant_equals_the_host_scoring_functions(h, w, Hl, Wl, seed, kind, mvt, down, blur):
    amap = T.seeded_map(h, w, seed, kind)
    label = T.seeded_label(h, w, Hl, Wl, seed)
    ref = T.reference(amap, label, mvt, down, blur, normalize=False)
    margin = SC.mask_margin_ulps(ref["x"], ref["mean"])
    assert margin >= 4.0, f"a cell lies {margin} fp32 ulps from the mean: the fp32 and fp64 means may disagree on it"
    assert np.array_equal(ref["coeff"].view(np.uint32), ref["x"].view(np.uint32))       # raw: the coefficient is x
    mask, out = _host_raw(ref["x"], label, mvt, down)
    assert np.array_equal(mask.astype(np.uint8), ref["mask"])
    _assert_host(ref, out, Hl * Wl, (h, w, Hl, Wl, kind, mvt, down, blur))
    assert ref["n11"] + ref["n10"] + ref["n01"] + ref["n00"] == Hl * Wl


@pytest.mark.parametrize("mvt,down", [(True, False), (False, False), (False, True)])
def test_the_raw_variant_with_inf_nan_and_negative_zero_cells(mvt, down):
    """get_ap_scores sends both stacked scores through np.nan_to_num: NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX, and its
    thresholds treat -0.0 and 0.0 as one score.  (The mean of such a map is NaN: no margin to assert, the mask is empty.)"""
    amap = T.seeded_map(16, 16, 9, "special")
    flat = amap.reshape(-1)
    assert np.isposinf(flat).sum() == 1 and np.isneginf(flat).sum() == 1 and np.isnan(flat).sum() == 1
    assert (np.signbit(flat) & (flat == 0)).sum() == 1 and (~np.signbit(flat) & (flat == 0)).sum() == 1
    label = T.seeded_label(16, 16, 64, 64, 9)
    ref = T.reference(amap, label, mvt, down, False, normalize=False)
    assert np.isnan(ref["mean"]) and ref["lo"] == -np.inf and ref["hi"] == np.inf
    mask, out = _host_raw(amap, label, mvt, down)
    assert np.array_equal(mask.astype(np.uint8), ref["mask"]) and (mask.sum() == 0) == mvt
    _assert_host(ref, out, label.size, ("special", mvt, down))
    # one threshold for the two zeros, FLT_MAX and -FLT_MAX at the ends
    plain = T.reference(np.where(np.isfinite(amap), amap, np.float32(0.5)).astype(np.float32), label, mvt, down, False, False)
    assert ref["thresholds"] <= 2 * 256 - 1 and plain["thresholds"] <= 2 * 256 - 1


@pytest.mark.parametrize("case", SC.CASES, ids=repr)
def test_normalised_it_is_the_restatement_of_seg_score(case):
    amap, label = case.inputs()
    want = SC.reference(amap, label, **case.flags)
    got = T.reference(amap, label, normalize=True, **case.flags)
    for k in COUNTS:
        assert got[k] == want[k], (case, k)
    for k in ("mean", "lo", "hi"):
        assert np.float32(got[k]).tobytes() == np.float32(want[k]).tobytes(), (case, k)
    assert got["ap"] == want["ap"], case
    assert np.array_equal(got["mask"], want["mask"])


@pytest.mark.parametrize("h,w,Hl,Wl", T.TABLE_SIZES)
@pytest.mark.parametrize("flags", T.ALL_FLAGS, ids=T._flag_name)
def test_counts_summed_over_the_cell_tables_equal_the_per_pixel_counts(h, w, Hl, Wl, flags):
    label = T.seeded_label(h, w, Hl, Wl, 3)
    down = flags["downscale_for_eval"]
    tab = T.tables(h, w, label, down)
    assert tab.shape == (4, h * w) and tab[0].sum() == tab[2].sum() == Hl * Wl and tab[1].sum() == tab[3].sum() == label.sum()
    assert (tab[1] <= tab[0]).all() and (tab[3] <= tab[2]).all()
    if not down:
        assert np.array_equal(tab[:2], tab[2:])                # the two mappings differ only under downscale
    if Hl < h:
        assert (tab[0] == 0).any() and (tab[2] == 0).any()     # a label smaller than the map leaves cells unread
    for seed, kind in enumerate(T.KINDS):
        amap = T.seeded_map(h, w, seed, kind)
        ref = T.score(amap, tab, label.size, flags["mean_value_threshold"], flags["apply_blur"], flags["normalize"])
        px = T.pixel_counts(ref["mask"], label, h, w, down)
        assert [ref[k] for k in ("n11", "n10", "n01", "n00")] == [px[k] for k in ("n11", "n10", "n01", "n00")], kind
        assert np.array_equal(px["tot"], tab[2]) and np.array_equal(px["pos"], tab[3])
        assert ref["n11"] + ref["n10"] + ref["n01"] + ref["n00"] == Hl * Wl


def test_the_case_table_names_every_flag_combination_and_every_path():
    seen = {T.flag_bits(**c.flags) for c in T.CASES}
    assert seen == set(range(16)), sorted(set(range(16)) - seen)
    assert {T.flag_bits(**c.flags) for c in T.FLAG_CASES} == set(range(16)) and len(T.FLAG_CASES) == 16
    by = {c.name: c for c in T.CASES}
    assert len(by) == len(T.CASES)
    assert {(c.h, c.w) for c in T.CASES} >= {(1, 1), (2, 2), (1, 3), (37, 53), (32, 64), (3, 683), (64, 64)}
    assert {(c.Hl, c.Wl) for c in T.CASES} >= {(1, 1), (7, 7), (224, 224), (375, 500), (4096, 4096)}
    assert {c.n_maps for c in T.CASES} >= {1, 2, 19, 257, 950} and {c.C for c in T.CASES} == {1, 4}
    assert by["map32x64-label224x224"].h * by["map32x64-label224x224"].w == 2048           # either side of the LDS limit
    assert by["map3x683-label224x224-raw"].h * by["map3x683-label224x224-raw"].w == 2049
    assert SC.lds_bytes(2048) <= SC.LDS_DEFAULT_LIMIT < SC.lds_bytes(2049)
    for c in T.CASES:
        assert c.h * c.w <= T.MAX_CELLS and c.Hl * c.Wl <= T.MAX_LABEL_PIXELS and c.n_maps <= T.MAX_MAPS
        assert not c.flags["apply_blur"] or (c.h >= 2 and c.w >= 2)
        assert 0 <= c.target < c.C
    maps = T.table_maps(17, 9, len(T.KINDS), 20)
    assert np.isnan(maps[T.KINDS.index("special")]).any() and np.isfinite(maps[:T.KINDS.index("special")]).all()
