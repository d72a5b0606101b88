"""The three scoring entries against the bytes they wrote BEFORE their shared arithmetic moved into csrc/ca_seg_core.h.

tests/golden/scoring_parent_records.npz holds what ops.seg_score, ops.segtab_score and ops.mseg_score wrote on an MI355X
for seeded inputs, recorded from the commit before the move (``record`` below wrote it; only outputs are stored):

  ``seg``        the 40-byte record of every case of seg_cases.CASES with Hl * Wl <= 224 * 224, in case order;
  ``segtab``     the records of every such case of segtab_cases.CASES, map after map;
  ``mseg``       the int32 counts of every such case of mseg_cases.CASES, item after item;
  ``nf_seg``,    the records of the non-finite set: 4 x 4 and 16 x 16 maps that hold +inf, -inf, NaN, -0.0, FLT_MAX,
  ``nf_segtab``  -FLT_MAX or a subnormal in two cells, and one map with all seven, against 7 x 7 and 64 x 64 labels under
                 every combination of the three flags; ca_segtab_score with ``normalize`` on and off.

Everything is compared bit for bit, the AP too: the sort network, the scan order and the fp64 summation tree are part of
the kernels' contract.  A NaN ``mean`` / ``lo`` / ``hi`` compares as a NaN (its sign and payload are the adder's own).  On
the non-finite set ca_seg_score and ca_segtab_score (normalised) also equal each other: without RAW a coefficient lies in
[0, 1] or is NaN, so nan_to_num's two infinity branches, which only ca_segtab.hip used to spell out, never fire."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mseg_cases as MC  # noqa: E402
import seg_cases as SC  # noqa: E402
import segtab_cases as TC  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from conceptattention_amd.segmentation import SEG_RECORD  # noqa: E402

DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scoring_parent_records.npz")
MAX_LABEL = 224 * 224
RECORD = SEG_RECORD
f32 = np.float32
SPECIALS = (np.inf, -np.inf, np.nan, -0.0, 3.4028234663852886e38, -3.4028234663852886e38, 1e-40)
NF_SIZES = [(4, 4), (16, 16)]
NF_LABELS = [(7, 7), (64, 64)]
NF_FLAGS = [dict(zip(("mean_value_threshold", "downscale_for_eval", "apply_blur"), bits))
            for bits in itertools.product((True, False), repeat=3)]


def small(cases) -> list:
    return [c for c in cases if c.Hl * c.Wl <= MAX_LABEL]


def nonfinite_maps(h, w) -> np.ndarray:
    """fp32 [8, h, w]: a signed map with one special value in two cells (seven maps), and with all seven (the eighth)."""
    base = SC.seeded_map(h, w, 77, "signed").reshape(-1)
    cells = np.random.default_rng(77 + h).permutation(h * w)
    out = []
    for i, v in enumerate(SPECIALS):
        m = base.copy()
        m[cells[2 * i:2 * i + 2]] = f32(v)
        out.append(m)
    m = base.copy()
    m[cells[:len(SPECIALS)]] = np.array(SPECIALS, dtype=f32)
    out.append(m)
    return np.stack(out).reshape(-1, h, w)


def nonfinite_label(h, w, Hl, Wl) -> np.ndarray:
    return SC.seeded_label(SC.seeded_map(h, w, 77, "heat"), Hl, Wl, 77)


def seg_score(maps, label, mean_value_threshold=True, downscale_for_eval=False, apply_blur=False) -> np.ndarray:
    """uint8 [n, 40]: ops.seg_score on n maps, each against ``label``."""
    n = len(maps)
    md = torch.from_numpy(np.ascontiguousarray(maps)).to(DEV)
    ld = torch.from_numpy(label).to(DEV)
    res = torch.full((n, 40), 0xAB, dtype=torch.uint8, device=DEV)
    ops.seg_score(list(md), [ld] * n, res, mean_value_threshold=mean_value_threshold,
                  downscale_for_eval=downscale_for_eval, blur_weights=ops.seg_blur_weights() if apply_blur else None)
    return res.cpu().numpy()


def segtab_score(maps, label, C=1, target=0, mean_value_threshold=True, downscale_for_eval=False, apply_blur=False,
                 normalize=True) -> np.ndarray:
    """uint8 [n, 40]: ops.segtab_score on plane ``target`` of a [n, C, h, w] table whose other planes are NaN."""
    n, h, w = maps.shape
    full = np.full((n, C, h, w), np.nan, dtype=f32)
    full[:, target] = maps
    md = torch.from_numpy(full).to(DEV)
    res = torch.full((n, 40), 0xAB, dtype=torch.uint8, device=DEV)
    ops.segtab_score(md, target, torch.from_numpy(label).to(DEV), res, mean_value_threshold=mean_value_threshold,
                     downscale_for_eval=downscale_for_eval, blur_weights=ops.seg_blur_weights() if apply_blur else None,
                     normalize=normalize)
    return res.cpu().numpy()


def mseg_counts(case) -> np.ndarray:
    """int32 [items * (2 + 2 nclass)]: ops.mseg_score on a case of mseg_cases."""
    maps, labels, tables, scale = case.inputs()
    counts = torch.full((case.items, 2 + 2 * case.nclass), -1234567, dtype=torch.int32, device=DEV)
    md = torch.empty(case.items, case.K, case.h, case.w, device=DEV).copy_(torch.from_numpy(np.stack(maps)))
    ld = torch.empty(case.items, case.Hl, case.Wl, dtype=torch.uint8, device=DEV).copy_(torch.from_numpy(np.stack(labels)))
    ops.mseg_score(md, ld, counts, tables, case.nclass, ignore_index=case.ignore, scale=scale,
                   blur_weights=ops.seg_blur_weights() if case.blur else None)
    return counts.cpu().numpy().reshape(-1)


@functools.lru_cache(maxsize=None)
def computed(family: str) -> np.ndarray:
    """What the library in this tree writes for one family of the fixture; the smallest launches come first."""
    if family == "seg":
        out = []
        for c in small(SC.CASES):
            amap, label = c.inputs()
            out.append(seg_score(amap[None], label, **c.flags))
        return np.concatenate(out)
    if family == "segtab":
        out = []
        for c in small(TC.CASES):
            maps, label = c.inputs()
            out.append(segtab_score(maps, label, c.C, c.target, **c.flags))
        return np.concatenate(out)
    if family == "mseg":
        return np.concatenate([mseg_counts(c) for c in small(MC.CASES)])
    out = []
    for (h, w), (Hl, Wl) in itertools.product(NF_SIZES, NF_LABELS):
        maps, label = nonfinite_maps(h, w), nonfinite_label(h, w, Hl, Wl)
        for flags in NF_FLAGS:
            if family == "nf_seg":
                out.append(seg_score(maps, label, **flags))
            else:
                out += [segtab_score(maps, label, normalize=nz, **flags) for nz in (True, False)]
    return np.concatenate(out)


FAMILIES = ("nf_seg", "nf_segtab", "seg", "segtab", "mseg")


def record(path: str) -> None:
    """Write the fixture from the library in this tree (run once, on the commit before the move)."""
    np.savez_compressed(path, **{f: computed(f) for f in FAMILIES})


def assert_same_records(got, want, what) -> None:
    got, want = np.ascontiguousarray(got).view(RECORD).reshape(-1), np.ascontiguousarray(want).view(RECORD).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for k in ("n11", "n10", "n01", "n00", "thresholds"):
        assert np.array_equal(got[k], want[k]), (what, k, np.nonzero(got[k] != want[k])[0][:8])
    a, b = got["ap"].copy().view(np.uint64), want["ap"].copy().view(np.uint64)
    assert np.array_equal(a, b), (what, "ap", np.nonzero(a != b)[0][:8])
    for k in ("mean", "lo", "hi"):
        a, b = got[k].copy(), want[k].copy()
        same = (np.isnan(a) & np.isnan(b)) | (a.view(np.uint32) == b.view(np.uint32))
        assert same.all(), (what, k, np.nonzero(~same)[0][:8])


@pytest.fixture(scope="module")
def parent():
    return np.load(FIXTURE)


@pytest.mark.parametrize("family", ("nf_seg", "nf_segtab", "seg", "segtab"))
def test_the_records_are_the_parents_bit_for_bit(parent, family):
    got = computed(family)
    print(family, got.shape[0], "records")
    assert_same_records(got, parent[family], family)


def test_the_multi_class_counts_are_the_parents_bit_for_bit(parent):
    got = computed("mseg")
    print("mseg", got.size, "counts")
    assert got.dtype == np.int32 and np.array_equal(got, parent["mseg"])


def test_on_non_finite_maps_seg_score_and_the_normalised_segtab_score_write_one_record(parent):
    seg = computed("nf_seg").reshape(-1, 8, 40)                    # [call, map, 40]
    tab = computed("nf_segtab").reshape(-1, 2, 8, 40)              # [call, normalize on / off, map, 40]
    assert seg.shape[0] == tab.shape[0] == len(NF_SIZES) * len(NF_LABELS) * len(NF_FLAGS)
    assert_same_records(tab[:, 0], seg, "segtab_score(normalize=True) against seg_score")
