"""The numpy restatement of ca_heatmap_render (tests/render_cases.py) pinned on the CPU: at the map's own size it is
pipeline.colorize_heatmaps byte for byte, its look-up rule is matplotlib's for every edge (under, over, bad, -0.0, a
constant group), and its bilinear values are torch's within a bound derived from the operation count."""
import numpy as np
import pytest
import torch

import render_cases as R
from conceptattention_amd.pipeline import colorize_heatmaps

F = np.float32


@pytest.mark.parametrize("cmap", ["plasma", "inferno", "jet"])
@pytest.mark.parametrize("family", ["heat", "signed", "distinct", "two", "negzero"])
def test_nearest_at_the_maps_size_is_colorize_heatmaps(cmap, family):
    lut = R.cmap_lut(cmap)
    for h, w, n in ((64, 64, 4), (37, 53, 3), (1, 3, 1)):
        planes = R.planes_of(family, n, h, w, seed=h + n)
        got, _ = R.render(planes, lut)
        want = np.stack([np.asarray(im) for im in colorize_heatmaps(planes, cmap)])
        assert np.array_equal(got, want), (cmap, family, h, w)


def _cmap_direct(planes, cmap, lo, hi):
    import matplotlib.pyplot as plt
    with np.errstate(all="ignore"):
        t = (planes - F(lo)) / (F(hi) - F(lo))
        return (plt.get_cmap(cmap)(t)[..., :3] * 255).astype(np.uint8)


@pytest.mark.parametrize("family", ["constant", "nan", "inf", "negzero"])
def test_edge_families_against_the_colour_map_itself(family):
    planes = R.planes_of(family, 3, 16, 12, seed=5)
    lo, hi = R.group_range(planes)
    for cmap in ("plasma", "jet"):
        got, _ = R.render(planes, R.cmap_lut(cmap))
        assert np.array_equal(got, _cmap_direct(planes, cmap, lo, hi)), (family, cmap)
    if family in ("constant", "nan"):                           # bad everywhere: matplotlib's transparent black
        assert not got.any()


@pytest.mark.parametrize("kind", R.GIVEN)
def test_given_ranges_against_the_colour_map_itself(kind):
    import matplotlib
    planes = R.planes_of("signed", 2, 16, 16, seed=9)
    given = R.given_range(kind, planes)
    cm = matplotlib.colormaps["jet"].with_extremes(under="white", over="black", bad="green")
    lut = (np.concatenate([cm(np.arange(256))[:, :3]] + [np.asarray(cm(v)).reshape(1, 4)[:, :3]
                                                         for v in (-np.inf, np.inf, np.nan)]) * 255).astype(np.uint8)
    assert lut[R.ROW_UNDER].tolist() == [255, 255, 255] and lut[R.ROW_OVER].tolist() == [0, 0, 0]
    assert lut[R.ROW_BAD].tolist() == [0, 127, 0] or lut[R.ROW_BAD].tolist() == [0, 128, 0]
    got, used = R.render(planes, lut, given=given)
    with np.errstate(all="ignore"):
        want = (cm((planes - F(given[0])) / (F(given[1]) - F(given[0])))[..., :3] * 255).astype(np.uint8)
    assert np.array_equal(got, want) and used == (F(given[0]), F(given[1]))
    rows = R.lut_rows(planes, *given)
    if kind == "narrow":
        assert (rows == R.ROW_UNDER).any() and (rows == R.ROW_OVER).any()
    if kind == "equal":
        assert (rows >= R.ROW_UNDER).all()                      # x / 0: +-inf is under / over, 0 / 0 bad


def test_the_row_rule_value_by_value():
    v = np.array([-0.0, 0.0, 1.0, np.nextafter(F(1), F(0)), np.nextafter(F(1), F(2)), -1e-30, np.nan, np.inf, -np.inf,
                  0.5, 255.0 / 256.0, 1.0 / 256.0], dtype=F)
    rows = R.lut_rows(v, 0.0, 1.0)
    assert rows.tolist() == [0, 0, 255, 255, R.ROW_OVER, R.ROW_UNDER, R.ROW_BAD, R.ROW_OVER, R.ROW_UNDER, 128, 255, 1]
    lut = R.synthetic_lut()
    assert len({tuple(r) for r in lut.tolist()}) == R.LUT_ROWS


def test_blend_rule():
    col = np.array([[[255, 0, 10]]], dtype=np.uint8)
    img = np.array([[[0, 255, 11]]], dtype=np.uint8)
    rows = np.array([[3]])
    assert R.blend(col, img, rows, 0.5).tolist() == [[[128, 128, 11]]]          # 127.5 + 0.5 and 10.5 + 0.5, truncated
    assert R.blend(col, img, rows, 0.0).tolist() == img.tolist() and R.blend(col, img, rows, 1.0).tolist() == col.tolist()
    assert R.blend(col, img, np.array([[R.ROW_BAD]]), 1.0).tolist() == img.tolist()


GEOMETRY = sorted({(c.h, c.w, c.H, c.W) for c in R.CASES if c.name.startswith("geo-")})


def _torch_bilinear(plane, H, W):
    return torch.nn.functional.interpolate(torch.from_numpy(plane)[None, None], size=(H, W), mode="bilinear",
                                           align_corners=False)[0, 0].numpy().astype(np.float64)


@pytest.mark.parametrize("h,w,H,W", GEOMETRY)
def test_bilinear_values_against_torch(h, w, H, W):
    """Within 16 * 2^-24 * max |cell| of torch on the CPU.  The bound is derived, not measured: seven rounded operations
    on values no larger than the largest cell, and the two implementations differ only in contraction and order.  That
    holds because the source coordinate is formed as torch's builds form it, scale * (y + 0.5) - 0.5 in ONE fused
    operation (render_cases.fmaf); see test_a_twice_rounded_coordinate_would_miss_the_bound."""
    for family in ("heat", "signed", "distinct"):
        plane = R.planes_of(family, 1, h, w, seed=3)[0]
        bound = 16 * 2.0 ** -24 * float(np.abs(plane).max())
        err = float(np.abs(R.values(plane, H, W, True).astype(np.float64) - _torch_bilinear(plane, H, W)).max())
        print(f"{h}x{w} -> {H}x{W} {family}: |restatement - torch| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (family, err, bound)


def test_a_twice_rounded_coordinate_would_miss_the_bound(monkeypatch):
    """Why the coordinate is the entry's one fused operation: with the product rounded before the subtraction, half an ulp
    of a coordinate near 60 is 2^-19, which the lerp multiplies by the difference of two neighbouring cells.  At 64 -> 224
    on all-distinct cells that is more than the bound above (42.9 against 16 when this was written); where the scale is a
    power of two (64 -> 1024) the product is exact and the two forms are the same bits."""
    fused = {g: R.values(R.planes_of("distinct", 1, 64, 64, seed=3)[0], g, g, True) for g in (224, 1024)}
    monkeypatch.setattr(R, "fmaf", lambda a, b, c: a * b + c)
    plane = R.planes_of("distinct", 1, 64, 64, seed=3)[0]
    twice = R.values(plane, 224, 224, True)
    assert twice.dtype == F
    bound = 16 * 2.0 ** -24 * float(np.abs(plane).max())
    assert float(np.abs(twice.astype(np.float64) - _torch_bilinear(plane, 224, 224)).max()) > bound
    assert float(np.abs(fused[224].astype(np.float64) - _torch_bilinear(plane, 224, 224)).max()) <= bound
    assert np.array_equal(R.values(plane, 1024, 1024, True), fused[1024])


def test_fmaf_is_one_rounding():
    a, b = F(64) / F(224), np.arange(224, dtype=F) + F(0.5)
    exact = [float(a) * float(v) - 0.5 for v in b]                 # exact in fp64 (render_cases.fmaf says why)
    import fractions
    assert all(fractions.Fraction(float(a)) * fractions.Fraction(float(v)) - fractions.Fraction(1, 2) ==
               fractions.Fraction(e) for v, e in zip(b, exact))
    assert np.array_equal(R.fmaf(a, b, F(-0.5)), np.array(exact).astype(F))
    assert not np.array_equal(R.fmaf(a, b, F(-0.5)), a * b - F(0.5))


@pytest.mark.parametrize("h,w,H,W", GEOMETRY)
def test_nearest_index_is_torchs(h, w, H, W):
    plane = np.arange(h * w, dtype=F).reshape(h, w)
    want = torch.nn.functional.interpolate(torch.from_numpy(plane)[None, None], size=(H, W), mode="nearest")[0, 0].numpy()
    assert np.array_equal(R.values(plane, H, W, False), want)


def test_the_case_list_covers_what_the_kernel_test_promises():
    geo = {(c.h, c.w, c.H, c.W, c.bilinear) for c in R.CASES}
    for g in [(1, 1, 1, 1), (1, 3, 1, 3), (2, 2, 2, 2), (37, 53, 37, 53), (64, 64, 64, 64), (128, 128, 128, 128),
              (64, 64, 224, 224), (37, 53, 100, 75), (128, 128, 1, 1), (1, 1, 17, 5)]:
        assert g + (False,) in geo and g + (True,) in geo, g
    assert any(c.H == 1024 and c.n_maps == 4 for c in R.CASES)
    assert {c.n_maps for c in R.CASES} >= {1, 4, 19, 257} and {c.groups for c in R.CASES} >= {1, 10, 16, 17}
    assert {c.family for c in R.CASES} == set(R.FAMILIES) and {c.given for c in R.CASES} >= set(R.GIVEN)
    assert {c.alpha for c in R.CASES} >= {0.0, 0.5, 1.0, 0.3} and {c.out_pad for c in R.CASES} == {0, 5}
    assert any(c.C > 1 for c in R.CASES) and any(c.C == 1 for c in R.CASES)
    refs = R.BY_NAME["blend-bad-keeps-picture"].references(R.synthetic_lut())
    pics = R.BY_NAME["blend-bad-keeps-picture"].inputs()[2]
    assert all(np.array_equal(plane, pics[0]) for plane in refs[0][0])
