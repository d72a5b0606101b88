"""tests/mseg_cases.reference pinned on the CPU against three things: the torch route that ends in MultiClassScores.update
(torch.argmax, interpolate(mode="nearest"), gaussian_blur3 where no cell's top-two gap is under 4 ulps), a literal
transcription of lines 207-233 of the reference's harness, and map_predictions_to_class_indices.  The aliasing of the
harness's in-place remap is shown by a test of its own.

One blur case is pinned less far than the others: where the blurred planes hold NaN or inf there is no ulp margin to
assert, so the torch route takes the restatement's own blurred planes and only the argmax, the lookup, the resize and the
counting are checked against torch there; the blur itself is pinned by the finite blur cases."""
import numpy as np
import pytest
import torch

import mseg_cases as T
from conceptattention_amd import segmentation as S

BLUR_MARGIN_ULPS = 4.0


@pytest.fixture(scope="module")
def refs():
    """name -> (inputs, the restatement per item), computed once and left unchanged."""
    out = {}
    for case in T.CASES:
        maps, labels, tables, scale = case.inputs()
        out[case.name] = ((maps, labels, tables, scale),
                          [T.reference(maps[i], labels[i], tables[i], case.nclass, case.ignore, scale, case.blur)
                           for i in range(case.items)])
    return out


def test_the_case_list_covers_what_it_promises():
    names = [c.name for c in T.CASES]
    assert len(set(names)) == len(names) and T.PLACEMENT_CASE in names
    assert {c.K for c in T.CASES} >= {1, 2, 11, 32}
    assert {(c.h, c.w) for c in T.CASES} >= {(1, 1), (2, 2), (16, 16), (37, 53), (64, 64), (128, 128)}
    assert {(c.Hl, c.Wl) for c in T.CASES} >= {(1, 1), (224, 224), (375, 500), (1024, 1024), (4096, 4096)}
    assert any((c.h, c.w) == (c.Hl, c.Wl) for c in T.CASES)
    assert {c.nclass for c in T.CASES} >= {1, 2, 21, 256}
    assert {c.ignore for c in T.CASES} >= {None, 255, 0, 250}
    assert {c.items for c in T.CASES} >= {1, 16, 17}
    assert {c.outputs for c in T.CASES} == {"both", "class", "index", "none"}
    assert {c.kind for c in T.CASES} >= {"quant", "dup", "special"} and any(c.scale for c in T.CASES)
    assert max(c.h * c.w for c in T.CASES) == T.MAX_CELLS and max(c.Hl * c.Wl for c in T.CASES) == T.MAX_LABEL_PIXELS


def test_the_value_families_hold_what_they_promise(refs):
    (maps, labels, _, _), ref = refs["k11-map16x16-label224x224-nclass21-border-counted"]
    assert (labels[0] >= 21).any(), "no label id >= nclass"
    (maps, labels, _, _), ref = refs["k32-map128x128-label128x128-nclass256-ignore-absent"]
    assert not (labels[0] == 250).any()
    (maps, _, _, _), _ = refs["quantised-k11-map16x16-label64x64"]
    assert len(np.unique(maps[0])) == 4
    top = np.sort(maps[0], axis=0)
    assert (top[-1] == top[-2]).mean() > 0.5, "most cells should tie"
    (maps, _, _, _), _ = refs["special-values-k11-map37x53-label224x224"]
    nan = np.isnan(maps[0])
    assert (nan.sum(0) == 1).any() and nan.all(0).any() and np.isinf(maps[0]).any()
    assert (np.signbit(maps[0]) & (maps[0] == 0)).any() and (~np.signbit(maps[0]) & (maps[0] == 0)).any()
    (_, _, tables, scale), _ = refs["items17-k8-map16x16-label64x64"]
    assert len({tuple(t) for t in tables}) > 1
    (_, _, _, scale), _ = refs["scaled-k11-map16x16-label224x224"]
    assert (scale == 0).any() and (scale < 0).any()


def test_argmax_first_is_torch_argmax_on_ties_zeros_nan_and_inf():
    nan, inf = np.nan, np.inf
    cols = [[1, 1, 0], [0.0, -0.0, -1], [-0.0, 0.0, -1], [nan, 5, nan], [5, nan, nan], [inf, inf, nan], [-inf, -inf, -inf],
            [nan, nan, nan], [3, inf, inf], [2, 7, 7]]
    s = np.array(cols, dtype=np.float32).T.reshape(3, 1, len(cols))
    want = torch.argmax(torch.from_numpy(s), dim=0).numpy()
    assert np.array_equal(T.argmax_first(s), want)
    assert want.reshape(-1).tolist() == [0, 0, 0, 0, 1, 2, 0, 0, 1, 1]


@pytest.mark.parametrize("case", T.CASES, ids=repr)
def test_reference_equals_the_torch_route(case, refs):
    (maps, labels, tables, scale), ref = refs[case.name]
    scores, total = S.MultiClassScores(case.nclass), np.zeros(2 + 2 * case.nclass, dtype=np.int64)
    for i in range(case.items):
        x = torch.from_numpy(maps[i])
        if case.blur:
            # torch's convolution adds the nine products in its own order: its argmax is the restatement's where no cell's
            # two largest values are within a few ulps; asserted on the case's own data.  With NaN / inf in the planes
            # there is no such margin: the restatement's own blur stands in, and torch pins what follows it
            s_ref = ref[i]["s"]
            if np.isfinite(s_ref).all():
                assert T.top2_gap_ulps(s_ref) >= BLUR_MARGIN_ULPS, (case.name, T.top2_gap_ulps(s_ref))
                x = S.gaussian_blur3(x)
            else:
                x = torch.from_numpy(T.scaled_planes(maps[i], None, True))
        if scale is not None:
            x = torch.from_numpy(scale)[:, None, None] * x
        index = torch.argmax(x, dim=0)
        assert np.array_equal(index.numpy(), ref[i]["index"].astype(np.int64)), case.name
        klass = S.map_predictions_to_class_indices(index, tables[i])
        assert np.array_equal(klass.numpy(), ref[i]["class"].astype(np.int64)), case.name
        pred = torch.nn.functional.interpolate(klass[None, None].float(), size=labels[i].shape, mode="nearest")[0, 0]
        got = scores.update(pred, labels[i], ignore_index=case.ignore)
        c = ref[i]["counts"].astype(np.int64)
        total += c
        assert (got["correct"], got["labelled"]) == (int(c[0]), int(c[1])), case.name
        assert np.array_equal(got["inter"], c[2:2 + case.nclass]) and np.array_equal(got["union"], c[2 + case.nclass:])
    assert (scores.correct, scores.labelled, scores.n) == (int(total[0]), int(total[1]), case.items)
    assert np.array_equal(scores.inter, total[2:2 + case.nclass]) and np.array_equal(scores.union, total[2 + case.nclass:])
    assert (scores.inter <= scores.union).all() and scores.correct == scores.inter.sum() <= scores.labelled


@pytest.mark.parametrize("case", [c for c in T.CASES if c.ignore is None], ids=repr)
def test_reference_equals_the_transcribed_harness_lines(case, refs):
    (maps, labels, tables, scale), ref = refs[case.name]
    scores = S.MultiClassScores(case.nclass)
    t_inter, t_union, t_cor, t_lab = np.zeros(case.nclass), np.zeros(case.nclass), 0.0, 0.0
    for i in range(case.items):
        cor, lab, inter, union = T.harness_counts(ref[i]["pred"].astype(np.float32), labels[i].astype(np.float32),
                                                  case.nclass)
        c = ref[i]["counts"].astype(np.int64)
        assert (cor, lab) == (int(c[0]), int(c[1])), case.name
        assert np.array_equal(inter, c[2:2 + case.nclass]) and np.array_equal(union, c[2 + case.nclass:]), case.name
        t_inter, t_union, t_cor, t_lab = t_inter + inter, t_union + union, t_cor + cor, t_lab + lab
        scores.add_counts(c)
    res = scores.result()
    assert res["mIoU"] == T.harness_miou(t_inter, t_union)
    assert res["pixAcc"] == np.float64(1.0) * t_cor / (np.spacing(1, dtype=np.float64) + t_lab)
    seen = t_union > 0
    assert np.array_equal(res["IoU"][seen], t_inter[seen] / t_union[seen]) and np.isnan(res["IoU"][~seen]).all()
    assert res["n"] == case.items


def test_add_counts_equals_update_and_result_is_empty_safe():
    rng = np.random.default_rng(0)
    pred, lab = rng.integers(0, 5, (8, 9)), rng.integers(0, 7, (8, 9))
    a, b = S.MultiClassScores(5), S.MultiClassScores(5)
    a.update(pred, lab, ignore_index=3)
    b.add_counts(T.counts_of(pred, lab, 5, 3))
    assert (a.correct, a.labelled, a.n) == (b.correct, b.labelled, b.n)
    assert np.array_equal(a.inter, b.inter) and np.array_equal(a.union, b.union)
    empty = S.MultiClassScores(3).result()
    assert empty["pixAcc"] == 0.0 and empty["mIoU"] == 0.0 and np.isnan(empty["IoU"]).all() and empty["n"] == 0
    with pytest.raises(ValueError):
        a.update(pred, lab[:4])
    with pytest.raises(ValueError):
        a.add_counts(np.zeros(5))


def test_the_table_and_the_harness_in_place_remap_disagree_where_a_concept_index_is_a_class_id():
    """run_multi_class_seg_experiment.py:25-37 remaps in place, class after class.  With 5 background concepts and the
    present classes cat, dog, sheep, bus, concept index 8 (bus) equals cat's VOC class id: every cell first mapped to cat
    is mapped again, to bus.  map_predictions_to_class_indices is the one-step table the harness means."""
    names = ["background", "aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow",
             "diningtable", "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"]
    background = ["background", "floor", "grass", "tree", "sky"]
    present = ["cat", "dog", "sheep", "bus"]
    table = S.multiclass_table(background, present, names)
    assert table == [0, 0, 0, 0, 0, 8, 12, 17, 6]
    index = torch.randint(0, 9, (64, 64), generator=torch.Generator().manual_seed(0))
    ours = S.map_predictions_to_class_indices(index, table)
    in_place = index.clone()                                   # lines 32-35, transcribed
    in_place[in_place < len(background)] = 0
    for k, name in enumerate(present):
        in_place[in_place == len(background) + k] = names.index(name)
    cat = index == 5
    assert cat.any() and (ours[cat] == 8).all() and (in_place[cat] == 6).all()
    differ = ours != in_place
    assert int(differ.sum()) == int(cat.sum()) > 0 and (differ == cat).all()
    assert np.array_equal(S.map_predictions_to_class_indices(index.numpy(), table), ours.numpy())
    with pytest.raises(ValueError, match="unicorn"):
        S.multiclass_table(background, ["cat", "unicorn"], names)


def test_the_placement_case_puts_the_4_gib_line_inside_every_roles_data():
    """tests/test_mseg_kernels_gpu._guarded asks for the boundary on element n // 2 of the n data elements (its buffer
    goes on for guard elements): with placement.straddle_start's 16-byte rounding at least 16 bytes of every role's data
    lie on either side, the small outputs (176 bytes of counts, 256 of each map) included."""
    import placement
    case = next(c for c in T.CASES if c.name == T.PLACEMENT_CASE)
    B = 1 << 32
    for role, nbytes in T.placement_data_bytes(case).items():
        item = 4 if role in ("maps", "counts") else 1
        n = nbytes // item
        start = placement.straddle_start(B, n // 2, item, (n + 256) * item)
        assert start % 16 == 0 and start + 16 <= B <= start + nbytes - 16, (role, B - start, nbytes)
