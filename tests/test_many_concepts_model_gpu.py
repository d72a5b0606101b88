"""More than 8 concepts through the model and the public calls, on the tiny geometry of tests/model_route_cases.py
(tiny_params, 256 x 256, 8 text tokens): 12 and 32 concepts, 1 and 3 items, softmax and sparsemax, with per-layer tables.

  * fused_heatmaps True (one ops.heatmap_many per captured layer and norm, no ops.heatmap_logits) and False (the
    three-launch form) give torch.equal accumulators and tables;
  * the maps stay inside model_route_cases.OUT_MAP_GATE / CROSS_MAP_GATE of the fp32 oracle;
  * two requests that share their accumulators are split into separate launches;
  * generate_image / encode_image with 17 concepts and sparsemax, score_multiclass_images with 12 concepts, and the
    ValueError for 33 concepts with a sparse norm before any forward."""
from dataclasses import replace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import model_route_cases as M  # noqa: E402
import test_model_routes_gpu as TM  # noqa: E402
from conceptattention_amd import ConceptAttentionFluxPipeline  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from conceptattention_amd import segmentation as S  # noqa: E402
from conceptattention_amd.flux_dit import HeatmapRequest  # noqa: E402
from conceptattention_amd.params import tiny_params  # noqa: E402

DEV = TM.DEV
LAYERS = (0, 1)
GRID = [(12, 1, L.NORM_SOFTMAX), (12, 3, L.NORM_SPARSEMAX), (32, 1, L.NORM_SPARSEMAX), (32, 3, L.NORM_SOFTMAX)]


def case_of(C, B, norm, **settings):
    name = f"many_c{C}_b{B}_{'softmax' if norm == L.NORM_SOFTMAX else 'sparsemax'}" + ("~unfused" if settings else "")
    return M.Case(name, settings=settings, C=C, B=B, return_vectors=False, layers=LAYERS, norm=norm)


def requests(case, n, shared=False):
    z = lambda *s: torch.zeros(*s, case.C, case.L, device=DEV)  # noqa: E731
    reqs = [HeatmapRequest(LAYERS, 1.0 / len(LAYERS), z(), z(), per_layer_out=z(len(LAYERS)),
                           per_layer_cross=z(len(LAYERS)), per_layer_weight=1.0, norm=case.norm) for _ in range(n)]
    if shared:                                   # every request accumulates into the first one's tensors
        for r in reqs[1:]:
            r.out_space, r.cross_space = reqs[0].out_space, reqs[0].cross_space
            r.per_layer_out, r.per_layer_cross = reqs[0].per_layer_out, reqs[0].per_layer_cross
    return reqs


class Calls:
    """Counts ops.heatmap_many / heatmap_fused / heatmap_logits while active (the calls still run)."""

    def __init__(self, monkeypatch):
        self.n = dict(heatmap_many=0, heatmap_fused=0, heatmap_logits=0)
        self.problems = []
        for name in self.n:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, real):
        def call(*a, **k):
            self.n[name] += 1
            if name == "heatmap_many":
                self.problems.append(len(a[0]))
            return real(*a, **k)
        return call


def run(case, monkeypatch, shared=False):
    calls = Calls(monkeypatch)
    out = TM.forward(TM.build(case), case, reqs=requests(case, case.B, shared))
    monkeypatch.undo()
    return out, calls


def tensors(req):
    return dict(out_space=req.out_space, cross_space=req.cross_space, per_layer_out=req.per_layer_out,
                per_layer_cross=req.per_layer_cross)


def assert_equal_requests(a, b, what):
    assert torch.equal(a.pred, b.pred), f"{what}: pred"
    for j, (x, y) in enumerate(zip(a.reqs, b.reqs)):
        for k, t in tensors(x).items():
            assert torch.equal(t, tensors(y)[k]), f"{what}: item {j} {k}"


@pytest.fixture(scope="module")
def oracle_cache():
    return {}


@pytest.mark.parametrize("C,B,norm", GRID)
def test_many_route_equals_the_three_launch_route_and_stays_inside_the_oracle_gates(C, B, norm, oracle_cache, monkeypatch):
    case = case_of(C, B, norm)
    assert not M.route_of(case, 1).use_part and M.route_of(case, 1).f32img       # (more than 8 concepts: the fp32 rows)
    fused, calls = run(case, monkeypatch)
    assert calls.n == dict(heatmap_many=len(LAYERS), heatmap_fused=0, heatmap_logits=0), calls.n
    assert calls.problems == [2 * B] * len(LAYERS), calls.problems               # all items, both spaces: one launch
    other = case_of(C, B, norm, fused_heatmaps=False)
    assert M.route_of(other, 1) == M.route_of(case, 1)
    unfused, calls3 = run(other, monkeypatch)
    assert calls3.n == dict(heatmap_many=0, heatmap_fused=0, heatmap_logits=2 * B * len(LAYERS)), calls3.n
    assert_equal_requests(fused, unfused, case.name)
    for j in range(B):
        _, d_o = TM.oracle(oracle_cache, case, j)
        for attr, space, gate in TM.SPACES:
            acc = getattr(fused.reqs[j], attr)
            err = TM.maxabs(acc, TM.reference_maps(case, d_o, space))
            print(f"  {case.name}: item {j} {attr} max err {err:.3e} / gate {gate:.3e} = {err / gate:.3f}")
            assert err < gate, (case.name, j, attr, err)
            assert abs(acc.sum(0) - 1).max().item() < 1e-5, (attr, "the weights over the concepts sum to 1")
            table = getattr(fused.reqs[j], "per_layer_out" if attr == "out_space" else "per_layer_cross")
            assert abs(table.sum(1) - 1).max().item() < 1e-5
            assert TM.maxabs(table.mean(0), acc) < 1e-6, "the accumulator is the mean of the per-layer rows"


def test_requests_that_share_their_accumulators_are_split_into_separate_launches(monkeypatch):
    case = case_of(12, 2, L.NORM_SPARSEMAX)
    fused, calls = run(case, monkeypatch, shared=True)
    # item 1's problems name item 0's tensors: a launch may not hold both (unordered read-modify-writes)
    assert calls.n["heatmap_many"] == 2 * len(LAYERS) and calls.problems == [2] * (2 * len(LAYERS)), (calls.n, calls.problems)
    unfused, _ = run(case_of(12, 2, L.NORM_SPARSEMAX, fused_heatmaps=False), monkeypatch, shared=True)
    assert_equal_requests(fused, unfused, "shared accumulators")
    acc = fused.reqs[0].out_space
    assert abs(acc.sum(0) - 2).max().item() < 1e-5, "both items were accumulated"


# ------------------------------------------------------------------------------------------------ public surface
SIDE = 256
WORDS = ["cat", "dog", "sheep", "bus", "car", "bird", "boat", "cow", "person", "train", "sofa", "chair", "horse", "tree",
         "sky", "grass", "floor", "road", "wall", "lamp", "cup", "book", "door", "hill", "rock", "lake", "sand", "snow",
         "roof", "fence", "sign", "bench", "cloud"]
NAMES = ["background", "aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable",
         "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"]
BACKGROUND = ["background", "floor", "grass", "tree", "sky"]
TARGETS = [["cat", "dog", "sheep", "bus", "car", "bird", "boat"], ["person", "cow", "horse", "sofa", "chair", "train", "bottle"]]
KW = dict(width=SIDE, height=SIDE, layers=[0, 1], num_steps=2, noise_timestep=1, batch=5)


@pytest.fixture(scope="module")
def pipe():
    return ConceptAttentionFluxPipeline("flux-schnell", device=DEV, weights="synthetic", params=tiny_params(),
                                        n_text_tokens=64, autoencoder="synthetic", text_encoder="synthetic-t5-clip")


def _picture(seed, size=(SIDE, SIDE)):
    import PIL.Image
    return PIL.Image.fromarray(np.random.default_rng(seed).integers(0, 256, size=(*size, 3), dtype=np.uint8))


def _check_maps(maps, C):
    maps = np.asarray(maps)
    assert maps.shape == (C, SIDE // 16, SIDE // 16) and np.isfinite(maps).all()
    assert np.abs(maps.sum(0) - 1).max() < 1e-5, "the weights over the concepts sum to 1 in every patch"
    assert (maps == 0).any(), "sparsemax left no exact zero"


def test_generate_image_and_encode_image_with_17_concepts_and_sparsemax(pipe, monkeypatch):
    concepts = WORDS[:17]
    calls = Calls(monkeypatch)
    out = pipe.generate_image("a cat and a dog on the grass", concepts, width=SIDE, height=SIDE, layer_indices=[0, 1],
                              num_inference_steps=2, return_pil_heatmaps=False, softmax=False, attention_norm="sparsemax")
    _check_maps(out.concept_heatmaps, 17), _check_maps(out.cross_attention_maps, 17)
    assert calls.n["heatmap_many"] > 0 and calls.n["heatmap_logits"] == calls.n["heatmap_fused"] == 0, calls.n
    out = pipe.encode_image(_picture(5), concepts, "a cat and a dog on the grass", width=SIDE, height=SIDE,
                            layer_indices=[0, 1], num_steps=2, noise_timestep=1, return_pil_heatmaps=False, softmax=False,
                            attention_norm="sparsemax")
    _check_maps(out.concept_heatmaps, 17), _check_maps(out.cross_attention_maps, 17)


def test_score_multiclass_images_with_12_concepts_equals_the_host_route(pipe, monkeypatch):
    images = [_picture(100 + i) for i in range(len(TARGETS))]
    captions = [",".join(f"a {c}" for c in t) for t in TARGETS]
    labels = []
    for i, t in enumerate(TARGETS):
        g = torch.Generator().manual_seed(300 + i)
        ids = torch.tensor([0] + [NAMES.index(c) for c in t])
        coarse = ids[torch.randint(0, len(ids), (7, 7), generator=g)]
        y = torch.nn.functional.interpolate(coarse[None, None].float(), size=(64, 64))[0, 0].numpy().astype(np.uint8)
        y[:2], y[-2:], y[:, :2], y[:, -2:] = 255, 255, 255, 255
        labels.append(y)
    assert all(len(BACKGROUND) + len(t) == 12 for t in TARGETS)
    seg = S.ConceptAttentionSegmentationModel(pipe)
    torch.manual_seed(7)       # the autoencoder draws its sampling noise from the device generator, one batch per forward
    host = S.MultiClassScores(len(NAMES))
    per_item = []
    for (pred, maps, _), y, t in zip(seg.segment_multiclass(images, captions, BACKGROUND, TARGETS, **KW), labels, TARGETS):
        assert tuple(maps.shape) == (12, SIDE // 16, SIDE // 16)
        klass = S.map_predictions_to_class_indices(pred, S.multiclass_table(BACKGROUND, t, NAMES))
        up = torch.nn.functional.interpolate(klass[None, None].float(), size=y.shape, mode="nearest")[0, 0]
        per_item.append(host.update(up, y, ignore_index=255))
    dev = S.DeviceMultiClassScores(len(NAMES), DEV)
    calls = Calls(monkeypatch)
    torch.manual_seed(7)
    seg.score_multiclass_images(images, captions, BACKGROUND, TARGETS, NAMES, labels, dev, ignore_index=255, **KW)
    monkeypatch.undo()
    assert calls.n["heatmap_many"] > 0 and calls.n["heatmap_logits"] == 0, calls.n
    got, rec, nc = dev.to_host(), dev.records(), len(NAMES)
    for row, i in zip(rec, dev.ids):
        want = per_item[i]
        assert (int(row[0]), int(row[1])) == (want["correct"], want["labelled"]), i
        assert np.array_equal(row[2:2 + nc], want["inter"]) and np.array_equal(row[2 + nc:], want["union"]), i
    assert (got.n, got.correct, got.labelled) == (host.n, host.correct, host.labelled) and host.n == len(TARGETS)
    assert np.array_equal(got.inter, host.inter) and np.array_equal(got.union, host.union)
    assert host.labelled > host.correct > 0, "the labels carry no signal"


def test_33_concepts_with_a_sparse_norm_are_refused_before_any_forward(pipe, monkeypatch):
    def no_forward(*a, **k):
        raise AssertionError("a forward was started")
    monkeypatch.setattr(pipe.flux_generator, "embed", no_forward)
    monkeypatch.setattr(pipe.flux_generator, "embed_many", no_forward)
    monkeypatch.setattr(type(pipe.flux_generator.model), "__call__", no_forward)
    sparse = dict(softmax=False, attention_norm="sparsemax")
    kw = dict(width=SIDE, height=SIDE, layer_indices=[0, 1])
    assert len(WORDS) == 33
    with pytest.raises(ValueError, match=r"33 concepts.*at most 32"):
        pipe.generate_image("a cat", WORDS, num_inference_steps=2, **kw, **sparse)
    with pytest.raises(ValueError, match=r"33 concepts.*at most 32"):
        pipe.encode_image(_picture(5), WORDS, "a cat", num_steps=2, noise_timestep=1, **kw, **sparse)
    with pytest.raises(ValueError, match=r"33 concepts.*at most 32"):
        pipe.generate_images(["a cat", "a dog"], [WORDS[:3], WORDS], num_inference_steps=2, **kw,
                             softmax=False, attention_norm="entmax15")
    with pytest.raises(ValueError, match=r"33 concepts.*at most 32"):
        pipe.encode_images([_picture(5), _picture(6)], WORDS, "a cat", num_steps=2, noise_timestep=1, **kw, **sparse)
    monkeypatch.undo()
    # the model call itself: refused where the norm is resolved, before the first launch
    case = case_of(33, 1, L.NORM_SPARSEMAX)
    m = TM.build(case)
    launched = []
    for name in ("gemm", "ln_modulate", "gemv", "attention", "timestep_embedding"):
        monkeypatch.setattr(ops, name, lambda *a, **k: launched.append(1))
    with pytest.raises(ValueError, match=r"33 concepts.*at most 32"):
        TM.forward(m, case, reqs=requests(case, 1))
    assert not launched
    monkeypatch.undo()
    # the softmax has no limit: 33 concepts take the three-launch form
    soft = case_of(33, 1, L.NORM_SOFTMAX)
    calls = Calls(monkeypatch)
    out = TM.forward(TM.build(soft), soft, reqs=requests(soft, 1))
    monkeypatch.undo()
    assert calls.n == dict(heatmap_many=0, heatmap_fused=0, heatmap_logits=2 * len(LAYERS)), calls.n
    assert abs(out.reqs[0].out_space.sum(0) - 1).max().item() < 1e-5
