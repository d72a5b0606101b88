"""head_maps through the public calls, on the tiny geometry (tiny_params, 256 x 256, 8 text tokens, the seeded-noise text
encoder): shapes and devices, raw_heatmaps against the mean of head_maps, the three baseline classes against the
pipeline, normalize_concepts against a torch restatement, the ValueErrors, batched calls item by item against single
calls, and that a call without head_maps launches what it launched before and never calls ops.head_maps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import headmap_cases as H  # noqa: E402
from conceptattention_amd import ConceptAttentionFluxPipeline  # noqa: E402
from conceptattention_amd import baselines, ops  # noqa: E402
from conceptattention_amd.params import tiny_params  # noqa: E402

DEV = "cuda:0"
SIDE = 256
MAP = SIDE // 16
LAT = (1, 16, SIDE // 8, SIDE // 8)
GEN = dict(width=SIDE, height=SIDE, layer_indices=[0, 1], num_inference_steps=2, return_pil_heatmaps=False)
ENC = dict(width=SIDE, height=SIDE, layer_indices=[0, 1], num_steps=2, noise_timestep=1, return_pil_heatmaps=False)
CONCEPTS = ["cat", "grass", "sky"]
SPACES = ("output", "cross", "value")


@pytest.fixture(scope="module")
def pipe():
    return ConceptAttentionFluxPipeline("flux-schnell", device=DEV, weights="synthetic", params=tiny_params(), n_text_tokens=8)


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _check_shapes(out, spaces, NH, C):
    assert set(out.head_maps) == set(out.raw_heatmaps) == set(spaces)
    for s in spaces:
        hm, raw = out.head_maps[s], out.raw_heatmaps[s]
        assert hm.shape == (NH, C, MAP, MAP) and raw.shape == (C, MAP, MAP)
        assert hm.dtype == raw.dtype == torch.float32 and hm.is_cuda and raw.is_cuda
        assert float(hm.abs().max()) > 0


def _check_mean(out, spaces, NH):
    """raw_heatmaps[space] against head_maps[space].mean(0) for a call of ONE layer and ONE forward (weight 1 onto zeros,
    so both tensors hold the launch's values themselves): the stored per-head value is one rounding of the weight's
    product (U each), the kernel's head sum NH - 1 + 2 additions, its 1 / NH and the product 2, the store 1: (NH + 6) U on
    sum_h |w_h| / NH."""
    for s in spaces:
        hm, raw = out.head_maps[s].double(), out.raw_heatmaps[s].double()
        slack = (NH + 6) * H.U * hm.abs().sum(0) / NH + 1e-30
        assert bool(((hm.mean(0) - raw).abs() <= slack).all()), (s, float(((hm.mean(0) - raw).abs() / slack).max()))


def test_generate_and_encode_return_the_head_maps(pipe):
    NH = pipe.params.num_heads
    lat = _randn(*LAT, seed=40)
    gen = pipe.generate_image("a cat", CONCEPTS, latent=lat, head_maps=SPACES, **GEN)
    _check_shapes(gen, SPACES, NH, 3)
    one = pipe.generate_image("a cat", CONCEPTS, latent=lat, head_maps="cross", head_norm="sparsemax", **GEN)
    _check_shapes(one, ("cross",), NH, 3)
    assert bool((one.head_maps["cross"] >= 0).all())
    assert torch.allclose(one.head_maps["cross"].sum(1), torch.ones(NH, MAP, MAP, device=DEV), atol=1e-5)   # per head
    enc = pipe.encode_image(_randn(*LAT, seed=41), CONCEPTS, prompt="a cat", noise=[_randn(*LAT, seed=6)], head_maps=SPACES,
                            head_norm=["softmax"], **ENC)
    _check_shapes(enc, SPACES, NH, 3)
    for norm in (None, "softmax", "sparsemax"):
        single = pipe.encode_image(_randn(*LAT, seed=41), CONCEPTS, prompt="a cat", noise=[_randn(*LAT, seed=6)],
                                   head_maps=SPACES, head_norm=norm, **{**ENC, "layer_indices": [1]})
        _check_mean(single, SPACES, NH)
    # without head_maps the fields stay None; the image and the cross-space maps are the same bytes with and without,
    # the output-space maps the same bytes when only "cross" is asked
    plain = pipe.generate_image("a cat", CONCEPTS, latent=lat, **GEN)
    assert plain.head_maps is None and plain.raw_heatmaps is None
    assert np.array_equal(plain.image, gen.image) and np.array_equal(plain.cross_attention_maps, gen.cross_attention_maps)
    assert np.array_equal(plain.image, one.image) and np.array_equal(plain.concept_heatmaps, one.concept_heatmaps)
    shift = float(np.abs(plain.concept_heatmaps - gen.concept_heatmaps).max())
    # (held to its bound where the rows are at hand: tests/test_headmap_model_gpu.py, test_d)
    print(f"\n  generate_image, output-space concept maps with head_maps 'output': max shift {shift:.3e}")


def test_batched_calls_give_every_item_the_bits_of_its_single_call(pipe):
    lats = [_randn(*LAT, seed=50 + i) for i in range(3)]
    prompts = ["a cat", "sky", "a bus"]
    many = pipe.generate_images(prompts, CONCEPTS, latents=lats, batch=3, head_maps=SPACES, head_norm="entmax15", **GEN)
    for i, o in enumerate(many):
        one = pipe.generate_image(prompts[i], CONCEPTS, latent=lats[i], head_maps=SPACES, head_norm="entmax15", **GEN)
        for s in SPACES:
            assert torch.equal(o.head_maps[s], one.head_maps[s]) and torch.equal(o.raw_heatmaps[s], one.raw_heatmaps[s]), (i, s)
        assert np.array_equal(o.concept_heatmaps, one.concept_heatmaps) and np.array_equal(o.image, one.image)
    noise = [[_randn(*LAT, seed=70 + i)] for i in range(3)]
    enc = pipe.encode_images(lats, CONCEPTS, prompts, noise=noise, batch=3, head_maps="value", **ENC)
    for i, o in enumerate(enc):
        one = pipe.encode_image(lats[i], CONCEPTS, prompt=prompts[i], noise=noise[i], head_maps="value", **ENC)
        assert torch.equal(o.head_maps["value"], one.head_maps["value"]), i


def test_several_norms_in_one_call_are_the_single_norm_calls(pipe, monkeypatch):
    lat = _randn(*LAT, seed=47)
    names = (None, "softmax", "entmax15")
    launches = []
    real = ops.head_maps
    monkeypatch.setattr(ops, "head_maps", lambda *a, **k: (launches.append(len(a[0])), real(*a, **k))[1])
    many = pipe.generate_image("a cat", CONCEPTS, latent=lat, head_maps=("output", "value"), head_norm=names, **GEN)
    assert launches == [2] * 12                               # 2 steps x 2 captured layers x 3 norms, both spaces in one
    assert set(many.head_maps) == set(many.raw_heatmaps) == {(s, n) for s in ("output", "value") for n in names}
    for n in names:
        one = pipe.generate_image("a cat", CONCEPTS, latent=lat, head_maps=("output", "value"), head_norm=n, **GEN)
        for s in ("output", "value"):
            assert torch.equal(many.head_maps[(s, n)], one.head_maps[s]), (s, n)
            assert torch.equal(many.raw_heatmaps[(s, n)], one.raw_heatmaps[s]), (s, n)
        assert np.array_equal(many.image, one.image)


@pytest.mark.parametrize("cls,space,normalize", [(baselines.RawOutputSpaceSegmentationModel, "output", True),
                                                 (baselines.RawValueSpaceSegmentationModel, "value", True),
                                                 (baselines.RawCrossAttentionSegmentationModel, "cross", False)])
@pytest.mark.parametrize("softmax", [False, True])
def test_the_baseline_classes_return_the_pipelines_maps(pipe, cls, space, normalize, softmax):
    lat, noise = _randn(*LAT, seed=44), [_randn(*LAT, seed=7)]
    model = cls(pipe)
    assert model.normalize_default is normalize
    kw = dict(num_steps=2, noise_timestep=1, height=SIDE, width=SIDE)
    maps, rec = model.segment_images([lat], [CONCEPTS], ["a cat"], noise=[noise], **kw)[0]
    assert rec is None and maps.shape == (3, MAP, MAP) and maps.is_cuda
    want = pipe.encode_image(lat, CONCEPTS, prompt="a cat", noise=noise, head_maps=space, head_norm="softmax" if softmax else None,
                             head_normalize_concepts=normalize,
                             **{**ENC, "layer_indices": list(range(pipe.params.depth))})
    got = model.segment_images([lat], [CONCEPTS], ["a cat"], noise=[noise], softmax=softmax, **kw)[0][0]
    assert torch.equal(got, want.raw_heatmaps[space])
    if not softmax:
        assert torch.equal(maps, got)
    # the single-image form is the batched form of one
    single = model.segment_individual_image(lat, CONCEPTS, "a cat", softmax=softmax, **kw)[0]
    assert single.shape == (3, MAP, MAP)


def test_normalize_concepts_changes_the_maps_as_the_restatement_says(pipe, monkeypatch):
    """The launch of a normalising call reads concept rows that are heatmaps.linear_normalization of the rows the plain
    call reads, and the same image rows."""
    from conceptattention_amd.heatmaps import linear_normalization
    seen = {}
    real = ops.head_maps

    def spy(problems, num_heads, norm=0):
        seen.setdefault(spy.key, []).append([(p.img.clone(), p.con.float().clone()) for p in problems])
        return real(problems, num_heads, norm)
    monkeypatch.setattr(ops, "head_maps", spy)
    lat, noise = _randn(*LAT, seed=45), [_randn(*LAT, seed=8)]
    for key in (False, True):
        spy.key = key
        pipe.encode_image(lat, CONCEPTS, prompt="a cat", noise=noise, head_maps=SPACES, head_normalize_concepts=key, **ENC)
    assert len(seen[False]) == len(seen[True]) == 2          # one launch per captured layer
    for plain, normed in zip(seen[False], seen[True]):
        assert len(plain) == len(normed) == 3
        for (img0, con0), (img1, con1) in zip(plain, normed):
            assert torch.equal(img0, img1)
            assert torch.equal(con1, linear_normalization(con0, dim=0))
            assert torch.allclose(con1.sum(0), torch.ones_like(con1[0]), atol=1e-5) and bool((con1 >= 0).all())


def test_the_refusals_are_value_errors(pipe):
    lat = _randn(*LAT, seed=40)
    with pytest.raises(ValueError, match="head_maps needs the fused route"):
        pipe.generate_image("a cat", CONCEPTS, latent=lat, head_maps="cross", fused=False, **GEN)
    with pytest.raises(ValueError, match="head_maps needs the fused route"):     # repeated timesteps: the stacked route
        pipe.generate_image("a cat", CONCEPTS, latent=lat, head_maps="cross", timesteps=[0, 0], **GEN)
    with pytest.raises(ValueError, match="head_maps = 'keys'"):
        pipe.generate_image("a cat", CONCEPTS, latent=lat, head_maps="keys", **GEN)
    with pytest.raises(ValueError, match="head_maps = "):
        pipe.encode_image(lat, CONCEPTS, prompt="a cat", head_maps=("cross", "cross"), **ENC)
    with pytest.raises(ValueError, match="head_norm = 'softmin'"):
        pipe.generate_image("a cat", CONCEPTS, latent=lat, head_maps="cross", head_norm="softmin", **GEN)
    with pytest.raises(ValueError, match="a sequence of distinct ones"):
        pipe.generate_image("a cat", CONCEPTS, latent=lat, head_maps="cross", head_norm=("softmax", "softmax"), **GEN)
    with pytest.raises(ValueError, match="head_norm is the norm of head_maps"):
        pipe.generate_image("a cat", CONCEPTS, latent=lat, head_norm="softmax", **GEN)
    with pytest.raises(ValueError, match="head maps: the ablation joint_attention_kwargs"):
        pipe.encode_image(lat, CONCEPTS, prompt="a cat", head_maps="value",
                          joint_attention_kwargs={"concept_cross_attention": False}, **ENC)
    with pytest.raises(ValueError, match="head_maps: 33 concepts"):
        pipe.encode_image(lat, [f"c{i}" for i in range(33)], prompt="a cat", head_maps="value", **ENC)
    pipe.model.capture_independent_image = True
    try:
        with pytest.raises(ValueError, match="capture_independent_image=True is not covered by the output-space head maps"):
            pipe.generate_image("a cat", CONCEPTS, latent=lat, head_maps=("cross", "output"), **GEN)
    finally:
        pipe.model.capture_independent_image = False
    out = pipe.encode_image(lat, CONCEPTS, prompt="a cat", keep_trace=True, **ENC)
    try:
        with pytest.raises(TypeError):                       # requery has no head_maps argument: a follow-up
            pipe.requery(out.trace, ["dog"], head_maps="cross")
    finally:
        out.trace.release()


def test_without_head_maps_the_launches_are_the_ones_of_a_call_that_never_heard_of_them(pipe, monkeypatch):
    """The list of launched GEMMs and attention launches (the ops hooks) and of every other entry point (the return-code
    check every call goes through) with head_maps=None: ops.head_maps is never called, and asking for head maps adds
    ca_head_maps launches and nothing else when the space needs no other route."""
    from conceptattention_amd import _lib as L
    lat = _randn(*LAT, seed=46)

    def launches(**kw):
        log, heads = [], []
        ops.set_gemm_hook(lambda arr, tile, launch: (log.append(("gemm", len(arr), tile)), launch())[1])
        ops.set_attn_hook(lambda *a: (log.append(("attn",)), a[-1]())[1])
        real_check, real_heads = L.check, ops.head_maps
        monkeypatch.setattr(L, "check", lambda rc, what="": (log.append(what), real_check(rc, what))[1])
        monkeypatch.setattr(ops, "head_maps", lambda *a, **k: (heads.append(len(a[0])), real_heads(*a, **k))[1])
        try:
            pipe.generate_image("a cat", CONCEPTS, latent=lat, **kw, **GEN)
        finally:
            ops.set_gemm_hook(None)
            ops.set_attn_hook(None)
            monkeypatch.undo()
        return log, heads
    base, heads0 = launches()
    again, _ = launches(head_maps=None)
    assert heads0 == [] and "ca_head_maps" not in base and base == again
    quiet, heads1 = launches(head_maps=("cross", "value"))
    assert heads1 == [2] * 4                                  # 2 steps x 2 captured layers, one launch for both spaces
    assert [x for x in quiet if x != "ca_head_maps"] == base
    assert quiet.count("ca_head_maps") == 4
