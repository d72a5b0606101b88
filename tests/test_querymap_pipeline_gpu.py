"""query_maps through the public calls, on the tiny geometry (tiny_params, 256 x 256, 64 text tokens, the synthetic T5 +
CLIP text encoders behind the toy byte tokenizer): the kinds and their shapes, the words, batched calls item by item
against single calls, device pictures against host pictures, the DAAM class against a direct call, and every refusal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conceptattention_amd import ConceptAttentionFluxPipeline, DAAMFluxSegmentationModel  # noqa: E402
from conceptattention_amd import heatmaps as HM  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from conceptattention_amd.baselines import daam_caption, daam_concept_tokens  # noqa: E402
from conceptattention_amd.params import tiny_params  # noqa: E402
from conceptattention_amd.segmentation import ConceptAttentionSegmentationModel  # noqa: E402

DEV = "cuda:0"
SIDE = 256
MAP = SIDE // 16
LAT = (1, 16, SIDE // 8, SIDE // 8)
GEN = dict(width=SIDE, height=SIDE, layer_indices=[0, 1], num_inference_steps=2)
ENC = dict(width=SIDE, height=SIDE, layer_indices=[0, 1], num_steps=2, noise_timestep=1)
CONCEPTS = ["cat", "grass", "sky"]
PROMPTS = ["a cat", "a cat on the grass", "sky over a cat"]     # different token counts
BOTH = ("tokens", "concepts")


@pytest.fixture(scope="module")
def pipe():
    return ConceptAttentionFluxPipeline("flux-schnell", device=DEV, weights="synthetic", params=tiny_params(),
                                        n_text_tokens=64, text_encoder="synthetic-t5-clip")


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_generate_and_encode_return_both_kinds_and_the_words(pipe, monkeypatch):
    prompt = PROMPTS[1]
    launches = []
    real = ops.query_maps
    monkeypatch.setattr(ops, "query_maps", lambda *a, **k: (launches.append(len(a[0])), real(*a, **k))[1])
    kw = dict(latent=_randn(*LAT, seed=40), token_maps=True, return_pil_heatmaps=False, **GEN)
    raw = pipe.generate_image(prompt, CONCEPTS, query_maps=BOTH, **kw)
    assert launches == [2] * 4                            # 2 steps x 2 captured layers, both kinds in one launch
    q = raw.query_heatmaps
    assert set(q) == {"tokens", "concepts", "words"}
    assert raw.tokens == list(prompt) and raw.words == prompt.split()
    assert tuple(q["tokens"].shape) == (len(prompt), MAP, MAP) and tuple(q["concepts"].shape) == (len(CONCEPTS), MAP, MAP)
    assert tuple(q["words"].shape) == (len(raw.words), MAP, MAP)
    for t in q.values():
        assert t.is_cuda and t.dtype == torch.float32 and float(t.min()) > 0
    # a probability per (row, image key): over the image keys AND the row's leading keys it sums to 1, so below 1 here
    assert float(q["tokens"].sum((1, 2)).max()) < 1 and float(q["concepts"].sum((1, 2)).max()) < 1
    # the words are the sums of their tokens' maps, in both directions
    groups = HM.word_groups(raw.tokens)
    assert [w for w, _ in groups] == raw.words and groups[1] == ("cat", [2, 3, 4])
    assert torch.equal(q["words"], torch.stack([q["tokens"][ix].sum(0) for _, ix in groups]))
    assert raw.word_heatmaps.shape == (len(raw.words), MAP, MAP) and raw.word_heatmaps.dtype == np.float32
    tok = torch.as_tensor(raw.token_heatmaps, device=DEV)   # (summed on the device, as word_maps does: torch's order)
    assert np.array_equal(raw.word_heatmaps, torch.stack([tok[ix].sum(0) for _, ix in groups]).cpu().numpy())
    assert np.allclose(raw.word_heatmaps, np.stack([raw.token_heatmaps[ix].sum(0) for _, ix in groups]), rtol=1e-6, atol=0)
    # each kind alone has the bits it has beside the other; nothing else changes
    plain = pipe.generate_image(prompt, CONCEPTS, **kw)
    assert plain.query_heatmaps is None and plain.words == raw.words
    assert np.array_equal(plain.word_heatmaps, raw.word_heatmaps)
    for name in ("image", "concept_heatmaps", "cross_attention_maps", "token_heatmaps"):
        assert np.array_equal(getattr(plain, name), getattr(raw, name)), name
    con = pipe.generate_image(prompt, CONCEPTS, latent=kw["latent"], query_maps="concepts", return_pil_heatmaps=False, **GEN)
    assert set(con.query_heatmaps) == {"concepts"} and torch.equal(con.query_heatmaps["concepts"], q["concepts"])
    assert con.tokens is None and con.words is None and con.word_heatmaps is None
    five = pipe.generate_image(prompt, CONCEPTS, latent=kw["latent"], token_maps=5, query_maps="tokens", return_pil_heatmaps=False,
                               **GEN)
    assert set(five.query_heatmaps) == {"tokens"} and torch.equal(five.query_heatmaps["tokens"], q["tokens"][:5])
    enc = pipe.encode_image(_randn(*LAT, seed=41), CONCEPTS, prompt=prompt, noise=[_randn(*LAT, seed=6)], token_maps=True,
                            query_maps=BOTH, return_pil_heatmaps=False, **ENC)
    assert set(enc.query_heatmaps) == {"tokens", "concepts", "words"} and enc.words == prompt.split()
    assert tuple(enc.query_heatmaps["tokens"].shape) == (len(prompt), MAP, MAP)


def test_batched_calls_give_every_item_the_bits_of_its_single_call(pipe):
    lats = [_randn(*LAT, seed=50 + i) for i in range(3)]
    kw = dict(return_pil_heatmaps=False, token_maps=True, query_maps=BOTH, **GEN)
    many = pipe.generate_images(PROMPTS, CONCEPTS, latents=lats, batch=3, **kw)
    assert len({len(o.tokens) for o in many}) == 3
    for i, o in enumerate(many):
        one = pipe.generate_image(PROMPTS[i], CONCEPTS, latent=lats[i], **kw)
        assert o.words == one.words == PROMPTS[i].split()
        for kind in ("tokens", "concepts", "words"):
            assert torch.equal(o.query_heatmaps[kind], one.query_heatmaps[kind]), (i, kind)
        assert np.array_equal(o.token_heatmaps, one.token_heatmaps) and np.array_equal(o.image, one.image)
    noise = [[_randn(*LAT, seed=70 + i)] for i in range(3)]
    ekw = dict(return_pil_heatmaps=False, token_maps=True, query_maps=BOTH, **ENC)
    enc = pipe.encode_images(lats, CONCEPTS, PROMPTS, noise=noise, batch=3, **ekw)
    for i, o in enumerate(enc):
        one = pipe.encode_image(lats[i], CONCEPTS, prompt=PROMPTS[i], noise=noise[i], **ekw)
        for kind in ("tokens", "concepts", "words"):
            assert torch.equal(o.query_heatmaps[kind], one.query_heatmaps[kind]), (i, kind)


def test_device_pictures_are_the_host_pictures_byte_for_byte(pipe):
    def same(a, b, what):
        for name in ("concept_heatmaps", "cross_attention_maps", "token_heatmaps", "word_heatmaps"):
            la, lb = getattr(a, name), getattr(b, name)
            assert len(la) == len(lb) > 0, (what, name)
            for k, (x, y) in enumerate(zip(la, lb)):
                assert x.size == y.size and np.array_equal(np.asarray(x), np.asarray(y)), (what, name, k)
        assert a.words == b.words and set(a.query_heatmaps) == set(b.query_heatmaps) == {"tokens", "concepts", "words"}
        for kind in a.query_heatmaps:
            la, lb = a.query_heatmaps[kind], b.query_heatmaps[kind]
            assert len(la) == len(lb) > 0, (what, kind)
            for k, (x, y) in enumerate(zip(la, lb)):
                assert x.mode == "RGB" and x.size == y.size and np.array_equal(np.asarray(x), np.asarray(y)), (what, kind, k)
    kw = dict(latent=_randn(*LAT, seed=40), token_maps=True, query_maps=BOTH, **GEN)
    host = pipe.generate_image(PROMPTS[1], CONCEPTS, **kw)
    assert len(host.query_heatmaps["concepts"]) == len(CONCEPTS) and host.query_heatmaps["tokens"][0].size == (MAP, MAP)
    same(host, pipe.generate_image(PROMPTS[1], CONCEPTS, heatmap_renderer="device", **kw), "generate_image")
    lats = [_randn(*LAT, seed=50 + i) for i in range(3)]
    noise = [[_randn(*LAT, seed=70 + i)] for i in range(3)]
    ekw = dict(noise=noise, batch=3, token_maps=True, query_maps=BOTH, **ENC)
    for i, (a, b) in enumerate(zip(pipe.encode_images(lats, CONCEPTS, PROMPTS, **ekw),
                                   pipe.encode_images(lats, CONCEPTS, PROMPTS, heatmap_renderer="device", **ekw))):
        same(a, b, f"encode_images[{i}]")
    big = pipe.generate_image(PROMPTS[0], CONCEPTS, heatmap_renderer="device", heatmap_size=40, **kw)
    assert all(p.size == (40, 40) for p in big.query_heatmaps["concepts"] + big.word_heatmaps)


@pytest.mark.parametrize("direction", ["image_to_text", "text_to_image"])
def test_the_daam_class_returns_the_word_sums_of_a_direct_call(pipe, direction):
    model = DAAMFluxSegmentationModel(pipe)
    lats = [_randn(*LAT, seed=60 + i) for i in range(2)]
    noise = [[_randn(*LAT, seed=80 + i)] for i in range(2)]
    concepts, captions = ["cat", "grass"], ["a cat on grass", "the cat"]
    kw = dict(layers=[0, 1], num_steps=2, noise_timestep=1, height=SIDE, width=SIDE)
    got = model.segment_images(lats, concepts, captions, direction=direction, noise=noise, **kw)
    for i, (maps, extra) in enumerate(got):
        assert extra is None and tuple(maps.shape) == (len(concepts), MAP, MAP) and maps.is_cuda and maps.dtype == torch.float32
        prompt = daam_caption(captions[i], concepts)
        assert prompt == captions[i] + ",a cat, a grass"
        direct = pipe.encode_image(lats[i], concepts, prompt=prompt, noise=noise[i], token_maps=True, query_maps="tokens",
                                   return_pil_heatmaps=False, **ENC)
        idx = daam_concept_tokens(direct.tokens, concepts)
        # "a cat on grass,a cat, a grass": "cat" twice, in the caption and in the appended list; "the cat,a cat, a grass": the
        # caption's last word runs into the appended "a" (the reference's format has no space there), so "cat" once
        n_cat = 2 if i == 0 else 1
        assert len(HM.find_words(HM.word_groups(direct.tokens), "cat")) == n_cat
        src = direct.query_heatmaps["tokens"] if direction == "text_to_image" else torch.as_tensor(direct.token_heatmaps, device=DEV)
        want = torch.stack([src[ix].sum(0) for ix in idx])
        assert torch.equal(maps, want), (i, direction)
        # the word sums of the direct call's own word maps: every occurrence of the concept's word
        words = direct.query_heatmaps["words"] if direction == "text_to_image" else torch.as_tensor(direct.word_heatmaps, device=DEV)
        hits = [k for k, w in enumerate(direct.words) if HM.normalize_word(w) == "cat"]
        assert len(hits) == n_cat and torch.allclose(maps[0], words[hits].sum(0), rtol=1e-6, atol=0)
    one = model.segment_individual_image(lats[0], concepts, captions[0], direction=direction, noise_timestep=1, num_steps=2,
                                         layers=[0, 1], height=SIDE, width=SIDE)
    assert tuple(one[0].shape) == (len(concepts), MAP, MAP) and one[1] is None
    with pytest.raises(ValueError, match="direction"):
        model.segment_images(lats, concepts, captions, direction="both", **kw)
    with pytest.raises(ValueError, match="has no whole occurrence"):             # 64 text rows: the appended names are cut off
        model.segment_images(lats[:1], concepts, ["x" * 70], direction=direction, **kw)


def test_every_refusal_fires_before_a_launch(pipe, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a launch after a refusal was due")
    lat = _randn(*LAT, seed=40)
    kw = dict(latent=lat, **GEN)
    monkeypatch.setattr(ops, "gemm", no_launch)
    monkeypatch.setattr(ops, "query_maps", no_launch)
    with pytest.raises(ValueError, match="query_maps = "):
        pipe.generate_image("a cat", CONCEPTS, query_maps="words", **kw)
    with pytest.raises(ValueError, match="query_maps = "):
        pipe.generate_image("a cat", CONCEPTS, query_maps=("tokens", "tokens"), token_maps=True, **kw)
    with pytest.raises(ValueError, match="needs token_maps="):
        pipe.generate_image("a cat", CONCEPTS, query_maps="tokens", **kw)
    with pytest.raises(ValueError, match="needs token_maps="):
        pipe.encode_images([lat], CONCEPTS, ["a cat"], query_maps=BOTH, **ENC)
    with pytest.raises(ValueError, match="fused"):
        pipe.generate_image("a cat", CONCEPTS, query_maps="concepts", fused=False, **kw)
    with pytest.raises(ValueError, match="fused"):          # repeated timesteps / layers fall back to the stacked route
        pipe.generate_image("a cat", CONCEPTS, query_maps="concepts", timesteps=[0, 0], **kw)
    with pytest.raises(ValueError, match="fused"):
        pipe.generate_images(["a cat"], CONCEPTS, latents=[lat], query_maps="concepts", width=SIDE, height=SIDE,
                             layer_indices=[1, 1], num_inference_steps=2)
    for jak in ({"concept_cross_attention": False}, {"concept_self_attention": False}):
        with pytest.raises(ValueError, match="ablation joint_attention_kwargs"):
            pipe.encode_image(lat, CONCEPTS, prompt="a cat", query_maps="concepts", joint_attention_kwargs=jak, **ENC)
    with pytest.raises(ValueError, match="layer_noise_sweep: query_maps"):
        pipe.layer_noise_sweep(lat, CONCEPTS, "a cat", [1], num_steps=2, layer_indices=[0, 1], width=SIDE, height=SIDE,
                               query_maps="concepts")
    with pytest.raises(ValueError, match="score_sweep: query_maps"):
        ConceptAttentionSegmentationModel(pipe).score_sweep([lat], ["cat"], CONCEPTS, ["a cat"], [np.zeros((224, 224), np.uint8)],
                                                            None, [1], query_maps="concepts")
    monkeypatch.undo()
    traced = pipe.generate_image("a cat", CONCEPTS, keep_trace=True, **kw)
    monkeypatch.setattr(ops, "gemm", no_launch)
    with pytest.raises(ValueError, match="requery: query_maps"):
        pipe.requery(traced.trace, ["dog"], query_maps="concepts")
    monkeypatch.undo()
    # the text rows' maps are covered under the ablations (their key set does not change)
    out = pipe.encode_image(lat, CONCEPTS, prompt="a cat", query_maps="tokens", token_maps=True, return_pil_heatmaps=False,
                            joint_attention_kwargs={"concept_self_attention": False}, **ENC)
    assert set(out.query_heatmaps) == {"tokens", "words"}
