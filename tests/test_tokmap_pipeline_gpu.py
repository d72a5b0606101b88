"""token_maps through the public calls, on the tiny geometry (tiny_params, 256 x 256, 64 text tokens, the synthetic T5 +
CLIP text encoders behind the toy byte tokenizer): the token list, the counts, the int route with the seeded-noise
encoder, the ValueErrors, batched calls item by item against single calls, and device pictures against host pictures."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conceptattention_amd import ConceptAttentionFluxPipeline  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from conceptattention_amd.params import tiny_params  # noqa: E402

DEV = "cuda:0"
SIDE = 256
MAP = SIDE // 16
LAT = (1, 16, SIDE // 8, SIDE // 8)
GEN = dict(width=SIDE, height=SIDE, layer_indices=[0, 1], num_inference_steps=2)
ENC = dict(width=SIDE, height=SIDE, layer_indices=[0, 1], num_steps=2, noise_timestep=1)
CONCEPTS = ["cat", "grass", "sky"]
PROMPTS = ["a cat", "a cat on the grass", "sky", "the dog by a tree in a park", "a bus"]     # different token counts


@pytest.fixture(scope="module")
def pipe():
    return ConceptAttentionFluxPipeline("flux-schnell", device=DEV, weights="synthetic", params=tiny_params(),
                                        n_text_tokens=64, text_encoder="synthetic-t5-clip")


@pytest.fixture(scope="module")
def noise_pipe():          # the seeded-noise text encoder: no tokenizer
    return ConceptAttentionFluxPipeline("flux-schnell", device=DEV, weights="synthetic", params=tiny_params(), n_text_tokens=8)


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _tokens(pipe, prompt):
    ids = pipe.text_encoder.tokenizer(prompt, max_length=64)["input_ids"][0]
    n = int((ids != 0).sum()) - 1                         # without the end-of-string token
    return [chr(int(i) - 3) for i in ids[:n]]


def test_generate_and_encode_return_one_map_per_token_of_the_prompt(pipe, monkeypatch):
    prompt = PROMPTS[1]
    want = _tokens(pipe, prompt)
    assert want == list(prompt) and want == pipe.text_encoder.tokenizer.tokenize(prompt)
    launches = []
    real = ops.token_maps
    monkeypatch.setattr(ops, "token_maps", lambda *a, **k: (launches.append(len(a[0])), real(*a, **k))[1])
    gen = pipe.generate_image(prompt, CONCEPTS, latent=_randn(*LAT, seed=40), token_maps=True, **GEN)
    assert launches == [1] * 4                            # 2 steps x 2 captured layers
    assert gen.tokens == want and len(gen.token_heatmaps) == len(want)
    assert gen.token_heatmaps[0].size == (MAP, MAP) and gen.token_heatmaps[0].mode == "RGB"
    enc = pipe.encode_image(_randn(*LAT, seed=41), CONCEPTS, prompt=prompt, noise=[_randn(*LAT, seed=6)], token_maps=True, **ENC)
    assert enc.tokens == want and len(enc.token_heatmaps) == len(want)
    raw = pipe.generate_image(prompt, CONCEPTS, latent=_randn(*LAT, seed=40), token_maps=True, return_pil_heatmaps=False, **GEN)
    assert raw.token_heatmaps.shape == (len(want), MAP, MAP) and raw.token_heatmaps.dtype == np.float32
    # a probability per (token, patch): positive, and over ALL 64 text rows and the image keys it sums to 1, so below 1 here
    assert raw.token_heatmaps.min() > 0 and raw.token_heatmaps.sum(0).max() < 1
    # without token_maps: the fields stay None and everything else is the same bytes
    plain = pipe.generate_image(prompt, CONCEPTS, latent=_randn(*LAT, seed=40), return_pil_heatmaps=False, **GEN)
    assert plain.token_heatmaps is None and plain.tokens is None
    assert np.array_equal(plain.image, raw.image) and np.array_equal(plain.concept_heatmaps, raw.concept_heatmaps)
    assert np.array_equal(plain.cross_attention_maps, raw.cross_attention_maps)
    # the first n rows by count are the first n tokens' maps
    five = pipe.generate_image(prompt, CONCEPTS, latent=_randn(*LAT, seed=40), token_maps=5, return_pil_heatmaps=False, **GEN)
    assert five.tokens is None and np.array_equal(five.token_heatmaps, raw.token_heatmaps[:5])


def test_an_int_works_without_a_tokenizer_and_true_raises(noise_pipe):
    kw = dict(latent=_randn(*LAT, seed=42), return_pil_heatmaps=False, **GEN)
    out = noise_pipe.generate_image("a cat", CONCEPTS, token_maps=3, **kw)
    assert out.tokens is None and out.token_heatmaps.shape == (3, MAP, MAP) and out.token_heatmaps.min() > 0
    all_rows = noise_pipe.generate_image("a cat", CONCEPTS, token_maps=8, **kw)
    assert np.array_equal(all_rows.token_heatmaps[:3], out.token_heatmaps)
    enc = noise_pipe.encode_image(_randn(*LAT, seed=43), CONCEPTS, prompt="a cat", token_maps=2, return_pil_heatmaps=False, **ENC)
    assert enc.token_heatmaps.shape == (2, MAP, MAP)
    with pytest.raises(ValueError, match="token_maps=True needs a text encoder whose tokenizer"):
        noise_pipe.generate_image("a cat", CONCEPTS, token_maps=True, **kw)
    with pytest.raises(ValueError, match="token_maps=True needs a text encoder whose tokenizer"):
        noise_pipe.encode_image(_randn(*LAT, seed=43), CONCEPTS, prompt="a cat", token_maps=True, **ENC)
    for bad in (0, 9, -1):
        with pytest.raises(ValueError, match="token_maps = "):
            noise_pipe.generate_image("a cat", CONCEPTS, token_maps=bad, **kw)
        with pytest.raises(ValueError, match="token_maps = "):       # the batched calls raise alike
            noise_pipe.generate_images(["a cat"], CONCEPTS, latents=[kw["latent"]], token_maps=bad, return_pil_heatmaps=False, **GEN)
        with pytest.raises(ValueError, match="token_maps = "):
            noise_pipe.encode_images([_randn(*LAT, seed=43)], CONCEPTS, ["a cat"], token_maps=bad, **ENC)
    assert noise_pipe.generate_images(["a cat"], CONCEPTS, latents=[kw["latent"]], token_maps=False, return_pil_heatmaps=False,
                                      **GEN)[0].token_heatmaps is None


def test_the_stacked_route_raises(pipe):
    with pytest.raises(ValueError, match="fused"):
        pipe.generate_image("a cat", CONCEPTS, latent=_randn(*LAT, seed=40), token_maps=True, fused=False, **GEN)
    with pytest.raises(ValueError, match="fused"):          # repeated timesteps fall back to the stacked route
        pipe.generate_image("a cat", CONCEPTS, latent=_randn(*LAT, seed=40), token_maps=True, timesteps=[0, 0], **GEN)
    with pytest.raises(ValueError, match="no tokens"):
        pipe.generate_image("", CONCEPTS, latent=_randn(*LAT, seed=40), token_maps=True, **GEN)


def test_batched_calls_give_every_item_the_bits_of_its_single_call(pipe):
    lats = [_randn(*LAT, seed=50 + i) for i in range(5)]
    kw = dict(return_pil_heatmaps=False, **GEN)
    many = pipe.generate_images(PROMPTS, CONCEPTS, latents=lats, batch=5, token_maps=True, **kw)
    assert len({len(o.tokens) for o in many}) > 2
    for i, o in enumerate(many):
        one = pipe.generate_image(PROMPTS[i], CONCEPTS, latent=lats[i], token_maps=True, **kw)
        assert o.tokens == one.tokens == list(PROMPTS[i])
        assert np.array_equal(o.token_heatmaps, one.token_heatmaps), i
        assert np.array_equal(o.concept_heatmaps, one.concept_heatmaps) and np.array_equal(o.image, one.image)
    noise = [[_randn(*LAT, seed=70 + i)] for i in range(5)]
    ekw = dict(return_pil_heatmaps=False, **ENC)
    enc = pipe.encode_images(lats, CONCEPTS, PROMPTS, noise=noise, batch=5, token_maps=True, **ekw)
    for i, o in enumerate(enc):
        one = pipe.encode_image(lats[i], CONCEPTS, prompt=PROMPTS[i], noise=noise[i], token_maps=True, **ekw)
        assert o.tokens == one.tokens and np.array_equal(o.token_heatmaps, one.token_heatmaps), i
    counted = pipe.generate_images(PROMPTS[:2], CONCEPTS, latents=lats[:2], batch=2, token_maps=2, **kw)
    assert all(o.tokens is None and np.array_equal(o.token_heatmaps, many[i].token_heatmaps[:2]) for i, o in enumerate(counted))
    assert all(o.token_heatmaps is None for o in pipe.generate_images(PROMPTS[:2], CONCEPTS, latents=lats[:2], batch=2, **kw))


def test_device_pictures_are_the_host_pictures_byte_for_byte(pipe):
    def same(a, b, what):
        for name in ("concept_heatmaps", "cross_attention_maps", "token_heatmaps"):
            la, lb = getattr(a, name), getattr(b, name)
            assert len(la) == len(lb) > 0, (what, name)
            for k, (x, y) in enumerate(zip(la, lb)):
                assert x.size == y.size and np.array_equal(np.asarray(x), np.asarray(y)), (what, name, k)
        assert a.tokens == b.tokens
    kw = dict(latent=_randn(*LAT, seed=40), token_maps=True, **GEN)
    same(pipe.generate_image(PROMPTS[1], CONCEPTS, **kw), pipe.generate_image(PROMPTS[1], CONCEPTS, heatmap_renderer="device", **kw),
         "generate_image")
    ekw = dict(prompt=PROMPTS[3], noise=[_randn(*LAT, seed=6)], token_maps=True, **ENC)
    lat = _randn(*LAT, seed=44)
    same(pipe.encode_image(lat, CONCEPTS, **ekw), pipe.encode_image(lat, CONCEPTS, heatmap_renderer="device", **ekw), "encode_image")
    lats = [_randn(*LAT, seed=50 + i) for i in range(3)]
    host = pipe.generate_images(PROMPTS[:3], CONCEPTS, latents=lats, batch=3, token_maps=True, **GEN)
    dev = pipe.generate_images(PROMPTS[:3], CONCEPTS, latents=lats, batch=3, token_maps=True, heatmap_renderer="device", **GEN)
    for i, (a, b) in enumerate(zip(host, dev)):
        same(a, b, f"generate_images[{i}]")
    big = pipe.generate_image(PROMPTS[0], CONCEPTS, heatmap_renderer="device", heatmap_size=40, **kw)
    assert all(p.size == (40, 40) for p in big.token_heatmaps)
