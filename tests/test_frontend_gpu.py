"""The batched front end on the GPU: image bytes and prompt strings in, heat maps (and image bytes) out, several items per
launch -- and every item with the bits of its own single call.  Tiny DiT, the full-size autoencoder and the two-block text
encoders on synthetic weights, 256 x 256.  No tolerance in this file: everything is torch.equal / np.array_equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conceptattention_amd import ConceptAttentionFluxPipeline, ops  # noqa: E402
from conceptattention_amd.params import tiny_params  # noqa: E402

DEV = "cuda:0"
SIDE = 256
SIZES = [(256, 256), (200, 300), (64, 64)]     # source sizes: identity, a non-integer resize, an upsample by 4


@pytest.fixture(scope="module")
def pipe():
    return ConceptAttentionFluxPipeline("flux-schnell", device=DEV, weights="synthetic", params=tiny_params(),
                                        n_text_tokens=64, autoencoder="synthetic", text_encoder="synthetic-t5-clip")


def _array(i, size=None):
    h, w = size or SIZES[i % len(SIZES)]
    return np.random.default_rng(100 + i).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _pil(i, size=None):
    import PIL.Image
    return PIL.Image.fromarray(_array(i, size))


def _todays_preprocessing(arr):
    """pipeline.encode_image's conversion before this path existed: the fp32 image tensor the autoencoder was given."""
    t = torch.from_numpy(arr).permute(2, 0, 1).float() / 255.0
    return torch.nn.functional.interpolate((2.0 * t - 1.0)[None].to(DEV), (SIDE, SIDE))


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_encode_pixels_equals_encode_of_todays_preprocessing(pipe):
    ae = pipe.autoencoder
    arrays = [_array(i) for i in range(3)]
    noise = _randn(3, 16, SIDE // 8, SIDE // 8, seed=1).to(DEV)
    want = ae.encode(torch.cat([_todays_preprocessing(a) for a in arrays]), noise=noise)
    got = ae.encode_pixels(arrays, SIDE, SIDE, noise=noise)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 16, SIDE // 8, SIDE // 8)
    assert torch.equal(got, want)
    assert torch.equal(ae.encode_pixels([torch.from_numpy(a) for a in arrays], SIDE, SIDE, sample=False),
                       ae.encode(torch.cat([_todays_preprocessing(a) for a in arrays]), sample=False))
    with pytest.raises(ValueError):
        ae.encode_pixels([arrays[0].astype(np.float32)], SIDE, SIDE)
    with pytest.raises(ValueError):
        ae.encode_pixels(arrays, SIDE + 4, SIDE)


def test_decode_pixels_equals_todays_byte_conversion(pipe):
    ae = pipe.autoencoder
    z = (3.0 * _randn(2, 16, 8, 8, seed=2)).to(DEV)           # (the clamp's edges are tests/test_pixel_kernels_gpu.py's)
    img = ae.decode(z)
    want = (127.5 * (img.clamp(-1, 1).permute(0, 2, 3, 1) + 1.0)).cpu().byte()
    got = ae.decode_pixels(z)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (2, 64, 64, 3)
    assert torch.equal(got.cpu(), want)
    print(f"decode_pixels: {len(torch.unique(want))} distinct bytes, {int((want == 0).sum())} at 0, {int((want == 255).sum())} at 255")
    assert len(torch.unique(want)) > 10                        # an image, not a constant


def test_pixel_routes_in_several_passes_equal_one_pass(pipe, monkeypatch):
    """At 1024 x 1024 one image fills a pass (MAX_PIXELS), so every batched call there takes the several-pass branches:
    the same branches with the bound lowered to one 256 x 256 image, and no launch larger than before."""
    ae = pipe.autoencoder
    arrays = [_array(i) for i in range(3)]
    noise = _randn(3, 16, SIDE // 8, SIDE // 8, seed=3).to(DEV)
    z = _randn(3, 16, 8, 8, seed=4).to(DEV)
    one_enc, one_dec = ae.encode_pixels(arrays, SIDE, SIDE, noise=noise), ae.decode_pixels(z)
    monkeypatch.setattr(ae, "MAX_PIXELS", SIDE * SIDE)
    assert ae._items_per_pass(SIDE, SIDE, "test") == 1
    assert torch.equal(ae.encode_pixels(arrays, SIDE, SIDE, noise=noise), one_enc)
    monkeypatch.setattr(ae, "MAX_PIXELS", 64 * 64)
    assert ae._items_per_pass(64, 64, "test") == 1
    assert torch.equal(ae.decode_pixels(z), one_dec)


def test_embed_many_equals_embed_per_item_and_encodes_each_string_once(pipe):
    gen = pipe.flux_generator
    gen.concept_cache.bind(None)                                # an empty cache, whatever ran before
    prompts = ["a cat on the grass", "a dog in the snow", "a cat on the grass"]
    concepts = [["cat", "grass"], ["dog", "snow", "sky"], ["grass", "sky"]]
    before = gen.t5_sequences_encoded
    many = gen.embed_many(prompts, concepts)
    assert gen.t5_sequences_encoded - before == 2 + 5           # the distinct prompts and the distinct concepts
    for item, p, c in zip(many, prompts, concepts):
        single = gen.embed(p, c)
        assert len(item) == len(single) == 5
        for a, b in zip(item, single):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    before = gen.t5_sequences_encoded
    again = gen.embed_many(["a bird", "a fish"], [["cat", "grass"], ["dog", "snow", "sky"]])
    assert gen.t5_sequences_encoded - before == 2               # only the new prompts: every concept came from the cache
    assert torch.equal(again[1][2], gen.embed("a fish", ["dog", "snow", "sky"])[2])


def _count_gemm_launches(fn):
    n = [0]

    def hook(arr, tile, launch):
        n[0] += 1
        launch()
    ops.set_gemm_hook(hook)
    try:
        out = fn()
    finally:
        ops.set_gemm_hook(None)
    return out, n[0]


def test_clip_sends_its_sequences_through_one_pass_and_seventeen_through_two(pipe):
    clip = pipe.text_encoder.clip_embedder
    enc = clip.encoder
    ids = clip.token_ids([f"prompt number {i} " + "x" * i for i in range(17)])
    one, n1 = _count_gemm_launches(lambda: enc.encode_ids(ids[:1]))
    five, n5 = _count_gemm_launches(lambda: enc.encode_ids(ids[:5]))
    assert n1 == 4 * enc.params.num_hidden_layers and n5 == n1  # as many GEMM launches for 5 sequences as for 1
    all17, n17 = _count_gemm_launches(lambda: enc.encode_ids(ids))
    assert n17 == 2 * n1                                        # 16 + 1
    ws = enc._ws
    for i in range(17):
        assert torch.equal(enc.encode_ids(ids[i:i + 1]), all17[i:i + 1]), i
    for n in range(1, 17):          # every count of a pass: each puts the sequences' rows into other row tiles
        assert torch.equal(enc.encode_ids(ids[:n]), all17[:n]), n
    assert torch.equal(five, all17[:5]) and torch.equal(one, all17[:1]) and enc._ws is ws
    hidden = enc.hidden_states(ids)
    assert torch.equal(enc.hidden_states(ids[16:17]), hidden[16:17]) and torch.equal(enc.hidden_states(ids[3:4]), hidden[3:4])
    assert torch.equal(clip.clip_many(["a", "b", "a"])[2:3], clip.clip("a"))


def test_encode_images_runs_in_chunks_and_every_item_equals_its_single_call(pipe, monkeypatch):
    n = 7
    images = [_pil(i) for i in range(n)]
    concepts = [["cat", "grass", "sky"] if i in (1, 4) else ["cat", "grass"] for i in range(n)]   # a second group
    prompts = [f"a cat on the grass, picture {i % 3}" for i in range(n)]
    lat_shape = (1, 16, SIDE // 8, SIDE // 8)
    noise = [[_randn(*lat_shape, seed=10 + i)] for i in range(n)]
    vae_noise = [_randn(*lat_shape, seed=30 + i) for i in range(n)]
    kw = dict(width=SIDE, height=SIDE, layer_indices=[0, 1], num_steps=2, noise_timestep=1, return_pil_heatmaps=False)
    forwards = []
    real = pipe._encode_maps

    def spy(model, latent, *a, **k):
        forwards.append(latent.shape[0])
        return real(model, latent, *a, **k)
    monkeypatch.setattr(pipe, "_encode_maps", spy)
    outs = pipe.encode_images(images, concepts, prompts, batch=5, noise=noise, vae_noise=vae_noise, **kw)
    assert forwards == [5, 2]                                    # the five 2-concept items, then the two 3-concept ones
    monkeypatch.undo()
    assert len(outs) == n
    for i in range(n):
        one = pipe.encode_image(images[i], concepts[i], prompt=prompts[i], noise=noise[i], vae_noise=vae_noise[i], **kw)
        assert outs[i].image is images[i]
        assert outs[i].concept_heatmaps.shape == (len(concepts[i]), SIDE // 16, SIDE // 16)
        assert np.array_equal(outs[i].concept_heatmaps, one.concept_heatmaps), i
        assert np.array_equal(outs[i].cross_attention_maps, one.cross_attention_maps), i
    assert not np.array_equal(outs[0].concept_heatmaps, outs[2].concept_heatmaps)
    # a smaller batch cuts the same groups into more forwards and changes no bit
    small = pipe.encode_images(images[:4], concepts[:4], prompts[:4], batch=2, noise=noise[:4], vae_noise=vae_noise[:4], **kw)
    for i in range(4):
        assert np.array_equal(small[i].concept_heatmaps, outs[i].concept_heatmaps), i


def test_encode_image_with_vae_noise_is_reproducible_and_equals_the_old_route(pipe):
    img = _pil(1)
    vn = _randn(1, 16, SIDE // 8, SIDE // 8, seed=5)
    kw = dict(prompt="a cat", width=SIDE, height=SIDE, layer_indices=[0, 1], num_steps=2, noise_timestep=1,
              return_pil_heatmaps=False, noise=[_randn(1, 16, SIDE // 8, SIDE // 8, seed=6)])
    a = pipe.encode_image(img, ["cat", "grass"], vae_noise=vn, **kw)
    b = pipe.encode_image(img, ["cat", "grass"], vae_noise=vn, **kw)
    assert np.array_equal(a.concept_heatmaps, b.concept_heatmaps)
    latent = pipe.autoencoder.encode(_todays_preprocessing(np.asarray(img)), noise=vn.to(DEV)).to(torch.bfloat16)
    c = pipe.encode_image(latent, ["cat", "grass"], **kw)       # the latent of the route this one replaced
    assert np.array_equal(a.concept_heatmaps, c.concept_heatmaps)
    assert np.array_equal(a.cross_attention_maps, c.cross_attention_maps)


def test_generate_images_equals_generate_image_per_item(pipe):
    prompts = ["a cat on the grass", "a dog in the snow", "a bird in the sky"]
    concepts = ["animal", "ground", "sky"]
    latents = [_randn(1, 16, SIDE // 8, SIDE // 8, seed=40 + i) for i in range(3)]
    kw = dict(width=SIDE, height=SIDE, layer_indices=[0, 1], num_inference_steps=2, return_pil_heatmaps=False)
    outs = pipe.generate_images(prompts, concepts, latents=latents, **kw)
    assert len(outs) == 3
    for i in range(3):
        one = pipe.generate_image(prompts[i], concepts, latent=latents[i], **kw)
        assert outs[i].image.size == (SIDE, SIDE)
        assert np.array_equal(np.asarray(outs[i].image), np.asarray(one.image)), i
        assert np.array_equal(outs[i].concept_heatmaps, one.concept_heatmaps), i
        assert np.array_equal(outs[i].cross_attention_maps, one.cross_attention_maps), i
    assert not np.array_equal(np.asarray(outs[0].image), np.asarray(outs[1].image))
