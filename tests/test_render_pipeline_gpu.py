"""heatmap_renderer="device" through the public calls, on the tiny geometry of tests/test_frontend_gpu.py: the default
pictures are the host route's byte for byte; overlays and resized pictures equal the numpy restatement
(tests/render_cases.py) applied to the downloaded accumulators and picture bytes; concept_attention_frames on a tiny sweep
table equals the restatement under both range rules.  No tolerance in this file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import render_cases as R  # noqa: E402
from conceptattention_amd import ConceptAttentionFluxPipeline, concept_attention_frames  # noqa: E402
from conceptattention_amd.params import tiny_params  # noqa: E402

DEV = "cuda:0"
SIDE = 256
MAP = SIDE // 16


@pytest.fixture(scope="module")
def pipe():
    return ConceptAttentionFluxPipeline("flux-schnell", device=DEV, weights="synthetic", params=tiny_params(),
                                        n_text_tokens=64, autoencoder="synthetic", text_encoder="synthetic-t5-clip")


def _pil(i, size=(SIDE, SIDE)):
    import PIL.Image
    return PIL.Image.fromarray(np.random.default_rng(100 + i).integers(0, 256, size=size + (3,), dtype=np.uint8))


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


LAT = (1, 16, SIDE // 8, SIDE // 8)
GEN = dict(width=SIDE, height=SIDE, layer_indices=[0, 1], num_inference_steps=2)
ENC = dict(width=SIDE, height=SIDE, layer_indices=[0, 1], num_steps=2, noise_timestep=1)


def _same_pictures(a, b, what):
    for name in ("concept_heatmaps", "cross_attention_maps"):
        la, lb = getattr(a, name), getattr(b, name)
        assert len(la) == len(lb) > 0, (what, name)
        for k, (x, y) in enumerate(zip(la, lb)):
            assert x.size == y.size and x.mode == y.mode == "RGB", (what, name, k)
            assert np.array_equal(np.asarray(x), np.asarray(y)), (what, name, k)


def _restated(raw, cmap, **kw):
    """The two lists of pictures the restatement makes from an output with return_pil_heatmaps=False."""
    lut = R.cmap_lut(cmap)
    return [R.render(np.ascontiguousarray(m, dtype=np.float32), lut, **kw)[0]
            for m in (raw.concept_heatmaps, raw.cross_attention_maps)]


def _equals_restatement(out, want, what):
    for name, ref in zip(("concept_heatmaps", "cross_attention_maps"), want):
        got = getattr(out, name)
        assert len(got) == len(ref), (what, name)
        for k in range(len(ref)):
            assert np.array_equal(np.asarray(got[k]), ref[k]), (what, name, k)


def test_generate_image_device_pictures_are_the_hosts_and_overlays_the_restatements(pipe):
    latent = _randn(*LAT, seed=40)
    kw = dict(latent=latent, **GEN)
    host = pipe.generate_image("a cat on the grass", ["cat", "grass", "sky"], **kw)
    dev = pipe.generate_image("a cat on the grass", ["cat", "grass", "sky"], heatmap_renderer="device", **kw)
    assert np.array_equal(np.asarray(host.image), np.asarray(dev.image))
    assert dev.concept_heatmaps[0].size == (MAP, MAP)
    _same_pictures(host, dev, "generate_image")
    jet = pipe.generate_image("a cat on the grass", ["cat", "grass", "sky"], heatmap_renderer="device", cmap="jet", **kw)
    _same_pictures(pipe.generate_image("a cat on the grass", ["cat", "grass", "sky"], cmap="jet", **kw), jet, "jet")
    raw = pipe.generate_image("a cat on the grass", ["cat", "grass", "sky"], return_pil_heatmaps=False, **kw)
    picture = np.asarray(raw.image)
    over = pipe.generate_image("a cat on the grass", ["cat", "grass", "sky"], heatmap_renderer="device",
                               heatmap_interpolation="bilinear", overlay_alpha=0.5, **kw)
    assert np.array_equal(np.asarray(over.image), picture) and over.concept_heatmaps[0].size == (SIDE, SIDE)
    _equals_restatement(over, _restated(raw, "plasma", H=SIDE, W=SIDE, bilinear=True, image=picture, alpha=0.5), "overlay")
    big = pipe.generate_image("a cat on the grass", ["cat", "grass", "sky"], heatmap_renderer="device",
                              heatmap_size=(40, 56), **kw)
    _equals_restatement(big, _restated(raw, "plasma", H=40, W=56), "heatmap_size")
    for bad in (dict(heatmap_size=32), dict(heatmap_interpolation="bilinear"), dict(overlay_alpha=0.5),
                dict(heatmap_renderer="gpu"), dict(heatmap_renderer="device", heatmap_interpolation="cubic"),
                dict(heatmap_renderer="device", overlay_alpha=1.5),
                dict(heatmap_renderer="device", overlay_alpha=0.5, heatmap_size=64)):
        with pytest.raises(ValueError):
            pipe.generate_image("a cat on the grass", ["cat", "grass", "sky"], **bad, **kw)


def test_encode_image_device_pictures_overlays_and_the_size_mismatch(pipe):
    img = _pil(1)
    kw = dict(prompt="a cat", noise=[_randn(*LAT, seed=6)], vae_noise=_randn(*LAT, seed=5), **ENC)
    host = pipe.encode_image(img, ["cat", "grass"], **kw)
    dev = pipe.encode_image(img, ["cat", "grass"], heatmap_renderer="device", **kw)
    _same_pictures(host, dev, "encode_image")
    raw = pipe.encode_image(img, ["cat", "grass"], return_pil_heatmaps=False, **kw)
    over = pipe.encode_image(img, ["cat", "grass"], heatmap_renderer="device", overlay_alpha=0.3, **kw)
    _equals_restatement(over, _restated(raw, "plasma", H=SIDE, W=SIDE, image=np.asarray(img), alpha=0.3), "overlay")
    with pytest.raises(ValueError, match="200 x 300.*256 x 256"):
        pipe.encode_image(_pil(2, (200, 300)), ["cat", "grass"], heatmap_renderer="device", overlay_alpha=0.3, **kw)
    with pytest.raises(ValueError, match="latent"):
        pipe.encode_image(_randn(*LAT, seed=7), ["cat", "grass"], heatmap_renderer="device", overlay_alpha=0.3,
                          prompt="a cat", noise=kw["noise"], **ENC)
    unchanged = pipe.encode_image(img, ["cat", "grass"], heatmap_renderer="device", return_pil_heatmaps=False, **kw)
    assert np.array_equal(unchanged.concept_heatmaps, raw.concept_heatmaps)


def test_the_batched_calls_render_chunk_by_chunk_with_the_hosts_bytes(pipe, monkeypatch):
    from conceptattention_amd import ops
    concepts = [["cat", "grass"], ["cat", "grass", "sky"], ["dog", "snow"]]        # two concept counts: two chunks
    prompts = ["a cat on the grass", "a dog in the snow", "a bird in the sky"]
    latents = [_randn(*LAT, seed=50 + i) for i in range(3)]
    launches = []
    real = ops.heatmap_render

    def spy(groups, *a, **k):
        launches.append([tuple(g.shape) for g in groups])
        return real(groups, *a, **k)
    monkeypatch.setattr(ops, "heatmap_render", spy)
    host = pipe.generate_images(prompts, concepts, latents=latents, **GEN)
    assert launches == []
    dev = pipe.generate_images(prompts, concepts, latents=latents, heatmap_renderer="device", **GEN)
    assert launches == [[(2, MAP, MAP)] * 4, [(3, MAP, MAP)] * 2]                  # a group per item and space
    for i in range(3):
        assert np.array_equal(np.asarray(host[i].image), np.asarray(dev[i].image))
        _same_pictures(host[i], dev[i], ("generate_images", i))
    over = pipe.generate_images(prompts, concepts, latents=latents, heatmap_renderer="device", overlay_alpha=0.5,
                                heatmap_interpolation="bilinear", **GEN)
    raw = pipe.generate_images(prompts, concepts, latents=latents, return_pil_heatmaps=False, **GEN)
    for i in range(3):
        pic = np.asarray(raw[i].image)
        _equals_restatement(over[i], _restated(raw[i], "plasma", H=SIDE, W=SIDE, bilinear=True, image=pic, alpha=0.5),
                            ("generate_images overlay", i))
    images = [_pil(10 + i) for i in range(3)]
    ekw = dict(noise=[[_randn(*LAT, seed=60 + i)] for i in range(3)], vae_noise=[_randn(*LAT, seed=70 + i) for i in range(3)],
               **ENC)
    del launches[:]
    host = pipe.encode_images(images, concepts, prompts, **ekw)
    dev = pipe.encode_images(images, concepts, prompts, heatmap_renderer="device", **ekw)
    assert launches == [[(2, MAP, MAP)] * 4, [(3, MAP, MAP)] * 2]
    for i in range(3):
        _same_pictures(host[i], dev[i], ("encode_images", i))
    over = pipe.encode_images(images, concepts, prompts, heatmap_renderer="device", overlay_alpha=0.3, **ekw)
    raw = pipe.encode_images(images, concepts, prompts, return_pil_heatmaps=False, **ekw)
    for i in range(3):
        _equals_restatement(over[i], _restated(raw[i], "plasma", H=SIDE, W=SIDE, image=np.asarray(images[i]), alpha=0.3),
                            ("encode_images overlay", i))
    with pytest.raises(ValueError, match="64 x 64.*256 x 256"):
        pipe.encode_images([images[0], _pil(3, (64, 64))], concepts[:2], prompts[:2], heatmap_renderer="device",
                           overlay_alpha=0.3, **ENC)


def test_concept_attention_frames_on_a_sweep_table_under_both_range_rules(pipe):
    latent = _randn(*LAT, seed=80).to(DEV)
    table, _ = pipe.layer_noise_sweep(latent, ["cat", "grass", "sky"], "a cat", [0, 2, 3], num_steps=4,
                                      width=SIDE, height=SIDE)
    assert tuple(table.shape) == (3, 2, 3, MAP, MAP)
    host = table.cpu().numpy()
    lut = R.cmap_lut("inferno")
    for layer in (0, 1):
        view = table[:, layer].permute(1, 0, 2, 3)                # (concepts, frames, h, w): not copied
        assert view.data_ptr() == table[0, layer].data_ptr() and not view.is_contiguous()
        maps = np.ascontiguousarray(host[:, layer].transpose(1, 0, 2, 3))
        own = concept_attention_frames(view)
        assert own.dtype == torch.uint8 and own.is_cuda and tuple(own.shape) == (3, 3, MAP, MAP, 3)
        for c in range(3):
            assert np.array_equal(own[c].cpu().numpy(), R.render(maps[c], lut)[0]), (layer, c)
        shared = concept_attention_frames(view, per_concept=False, size=(24, 40), interpolation="bilinear")
        given = (maps.min(), maps.max())
        for c in range(3):
            ref = R.render(maps[c], lut, H=24, W=40, bilinear=True, given=given)[0]
            assert np.array_equal(shared[c].cpu().numpy(), ref), (layer, c)
    assert torch.equal(table.cpu(), torch.from_numpy(host))       # the table is only read
    with pytest.raises(ValueError):
        concept_attention_frames(table[0, 0])
    with pytest.raises(ValueError):
        concept_attention_frames(table[:, 0], interpolation="cubic")
