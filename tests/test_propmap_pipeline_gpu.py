"""propagate= through the public calls, on the tiny geometry (tiny_params, 256 x 256, 64 text tokens, the synthetic T5 +
CLIP text encoders behind the toy byte tokenizer): the spaces and their shapes, nothing else moves, batched calls item by
item against single calls on generate and on encode, device pictures against host pictures, the tensors as the scoring
kernel's input, and every refusal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conceptattention_amd import ConceptAttentionFluxPipeline  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from conceptattention_amd.params import tiny_params  # noqa: E402
from conceptattention_amd.segmentation import ConceptAttentionSegmentationModel  # noqa: E402

DEV = "cuda:0"
SIDE = 256
MAP = SIDE // 16
LAT = (1, 16, SIDE // 8, SIDE // 8)
GEN = dict(width=SIDE, height=SIDE, layer_indices=[0, 1], num_inference_steps=2)
ENC = dict(width=SIDE, height=SIDE, layer_indices=[0, 1], num_steps=2, noise_timestep=1)
CONCEPTS = ["cat", "grass", "sky"]
PROMPTS = ["a cat", "a cat on the grass", "sky over a cat"]
BOTH = ("output", "cross")


@pytest.fixture(scope="module")
def pipe():
    return ConceptAttentionFluxPipeline("flux-schnell", device=DEV, weights="synthetic", params=tiny_params(),
                                        n_text_tokens=64, text_encoder="synthetic-t5-clip")


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_generate_and_encode_return_the_spaces_and_nothing_else_moves(pipe, monkeypatch):
    prompt = PROMPTS[1]
    launches = []
    real = ops.propagate_maps
    monkeypatch.setattr(ops, "propagate_maps", lambda *a, **k: (launches.append(len(a[0])), real(*a, **k))[1])
    kw = dict(latent=_randn(*LAT, seed=40), token_maps=True, query_maps="concepts", head_maps="cross",
              return_pil_heatmaps=False, **GEN)
    plain = pipe.generate_image(prompt, CONCEPTS, **kw)
    assert launches == [] and plain.propagated_heatmaps is None      # without the keyword nothing is launched
    raw = pipe.generate_image(prompt, CONCEPTS, propagate=BOTH, propagate_steps=2, **kw)
    assert launches == [2] * 8                            # 2 steps x 2 captured layers x 2 propagation steps, both spaces
    p = raw.propagated_heatmaps
    assert set(p) == {"output", "cross"}
    for space, t in p.items():
        assert tuple(t.shape) == (len(CONCEPTS), MAP, MAP) and t.is_cuda and t.dtype == torch.float32 and float(t.min()) > 0
    # the latent, the image, the concept maps, the token, query and head maps keep their bits
    for name in ("image", "concept_heatmaps", "cross_attention_maps", "token_heatmaps", "word_heatmaps"):
        assert np.array_equal(getattr(plain, name), getattr(raw, name)), name
    assert torch.equal(plain.query_heatmaps["concepts"], raw.query_heatmaps["concepts"])
    assert torch.equal(plain.head_maps["cross"], raw.head_maps["cross"])
    assert torch.equal(plain.raw_heatmaps["cross"], raw.raw_heatmaps["cross"])
    # the softmax over the concepts survives a row-stochastic propagation: per patch the maps of a space sum as before
    for space, maps in (("output", raw.concept_heatmaps), ("cross", raw.cross_attention_maps)):
        assert np.allclose(p[space].sum(0).cpu().numpy(), np.asarray(maps).sum(0), rtol=1e-5, atol=0)
        assert not np.allclose(p[space].cpu().numpy(), np.asarray(maps), rtol=1e-3, atol=0)
    # one space alone has the bits it has beside the other; one step differs from two
    launches.clear()
    one = pipe.generate_image(prompt, CONCEPTS, latent=kw["latent"], propagate="cross", propagate_steps=2,
                              return_pil_heatmaps=False, **GEN)
    assert launches == [1] * 8 and set(one.propagated_heatmaps) == {"cross"}
    assert torch.equal(one.propagated_heatmaps["cross"], p["cross"])
    step1 = pipe.generate_image(prompt, CONCEPTS, latent=kw["latent"], propagate="cross", return_pil_heatmaps=False, **GEN)
    assert not torch.equal(step1.propagated_heatmaps["cross"], p["cross"])
    enc = pipe.encode_image(_randn(*LAT, seed=41), CONCEPTS, prompt=prompt, noise=[_randn(*LAT, seed=6)], propagate=BOTH,
                            return_pil_heatmaps=False, **ENC)
    assert set(enc.propagated_heatmaps) == {"output", "cross"}
    assert tuple(enc.propagated_heatmaps["output"].shape) == (len(CONCEPTS), MAP, MAP)


def test_batched_calls_give_every_item_the_bits_of_its_single_call(pipe):
    lats = [_randn(*LAT, seed=50 + i) for i in range(3)]
    kw = dict(return_pil_heatmaps=False, propagate=BOTH, propagate_steps=2, **GEN)
    many = pipe.generate_images(PROMPTS, CONCEPTS, latents=lats, batch=3, **kw)
    for i, o in enumerate(many):
        one = pipe.generate_image(PROMPTS[i], CONCEPTS, latent=lats[i], **kw)
        for space in BOTH:
            assert torch.equal(o.propagated_heatmaps[space], one.propagated_heatmaps[space]), (i, space)
        assert np.array_equal(o.concept_heatmaps, one.concept_heatmaps) and np.array_equal(o.image, one.image)
    noise = [[_randn(*LAT, seed=70 + i)] for i in range(3)]
    ekw = dict(return_pil_heatmaps=False, propagate=BOTH, **ENC)
    enc = pipe.encode_images(lats, CONCEPTS, PROMPTS, noise=noise, batch=3, **ekw)
    for i, o in enumerate(enc):
        one = pipe.encode_image(lats[i], CONCEPTS, prompt=PROMPTS[i], noise=noise[i], **ekw)
        for space in BOTH:
            assert torch.equal(o.propagated_heatmaps[space], one.propagated_heatmaps[space]), (i, space)
    assert not torch.equal(enc[0].propagated_heatmaps["output"], enc[1].propagated_heatmaps["output"])


def test_device_pictures_are_the_host_pictures_byte_for_byte(pipe):
    def same(a, b, what):
        for name in ("concept_heatmaps", "cross_attention_maps"):
            for k, (x, y) in enumerate(zip(getattr(a, name), getattr(b, name))):
                assert x.size == y.size and np.array_equal(np.asarray(x), np.asarray(y)), (what, name, k)
        assert set(a.propagated_heatmaps) == set(b.propagated_heatmaps) == set(BOTH)
        for space in BOTH:
            la, lb = a.propagated_heatmaps[space], b.propagated_heatmaps[space]
            assert len(la) == len(lb) == len(CONCEPTS), (what, space)
            for k, (x, y) in enumerate(zip(la, lb)):
                assert x.mode == "RGB" and x.size == y.size and np.array_equal(np.asarray(x), np.asarray(y)), (what, space, k)
    kw = dict(latent=_randn(*LAT, seed=40), propagate=BOTH, **GEN)
    host = pipe.generate_image(PROMPTS[1], CONCEPTS, **kw)
    assert host.propagated_heatmaps["output"][0].size == (MAP, MAP)
    same(host, pipe.generate_image(PROMPTS[1], CONCEPTS, heatmap_renderer="device", **kw), "generate_image")
    lats = [_randn(*LAT, seed=50 + i) for i in range(3)]
    noise = [[_randn(*LAT, seed=70 + i)] for i in range(3)]
    ekw = dict(noise=noise, batch=3, propagate=BOTH, **ENC)
    for i, (a, b) in enumerate(zip(pipe.encode_images(lats, CONCEPTS, PROMPTS, **ekw),
                                   pipe.encode_images(lats, CONCEPTS, PROMPTS, heatmap_renderer="device", **ekw))):
        same(a, b, f"encode_images[{i}]")
    big = pipe.generate_image(PROMPTS[0], CONCEPTS, heatmap_renderer="device", heatmap_size=40, **kw)
    assert all(p.size == (40, 40) for p in big.propagated_heatmaps["cross"])


def test_the_tensors_feed_the_scoring_kernel_unchanged(pipe):
    """ops.seg_score, the launch behind score_images, takes the (C, h, w) tensor as it is returned: fp32, contiguous, on
    the device; the records are those of a copy, and the propagated map scores differently from the plain one."""
    out = pipe.encode_image(_randn(*LAT, seed=41), CONCEPTS, prompt=PROMPTS[1], noise=[_randn(*LAT, seed=6)], propagate="output",
                            return_pil_heatmaps=False, **ENC)
    maps = out.propagated_heatmaps["output"]
    assert maps.dtype == torch.float32 and maps.is_contiguous() and maps.is_cuda
    g = torch.Generator().manual_seed(3)
    labels = [(torch.rand(224, 224, generator=g) > 0.5).to(torch.uint8).to(DEV) for _ in CONCEPTS]
    rec, rec_copy, rec_plain = (torch.zeros(len(CONCEPTS), ops.SEG_RECORD_BYTES, dtype=torch.uint8, device=DEV) for _ in range(3))
    ops.seg_score(maps, labels, rec)
    ops.seg_score(maps.clone(), labels, rec_copy)
    ops.seg_score(torch.as_tensor(np.asarray(out.concept_heatmaps), device=DEV).float().contiguous(), labels, rec_plain)
    torch.cuda.synchronize()
    assert torch.equal(rec, rec_copy) and bool(rec.any()) and not torch.equal(rec, rec_plain)


def test_every_refusal_fires_before_a_launch(pipe, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a launch after a refusal was due")
    lat = _randn(*LAT, seed=40)
    kw = dict(latent=lat, **GEN)
    monkeypatch.setattr(ops, "gemm", no_launch)
    monkeypatch.setattr(ops, "propagate_maps", no_launch)
    for bad in ("value", "words", ("output", "output"), ()):      # a space whose concept maps the call does not compute
        with pytest.raises(ValueError, match="propagate = "):
            pipe.generate_image("a cat", CONCEPTS, propagate=bad, **kw)
        with pytest.raises(ValueError, match="propagate = "):
            pipe.encode_images([lat], CONCEPTS, ["a cat"], propagate=bad, **ENC)
    for steps in (0, 5, 1.5, True):
        with pytest.raises(ValueError, match="propagate_steps = "):
            pipe.generate_image("a cat", CONCEPTS, propagate="output", propagate_steps=steps, **kw)
        with pytest.raises(ValueError, match="propagate_steps = "):
            pipe.encode_image(lat, CONCEPTS, prompt="a cat", propagate="output", propagate_steps=steps, **ENC)
    with pytest.raises(ValueError, match="propagate: 0 concepts"):
        pipe.generate_image("a cat", [], propagate="output", **kw)
    with pytest.raises(ValueError, match="propagate: 0 concepts"):
        pipe.encode_image(lat, [], prompt="a cat", propagate="cross", **ENC)
    with pytest.raises(ValueError, match="fused"):
        pipe.generate_image("a cat", CONCEPTS, propagate="output", fused=False, **kw)
    with pytest.raises(ValueError, match="fused"):          # repeated timesteps / layers fall back to the stacked route
        pipe.generate_image("a cat", CONCEPTS, propagate="output", timesteps=[0, 0], **kw)
    with pytest.raises(ValueError, match="fused"):
        pipe.generate_images(["a cat"], CONCEPTS, latents=[lat], propagate="output", width=SIDE, height=SIDE,
                             layer_indices=[1, 1], num_inference_steps=2)
    with pytest.raises(ValueError, match="layer_noise_sweep: propagated maps"):
        pipe.layer_noise_sweep(lat, CONCEPTS, "a cat", [1], num_steps=2, layer_indices=[0, 1], width=SIDE, height=SIDE,
                               propagate="output")
    with pytest.raises(ValueError, match="score_sweep: propagated maps"):
        ConceptAttentionSegmentationModel(pipe).score_sweep([lat], ["cat"], CONCEPTS, ["a cat"], [np.zeros((224, 224), np.uint8)],
                                                            None, [1], propagate="output")
    monkeypatch.undo()
    traced = pipe.generate_image("a cat", CONCEPTS, keep_trace=True, **kw)
    monkeypatch.setattr(ops, "gemm", no_launch)
    with pytest.raises(ValueError, match="requery: propagated maps"):
        pipe.requery(traced.trace, ["dog"], propagate="output")
    monkeypatch.undo()
    # the model's own refusal: a re-query request that carries propagated maps
    from conceptattention_amd.flux_dit import HeatmapRequest
    step = traced.trace.steps[traced.trace.timesteps[0]]
    z = torch.zeros(1, step.L, device=DEV)
    emb = pipe.flux_generator.embed_concepts_many([["dog"]])
    with pytest.raises(ValueError, match="requery: propagated maps"):
        pipe.model.requery([step], emb[0][0], emb[0][1], [HeatmapRequest(tuple(traced.trace.layer_indices), 1.0, z, z.clone(),
                                                                        prop_out=z.clone())])


def test_fp8_is_served(pipe):
    """precision="fp8" quantises GEMM operands; the rotated q / k rows in QKV stay bf16 (or half) rows, which is all the
    propagation reads: the route serves it, and the concept maps keep the bits they have without the keyword."""
    kw = dict(latent=_randn(*LAT, seed=40), return_pil_heatmaps=False, **GEN)
    pipe.model.set_precision("fp8")
    try:
        plain = pipe.generate_image("a cat", CONCEPTS, **kw)
        out = pipe.generate_image("a cat", CONCEPTS, propagate="output", **kw)
    finally:
        pipe.model.set_precision("bf16")
    assert float(out.propagated_heatmaps["output"].min()) > 0
    assert np.array_equal(plain.concept_heatmaps, out.concept_heatmaps) and np.array_equal(plain.image, out.image)
