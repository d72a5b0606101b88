"""Concept re-query through the public calls, on the tiny geometry of tests/test_frontend_gpu.py (H = 256, 2 + 2 blocks,
256 x 256 pictures = 256 image tokens): keep_trace=True changes neither image nor latent, keeps only the asked steps, and
``pipe.requery`` gives the maps of a fresh call with the new words -- bit for bit, when that fresh call takes the tracing
routes (keep_trace=True: the captured layers' output-space logits from the fp32 image rows).  No tolerance in this file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conceptattention_amd import ConceptAttentionFluxPipeline, ops  # noqa: E402
from conceptattention_amd.params import tiny_params  # noqa: E402
from conceptattention_amd.pipeline import ImageTrace, trace_nbytes  # noqa: E402

DEV = "cuda:0"
SIDE = 256
T = 64
LAT = (1, 16, SIDE // 8, SIDE // 8)
GEN = dict(width=SIDE, height=SIDE, layer_indices=[0, 1], num_inference_steps=2, timesteps=[1])
ENC = dict(width=SIDE, height=SIDE, layer_indices=[0, 1], num_steps=2, noise_timestep=1)
RAW = dict(return_pil_heatmaps=False)
WORDS, OTHER = ["cat", "grass", "sky"], ["dog", "tree", "road", "cloud", "sun"]


def _pipe():
    return ConceptAttentionFluxPipeline("flux-schnell", device=DEV, weights="synthetic", params=tiny_params(),
                                        n_text_tokens=T, autoencoder="synthetic", text_encoder="synthetic-t5-clip")


@pytest.fixture(scope="module")
def pipe():
    return _pipe()


def _pil(i):
    import PIL.Image
    return PIL.Image.fromarray(np.random.default_rng(100 + i).integers(0, 256, size=(SIDE, SIDE, 3), dtype=np.uint8))


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _same_maps(a, b, what=""):
    for name in ("concept_heatmaps", "cross_attention_maps"):
        x, y = np.asarray(getattr(a, name)), np.asarray(getattr(b, name))
        assert x.shape == y.shape and np.array_equal(x, y), (what, name, float(np.abs(x - y).max()))


@pytest.fixture(scope="module")
def generated(pipe):
    kw = dict(latent=_randn(*LAT, seed=40), **GEN, **RAW)
    return kw, pipe.generate_image("a cat on the grass", WORDS, keep_trace=True, **kw)


# ------------------------------------------------------------------------------------ 7. generate_image
def test_generate_image_keep_trace_and_requery(pipe, generated):
    kw, traced = generated
    plain = pipe.generate_image("a cat on the grass", WORDS, **kw)
    assert plain.trace is None and isinstance(traced.trace, ImageTrace)
    assert np.array_equal(np.asarray(plain.image), np.asarray(traced.image))
    # the latent itself, from the device core with and without a trace
    txt, vec, con = pipe._embed_chunk(["a cat on the grass"], [WORDS], [0], 3)
    core = dict(layer_indices=[0, 1], num_inference_steps=2, timesteps=[1])
    x = kw["latent"].to(DEV, torch.bfloat16)
    lat0 = pipe.generate_on_device(x, txt, vec, con, **core)[0]
    lat1 = pipe.generate_on_device(x, txt, vec, con, traces={}, **core)[0]
    assert torch.equal(lat0, lat1)
    # only step 1 is traced, at the documented price
    tr = traced.trace
    assert tr.timesteps == [1] and tr.layer_indices == [0, 1] and tr.image is traced.image
    assert tr.nbytes == trace_nbytes(pipe.params, len(WORDS), T, 256, [0, 1], 1)
    assert tr.settings["call"] == "generate_image" and tr.settings["num_inference_steps"] == 2
    # a re-query with other words is the fresh call with them (same seed and settings, the tracing routes)
    rq = pipe.requery(tr, OTHER, **RAW)
    fresh = pipe.generate_image("a cat on the grass", OTHER, keep_trace=True, **kw)
    assert rq.image is tr.image and rq.token_heatmaps is None and rq.trace is None
    assert np.asarray(rq.concept_heatmaps).shape == (len(OTHER), 16, 16)
    _same_maps(rq, fresh, "requery vs fresh")
    _same_maps(pipe.requery(tr, WORDS, **RAW), traced, "requery with the traced words")
    # A subset of the layers.  A fresh call that captures layer 1 alone has another latent (README, "the latent and
    # layer_indices"), so the expectation is the maps of the TRACED image: the per-layer tables of the traced step, which
    # tests/test_requery_model_gpu.py::test_subset_of_the_traced_layers ties to the tables of a fresh tracing forward.
    from conceptattention_amd.flux_dit import HeatmapRequest
    con, con_ids = pipe.flux_generator.embed_concepts_many([OTHER])[0]
    tables = HeatmapRequest((0, 1), 0.0, None, None, per_layer_out=torch.zeros(2, len(OTHER), 256, device=DEV),
                            per_layer_cross=torch.zeros(2, len(OTHER), 256, device=DEV))
    pipe.model.requery([tr.steps[1]], con, con_ids, [tables])
    for li in (0, 1):
        one = pipe.requery(tr, OTHER, layer_indices=[li], **RAW)
        for name, table in (("concept_heatmaps", tables.per_layer_out), ("cross_attention_maps", tables.per_layer_cross)):
            assert np.array_equal(np.asarray(getattr(one, name)), table[li].view(-1, 16, 16).cpu().numpy()), (li, name)
    assert not torch.equal(tables.per_layer_out[0], tables.per_layer_out[1])
    _same_maps(pipe.requery(tr, OTHER, timesteps=[-1], **RAW), rq, "timesteps=[-1] is step 1 of 2")


# ------------------------------------------------------------------------------------ 8. the other calls
def test_encode_image_traces_every_noise_sample(pipe):
    kw = dict(prompt="a cat", noise=[_randn(*LAT, seed=6), _randn(*LAT, seed=8)], vae_noise=_randn(*LAT, seed=5),
              num_samples=2, **ENC, **RAW)
    img = _pil(1)
    plain = pipe.encode_image(img, WORDS, **kw)
    traced = pipe.encode_image(img, WORDS, keep_trace=True, **kw)
    assert plain.trace is None and traced.trace.timesteps == [0, 1] and traced.trace.image is img
    assert traced.trace.nbytes == trace_nbytes(pipe.params, len(WORDS), T, 256, [0, 1], 2)
    rq = pipe.requery(traced.trace, OTHER, **RAW)
    _same_maps(rq, pipe.encode_image(img, OTHER, keep_trace=True, **kw), "encode requery vs fresh")
    first = pipe.requery(traced.trace, OTHER, timesteps=[0], **RAW)
    _same_maps(first, pipe.encode_image(img, OTHER, keep_trace=True, **dict(kw, num_samples=1, noise=kw["noise"][:1])),
               "sample 0 alone")


def test_batched_calls_give_per_item_traces_requeried_as_a_list(pipe):
    prompts = ["a cat", "a dog in the snow", "a red car"]
    new = [["dog", "tree"], ["snow", "fur", "ice", "sky"], ["car", "road"]]     # two concept counts: two groups
    lats = [_randn(*LAT, seed=50 + i) for i in range(3)]
    gkw = dict(latents=lats, batch=2, **GEN, **RAW)
    traced = pipe.generate_images(prompts, WORDS, keep_trace=True, **gkw)
    assert all(isinstance(o.trace, ImageTrace) and o.trace.timesteps == [1] for o in traced)
    assert traced[0].trace.steps[1].qkv[0].data_ptr() == traced[1].trace.steps[1].qkv[0].data_ptr()   # one forward's storage
    assert traced[0].trace.steps[1].item == 0 and traced[1].trace.steps[1].item == 1 and traced[2].trace.steps[1].item == 0
    rq = pipe.requery([o.trace for o in traced], new, **RAW)
    fresh = pipe.generate_images(prompts, new, keep_trace=True, **gkw)
    assert len(rq) == 3
    for i in range(3):
        assert rq[i].image is traced[i].image and np.asarray(rq[i].concept_heatmaps).shape[0] == len(new[i])
        _same_maps(rq[i], fresh[i], f"generate_images item {i}")
    imgs = [_pil(i) for i in range(3)]
    ekw = dict(noise=[[_randn(*LAT, seed=60 + i)] for i in range(3)], vae_noise=[_randn(*LAT, seed=70 + i) for i in range(3)],
               batch=2, **ENC, **RAW)
    etr = pipe.encode_images(imgs, WORDS, prompts, keep_trace=True, **ekw)
    erq = pipe.requery([o.trace for o in etr], new, **RAW)
    efresh = pipe.encode_images(imgs, new, prompts, keep_trace=True, **ekw)
    for i in range(3):
        assert erq[i].image is imgs[i]
        _same_maps(erq[i], efresh[i], f"encode_images item {i}")


def test_device_pictures_of_a_requery_are_the_hosts(pipe, generated):
    tr = generated[1].trace
    host = pipe.requery(tr, OTHER)
    dev = pipe.requery(tr, OTHER, heatmap_renderer="device")
    for name in ("concept_heatmaps", "cross_attention_maps"):
        la, lb = getattr(host, name), getattr(dev, name)
        assert len(la) == len(lb) == len(OTHER)
        for x, y in zip(la, lb):
            assert x.size == y.size == (16, 16) and np.array_equal(np.asarray(x), np.asarray(y)), name
    over = pipe.requery(tr, OTHER, heatmap_renderer="device", overlay_alpha=0.5)
    assert over.concept_heatmaps[0].size == (SIDE, SIDE)


# ------------------------------------------------------------------------------------ 9. refusals
def test_every_refusal_names_its_setting_and_launches_nothing(pipe, generated):
    kw, traced = generated
    tr = traced.trace
    other = _pipe()                               # the same weights in another model object
    foreign = other.generate_image("a cat", WORDS, keep_trace=True, **kw).trace
    calls = []
    ops.set_gemm_hook(lambda arr, tile, launch: (calls.append("gemm"), launch()))
    ops.set_attn_hook(lambda arr, nh, launch: (calls.append("attn"), launch()))

    def refused(match, fn, exc=ValueError):
        with pytest.raises(exc, match=match):
            fn()
        assert calls == [], match
    gen = lambda **k: pipe.generate_image("a cat", WORDS, keep_trace=True, **dict(kw, **k))  # noqa: E731
    enc = lambda **k: pipe.encode_image(_pil(3), WORDS, prompt="a cat", keep_trace=True, **ENC, **k)  # noqa: E731
    m = pipe.model
    try:
        m.set_precision("fp8")
        refused("precision", gen)
        refused("precision", enc)
        refused("precision", lambda: pipe.requery(tr, OTHER))
        m.set_precision("bf16")
        m.capture_independent_image = True
        refused("capture_independent_image", gen)
        refused("capture_independent_image", enc)
        refused("capture_independent_image", lambda: pipe.requery(tr, OTHER))
        m.capture_independent_image = False
        refused("joint_attention_kwargs", lambda: enc(joint_attention_kwargs={"concept_cross_attention": False}))
        refused("fused", lambda: gen(fused=False))
        refused("layer_indices", lambda: pipe.requery(tr, OTHER, layer_indices=[0, 2]))
        refused("timesteps", lambda: pipe.requery(tr, OTHER, timesteps=[0]))
        refused("33 concepts", lambda: pipe.requery(tr, [f"w{i}" for i in range(33)], softmax=False,
                                                    attention_norm="sparsemax"))
        refused("another model", lambda: pipe.requery(foreign, OTHER))
        foreign.release()
        assert foreign.released and foreign.nbytes == 0
        refused("released", lambda: other.requery(foreign, OTHER))
    finally:
        m.set_precision("bf16")
        m.capture_independent_image = False
        ops.set_gemm_hook(None)
        ops.set_attn_hook(None)
