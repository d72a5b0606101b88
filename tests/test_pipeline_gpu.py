"""Pipeline-level behaviour on the GPU: public API surface, fused vs stacked heat maps, encode path,
the reference's heat-map known answers through the HIP reduction."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conceptattention_amd import ConceptAttentionFluxPipeline  # noqa: E402
from conceptattention_amd.heatmaps import compute_heatmaps_from_vectors  # noqa: E402
from conceptattention_amd.params import tiny_params  # noqa: E402
from oracle import flux_oracle as O  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def pipe():
    return ConceptAttentionFluxPipeline("flux-schnell", device=DEV, weights="synthetic", params=tiny_params(),
                                        n_text_tokens=8)


def test_generate_image_api_and_fused_equals_stacked(pipe):
    concepts = ["cat", "grass", "sky"]
    kw = dict(prompt="A cat in a park", concepts=concepts, width=256, height=256, layer_indices=[0, 1],
              num_inference_steps=2, seed=3, return_pil_heatmaps=False)
    a = pipe.generate_image(**kw)
    b = pipe.generate_image(fused=False, **kw)
    assert a.concept_heatmaps.shape == (3, 16, 16) and a.cross_attention_maps.shape == (3, 16, 16)
    assert a.image.shape == (16, 32, 32)  # no autoencoder injected: the unpacked latent
    assert np.abs(a.concept_heatmaps.sum(0) - 1).max() < 1e-5
    # same kernels, same order of operations except what the fused path keeps in fp32 and the stacked dict carries in
    # the activations' dtype (bf16, as the reference's dict): the concept rows' attention output (output space) and
    # the pre-RoPE q vectors of both sides (cross space)
    assert np.abs(a.concept_heatmaps - b.concept_heatmaps).max() < 2e-3
    assert np.abs(a.cross_attention_maps - b.cross_attention_maps).max() < 2e-3
    assert np.array_equal(a.image, b.image)
    c = pipe.generate_image(**{**kw, "return_pil_heatmaps": True})
    assert len(c.concept_heatmaps) == 3 and c.concept_heatmaps[0].size == (16, 16)
    # determinism: same seed -> identical maps
    a2 = pipe.generate_image(**kw)
    assert np.array_equal(a.concept_heatmaps, a2.concept_heatmaps)
    # repeated timestep indices (fancy-index semantics of the reference) route through the stacked path
    d = pipe.generate_image(**{**kw, "timesteps": [1, 1]})
    e = pipe.generate_image(**{**kw, "timesteps": [1]})
    assert np.abs(d.concept_heatmaps - e.concept_heatmaps).max() < 2e-3


def test_flux_generator_contract(pipe):
    """FluxGenerator.generate_image returns (image, dict) with the reference's four keys stacked over
    [steps, double blocks, batch, ...] (image_generator.py:87-205, sampling.py:149-150); feeding that dict
    to compute_heatmaps_from_vectors reproduces the pipeline's stacked-path maps."""
    gen = pipe.flux_generator
    lat = torch.randn(1, 16, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV, torch.bfloat16)
    img, d = gen.generate_image(width=256, height=256, num_steps=2, guidance=0.0, seed=0, prompt="a cat",
                                concepts=["cat", "sky"], latent=lat)
    nb = pipe.params.depth
    assert d["output_space_image_vectors"].shape == (2, nb, 1, 256, 256)
    assert d["output_space_concept_vectors"].shape == (2, nb, 1, 2, 256)
    assert d["cross_attention_image_vectors"].shape == (2, nb, 1, 2, 256, 128)
    assert d["cross_attention_concept_vectors"].shape == (2, nb, 1, 2, 2, 128)
    assert img.shape == (16, 32, 32)
    hm = compute_heatmaps_from_vectors(d["output_space_image_vectors"], d["output_space_concept_vectors"],
                                       layer_indices=[0, 1], timesteps=[0, 1])
    out = pipe.generate_image("a cat", ["cat", "sky"], width=256, height=256, layer_indices=[0, 1],
                              num_inference_steps=2, latent=lat, fused=False, return_pil_heatmaps=False)
    assert np.abs(hm[0].cpu().numpy() - out.concept_heatmaps).max() < 1e-6


def test_two_streams_equal_sequential(pipe):
    """Throughput mode (independent items on separate HIP streams, shared weights) is bit-identical
    to running the items one after the other."""
    from conceptattention_amd.weights import synthetic_inputs
    items = []
    for j in range(3):
        inp = synthetic_inputs(pipe.params, 256, 256, 8, 3, seed=50 + j, dtype=torch.bfloat16)
        items.append({k: inp[k].to(DEV) for k in ("latent", "txt", "vec", "concepts")})
    kw = dict(layer_indices=[0, 1], num_inference_steps=2)
    seq = [pipe.generate_on_device(i["latent"], i["txt"], i["vec"], i["concepts"], **kw) for i in items]
    par = pipe.generate_many_on_device(items, n_streams=2, **kw)
    torch.cuda.synchronize()
    for a, b in zip(seq, par):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_two_streams_share_the_first_models_settings(pipe):
    """A setting changed on pipe.model holds on every stream: with bf16 q / k everywhere (qk_f16 = "0", which only acts
    in layers whose maps are requested) two streams give the bits of one stream."""
    from conceptattention_amd.weights import synthetic_inputs
    items = []
    for j in range(3):
        inp = synthetic_inputs(pipe.params, 256, 256, 8, 3, seed=50 + j, dtype=torch.bfloat16)
        items.append({k: inp[k].to(DEV) for k in ("latent", "txt", "vec", "concepts")})
    kw = dict(layer_indices=[0, 1], num_inference_steps=2)
    before = pipe.model.qk_f16
    pipe.model.qk_f16 = "0"
    try:
        one = pipe.generate_many_on_device(items, n_streams=1, **kw)
        two = pipe.generate_many_on_device(items, n_streams=2, **kw)
        torch.cuda.synchronize()
    finally:
        pipe.model.qk_f16 = before
    for a, b in zip(one, two):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_generate_image_argument_checks(pipe):
    with pytest.raises(AssertionError):
        pipe.generate_image("p", ["a"], width=256, height=128)
    with pytest.raises(AssertionError):
        pipe.generate_image("p", ["a"], width=256, height=256, layer_indices=[7])
    with pytest.raises(AssertionError):
        pipe.generate_image("p", ["a"], width=256, height=256, return_cross_attention=True)
    with pytest.raises(ValueError):  # concept_attention_pipeline.py:70-71
        pipe.generate_image("p", ["a"], width=256, height=256, layer_indices=[0], softmax=False,
                            attention_norm="unknown")


def test_encode_image_runs_double_blocks_only(pipe):
    latent = torch.randn(1, 16, 32, 32, generator=torch.Generator().manual_seed(0))
    out = pipe.encode_image(latent, ["dragon", "rock"], prompt="A dragon", width=256, height=256,
                            layer_indices=[0, 1], num_samples=2, return_pil_heatmaps=False)
    assert out.concept_heatmaps.shape == (2, 16, 16)
    assert np.abs(out.concept_heatmaps.sum(0) - 1).max() < 1e-5
    with pytest.raises(ValueError):
        pipe.encode_image(object(), ["x"], width=256, height=256, layer_indices=[0])


def test_layer_noise_sweep_matches_oracle(pipe):
    """Per-(noise level, layer) tables: every entry equals the oracle's map for that single forward, and
    sharding the levels over 2 'ranks' then summing reproduces the unsharded table."""
    from conceptattention_amd import sampling
    from conceptattention_amd.weights import synthetic_inputs
    p = pipe.params
    inp = synthetic_inputs(p, 256, 256, 8, 3, seed=9, dtype=torch.bfloat16)
    x = {k: inp[k].to(DEV) for k in ("latent", "txt", "vec", "concepts")}
    levels = [1, 3]
    out, cross = pipe.layer_noise_sweep_on_device(x["latent"], x["txt"], x["vec"], x["concepts"], levels,
                                                  num_steps=4, seed=5)
    assert out.shape == (2, p.depth, 3, 16, 16)
    parts = [pipe.layer_noise_sweep_on_device(x["latent"], x["txt"], x["vec"], x["concepts"], levels, num_steps=4,
                                              seed=5, rank=r, world=2)[0] for r in range(2)]
    assert torch.equal(parts[0] + parts[1], out)
    # several levels per forward (each level = one work item with its own timestep): bit-identical per level
    lv3 = [0, 1, 3, 2]
    one = pipe.layer_noise_sweep_on_device(x["latent"], x["txt"], x["vec"], x["concepts"], lv3, num_steps=4, seed=5)
    many = pipe.layer_noise_sweep_on_device(x["latent"], x["txt"], x["vec"], x["concepts"], lv3, num_steps=4, seed=5,
                                            batch=3)
    assert torch.equal(one[0], many[0]) and torch.equal(one[1], many[1])
    assert torch.equal(one[0][1], out[0]) and torch.equal(one[0][2], out[1])
    # oracle for level index 1 (schedule[3]) with the same noise tensor
    sd = {k: v.float().cpu() for k, v in pipe.model.state_dict().items()}
    sched = sampling.get_schedule(4, 256, shift=False)
    t = sched[3]
    noise = sampling.get_noise(1, 256, 256, torch.device(DEV), torch.bfloat16, 5)
    xn = (t * noise.float() + (1.0 - t) * x["latent"].float()).to(torch.bfloat16).float().cpu()
    f = {k: v.float().cpu() for k, v in inp.items() if v.is_floating_point()}
    _, d = O.dit_forward(sd, p, O.patchify(xn), inp["img_ids"], f["txt"], inp["txt_ids"], f["concepts"],
                         inp["concept_ids"], f["concept_vec"], torch.tensor([t]), f["concept_vec"],
                         stop_after_multimodal_attentions=True)
    for layer in range(p.depth):
        st = {k: v[None] for k, v in d.items()}
        ref = O.compute_heatmaps(st["output_space_image_vectors"], st["output_space_concept_vectors"], [layer], [0])
        assert (out[1, layer].cpu() - ref[0]).abs().max() < 3e-3, layer


def test_heatmap_known_answers_through_hip(golden):
    g = golden("heatmap_kat.npz")
    iv = torch.from_numpy(g["iv"]).float().bfloat16()
    cv = torch.from_numpy(g["cv"]).float().bfloat16()
    ref = O.compute_heatmaps(iv.float(), cv.float(), [1, 3, 4], [0, 2])  # oracle on the bf16-rounded inputs
    out = compute_heatmaps_from_vectors(iv.to(DEV), cv.to(DEV), layer_indices=[1, 3, 4], timesteps=[0, 2])
    assert out.shape == (1, 4, 64, 64)
    assert (out.cpu() - ref).abs().max() < 1e-5
    # and within bf16 input rounding of the reference's own fp32 answer
    assert (out.cpu() - torch.from_numpy(g["out_a"])).abs().max() < 2e-2
    iv6 = torch.from_numpy(g["iv6"]).float().bfloat16()
    cv6 = torch.from_numpy(g["cv6"]).float().bfloat16()
    ref6 = O.compute_heatmaps(iv6.float(), cv6.float(), [0, 1], [0, 1])
    out6 = compute_heatmaps_from_vectors(iv6.to(DEV), cv6.to(DEV), layer_indices=[0, 1], timesteps=[0, 1])
    assert (out6.cpu() - ref6).abs().max() < 1e-5
    refn = O.compute_heatmaps(iv.float(), cv.float(), [2], [1], normalize_concepts=True)
    outn = compute_heatmaps_from_vectors(iv.to(DEV), cv.to(DEV), layer_indices=[2], timesteps=[1],
                                         normalize_concepts=True)
    assert (outn.cpu() - refn).abs().max() < 5e-3  # normalised concepts are re-rounded to bf16


def test_segmentation_model_contract(pipe):
    """The segmentation wrapper (concept_attention/segmentation.py:34-81): target-concept masks are the
    mean-thresholded heat map of encode_image; the ablation kwargs reach the blocks."""
    from conceptattention_amd.segmentation import ConceptAttentionSegmentationModel, SegmentationScores, \
        prepare_for_scoring
    seg = ConceptAttentionSegmentationModel(pipe)
    latent = torch.randn(1, 16, 32, 32, generator=torch.Generator().manual_seed(0))
    concepts = ["dragon", "rock", "sky"]
    kw = dict(width=256, height=256, layers=[0, 1], num_samples=1, seed=3)
    masks, coeffs, recon = seg([latent, latent], target_concepts=["rock", "dragon"], concepts=concepts,
                               captions=["a rock", "a dragon"], **kw)
    assert len(masks) == 2 and masks[0].shape == (16, 16) and masks[0].dtype == np.bool_ and recon == [None, None]
    ref = pipe.encode_image(latent, concepts, prompt="a rock", width=256, height=256, layer_indices=[0, 1],
                            seed=3, return_pil_heatmaps=False).concept_heatmaps
    assert np.array_equal(coeffs[0], np.asarray(ref)[1])
    assert np.array_equal(masks[0], coeffs[0] > coeffs[0].mean())
    all_masks, all_coeffs, _ = seg(latent, target_concepts=None, concepts=concepts, captions=["a rock"], **kw)
    assert all_masks[0].shape == (3, 16, 16) and all_masks[0].dtype == torch.bool
    _, abl, _ = seg(latent, target_concepts=["rock"], concepts=concepts, captions=["a rock"],
                    joint_attention_kwargs={"concept_cross_attention": True, "concept_self_attention": False}, **kw)
    assert not np.array_equal(abl[0], coeffs[0])
    sc = SegmentationScores()
    c, m = prepare_for_scoring(coeffs[0], masks[0], size=32)
    sc.update(m, c, m.bool().numpy())                   # a mask scored against itself: every pixel correct
    r = sc.result()
    assert r["pixAcc"] == pytest.approx(1.0) and r["mIoU"] == pytest.approx(1.0) and 0.5 < r["mAP"] <= 1.0


@pytest.mark.parametrize("size,n_txt,C", [(208, 5, 1), (400, 11, 6)])
def test_odd_sizes_end_to_end_vs_oracle(size, n_txt, C):
    """Ragged everything at once: 13x13 / 25x25 image tokens (no multiple of the 64-key attention tile or the 256-row
    GEMM tile), odd text lengths, 1 and 6 concepts (6 = two passes of the 4-concept logits kernel); two
    diffusion steps through the fused pipeline against the fp32 oracle."""
    from conceptattention_amd.weights import synthetic_inputs, synthetic_state_dict
    p = tiny_params()
    sd = {k: v.bfloat16().float() for k, v in synthetic_state_dict(p, seed=4).items()}
    inp = {k: (v.bfloat16().float() if v.is_floating_point() else v)
           for k, v in synthetic_inputs(p, size, size, n_txt=n_txt, n_concepts=C, seed=6).items()}
    pl = ConceptAttentionFluxPipeline("flux-schnell", device=DEV, weights=sd, params=p, n_text_tokens=n_txt)
    img, hm, cm = pl.generate_on_device(inp["latent"].to(DEV), inp["txt"].to(DEV), inp["vec"].to(DEV),
                                        inp["concepts"].to(DEV), layer_indices=[0, 1], num_inference_steps=2)
    side = size // 16
    assert hm.shape == (1, C, side, side)
    ts = O.get_schedule(2, side * side, shift=False)
    img_o, d = O.denoise(sd, p, O.patchify(inp["latent"]), inp["img_ids"], inp["txt"], inp["txt_ids"], inp["vec"],
                         ts, 0.0, inp["concepts"], inp["concept_ids"], inp["concept_vec"])
    hm_o = O.compute_heatmaps(d["output_space_image_vectors"], d["output_space_concept_vectors"], [0, 1], [0, 1])
    cm_o = O.compute_heatmaps(d["cross_attention_image_vectors"], d["cross_attention_concept_vectors"], [0, 1], [0, 1])
    assert (img.float().cpu() - img_o).abs().max() < 0.1
    assert (hm.cpu() - hm_o).abs().max() < 5e-3     # two steps, not teacher-forced (smoke() uses the same bound)
    assert (cm.cpu() - cm_o).abs().max() < 2e-2


def test_reference_shaped_bf16_latent_loop_stays_exercised():
    """HipFluxDiT.fp32_latent = False: the Euler state is a bf16 tensor re-rounded after every step
    and the prediction is bf16 -- the reference's own loop, flux/sampling.py:141 -- next to the default fp32 state.  Both
    against the fp32 oracle; the default is at least as close, and the two latents differ by about 2^-9 per step, which
    is what a caller comparing returned latents with a bf16 reference run will see."""
    from conceptattention_amd.weights import synthetic_inputs, synthetic_state_dict
    p = tiny_params()
    sd = {k: v.bfloat16().float() for k, v in synthetic_state_dict(p, seed=4).items()}
    inp = {k: (v.bfloat16().float() if v.is_floating_point() else v)
           for k, v in synthetic_inputs(p, 256, 256, n_txt=8, n_concepts=3, seed=6).items()}
    pl = ConceptAttentionFluxPipeline("flux-schnell", device=DEV, weights=sd, params=p, n_text_tokens=8)
    args = (inp["latent"].to(DEV), inp["txt"].to(DEV), inp["vec"].to(DEV), inp["concepts"].to(DEV))
    kw = dict(layer_indices=[0, 1], num_inference_steps=4)
    default = pl.model.fp32_latent                     # True
    pl.model.fp32_latent = True
    img32, hm32, _ = pl.generate_on_device(*args, **kw)
    pl.model.fp32_latent = False
    try:
        img16, hm16, _ = pl.generate_on_device(*args, **kw)
    finally:
        pl.model.fp32_latent = default
    assert img32.dtype == torch.bfloat16 and img16.dtype == torch.bfloat16      # what generate returns is bf16 either way
    ts = O.get_schedule(4, 256, shift=False)
    img_o, d = O.denoise(sd, p, O.patchify(inp["latent"]), inp["img_ids"], inp["txt"], inp["txt_ids"], inp["vec"],
                         ts, 0.0, inp["concepts"], inp["concept_ids"], inp["concept_vec"])
    hm_o = O.compute_heatmaps(d["output_space_image_vectors"], d["output_space_concept_vectors"], [0, 1], list(range(4)))
    e32 = (img32.float().cpu() - img_o).pow(2).mean().sqrt().item()
    e16 = (img16.float().cpu() - img_o).pow(2).mean().sqrt().item()
    scale = img_o.pow(2).mean().sqrt().item()
    assert e16 < 0.02 * scale and e32 <= e16 * 1.05, (e32, e16, scale)
    assert (hm16.cpu() - hm_o).abs().max() < 5e-3 and (hm32.cpu() - hm_o).abs().max() < 5e-3
    diff = (img32.float() - img16.float()).abs().max().item()
    assert 0 < diff < 8 * 2.0 ** -9 * img_o.abs().max().item(), diff


def test_encode_many_equals_one_by_one(pipe):
    """Image batches on two streams (configs[3] shape of work) give the maps of encode_image item by item."""
    from conceptattention_amd.weights import synthetic_inputs
    p = pipe.params
    items = []
    for j in range(3):
        inp = synthetic_inputs(p, 256, 256, 8, 2, seed=20 + j, dtype=torch.bfloat16)
        items.append({k: inp[k].to(DEV) for k in ("latent", "txt", "vec", "concepts")})
    kw = dict(layer_indices=[0, 1], num_samples=2, num_steps=4, noise_timestep=2, seed=5)
    many = pipe.encode_many_on_device(items, n_streams=2, **kw)
    batched = pipe.encode_many_on_device(items, n_streams=1, batch=3, **kw)   # three images through every launch
    assert len(many) == 3 and many[0][0].shape == (1, 2, 16, 16)
    for it, (hm, cm), (hb, cb) in zip(items, many, batched):
        one = pipe.encode_many_on_device([it], n_streams=1, **kw)[0]
        assert torch.equal(hm, one[0]) and torch.equal(cm, one[1])
        assert torch.equal(hb, one[0]) and torch.equal(cb, one[1])
        assert (hm.sum(1) - 1).abs().max() < 1e-5
