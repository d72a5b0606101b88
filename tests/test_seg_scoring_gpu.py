"""score_images + DeviceSegmentationScores on the GPU against the host route on the same pipeline (seg(...) +
prepare_for_scoring + SegmentationScores.update): integer counters equal, AP within 1e-12 (derived in tests/seg_cases.py).
Tiny DiT, the synthetic autoencoder and text encoders, 256 x 256 -> 16 x 16 maps, 224 x 224 labels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import seg_cases as T  # noqa: E402
from conceptattention_amd import ConceptAttentionFluxPipeline  # noqa: E402
from conceptattention_amd import segmentation as S  # noqa: E402
from conceptattention_amd.params import tiny_params  # noqa: E402

DEV = "cuda:0"
SIDE, SIZE, N = 256, 224, 6
SIZES = [(256, 256), (200, 300), (64, 64)]
CONCEPTS = ["cat", "grass", "sky"]
TARGETS = ["cat", "grass", "cat", "sky", "cat", "grass"]
KW = dict(width=SIDE, height=SIDE, layers=[0, 1], num_steps=2, noise_timestep=1, batch=5)
AP_TOL = 1e-12


@pytest.fixture(scope="module")
def pipe():
    return ConceptAttentionFluxPipeline("flux-schnell", device=DEV, weights="synthetic", params=tiny_params(),
                                        n_text_tokens=64, autoencoder="synthetic", text_encoder="synthetic-t5-clip")


@pytest.fixture(scope="module")
def data():
    import PIL.Image
    images = [PIL.Image.fromarray(np.random.default_rng(100 + i).integers(0, 256, size=(*SIZES[i % 3], 3), dtype=np.uint8))
              for i in range(N)]
    labels = []
    for i in range(N):
        g = torch.Generator().manual_seed(200 + i)
        labels.append((torch.nn.functional.interpolate(torch.rand(1, 1, 7, 7, generator=g), size=(SIZE, SIZE))[0, 0] > 0.5)
                      .numpy().astype(np.uint8))
    captions = [f"a cat on the grass, picture {i % 3}" for i in range(N)]
    return images, labels, captions


@pytest.fixture(scope="module")
def host_route(pipe, data):
    """Today's route, once: (masks, coefficients, per-item update results, the running SegmentationScores)."""
    images, labels, captions = data
    seg = S.ConceptAttentionSegmentationModel(pipe)
    torch.manual_seed(7)       # the autoencoder draws its sampling noise from the device generator, one batch per forward
    masks, coeffs, _ = seg(images, TARGETS, CONCEPTS, captions, **KW)
    scores, per_item = S.SegmentationScores(), []
    for m, c, y in zip(masks, coeffs, labels):
        cc, mm = S.prepare_for_scoring(c, m, size=SIZE)
        per_item.append(scores.update(mm, cc, y.astype(bool)))
    return masks, coeffs, per_item, scores


class _Downloads:
    """Counts Tensor.cpu on device tensors and Tensor.numpy while active."""

    def __init__(self, monkeypatch):
        self.cpu = self.numpy = 0
        real_cpu, real_numpy = torch.Tensor.cpu, torch.Tensor.numpy
        me = self

        def cpu(t, *a, **k):
            me.cpu += int(t.is_cuda)
            return real_cpu(t, *a, **k)

        def numpy(t, *a, **k):
            me.numpy += 1
            return real_numpy(t, *a, **k)
        monkeypatch.setattr(torch.Tensor, "cpu", cpu)
        monkeypatch.setattr(torch.Tensor, "numpy", numpy)


def test_score_images_equals_the_host_route_and_downloads_once(pipe, data, host_route, monkeypatch):
    images, labels, captions = data
    masks, coeffs, per_item, host = host_route
    for i, c in enumerate(coeffs):     # the mask-margin condition: the fp32 and the fp64 mean agree on every cell
        margin = T.mask_margin_ulps(np.asarray(c), T.mean_tree(np.asarray(c)))
        assert margin >= 4.0, (i, margin)
    seg = S.ConceptAttentionSegmentationModel(pipe)
    dev = S.DeviceSegmentationScores(DEV, chunk=4)       # (6 items: the buffer grows once)
    count = _Downloads(monkeypatch)
    torch.manual_seed(7)
    out = seg.score_images(images, TARGETS, CONCEPTS, captions, labels, dev, size=SIZE, **KW)
    assert out is None and (count.cpu, count.numpy) == (0, 0), "score_images downloaded something"
    result = dev.result()
    assert count.cpu == 1 and count.numpy <= 1, (count.cpu, count.numpy)
    got = dev.to_host()
    rec = dev.records()
    dev.all_reduce()
    assert count.cpu == 1, "the records were downloaded again"
    monkeypatch.undo()
    assert got.n == host.n == N and int(got.correct) == int(host.correct) and int(got.labelled) == int(host.labelled)
    assert [int(v) for v in got.inter] == [int(v) for v in host.inter]
    assert [int(v) for v in got.union] == [int(v) for v in host.union]
    for i in range(N):
        agree = int(rec[i]["n11"]) + int(rec[i]["n00"])
        assert 2 * agree == int(per_item[i]["correct"]) and [agree, agree] == [int(v) for v in per_item[i]["inter"]], i
        print(i, "ap", float(rec[i]["ap"]), "host", per_item[i]["ap"], "diff", abs(float(rec[i]["ap"]) - per_item[i]["ap"]))
        assert abs(float(rec[i]["ap"]) - per_item[i]["ap"]) <= AP_TOL, i
    want = host.result()
    for k in ("pixAcc", "mIoU", "mAP"):
        assert abs(result[k] - want[k]) <= AP_TOL, (k, result[k], want[k])
    assert result["n"] == N


def test_return_masks_hands_out_what_call_returns(pipe, data, host_route):
    images, labels, captions = data
    masks, coeffs, _, _ = host_route
    seg = S.ConceptAttentionSegmentationModel(pipe)
    dev = S.DeviceSegmentationScores(DEV)
    torch.manual_seed(7)
    got_m, got_c = seg.score_images(images, TARGETS, CONCEPTS, captions, labels, dev, size=SIZE, return_masks=True, **KW)
    assert len(got_m) == len(got_c) == N and dev.n == N
    for i in range(N):
        assert got_m[i].dtype == np.bool_ and got_m[i].shape == (SIDE // 16, SIDE // 16)
        assert np.array_equal(got_m[i], np.asarray(masks[i])), i
        assert np.array_equal(got_c[i], np.asarray(coeffs[i])), i


def test_encode_images_is_unchanged_around_a_score_images_call(pipe, data):
    images, labels, captions = data
    lat = (1, 16, SIDE // 8, SIDE // 8)
    vae_noise = [torch.randn(*lat, generator=torch.Generator().manual_seed(30 + i)) for i in range(N)]
    kw = dict(width=SIDE, height=SIDE, layer_indices=[0, 1], num_steps=2, noise_timestep=1, return_pil_heatmaps=False,
              vae_noise=vae_noise)
    before = pipe.encode_images(images, CONCEPTS, captions, **kw)
    seg = S.ConceptAttentionSegmentationModel(pipe)
    dev = S.DeviceSegmentationScores(DEV)
    seg.score_images(images, TARGETS, CONCEPTS, captions, labels, dev, size=SIZE, vae_noise=vae_noise, **KW)
    after = pipe.encode_images(images, CONCEPTS, captions, **kw)
    for a, b in zip(before, after):
        assert torch.equal(torch.from_numpy(a.concept_heatmaps), torch.from_numpy(b.concept_heatmaps))
        assert torch.equal(torch.from_numpy(a.cross_attention_maps), torch.from_numpy(b.cross_attention_maps))
    # and the scored planes are those maps: the records of the restatement on the downloaded maps
    rec = dev.records()
    for i in range(N):
        ref = T.reference(before[i].concept_heatmaps[CONCEPTS.index(TARGETS[i])], labels[i])
        assert [int(rec[i][k]) for k in ("n11", "n10", "n01", "n00", "thresholds")] == \
               [ref[k] for k in ("n11", "n10", "n01", "n00", "thresholds")], i
        assert abs(float(rec[i]["ap"]) - ref["ap"]) <= AP_TOL, i


def test_score_images_rejects_what_it_does_not_cover(pipe, data):
    images, labels, captions = data
    seg = S.ConceptAttentionSegmentationModel(pipe)
    dev = S.DeviceSegmentationScores(DEV)
    with pytest.raises(ValueError):
        seg.score_images(images, None, CONCEPTS, captions, labels, dev, size=SIZE, **KW)
    with pytest.raises(ValueError):
        seg.score_images(images, TARGETS, CONCEPTS, captions, [y[:100] for y in labels], dev, size=SIZE, **KW)
    assert dev.n == 0
