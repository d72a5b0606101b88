"""score_multiclass_images + DeviceMultiClassScores on the GPU against the host route on the same pipeline
(segment_multiclass + map_predictions_to_class_indices + nearest resize + MultiClassScores.update): every counter equal,
per image and in total.  The tiny pipeline of tests/test_seg_scoring_gpu.py: 256 x 256 -> 16 x 16 maps, synthetic 21-class
labels with a 255 border at 64 x 64 and 224 x 224, six images whose present-class lists have 1, 2 and 3 entries."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mseg_cases as T  # noqa: E402
from conceptattention_amd import ConceptAttentionFluxPipeline  # noqa: E402
from conceptattention_amd import segmentation as S  # noqa: E402
from conceptattention_amd.params import tiny_params  # noqa: E402

DEV = "cuda:0"
SIDE, N = 256, 6
SIZES = [(256, 256), (200, 300), (64, 64)]
NAMES = ["background", "aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable",
         "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"]
BACKGROUND = ["background", "floor", "grass", "tree", "sky"]
TARGETS = [["cat"], ["dog", "sheep"], ["cat", "dog", "bus"], ["person"], ["bus", "car"], ["bird", "boat", "cow"]]
KW = dict(width=SIDE, height=SIDE, layers=[0, 1], num_steps=2, noise_timestep=1, batch=5)
IGNORE = 255


@pytest.fixture(scope="module")
def pipe():
    return ConceptAttentionFluxPipeline("flux-schnell", device=DEV, weights="synthetic", params=tiny_params(),
                                        n_text_tokens=64, autoencoder="synthetic", text_encoder="synthetic-t5-clip")


def _labels(size):
    """Per image a coarse random map of the background and the image's present classes, a 255 frame around it."""
    out = []
    for i in range(N):
        g = torch.Generator().manual_seed(200 + i)
        ids = torch.tensor([0] + [NAMES.index(c) for c in TARGETS[i]] + [NAMES.index("train")])   # (train: never predicted)
        coarse = ids[torch.randint(0, len(ids), (7, 7), generator=g)]
        y = torch.nn.functional.interpolate(coarse[None, None].float(), size=(size, size))[0, 0].numpy().astype(np.uint8)
        t = max(1, size // 32)
        y[:t], y[-t:], y[:, :t], y[:, -t:] = 255, 255, 255, 255
        out.append(y)
    return out


@pytest.fixture(scope="module")
def data():
    import PIL.Image
    images = [PIL.Image.fromarray(np.random.default_rng(100 + i).integers(0, 256, size=(*SIZES[i % 3], 3), dtype=np.uint8))
              for i in range(N)]
    captions = [",".join(f"a {c}" for c in TARGETS[i]) for i in range(N)]
    return images, {64: _labels(64), 224: _labels(224)}, captions


@pytest.fixture(scope="module")
def host_route(pipe, data):
    """The host route, once: per image (argmax map, maps, class map at map resolution)."""
    images, _, captions = data
    seg = S.ConceptAttentionSegmentationModel(pipe)
    torch.manual_seed(7)       # the autoencoder draws its sampling noise from the device generator, one batch per forward
    out = seg.segment_multiclass(images, captions, BACKGROUND, TARGETS, **KW)
    assert len(out) == N
    res = []
    for i, (pred, maps, recon) in enumerate(out):
        assert recon is None and pred.dtype == torch.int64 and tuple(pred.shape) == (SIDE // 16, SIDE // 16)
        assert maps.dtype == torch.float32 and tuple(maps.shape) == (len(BACKGROUND) + len(TARGETS[i]), SIDE // 16, SIDE // 16)
        table = S.multiclass_table(BACKGROUND, TARGETS[i], NAMES)
        res.append((pred, maps, S.map_predictions_to_class_indices(pred, table)))
    return res


def _host_scores(host_route, labels, ignore):
    scores, per_item = S.MultiClassScores(len(NAMES)), []
    for (pred, maps, klass), y in zip(host_route, labels):
        up = torch.nn.functional.interpolate(klass[None, None].float(), size=y.shape, mode="nearest")[0, 0]
        per_item.append(scores.update(up, y, ignore_index=ignore))
    return scores, per_item


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


@pytest.mark.parametrize("size,ignore", [(64, IGNORE), (224, IGNORE), (64, None)])
def test_score_multiclass_images_equals_the_host_route_and_downloads_once(pipe, data, host_route, monkeypatch, size, ignore):
    images, labels, captions = data
    labels = labels[size]
    host, per_item = _host_scores(host_route, labels, ignore)
    seg = S.ConceptAttentionSegmentationModel(pipe)
    dev = S.DeviceMultiClassScores(len(NAMES), DEV, chunk=4)       # (6 items: the buffer grows once)
    count = _Downloads(monkeypatch)
    torch.manual_seed(7)
    out = seg.score_multiclass_images(images, captions, BACKGROUND, TARGETS, NAMES, labels, dev, ignore_index=ignore, **KW)
    assert out is None and (count.cpu, count.numpy) == (0, 0), "score_multiclass_images downloaded something"
    result = dev.result()
    assert count.cpu == 1 and count.numpy <= 1, (count.cpu, count.numpy)
    got = dev.to_host()
    rec = dev.records()
    dev.all_reduce()
    assert count.cpu == 1, "the rows were downloaded again"
    monkeypatch.undo()
    nc = len(NAMES)
    assert sorted(dev.ids) == list(range(N)) and rec.shape == (N, 2 + 2 * nc) and rec.dtype == np.int32
    assert len({len(t) for t in TARGETS}) == 3, "several chunks"
    for row, i in zip(rec, dev.ids):
        want = per_item[i]
        print(i, "correct, labelled", row[:2].tolist(), "host", want["correct"], want["labelled"])
        assert (int(row[0]), int(row[1])) == (want["correct"], want["labelled"]), i
        assert np.array_equal(row[2:2 + nc], want["inter"]) and np.array_equal(row[2 + nc:], want["union"]), i
    assert (got.n, got.correct, got.labelled) == (host.n, host.correct, host.labelled) and host.n == N
    assert np.array_equal(got.inter, host.inter) and np.array_equal(got.union, host.union)
    assert host.correct > 0 and host.labelled > host.correct, "the labels carry no signal"
    if ignore is None:
        assert host.labelled == N * size * size
    want = host.result()
    assert result["pixAcc"] == want["pixAcc"] and result["mIoU"] == want["mIoU"] and result["n"] == N
    assert np.array_equal(result["IoU"], want["IoU"], equal_nan=True)


def test_return_predictions_hands_out_the_host_routes_class_maps(pipe, data, host_route):
    images, labels, captions = data
    seg = S.ConceptAttentionSegmentationModel(pipe)
    dev = S.DeviceMultiClassScores(len(NAMES), DEV)
    torch.manual_seed(7)
    got = seg.score_multiclass_images(images, captions, BACKGROUND, TARGETS, NAMES, labels[64], dev, ignore_index=IGNORE,
                                      return_predictions=True, **KW)
    assert len(got) == N and dev.n == N
    for i in range(N):
        assert got[i].dtype == np.uint8 and got[i].shape == (SIDE // 16, SIDE // 16)
        assert np.array_equal(got[i].astype(np.int64), host_route[i][2].numpy()), i


def test_blur_and_scale_equal_the_restatement_on_the_downloaded_planes(pipe, data):
    images, labels, captions = data
    labels = labels[224]
    lat = (1, 16, SIDE // 8, SIDE // 8)
    vae_noise = [torch.randn(*lat, generator=torch.Generator().manual_seed(30 + i)) for i in range(N)]
    concepts = [BACKGROUND + t for t in TARGETS]
    before = pipe.encode_images(images, concepts, captions, width=SIDE, height=SIDE, layer_indices=[0, 1], num_steps=2,
                                noise_timestep=1, return_pil_heatmaps=False, vae_noise=vae_noise)
    seg = S.ConceptAttentionSegmentationModel(pipe)
    nc = len(NAMES)
    scales = [None if i % 2 else [0.0] + [1.0] * (len(concepts[i]) - 2) + [-2.5] for i in range(N)]
    for blur, scale_values in ((True, None), (False, scales), (True, scales)):
        dev = S.DeviceMultiClassScores(nc, DEV)
        got = seg.score_multiclass_images(images, captions, BACKGROUND, TARGETS, NAMES, labels, dev, ignore_index=IGNORE,
                                          apply_blur=blur, concept_scale_values=scale_values, return_predictions=True,
                                          vae_noise=vae_noise, **KW)
        rec = dev.records()
        assert sorted(dev.ids) == list(range(N))
        for row, i in zip(rec, dev.ids):
            sc = None if scale_values is None or scale_values[i] is None else np.asarray(scale_values[i], dtype=np.float32)
            ref = T.reference(before[i].concept_heatmaps, labels[i], S.multiclass_table(BACKGROUND, TARGETS[i], NAMES), nc,
                              IGNORE, sc, blur)
            assert np.array_equal(row, ref["counts"]), (blur, i)
            assert np.array_equal(got[i], ref["class"]), (blur, i)


def test_argument_errors_are_raised_before_any_forward(pipe, data, monkeypatch):
    images, labels, captions = data
    labels = labels[64]
    seg = S.ConceptAttentionSegmentationModel(pipe)
    dev = S.DeviceMultiClassScores(len(NAMES), DEV)

    def no_forward(*a, **k):
        raise AssertionError("a forward was started")
    monkeypatch.setattr(pipe, "_encode_chunks", no_forward)
    monkeypatch.setattr(pipe, "encode_images", no_forward)

    def score(images=images, captions=captions, targets=TARGETS, names=NAMES, labels=labels, scores=dev, **kw):
        return seg.score_multiclass_images(images, captions, BACKGROUND, targets, names, labels, scores, **{**KW, **kw})
    with pytest.raises(ValueError):
        score(targets=TARGETS[:5])
    with pytest.raises(ValueError):
        score(labels=labels[:5])
    with pytest.raises(ValueError):
        score(captions=captions[:3])
    with pytest.raises(ValueError):
        score(targets=None)
    with pytest.raises(ValueError, match="unicorn"):
        score(targets=TARGETS[:5] + [["cat", "unicorn"]])
    with pytest.raises(ValueError, match="labels"):
        score(labels=[y.astype(np.int64) for y in labels])
    with pytest.raises(ValueError, match="labels"):
        score(labels=labels[:5] + [labels[5][:40]])
    with pytest.raises(ValueError, match="16384"):
        score(width=2064, height=2064)
    with pytest.raises(ValueError):
        score(scores=S.DeviceMultiClassScores(5, DEV))
    with pytest.raises(ValueError):
        score(concept_scale_values=[[1.0]] * N)
    with pytest.raises(ValueError):
        score(target_space="value")
    with pytest.raises(TypeError, match="size"):
        score(size=64)
    with pytest.raises(ValueError):
        seg.segment_multiclass(images, captions, BACKGROUND, TARGETS[:2], **KW)
    with pytest.raises(TypeError):
        seg.segment_multiclass(images, captions, BACKGROUND, TARGETS, downscale_for_eval=True, **KW)
    assert dev.n == 0
