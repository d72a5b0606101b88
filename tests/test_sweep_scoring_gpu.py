"""score_sweep + DeviceSweepScores on the GPU against the tables of layer_noise_sweep under the same seeds and autoencoder
noise, downloaded and scored map by map with the numpy restatement (tests/segtab_cases.py): every counter of every (space,
level, column) equal, the AP within 1e-12 per map (derived in tests/seg_cases.py).  Both sides score the same downloaded
bits, so no threshold-margin condition enters.  Tiny DiT, the synthetic autoencoder and text encoders, 256 x 256 ->
16 x 16 maps, 224 x 224 labels, 3 images, 3 concepts, noise levels [0, 1, 3] of 4 steps, all double blocks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import seg_cases as SC  # noqa: E402
import segtab_cases as T  # noqa: E402
from conceptattention_amd import ConceptAttentionFluxPipeline  # noqa: E402
from conceptattention_amd import segmentation as S  # noqa: E402
from conceptattention_amd.params import tiny_params  # noqa: E402

DEV = "cuda:0"
SIDE, SIZE, N = 256, 224, 3
SIZES = [(256, 256), (200, 300), (64, 64)]
CONCEPTS = ["cat", "grass", "sky"]
TARGETS = ["cat", "grass", "sky"]
LEVELS = [0, 1, 3]
KW = dict(num_steps=4, width=SIDE, height=SIDE, seed=11, batch=2)
AP_TOL = 1e-12


class _Downloads:
    """Counts Tensor.cpu on device tensors and Tensor.numpy while active (the counter of test_seg_scoring_gpu.py)."""

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


@pytest.fixture(scope="module")
def pipe():
    return ConceptAttentionFluxPipeline("flux-schnell", device=DEV, weights="synthetic", params=tiny_params(),
                                        n_text_tokens=64, autoencoder="synthetic", text_encoder="synthetic-t5-clip")


@pytest.fixture(scope="module")
def data():
    import PIL.Image
    images = [PIL.Image.fromarray(np.random.default_rng(300 + i).integers(0, 256, size=(*SIZES[i], 3), dtype=np.uint8))
              for i in range(N)]
    labels = []
    for i in range(N):
        g = torch.Generator().manual_seed(400 + i)
        labels.append((torch.nn.functional.interpolate(torch.rand(1, 1, 7, 7, generator=g), size=(SIZE, SIZE))[0, 0] > 0.5)
                      .numpy().astype(np.uint8))
    captions = [f"a cat on the grass under the sky, picture {i}" for i in range(N)]
    vae_noise = [torch.randn(1, 16, SIDE // 8, SIDE // 8, generator=torch.Generator().manual_seed(500 + i)) for i in range(N)]
    return images, labels, captions, vae_noise


@pytest.fixture(scope="module")
def tables(pipe, data):
    """Per image the two tables of layer_noise_sweep with the layer mean appended as an extra column, on the host:
    {space: fp32 [levels, layers + 1, C, 16, 16]}."""
    images, _, captions, vae_noise = data
    out = []
    for i in range(N):
        tabs = pipe.layer_noise_sweep(images[i], CONCEPTS, captions[i], LEVELS, vae_noise=vae_noise[i], **KW)
        assert tabs[0].is_cuda and tabs[0].shape == (len(LEVELS), pipe.params.depth, len(CONCEPTS), SIDE // 16, SIDE // 16)
        out.append({s: torch.cat([t, t.mean(dim=1, keepdim=True)], dim=1).cpu().numpy() for s, t in zip(S.SWEEP_SPACES, tabs)})
    return out


@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "raw"])
def test_score_sweep_equals_the_restatement_on_the_downloaded_tables(pipe, data, tables, normalize, monkeypatch):
    images, labels, captions, vae_noise = data
    depth = pipe.params.depth
    seg = S.ConceptAttentionSegmentationModel(pipe)
    dev = S.DeviceSweepScores(len(LEVELS), depth + 1, DEV, chunk=16)     # (36 records: the buffer grows)
    count = _Downloads(monkeypatch)
    out = seg.score_sweep(images, TARGETS, CONCEPTS, captions, labels, dev, LEVELS, size=SIZE, normalize=normalize,
                          layer_mean=True, vae_noise=vae_noise, **KW)
    assert out is None and (count.cpu, count.numpy) == (0, 0), "score_sweep downloaded something"
    result = {s: dev.result(s) for s in S.SWEEP_SPACES}
    assert count.cpu == 1 and count.numpy <= 1, (count.cpu, count.numpy)
    got = dev.to_host()
    calls = dev.records()
    rows = {s: list(dev.rows(s)) for s in S.SWEEP_SPACES}
    dev.all_reduce()
    assert count.cpu == 1, "the records were downloaded again"
    monkeypatch.undo()
    # the calls: per image and space the layers, then the mean column
    assert len(calls) == N * 2 * 2
    want = S.SweepScores(len(LEVELS), depth + 1)
    call = iter(calls)
    worst = 0.0
    for i in range(N):
        k = CONCEPTS.index(TARGETS[i])
        tab = T.tables(SIDE // 16, SIDE // 16, labels[i])
        for space in S.SWEEP_SPACES:
            for cols in (list(range(depth)), [depth]):
                s, c, rec = next(call)
                assert (s, list(c)) == (space, cols) and rec.shape == (len(LEVELS), len(cols))
                for lv in range(len(LEVELS)):
                    for j, col in enumerate(cols):
                        ref = T.score(tables[i][space][lv, col, k], tab, SIZE * SIZE, normalize=normalize)
                        r = rec[lv, j]
                        assert [int(r[f]) for f in ("n11", "n10", "n01", "n00", "thresholds")] == \
                               [ref[f] for f in ("n11", "n10", "n01", "n00", "thresholds")], (i, space, lv, col)
                        d = abs(float(r["ap"]) - ref["ap"])
                        worst = max(worst, d)
                        assert d <= AP_TOL, (i, space, lv, col, float(r["ap"]), ref["ap"])
                        hc = SC.host_counters(ref, SIZE * SIZE)
                        want._add(space, lv, col, hc["correct"], hc["labelled"], np.array(hc["inter"]),
                                  np.array(hc["union"]), ref["ap"])
    print("normalize", normalize, "worst |ap - restatement| over", N * 2 * len(LEVELS) * (depth + 1), "maps:", worst)
    for space in S.SWEEP_SPACES:
        a, b = got.tables[space], want.tables[space]
        for f in ("correct", "labelled", "inter", "union", "n"):
            assert np.array_equal(a[f], b[f]), (space, f)
        assert (a["n"] == N).all()
        assert (np.abs(a["ap_sum"] - b["ap_sum"]) <= N * AP_TOL).all(), space
        w = want.result(space)
        for f in ("pixAcc", "mIoU", "mAP"):
            assert result[space][f].shape == (len(LEVELS), depth + 1)
            assert (np.abs(result[space][f] - w[f]) <= AP_TOL).all(), (space, f)
        # rows(): the scripts' CSV order, level by level, column by column
        assert [(lv, col) for lv, col, *_ in rows[space]] == [(lv, col) for lv in range(len(LEVELS)) for col in range(depth + 1)]
        for lv, col, pa, miou, mAP in rows[space]:
            assert (pa, miou, mAP) == (result[space]["pixAcc"][lv, col], result[space]["mIoU"][lv, col],
                                       result[space]["mAP"][lv, col])


def test_one_space_no_mean_column_and_what_score_sweep_rejects(pipe, data, tables):
    images, labels, captions, vae_noise = data
    depth = pipe.params.depth
    seg = S.ConceptAttentionSegmentationModel(pipe)
    dev = S.DeviceSweepScores(1, depth, DEV)
    seg.score_sweep(images[:1], TARGETS[:1], CONCEPTS, captions, labels[:1], dev, [LEVELS[1]], size=SIZE, normalize=False,
                    target_space="cross_attention", vae_noise=vae_noise[:1], **KW)       # the per-layer script's call
    (space, cols, rec), = dev.records()
    assert space == "cross_attention" and list(cols) == list(range(depth))
    tab = T.tables(SIDE // 16, SIDE // 16, labels[0])
    for col in range(depth):
        ref = T.score(tables[0]["cross_attention"][1, col, 0], tab, SIZE * SIZE, normalize=False)
        assert [int(rec[0, col][f]) for f in ("n11", "n10", "n01", "n00")] == [ref[f] for f in ("n11", "n10", "n01", "n00")]
        assert abs(float(rec[0, col]["ap"]) - ref["ap"]) <= AP_TOL
    assert (dev.result("output")["n"] == 0).all() and (dev.result("cross_attention")["n"] == 1).all()
    with pytest.raises(ValueError, match="4096"):
        seg.score_sweep(images[:1], TARGETS[:1], CONCEPTS, captions, labels[:1], S.DeviceSweepScores(1, depth, DEV), [1],
                        size=SIZE, num_steps=4, width=2048, height=2048)
    with pytest.raises(ValueError):
        seg.score_sweep(images[:1], TARGETS[:1], CONCEPTS, captions, labels[:1], dev, LEVELS, size=SIZE, **KW)   # 3 levels
    with pytest.raises(ValueError):
        seg.score_sweep(images[:1], TARGETS[:1], CONCEPTS, captions, [labels[0][:100]], dev, [1], size=SIZE, **KW)
    with pytest.raises(TypeError):
        seg.score_sweep(images[:1], TARGETS[:1], CONCEPTS, captions, labels[:1], dev, [1], size=SIZE, noise_timestep=2)
