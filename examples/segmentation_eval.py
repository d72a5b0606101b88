"""Image-sharded zero-shot segmentation scoring (the loop of experiments/imagenet_segmentation/run_experiment.py
on the MI355X path): every rank encodes its share of the images, thresholds the target concept's heat map at its
mean and accumulates pixAcc / mIoU / mAP; one all_reduce of seven numbers at the end.

    python examples/segmentation_eval.py                      # 1 GPU
    python examples/segmentation_eval.py --pixels             # PIL images in: HIP autoencoder and text encoders in front
    python examples/segmentation_eval.py --pixels --device-scores   # and the scores on the device (ca_seg_score)
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/segmentation_eval.py

No dataset can be fetched here, so the 'images' are seeded random latents and the 'labels' random blobs: the
scores are meaningless, the data flow is the real one.  With ``--pixels`` the 'images' are seeded random PIL images of
mixed sizes and the pipeline is built with the synthetic autoencoder, T5 and CLIP encoders: a rank hands its whole share
to the segmentation model as ONE list, which sends it through ``pipeline.encode_images`` five images per forward.
``--device-scores`` hands the labels over as well (``score_images``): every chunk's target maps are scored where they
are, and the only download is that of the 40-byte records, once, before the all_reduce."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from conceptattention_amd import ConceptAttentionFluxPipeline
from conceptattention_amd import distributed as D
from conceptattention_amd.segmentation import (ConceptAttentionSegmentationModel, DeviceSegmentationScores,
                                               SegmentationScores, prepare_for_scoring)

rank, world, local = D.init_from_env()
dev = torch.device(os.environ.get("CA_BENCH_DEVICE") or f"cuda:{local}")
torch.cuda.set_device(dev)
n_images = int(os.environ.get("N_IMAGES", 8))
pixels = "--pixels" in sys.argv[1:]
device_scores = "--device-scores" in sys.argv[1:]
pipe = ConceptAttentionFluxPipeline("flux-schnell", device=dev, **(
    dict(autoencoder="synthetic", text_encoder="synthetic-t5-clip") if pixels else {}))
seg = ConceptAttentionSegmentationModel(pipe)
scores = DeviceSegmentationScores(dev) if device_scores else SegmentationScores()
background = ["background", "floor", "grass", "tree", "sky"]
kw = dict(layers=list(range(19)), num_samples=1, num_steps=4, noise_timestep=2)


def label_of(g):
    return torch.nn.functional.interpolate(torch.rand(1, 1, 7, 7, generator=g), size=(224, 224))[0, 0] > 0.5


if pixels:
    import numpy as np
    import PIL.Image
    mine = list(D.shard_items(n_images, rank, world))
    sizes = [(1024, 1024), (500, 375), (333, 500)]                    # (ImageNet-S pictures come in every size)
    images = [PIL.Image.fromarray(np.random.default_rng(100 + j).integers(0, 256, (*sizes[j % 3], 3), dtype=np.uint8))
              for j in mine]
    if images and device_scores:
        labels = [label_of(torch.Generator().manual_seed(100 + j)).numpy() for j in mine]
        seg.score_images(images, ["object"] * len(mine), ["object"] + background, ["a object"] * len(mine), labels, scores,
                         size=224, **kw)
    elif images:
        masks, coeffs, _ = seg(images, target_concepts=["object"] * len(mine), concepts=["object"] + background,
                               captions=["a object"] * len(mine), **kw)
        for k, j in enumerate(mine):
            c, m = prepare_for_scoring(coeffs[k], masks[k], size=224)
            scores.update(m, c, label_of(torch.Generator().manual_seed(100 + j)).numpy())
else:
    for j in D.shard_items(n_images, rank, world):
        g = torch.Generator().manual_seed(100 + j)
        latent = torch.randn(1, 16, 128, 128, generator=g)
        label = label_of(g)
        if device_scores:
            seg.score_images([latent], ["object"], ["object"] + background, ["a object"], [label.numpy()], scores, size=224,
                             **kw)
            continue
        masks, coeffs, _ = seg(latent, target_concepts=["object"], concepts=["object"] + background, captions=["a object"],
                               **kw)
        c, m = prepare_for_scoring(coeffs[0], masks[0], size=224)
        scores.update(m, c, label.numpy())
result = scores.all_reduce().result()
if rank == 0:
    print(f"images {result['n']}: pixAcc {result['pixAcc']:.4f}  mIoU {result['mIoU']:.4f}  mAP {result['mAP']:.4f}")
D.barrier()
if torch.distributed.is_initialized():
    torch.distributed.destroy_process_group()
