"""Image-sharded multi-class zero-shot segmentation scoring (the loop of
experiments/pascal_voc_segmentation/run_multi_class_seg_experiment.py on the MI355X path): every rank encodes its share of
the images with the background concepts plus the classes present in each image, takes the argmax over the concepts, maps it
to VOC class ids and accumulates pixAcc and the per-class intersection / union; one all_reduce of the counters at the end.

    python examples/multiclass_segmentation_eval.py                    # 1 GPU, scores on the host
    python examples/multiclass_segmentation_eval.py --device-scores    # argmax, class map and counts on the device (ca_mseg_score)
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/multiclass_segmentation_eval.py

No dataset can be fetched here, so the 'images' are seeded random PIL images of mixed sizes and the 'labels' random 21-class
maps at 64 x 64 (the harness's label size) with a frame of 255, VOC's void label: the scores are meaningless, the data flow is
the real one.  The pipeline is built with the synthetic autoencoder, T5 and CLIP encoders; a rank hands its whole share over
as ONE list, which goes through ``pipeline.encode_images`` five images of one concept count per forward.  ``--device-scores``
hands the labels over as well (``score_multiclass_images``): every item's maps are scored where they are, and the only
download is that of the count rows, once, before the all_reduce.  The 255 frame is skipped (``ignore_index=255``); the
harness itself skips nothing, which ``--count-void`` reproduces."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import PIL.Image
import torch

from conceptattention_amd import ConceptAttentionFluxPipeline
from conceptattention_amd import distributed as D
from conceptattention_amd.segmentation import (ConceptAttentionSegmentationModel, DeviceMultiClassScores, MultiClassScores,
                                               map_predictions_to_class_indices, multiclass_table)

NAMES = ["background", "aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable",
         "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"]
BACKGROUND = ["background", "floor", "grass", "tree", "sky"]
SIZE = 64

rank, world, local = D.init_from_env()
dev = torch.device(os.environ.get("CA_BENCH_DEVICE") or f"cuda:{local}")
torch.cuda.set_device(dev)
n_images = int(os.environ.get("N_IMAGES", 8))
device_scores = "--device-scores" in sys.argv[1:]
ignore = None if "--count-void" in sys.argv[1:] else 255
pipe = ConceptAttentionFluxPipeline("flux-schnell", device=dev, autoencoder="synthetic", text_encoder="synthetic-t5-clip")
seg = ConceptAttentionSegmentationModel(pipe)
scores = DeviceMultiClassScores(len(NAMES), dev) if device_scores else MultiClassScores(len(NAMES))
kw = dict(layers=list(range(14, 18)), num_samples=1, num_steps=4, noise_timestep=3)      # (the harness's defaults)


def present_classes(j):
    """1 to 3 class names of image j, as the dataset would hand them over (background removed)."""
    rng = np.random.default_rng(500 + j)
    return [NAMES[k] for k in sorted(rng.choice(np.arange(1, len(NAMES)), size=1 + j % 3, replace=False))]


def label_of(j, present):
    g = torch.Generator().manual_seed(100 + j)
    ids = torch.tensor([0] + [NAMES.index(c) for c in present])
    coarse = ids[torch.randint(0, len(ids), (7, 7), generator=g)]
    y = torch.nn.functional.interpolate(coarse[None, None].float(), size=(SIZE, SIZE))[0, 0].numpy().astype(np.uint8)
    y[:2], y[-2:], y[:, :2], y[:, -2:] = 255, 255, 255, 255
    return y


mine = list(D.shard_items(n_images, rank, world))
sizes = [(1024, 1024), (500, 375), (333, 500)]                        # (VOC pictures come in every size)
images = [PIL.Image.fromarray(np.random.default_rng(100 + j).integers(0, 256, (*sizes[j % 3], 3), dtype=np.uint8))
          for j in mine]
targets = [present_classes(j) for j in mine]
captions = [",".join(f"a {c}" for c in t) for t in targets]
labels = [label_of(j, t) for j, t in zip(mine, targets)]
torch.manual_seed(0)      # (the autoencoder draws its sampling noise from the device generator: both routes print the same)
if images and device_scores:
    seg.score_multiclass_images(images, captions, BACKGROUND, targets, NAMES, labels, scores, ignore_index=ignore, **kw)
elif images:
    out = seg.segment_multiclass(images, captions, BACKGROUND, targets, **kw)
    for (index, _, _), t, y in zip(out, targets, labels):
        klass = map_predictions_to_class_indices(index, multiclass_table(BACKGROUND, t, NAMES))
        up = torch.nn.functional.interpolate(klass[None, None].float(), size=y.shape, mode="nearest")[0, 0]
        scores.update(up, y, ignore_index=ignore)
result = scores.all_reduce().result()
if rank == 0:
    print(f"images {result['n']}: pixAcc {result['pixAcc']:.4f}  mIoU {result['mIoU']:.4f}")
    print("IoU per class: " + "  ".join(f"{n} {v:.3f}" for n, v in zip(NAMES, result["IoU"]) if not np.isnan(v)))
D.barrier()
if torch.distributed.is_initialized():
    torch.distributed.destroy_process_group()
