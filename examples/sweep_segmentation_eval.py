"""Image-sharded per-layer x per-noise-level segmentation scoring (the loops of
experiments/per_layer_segmentation/test_segmentations_per_layer.py and
experiments/per_timestep_segmentation/test_segmentations_per_time.py on the MI355X path): every rank runs the sweep of its
share of the images, scores every (noise level, layer) map of the target concept against the image's label and accumulates
the tables of pixAcc / mIoU / mAP; one all_reduce of the tables at the end, then the CSV rows.

    python examples/sweep_segmentation_eval.py                    # 1 GPU, scores on the host
    python examples/sweep_segmentation_eval.py --device-scores    # every table scored where it is (ca_segtab_score)
    python examples/sweep_segmentation_eval.py --raw              # the per-layer script: raw coefficients, no min-max
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/sweep_segmentation_eval.py

No dataset can be fetched here, so the 'images' are seeded random PIL images and the 'labels' random blobs at 224 x 224:
the scores are meaningless, the data flow is the real one.  The pipeline is built with synthetic weights, the synthetic
autoencoder, T5 and CLIP encoders.  N_IMAGES (4), N_LEVELS (5 of 50 steps) and SIDE (1024) come from the environment.  The
last column of every level is the mean over the layers (the per-timestep script's row)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import PIL.Image
import torch

from conceptattention_amd import ConceptAttentionFluxPipeline
from conceptattention_amd import distributed as D
from conceptattention_amd import segmentation as S

CONCEPTS = ["object", "background", "grass", "sky"]
SIZE, NUM_STEPS = 224, 50

rank, world, local = D.init_from_env()
dev = torch.device(os.environ.get("CA_BENCH_DEVICE") or f"cuda:{local}")
torch.cuda.set_device(dev)
n_images, n_levels, side = (int(os.environ.get(k, d)) for k, d in (("N_IMAGES", 4), ("N_LEVELS", 5), ("SIDE", 1024)))
device_scores, normalize = "--device-scores" in sys.argv[1:], "--raw" not in sys.argv[1:]
pipe = ConceptAttentionFluxPipeline("flux-schnell", device=dev, autoencoder="synthetic", text_encoder="synthetic-t5-clip")
seg = S.ConceptAttentionSegmentationModel(pipe)
depth = pipe.params.depth
levels = [int(v) for v in np.linspace(0, NUM_STEPS - 1, n_levels).round()]
scores = S.DeviceSweepScores(n_levels, depth + 1, dev) if device_scores else S.SweepScores(n_levels, depth + 1)
kw = dict(num_steps=NUM_STEPS, width=side, height=side, batch=5)


def label_of(j):
    g = torch.Generator().manual_seed(100 + j)
    return (torch.nn.functional.interpolate(torch.rand(1, 1, 7, 7, generator=g), size=(SIZE, SIZE))[0, 0] > 0.5) \
        .numpy().astype(np.uint8)


mine = list(D.shard_items(n_images, rank, world))
images = [PIL.Image.fromarray(np.random.default_rng(100 + j).integers(0, 256, (side, side, 3), dtype=np.uint8)) for j in mine]
captions = [f"a photo of object number {j}" for j in mine]
labels = [label_of(j) for j in mine]
lat = (1, 16, side // 8, side // 8)
vae_noise = [torch.randn(*lat, generator=torch.Generator().manual_seed(30 + j)) for j in mine]   # both routes print the same
if images and device_scores:
    seg.score_sweep(images, ["object"] * len(mine), CONCEPTS, captions, labels, scores, levels, size=SIZE, normalize=normalize,
                    layer_mean=True, vae_noise=vae_noise, **kw)
else:
    for im, cap, y, vn in zip(images, captions, labels, vae_noise):
        tabs = pipe.layer_noise_sweep(im, CONCEPTS, cap, levels, vae_noise=vn, **kw)
        for space, table in zip(S.SWEEP_SPACES, tabs):
            table = torch.cat([table, table.mean(dim=1, keepdim=True)], dim=1)[:, :, 0].cpu()     # the target's planes
            for lv in range(n_levels):
                for col in range(depth + 1):
                    x = table[lv, col]
                    mask = x > x.mean()
                    if normalize:
                        c, m = S.prepare_for_scoring(x.numpy(), mask.numpy(), size=SIZE)
                    else:
                        c, m = S._resize_nearest(x, (SIZE, SIZE)), S._resize_nearest(mask.float(), (SIZE, SIZE))
                    scores.update(space, lv, col, m, c, y.astype(bool))
total = scores.all_reduce()
if rank == 0:
    for space in S.SWEEP_SPACES:
        print(f"space,noise_level,layer,pixAcc,mIoU,mAP   # {space}, {int(total.tables[space]['n'].max())} images")
        for lv, col, pa, miou, m_ap in total.rows(space):
            print(f"{space},{levels[lv]},{'mean' if col == depth else col},{pa:.6f},{miou:.6f},{m_ap:.6f}")
D.barrier()
if torch.distributed.is_initialized():
    torch.distributed.destroy_process_group()
