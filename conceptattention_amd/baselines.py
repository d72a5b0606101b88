"""The reference's three "raw" baselines (concept_attention/binary_segmentation_baselines/raw_output_space.py,
raw_value_space.py, raw_cross_attention.py; the RawOutputSpace / RawValueSpace / RawCrossAttention choices of
experiments/imagenet_segmentation/run_experiment.py) over a ``ConceptAttentionFluxPipeline``.

Their maps are stated by one einsum, "layers timesteps heads concepts dims, layers timesteps heads pixels dims -> layers
timesteps heads concepts pixels", an optional softmax over the concepts PER HEAD, and the mean over layers, samples and
heads.  That is ``ops.head_maps`` (``encode_images(head_maps=space)``: ``raw_heatmaps[space]``), run inside the forward on
the rows the layer has just written; nothing is stacked on the host.

The spaces:
  RawOutputSpaceSegmentationModel     attention outputs, concept rows against image rows            ("output")
  RawValueSpaceSegmentationModel      the v projections, concept v against image v                  ("value")
  RawCrossAttentionSegmentationModel  post-QK-norm, pre-RoPE q, concept q against image q           ("cross")
RawCrossAttention is the per-head form of this project's cross-attention space, i.e. the vectors the reference's dict calls
``cross_attention_*_vectors``; the reference's own file reads a variable that no longer exists there.

``normalize_concepts`` has the default of the reference's class (output and value: True, cross: False) and applies
``heatmaps.linear_normalization`` across the concepts to the [C, hidden] concept rows before the launch.  (The reference's
output-space class accepts the keyword and has the normalisation commented out; here the keyword does what it says in
all three.)"""
from __future__ import annotations

import torch

from .segmentation import encode_settings


class _RawSpaceSegmentationModel:
    space = None                   # the head_maps space of the subclass
    normalize_default = True       # the reference class's normalize_concepts default

    def __init__(self, pipeline):
        self.pipeline = pipeline

    @torch.no_grad()
    def segment_individual_image(self, image, concepts, caption, layers=None, softmax: bool = False,
                                 normalize_concepts=None, num_samples: int = 1, num_steps: int = 4, noise_timestep: int = 2,
                                 seed: int = 0, height: int = 1024, width: int = 1024, joint_attention_kwargs=None):
        """(maps fp32 (C, h, w) on the device, None): the baseline's coefficients of one image (a latent (1,16,h/8,w/8)
        or, with an autoencoder in the pipeline, a PIL image).  ``layers``: None is every double block of the model (the
        reference's range(19) on Flux); ``softmax``: over the concepts per head, before the mean."""
        return self.segment_images([image], [concepts], [caption], layers, softmax, normalize_concepts, num_samples,
                                   num_steps, noise_timestep, seed, height, width, joint_attention_kwargs)[0]

    @torch.no_grad()
    def segment_images(self, images, concepts, captions, layers=None, softmax: bool = False,
                       normalize_concepts=None, num_samples: int = 1, num_steps: int = 4, noise_timestep: int = 2,
                       seed: int = 0, height: int = 1024, width: int = 1024, joint_attention_kwargs=None, batch: int = 5,
                       noise=None, vae_noise=None):
        """``segment_individual_image`` for a list of images through ``pipeline.encode_images``: up to ``batch`` images
        per forward, every image with the maps of its own call."""
        layers = list(range(self.pipeline.params.depth)) if layers is None else list(layers)
        kw = dict(layers=layers, num_samples=num_samples, num_steps=num_steps, noise_timestep=noise_timestep, seed=seed,
                  height=height, width=width, joint_attention_kwargs=joint_attention_kwargs, batch=batch)
        settings = encode_settings(kw)
        normalize = self.normalize_default if normalize_concepts is None else bool(normalize_concepts)
        outs = self.pipeline.encode_images(images, concepts, list(captions[:len(images)]), noise=noise, vae_noise=vae_noise,
                                           return_pil_heatmaps=False, head_maps=self.space,
                                           head_norm="softmax" if softmax else None, head_normalize_concepts=normalize,
                                           **settings.keywords())
        return [(o.raw_heatmaps[self.space], None) for o in outs]


class RawOutputSpaceSegmentationModel(_RawSpaceSegmentationModel):
    space, normalize_default = "output", True


class RawValueSpaceSegmentationModel(_RawSpaceSegmentationModel):
    space, normalize_default = "value", True


class RawCrossAttentionSegmentationModel(_RawSpaceSegmentationModel):
    space, normalize_default = "cross", False
