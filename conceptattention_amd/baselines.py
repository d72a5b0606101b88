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
all three.)

``DAAMFluxSegmentationModel`` is the fourth baseline of that harness, DAAM, on this model (the reference's daam_sdxl.py /
daam_sd2.py run it on UNet pipelines): the caption is extended by the concepts' names, and a concept's map is the sum of
the prompt-token maps of its word(s), every occurrence of them."""
from __future__ import annotations

import torch

from .heatmaps import find_words, word_groups
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


def daam_caption(caption: str, concepts) -> str:
    """The caption DAAM's baseline runs on (daam_sdxl.py:155): the concepts appended, so that each has tokens of its own."""
    return caption + "," + ", ".join(f"a {c}" for c in concepts)


def daam_concept_tokens(tokens, concepts) -> list:
    """Per concept, the token indices of every occurrence of its word(s) among ``tokens`` (the caption's token strings,
    already cut to the text length): what its map is summed over.  ValueError for a concept none of whose occurrences
    is left (its words were cut off by the text length, or the tokenizer split them beyond recognition)."""
    groups = word_groups(tokens)
    out = []
    for c in concepts:
        hits = find_words(groups, c)
        if not hits:
            raise ValueError(f"DAAM: the concept {c!r} has no whole occurrence among the caption's {len(tokens)} tokens "
                             "(cut off by the text length?); shorten the caption or raise the text length")
        out.append(sorted({i for h in hits for i in h}))
    return out


class DAAMFluxSegmentationModel:
    """DAAM for Flux as a segmentation baseline, usable wherever the raw-space classes are.  ``direction``:
    "image_to_text" (DAAM's own: the attention the image rows give the word's text keys; ``token_maps``) or
    "text_to_image" (where the word's own text rows look in the image; ``query_maps="tokens"``).

    Differences from the reference's DAAM files, all deliberate: the maps come from the MM-DiT's joint attention in the
    double blocks ``layers`` of one noised forward per sample, not from a UNet's cross-attention over a 50-step
    trajectory; words are matched on the tokenizer's own pieces (heatmaps.word_groups) case-insensitively with the
    surrounding punctuation stripped, where daam matches lemmatised words; and a concept that has no tokens left inside
    the text length raises instead of returning an empty map."""

    DIRECTIONS = ("image_to_text", "text_to_image")

    def __init__(self, pipeline):
        self.pipeline = pipeline

    @torch.no_grad()
    def segment_individual_image(self, image, concepts, caption, layers=None, direction: str = "image_to_text",
                                 num_samples: int = 1, num_steps: int = 4, noise_timestep: int = 2, seed: int = 0,
                                 height: int = 1024, width: int = 1024):
        """(maps fp32 (C, h, w) on the device, None) of one image (a latent (1,16,h/8,w/8) or, with an autoencoder in the
        pipeline, a PIL image).  ``layers``: None is every double block of the model."""
        return self.segment_images([image], [concepts], [caption], layers, direction, num_samples, num_steps,
                                   noise_timestep, seed, height, width)[0]

    @torch.no_grad()
    def segment_images(self, images, concepts, captions, layers=None, direction: str = "image_to_text",
                       num_samples: int = 1, num_steps: int = 4, noise_timestep: int = 2, seed: int = 0, height: int = 1024,
                       width: int = 1024, batch: int = 5, noise=None, vae_noise=None):
        """``segment_individual_image`` for a list of images through ``pipeline.encode_images``: up to ``batch`` images
        per forward, every image with the maps of its own call.  ``concepts``: one list for all or one per image."""
        if direction not in self.DIRECTIONS:
            raise ValueError(f"direction = {direction!r}: one of {list(self.DIRECTIONS)}")
        images = list(images)
        n = len(images)
        per_item = list(concepts) if concepts and not isinstance(concepts[0], str) else [list(concepts)] * n
        if len(per_item) != n or len(captions) < n:
            raise ValueError(f"DAAM: {n} images need {n} concept lists (or one for all) and captions")
        prompts = [daam_caption(captions[i], per_item[i]) for i in range(n)]
        # the concepts' tokens, before anything is launched: a concept cut off by the text length is an error
        index = [daam_concept_tokens(self.pipeline._token_request(p, True)[1], c) for p, c in zip(prompts, per_item)]
        layers = list(range(self.pipeline.params.depth)) if layers is None else list(layers)
        settings = encode_settings(dict(layers=layers, num_samples=num_samples, num_steps=num_steps,
                                        noise_timestep=noise_timestep, seed=seed, height=height, width=width,
                                        joint_attention_kwargs=None, batch=batch))
        outs = self.pipeline.encode_images(images, per_item, prompts, noise=noise, vae_noise=vae_noise,
                                           return_pil_heatmaps=False, token_maps=True,
                                           query_maps="tokens" if direction == "text_to_image" else None,
                                           **settings.keywords())
        results = []
        for o, idx in zip(outs, index):
            maps = o.query_heatmaps["tokens"] if direction == "text_to_image" else \
                torch.as_tensor(o.token_heatmaps, device=self.pipeline.device)
            results.append((torch.stack([maps[ix].sum(0) for ix in idx]), None))
        return results
