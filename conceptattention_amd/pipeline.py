"""ConceptAttentionFluxPipeline on MI355X: same public surface as the reference's
``concept_attention/concept_attention_pipeline.py:94-357`` (constructor arguments, ``generate_image``
and ``encode_image`` signatures and defaults, ``ConceptAttentionPipelineOutput``), running the DiT
and the heat-map reduction in the gfx950 kernels.

Text and image plumbing.  The autoencoder (``vae.py``), the T5 encoder (``t5.py``) and the CLIP text encoder (``clip.py``)
run in HIP and are opt-in: ``autoencoder="synthetic"`` or a ``.safetensors`` path; ``text_encoder`` = a
``t5.HipTextEncoder`` (T5 weights from a local file, any tokenizer callable, ``clip=`` a ``clip.HipClipEmbedder``),
``"synthetic-t5"`` (the T5 encoder on synthetic weights behind a toy byte tokenizer) or ``"synthetic-t5-clip"`` (that plus
a synthetic CLIP text encoder for the pooled ``vec``).
No checkpoint or vocabulary file is available offline, so the default is still *synthetic conditioning*: prompt and
concept strings are mapped to seeded N(0,1) embeddings of the right shapes (``SyntheticTextEncoder``) and ``image`` is
returned as the unpacked latent -- exactly the configuration BASELINE.json measures.  Still out of scope: tokenizer
vocabularies.
"""
from __future__ import annotations

import zlib
from dataclasses import InitVar, dataclass, field, fields
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, ops, sampling
from .flux_dit import HeatmapRequest, HipFluxDiT, StepTrace, on_own_device
from .heatmaps import check_concept_count, compute_heatmaps_from_vectors, resolve_norm, word_groups, word_maps
from .params import configs


@dataclass
class ConceptAttentionPipelineOutput:
    """concept_attention_pipeline.py:20-24."""
    image: object  # PIL.Image.Image | np.ndarray
    concept_heatmaps: list
    cross_attention_maps: list
    # prompt-token maps (token_maps=True or an int): one map per prompt token, the attention the image tokens give that
    # token's key in the captured double blocks (mean over heads, layers and steps; DAAM), and the tokenizer's strings
    # (None when the maps were asked for by count)
    token_heatmaps: Optional[list] = None
    tokens: Optional[list] = None
    # keep_trace=True: the image side of the call's traced steps, for ``ConceptAttentionFluxPipeline.requery``
    trace: Optional["ImageTrace"] = None
    # head_maps="output" | "cross" | "value" (or a tuple of them): per space the head-resolved concept maps, an fp32 device
    # tensor (num_heads, C, h, w), and their mean over the heads (C, h, w): the raw-space baselines' maps (ops.head_maps)
    head_maps: Optional[dict] = None
    raw_heatmaps: Optional[dict] = None
    # token_maps=True: the prompt's words (heatmaps.word_groups of ``tokens``) and one map per word, the sum of its tokens'
    # maps (DAAM's rule; heatmaps.word_maps), in the form of ``token_heatmaps``
    words: Optional[list] = None
    word_heatmaps: Optional[object] = None
    # query_maps="tokens" | "concepts" (or both): the other direction, where a token's / a concept's own query row looks in
    # the image (ops.query_maps), keyed by kind; "words" beside "tokens" when the call has the token strings.  fp32 device
    # tensors (n, h, w) with return_pil_heatmaps=False, lists of PIL pictures otherwise (one min-max per item and kind)
    query_heatmaps: Optional[dict] = None
    # propagate="output" | "cross" (or both): per space the concept maps carried through the image rows' own attention
    # (ops.propagate_maps): every captured layer's map replaced by the attention-weighted mean of the patches each patch
    # attends to, mean over heads, layers and steps.  fp32 device tensors (C, h, w) with return_pil_heatmaps=False, lists
    # of PIL pictures otherwise (one min-max per item and space)
    propagated_heatmaps: Optional[dict] = None


PROPAGATE_SPACES = {"output": "prop_out", "cross": "prop_cross"}   # space -> its HeatmapRequest field
QUERY_KINDS = ("tokens", "concepts")
HEAD_SPACES = {"output": ("heads_out", "raw_out"), "cross": ("heads_cross", "raw_cross"),
               "value": ("heads_value", "raw_value")}   # space -> its two HeatmapRequest fields


@dataclass
class HeadMapAccumulators:
    """One item's per-head maps while its forwards run: per asked space the zeroed fp32 [num_heads, C, patches] and
    [C, patches] accumulators, the norm across the concepts (None: the logits themselves) and whether the concept rows
    are linearly normalised across the concepts first."""
    heads: dict
    raw: dict
    norm: Optional[int] = None
    normalize_concepts: bool = False
    name: Optional[str] = None    # the norm's name in the call's ``head_norm``
    more: tuple = ()              # the same spaces under the call's further norms (several names in ``head_norm``)

    def request_fields(self) -> dict:
        """The keywords of this item's ``HeatmapRequest``."""
        kw = dict(head_norm=self.norm, head_normalize_concepts=self.normalize_concepts)
        for space, (hf, rf) in HEAD_SPACES.items():
            if space in self.heads:
                kw[hf], kw[rf] = self.heads[space], self.raw[space]
        if self.more:
            kw["head_more"] = tuple(HeatmapRequest((), 0.0, None, None, **m.request_fields()) for m in self.more)
        return kw

    def outputs(self, side: int) -> tuple:
        """(head_maps, raw_heatmaps) of the finished item: dicts space -> (num_heads, C, side, side) / (C, side, side);
        with several norms in the call the keys are (space, norm name)."""
        every = (self,) + tuple(self.more)
        key = (lambda s, a: (s, a.name)) if self.more else (lambda s, a: s)
        return ({key(s, a): t.view(*t.shape[:2], side, side) for a in every for s, t in a.heads.items()},
                {key(s, a): t.view(t.shape[0], side, side) for a in every for s, t in a.raw.items()})


def head_request_fields(head_acc, j: int) -> dict:
    return {} if head_acc is None or head_acc[j] is None else head_acc[j].request_fields()


def query_request_fields(query_acc, j: int) -> dict:
    """The HeatmapRequest keywords of item j's query-row accumulators (a dict kind -> fp32 [n, patches], or None)."""
    acc = {} if query_acc is None or query_acc[j] is None else query_acc[j]
    return dict(token_query_space=acc.get("tokens"), concept_query_space=acc.get("concepts"))


def propagate_request_fields(prop_acc, j: int) -> dict:
    """The HeatmapRequest keywords of item j's propagated-map accumulators ((dict space -> fp32 [C, patches], steps), or
    None)."""
    if prop_acc is None or prop_acc[j] is None:
        return {}
    acc, steps = prop_acc[j]
    return dict(prop_steps=steps, **{PROPAGATE_SPACES[space]: t for space, t in acc.items()})


@dataclass
class ImageTrace:
    """What a ``keep_trace=True`` call keeps of ONE item: per traced step (a ``timesteps`` index of a generate call, a
    noise-sample index of an encode call) the item's ``flux_dit.StepTrace``, the settings of the call and the finished
    image.  ``nbytes`` is the device memory it holds (INTEGRATION.md "Concept re-query"); ``release()`` lets go of it."""
    steps: dict                   # step key -> StepTrace (the item's view of its forward's storage)
    settings: dict                # the keywords of the call that made it ("call": "generate_image" | "encode_image")
    image: object                 # what the call returned as ``image``
    released: bool = False

    @property
    def layer_indices(self) -> list:
        return list(next(iter(self.steps.values())).layers) if self.steps else []

    @property
    def timesteps(self) -> list:
        return list(self.steps)

    @property
    def nbytes(self) -> int:
        return sum(s.nbytes for s in self.steps.values())

    def release(self) -> None:
        for s in self.steps.values():
            s.release()
        self.released = True


def trace_nbytes(params, n_concepts: int, n_text: int, n_image: int, layer_indices, n_steps: int) -> int:
    """``ImageTrace.nbytes`` of an item from the call's settings alone: ``n_steps`` traced steps, each the double blocks
    0 .. max(layer_indices) and the captured layers' fp32 rows (``flux_dit.step_trace_nbytes``).  Pure arithmetic."""
    from .flux_dit import step_trace_nbytes
    layers = sorted({int(l) for l in layer_indices})
    return n_steps * step_trace_nbytes(params, n_concepts, n_text, n_image, layers[-1] + 1 if layers else 0, len(layers))


class SyntheticTextEncoder:
    """Stand-in for HFEmbedder (flux/modules/conditioner.py): deterministic N(0,1) embeddings
    keyed by the text, T5-like (1,T,4096) and CLIP-like pooled (1,768)."""

    def __init__(self, n_tokens: int, context_dim: int = 4096, vec_dim: int = 768, device="cuda:0"):
        self.n_tokens, self.context_dim, self.vec_dim, self.device = n_tokens, context_dim, vec_dim, device

    def _gen(self, text: str, salt: int):
        g = torch.Generator(device="cpu")
        g.manual_seed((zlib.crc32(text.encode()) * 31 + salt) & 0x7FFFFFFF)
        return g

    def t5(self, text: str) -> torch.Tensor:
        return torch.randn(1, self.n_tokens, self.context_dim, generator=self._gen(text, 1)).to(
            self.device, torch.bfloat16)

    def clip(self, text: str) -> torch.Tensor:
        return torch.randn(1, self.vec_dim, generator=self._gen(text, 2)).to(self.device, torch.bfloat16)


def colorize_heatmaps(heatmaps: np.ndarray, cmap: str = "plasma") -> list:
    """Global min-max over ALL concepts, matplotlib colormap, uint8 RGB -> PIL
    (concept_attention_pipeline.py:174-196)."""
    import matplotlib.pyplot as plt
    import PIL.Image
    lo, hi = heatmaps.min(), heatmaps.max()
    out = []
    for hm in heatmaps:
        hm = (hm - lo) / (hi - lo)
        rgb = (plt.get_cmap(cmap)(hm)[:, :, :3] * 255).astype(np.uint8)
        out.append(PIL.Image.fromarray(rgb))
    return out


MAX_ITEMS_PER_FORWARD = min(_lib.ATTN_MAX_PROBLEMS // 2, _lib.MAX_SEGMENTS // 3)   # launch limits: 5 items


def items_per_forward(batch: int) -> int:
    """What a ``batch`` argument means: 1 .. MAX_ITEMS_PER_FORWARD work items in one forward."""
    return max(1, min(int(batch), MAX_ITEMS_PER_FORWARD))


@dataclass(frozen=True)
class EncodeSettings:
    """What an encode call is asked to do, apart from its images, strings and noise.  The defaults are written here, once
    (tests/test_frontend_cpu.py holds the public signatures to them); the constructor makes the checks of such a call."""
    layer_indices: Sequence = field(default_factory=lambda: list(range(15, 19)))
    num_samples: int = 1
    num_steps: int = 4
    noise_timestep: int = 2
    seed: int = 0
    width: int = 1024
    height: int = 1024
    batch: int = 5
    stop_after_multi_modal_attentions: bool = True
    joint_attention_kwargs: Optional[dict] = None
    attention_norm: str = "sparsemax"
    softmax: bool = True
    norm: int = field(init=False, default=_lib.NORM_SOFTMAX)   # the resolved (softmax, attention_norm)
    depth: InitVar[Optional[int]] = None     # the model's double blocks, when the layer indices are to be checked
    n_concepts: InitVar[int] = 0             # the largest concept count of the call

    def __post_init__(self, depth, n_concepts):
        assert depth is None or all([0 <= li < depth for li in self.layer_indices]), "Invalid layer index"
        assert self.height == self.width, "Height and width must be the same for now"
        object.__setattr__(self, "norm", resolve_norm(self.softmax, self.attention_norm))   # ValueError on an unknown name
        check_concept_count(self.norm, n_concepts)

    def keywords(self) -> dict:
        """The settings under the parameter names of ``encode_images``."""
        return {f.name: getattr(self, f.name) for f in fields(self) if f.init}


def _cat(tensors) -> torch.Tensor:
    """The items of a forward along the item axis; one item is passed on as it is (no copy)."""
    tensors = list(tensors)
    return tensors[0] if len(tensors) == 1 else torch.cat(tensors, 0)


def plan_batches(keys: Sequence, batch: int) -> list:
    """The forwards of a batched call, as lists of item indices.  ``keys[i]`` is whatever item i must share with the
    others of its forward -- (latent shape, concept count, text length).  Items of one key form a group, the groups in the
    order of their first item; a group is cut into chunks of at most min(batch, MAX_ITEMS_PER_FORWARD) items in their
    original order.  Pure: no device, no tensors."""
    size = items_per_forward(batch)
    groups: dict = {}
    for i, k in enumerate(keys):
        groups.setdefault(k, []).append(i)
    return [idx[c0:c0 + size] for idx in groups.values() for c0 in range(0, len(idx), size)]


def plan_requery(geometries: Sequence, concept_counts: Sequence) -> list:
    """The forwards of a ``requery`` call, as lists of item indices: items that share ``geometries[i]`` (whatever a
    trace needs the others of its forward to share) and a concept count go through one concept-row pass, at most
    MAX_ITEMS_PER_FORWARD at a time, in item order (``plan_batches``).  Pure: no device, no tensors."""
    if len(geometries) != len(concept_counts):
        raise ValueError("plan_requery: one geometry and one concept count per item")
    return plan_batches(list(zip(geometries, concept_counts)), MAX_ITEMS_PER_FORWARD)


def _per_item(value, n: int, what: str) -> list:
    """``concepts``-style argument: one list of strings for all n items, or one list per item."""
    value = list(value)
    if value and all(isinstance(v, str) for v in value):
        return [value] * n
    if len(value) != n:
        raise ValueError(f"{what}: one list for all items, or one list per item ({n} items, got {len(value)})")
    return [list(v) for v in value]


class ConceptAttentionFluxPipeline:
    def __init__(self, model_name: str = "flux-schnell", offload_model: bool = False, device="cuda:0",
                 weights="synthetic", weight_seed: int = 0, text_encoder=None, autoencoder=None,
                 params=None, n_text_tokens: Optional[int] = None, precision: str = "bf16",
                 residual_dtype=torch.float32, capture_independent_image: bool = False, t5_precision: str = "bf16"):
        """model_name / offload_model / device as in the reference (:100-113).  ``weights`` is
        "synthetic" (seeded random init), a path to a flux1-*.safetensors file, or a state dict.
        ``precision="fp8"`` runs the large projections on e4m3 operands (HipFluxDiT.set_precision);
        ``residual_dtype`` is the storage type of the residual streams (fp32 by default, HipFluxDiT.__init__);
        ``text_encoder``: None (seeded-noise stand-in), "synthetic-t5", "synthetic-t5-clip", or an object with ``t5`` / ``clip`` (a
        ``t5.HipTextEncoder``; one with ``t5_many`` encodes prompt and concepts in one forward).
        ``t5_precision``: "bf16" (default) or "fp8", the precision of the T5 encoder a ``text_encoder`` NAME builds
        (t5.T5Encoder: e4m3 projections, opt-in; independent of ``precision``, which is the DiT's).
        ``capture_independent_image=True`` makes the returned latent (and every map) independent of ``layer_indices``
        bit for bit, as in the reference, for the image rows' attention twice in the captured layers
        (HipFluxDiT.capture_independent_image)."""
        if params is None and model_name not in configs:
            raise KeyError(model_name)
        self.model_name = model_name
        self.offload_model = offload_model
        self.device = torch.device(device)
        self.is_schnell = model_name == "flux-schnell"
        self.params = params if params is not None else configs[model_name]
        # the generator owns model / encoders / autoencoder, as in the reference (:104-113)
        from .image_generator import FluxGenerator
        self.flux_generator = FluxGenerator(model_name=model_name, offload=offload_model, device=self.device,
                                            weights=weights, weight_seed=weight_seed, text_encoder=text_encoder,
                                            autoencoder=autoencoder, params=self.params,
                                            n_text_tokens=n_text_tokens, residual_dtype=residual_dtype,
                                            t5_precision=t5_precision)
        self.model = self.flux_generator.model
        self.model.set_precision(precision)
        self.model.capture_independent_image = bool(capture_independent_image)
        self.fp8_keep_heatmap_layers = True  # generate path only; the sweeps/encode path run every block in fp8
        self._replicas = [self.model]  # activation sets that share self.model's weights (one per stream)
        self._streams = []
        self.text_encoder = self.flux_generator.text_encoder
        self.autoencoder = self.flux_generator.ae   # (a name or path was built into the HIP AutoEncoder there)

    # ------------------------------------------------------------------ conditioning
    def _embed(self, prompt: str, concepts: Sequence[str]):
        return self.flux_generator.embed(prompt, concepts)

    def _finish(self, image, concept_heatmaps, cross_attention_maps, return_pil_heatmaps, cmap, token_maps=None,
                tokens=None):
        """``token_maps``: the item's prompt-token maps fp32 [n_tok, side, side] on the device, or None."""
        concept_heatmaps = concept_heatmaps.to(torch.float32).detach().cpu().numpy()[0]
        cross_attention_maps = cross_attention_maps.to(torch.float32).detach().cpu().numpy()[0]
        if token_maps is not None:
            token_maps = token_maps.to(torch.float32).detach().cpu().numpy()
        if return_pil_heatmaps:
            concept_heatmaps = colorize_heatmaps(concept_heatmaps, cmap)
            cross_attention_maps = colorize_heatmaps(cross_attention_maps, cmap)
            if token_maps is not None:                   # (global min-max over the prompt's tokens)
                token_maps = colorize_heatmaps(token_maps, cmap)
        return ConceptAttentionPipelineOutput(image=image, concept_heatmaps=concept_heatmaps,
                                              cross_attention_maps=cross_attention_maps, token_heatmaps=token_maps,
                                              tokens=tokens)

    # ------------------------------------------------------------------ prompt-token maps
    def _token_request(self, prompt: str, token_maps):
        """(n_tok, tokens) of a call's ``token_maps`` argument: None / False -> (0, None); True -> the tokenizer's tokens of
        the prompt without the end-of-string token (DAAM keeps maps[:len(tokens)]), truncated to the text length; an int n
        -> the first n text rows, tokens None (the route for a text encoder without a tokenizer)."""
        if token_maps is None or token_maps is False:
            return 0, None
        T = self._text_length()
        if token_maps is True:
            tokenizer = getattr(self.text_encoder, "tokenizer", None)
            if tokenizer is None or not hasattr(tokenizer, "tokenize"):
                raise ValueError("token_maps=True needs a text encoder whose tokenizer has .tokenize (text_encoder="
                                 "\"synthetic-t5\", \"synthetic-t5-clip\" or a HipTextEncoder); pass an int n for the first n "
                                 "text rows")
            tokens = list(tokenizer.tokenize(prompt))[:T]
            if not tokens:
                raise ValueError("token_maps=True: the prompt has no tokens")
            return len(tokens), tokens
        n = int(token_maps)
        if not 1 <= n <= min(T, _lib.TOKMAP_MAX_TEXT):
            raise ValueError(f"token_maps = {n}: 1 .. {min(T, _lib.TOKMAP_MAX_TEXT)} (the text length) rows")
        return n, None

    def _token_plan(self, prompts, token_maps, n_patches) -> tuple:
        """(token_acc, tokens) of a call's ``token_maps`` argument: per item a zeroed fp32 [n_tok, n_patches[i]]
        accumulator and the token strings of its prompt (``_token_request``); (None, None) when no maps are asked for."""
        if token_maps is None or token_maps is False:
            return None, None
        treq = [self._token_request(p, token_maps) for p in prompts]
        return [torch.zeros(n, p, device=self.device) for (n, _), p in zip(treq, n_patches)], [t for _, t in treq]

    # ------------------------------------------------------------------ query-row maps
    @staticmethod
    def _query_kinds(query_maps) -> tuple:
        """The kinds a call's ``query_maps`` argument names, in QUERY_KINDS' order; () for None / False."""
        if query_maps is None or query_maps is False:
            return ()
        kinds = (query_maps,) if isinstance(query_maps, str) else tuple(query_maps)
        if not kinds or len(set(kinds)) != len(kinds) or any(k not in QUERY_KINDS for k in kinds):
            raise ValueError(f"query_maps = {query_maps!r}: one of {list(QUERY_KINDS)} or a tuple of distinct ones")
        return tuple(k for k in QUERY_KINDS if k in kinds)

    def _query_plan(self, query_maps, prompts, token_maps, concept_counts, n_patches, joint_attention_kwargs=None):
        """query_acc of a call's ``query_maps`` argument: per item a dict kind -> zeroed fp32 [n, n_patches[i]] accumulator
        (n: the item's token count as ``token_maps`` gives it, or its concept count); None when no query maps are asked
        for.  ValueError, before anything is launched, for an unknown kind, "tokens" without ``token_maps`` (which says
        which tokens), and "concepts" with the ablation ``joint_attention_kwargs`` (they change the concept rows' key set)."""
        kinds = self._query_kinds(query_maps)
        if not kinds:
            return None
        if "tokens" in kinds and (token_maps is None or token_maps is False):
            raise ValueError("query_maps: \"tokens\" needs token_maps= (True or a count) to say which tokens")
        jak = joint_attention_kwargs or {}
        if "concepts" in kinds and not (jak.get("concept_cross_attention", True) and jak.get("concept_self_attention", True)):
            raise ValueError("query_maps: \"concepts\" is not covered under the ablation joint_attention_kwargs "
                             "(concept_cross_attention / concept_self_attention = False change the concept rows' key set)")
        for C in concept_counts:
            if "concepts" in kinds and not 1 <= C <= _lib.QUERYMAP_MAX_QUERIES:
                raise ValueError(f"query_maps: {C} concepts; 1 .. {_lib.QUERYMAP_MAX_QUERIES} per item")
        acc = []
        for prompt, C, p in zip(prompts, concept_counts, n_patches):
            d = {}
            if "tokens" in kinds:
                d["tokens"] = torch.zeros(self._token_request(prompt, token_maps)[0], p, device=self.device)
            if "concepts" in kinds:
                d["concepts"] = torch.zeros(C, p, device=self.device)
            acc.append(d)
        return acc

    # ------------------------------------------------------------------ propagated maps
    @staticmethod
    def _propagate_spaces(propagate) -> tuple:
        """The spaces a call's ``propagate`` argument names, in PROPAGATE_SPACES' order; () for None / False."""
        if propagate is None or propagate is False:
            return ()
        spaces = (propagate,) if isinstance(propagate, str) else tuple(propagate)
        if not spaces or len(set(spaces)) != len(spaces) or any(s not in PROPAGATE_SPACES for s in spaces):
            raise ValueError(f"propagate = {propagate!r}: one of {list(PROPAGATE_SPACES)} or a tuple of distinct ones (the "
                             "spaces whose concept maps the call computes)")
        return tuple(s for s in PROPAGATE_SPACES if s in spaces)

    def _propagate_plan(self, propagate, propagate_steps, concept_counts, n_patches, fused: bool = True):
        """prop_acc of a call's ``propagate`` / ``propagate_steps`` arguments: per item (dict space -> zeroed fp32
        [C, n_patches[i]] accumulator, steps); None when no propagated maps are asked for.  ValueError, before anything
        is launched, for an unknown space, steps outside 1 .. 4, an item without concepts or with more than the kernel
        takes, and the stacked route (fused=False keeps no q / k rows to propagate through)."""
        spaces = self._propagate_spaces(propagate)
        if not spaces:
            return None
        if not isinstance(propagate_steps, int) or isinstance(propagate_steps, bool) or not 1 <= propagate_steps <= 4:
            raise ValueError(f"propagate_steps = {propagate_steps!r}: an int in 1 .. 4")
        if not fused:
            raise ValueError("propagate needs the fused route (fused=True)")
        for C in concept_counts:
            if not 1 <= C <= _lib.PROPMAP_MAX_CONCEPTS:
                raise ValueError(f"propagate: {C} concepts; 1 .. {_lib.PROPMAP_MAX_CONCEPTS} per item")
        return [({s: torch.zeros(C, p, device=self.device) for s in spaces}, propagate_steps)
                for C, p in zip(concept_counts, n_patches)]

    # ------------------------------------------------------------------ per-head maps
    def _head_plan(self, head_maps, head_norm, concept_counts, n_patches, normalize_concepts: bool = False):
        """head_acc of a call's ``head_maps`` / ``head_norm`` arguments: per item a ``HeadMapAccumulators`` with zeroed
        accumulators for the asked spaces; None when no head maps are asked for.  ValueError for an unknown space or
        norm name."""
        if head_maps is None or head_maps is False:
            if head_norm is not None:
                raise ValueError("head_norm is the norm of head_maps=; the call asks for no head maps")
            return None
        spaces = (head_maps,) if isinstance(head_maps, str) else tuple(head_maps)
        unknown = [s for s in spaces if s not in HEAD_SPACES]
        if unknown or not spaces or len(set(spaces)) != len(spaces):
            raise ValueError(f"head_maps = {head_maps!r}: one of {list(HEAD_SPACES)} or a tuple of distinct ones")
        names = [head_norm] if head_norm is None or isinstance(head_norm, str) else list(head_norm)
        if not names or len(set(names)) != len(names) or any(n is not None and n not in _lib.NORMS for n in names):
            raise ValueError(f"head_norm = {head_norm!r}: None or one of {list(_lib.NORMS)}, or a sequence of distinct ones")
        if "output" in spaces and self.model.capture_independent_image:
            raise ValueError("head_maps: capture_independent_image=True is not covered by the output-space head maps")
        NH = self.params.num_heads
        for C in concept_counts:
            if not 1 <= C <= _lib.HEATMAP_MAX_CONCEPTS:
                raise ValueError(f"head_maps: {C} concepts; 1 .. {_lib.HEATMAP_MAX_CONCEPTS} per item")
        def one(C, p, name, more=()):
            return HeadMapAccumulators({s: torch.zeros(NH, C, p, device=self.device) for s in spaces},
                                       {s: torch.zeros(C, p, device=self.device) for s in spaces},
                                       None if name is None else _lib.NORMS[name], bool(normalize_concepts), name, more)
        return [one(C, p, names[0], tuple(one(C, p, n) for n in names[1:])) for C, p in zip(concept_counts, n_patches)]

    @staticmethod
    def _device_renderer(return_pil_heatmaps, cmap, heatmap_renderer, heatmap_size, heatmap_interpolation,
                         overlay_alpha) -> tuple:
        """A call's presentation keywords, checked once, as ``_chunk_outputs`` takes them; the first entry is True when
        the pictures are made on the device (heatmap_renderer="device" and PIL heat maps asked for).  ValueError for an
        unknown renderer or interpolation, an alpha outside [0, 1], or a device-only keyword with the host renderer."""
        if heatmap_renderer not in ("host", "device"):
            raise ValueError(f"heatmap_renderer = {heatmap_renderer!r}: \"host\" or \"device\"")
        if heatmap_interpolation not in ("nearest", "bilinear"):
            raise ValueError(f"heatmap_interpolation = {heatmap_interpolation!r}: \"nearest\" or \"bilinear\"")
        if overlay_alpha is not None and not 0.0 <= float(overlay_alpha) <= 1.0:
            raise ValueError(f"overlay_alpha = {overlay_alpha} outside 0..1")
        if heatmap_renderer == "host" and (heatmap_size is not None or heatmap_interpolation != "nearest" or
                                           overlay_alpha is not None):
            raise ValueError("heatmap_size, heatmap_interpolation and overlay_alpha need heatmap_renderer=\"device\"")
        return (heatmap_renderer == "device" and bool(return_pil_heatmaps), return_pil_heatmaps, cmap, heatmap_size,
                heatmap_interpolation, overlay_alpha)

    def _chunk_outputs(self, idx, images, concept_heatmaps, cross_attention_maps, show, token_acc=None, tokens=None,
                       pictures=None, head_acc=None, query_acc=None, prop_acc=None) -> list:
        """The one way out of every call: the ConceptAttentionPipelineOutput of the items ``idx`` of a call after their
        forward.  ``images``: what ``image`` becomes; the two maps [len(idx), C, side, side] on the device; ``show``:
        ``_device_renderer``'s tuple; ``token_acc`` / ``tokens``: the call's (``_token_plan``); ``pictures``: with an
        overlay, the chunk's uint8 [H, W, 3] device tensors the maps are laid over; ``head_acc``: the call's
        (``_head_plan``); ``query_acc``: the call's (``_query_plan``); ``prop_acc``: the call's (``_propagate_plan``)."""
        on_device, return_pil_heatmaps, cmap, heatmap_size, heatmap_interpolation, overlay_alpha = show
        grid = tuple(concept_heatmaps.shape[-2:])
        tok = [None if token_acc is None else token_acc[i].view(-1, *grid) for i in idx]
        tokens = [None if tokens is None else tokens[i] for i in idx]
        # the word maps and the query-row maps: per item, name -> fp32 [n, side, side] on the device ("word": the summed
        # token maps; "q:<kind>": a kind of query_heatmaps; "p:<space>": a space of propagated_heatmaps)
        extras, words = [{} for _ in idx], [None] * len(idx)
        for k, i in enumerate(idx):
            groups = None
            if tokens[k] is not None and tok[k] is not None:
                groups = word_groups(tokens[k])
                words[k] = [w for w, _ in groups]
                extras[k]["word"] = word_maps(tok[k], groups)
            for kind, acc in (query_acc[i] if query_acc is not None and query_acc[i] else {}).items():
                extras[k]["q:" + kind] = acc.view(-1, *grid)
                if kind == "tokens" and groups is not None:
                    extras[k]["q:words"] = word_maps(extras[k]["q:tokens"], groups)
            for space, acc in (prop_acc[i][0] if prop_acc is not None and prop_acc[i] else {}).items():
                extras[k]["p:" + space] = acc.view(-1, *grid)
        if on_device:
            outs = self._finish_device(images, concept_heatmaps, cross_attention_maps, cmap, heatmap_size,
                                       heatmap_interpolation, overlay_alpha, pictures, tok, tokens, extras)
        else:
            outs = [self._finish(images[k], concept_heatmaps[k:k + 1], cross_attention_maps[k:k + 1], return_pil_heatmaps,
                                 cmap, tok[k], tokens[k]) for k in range(len(idx))]
            for out, ex in zip(outs, extras):                # (one global min-max per item and kind, as the token maps)
                for name, maps in ex.items():
                    if return_pil_heatmaps:
                        maps = colorize_heatmaps(maps.to(torch.float32).cpu().numpy(), cmap) if maps.shape[0] else []
                    elif name == "word":
                        maps = maps.to(torch.float32).cpu().numpy()
                    self._set_extra(out, name, maps)
        for out, w in zip(outs, words):
            out.words = w
        if head_acc is not None:
            for out, i in zip(outs, idx):
                out.head_maps, out.raw_heatmaps = head_acc[i].outputs(concept_heatmaps.shape[-1])
        return outs

    @staticmethod
    def _set_extra(out, name: str, maps) -> None:
        """An extra map set of ``_chunk_outputs`` into its output field."""
        if name == "word":
            out.word_heatmaps = maps
        elif name.startswith("p:"):
            out.propagated_heatmaps = dict(out.propagated_heatmaps or {})
            out.propagated_heatmaps[name[2:]] = maps
        else:
            out.query_heatmaps = dict(out.query_heatmaps or {})
            out.query_heatmaps[name[2:]] = maps

    def _input_picture(self, image, height: int, width: int) -> torch.Tensor:
        """The bytes of an encode call's input image on the device, for overlays: uint8 [height, width, 3]."""
        if isinstance(image, torch.Tensor):
            raise ValueError("overlay_alpha needs the input as an image; a latent tensor has no picture to lay the maps over")
        arr = np.asarray(image.convert("RGB"))
        if arr.shape[:2] != (height, width):
            raise ValueError(f"overlay_alpha: the input image is {arr.shape[0]} x {arr.shape[1]} (height x width) and the "
                             f"call asks for {height} x {width}; resize the image first")
        return torch.from_numpy(np.ascontiguousarray(arr)).to(self.device)

    def _finish_device(self, images, concept_heatmaps, cross_attention_maps, cmap, heatmap_size=None,
                       heatmap_interpolation="nearest", overlay_alpha=None, pictures=None, token_maps=None,
                       tokens=None, extras=None) -> list:
        """``_finish`` with PIL heat maps for the B items of a chunk, the pictures made on the device (ops.heatmap_render):
        one group per item and space (the reference's "global min-max over ALL concepts"), one launch, one download of
        bytes.  Without the three options the bytes are those of ``colorize_heatmaps``.  ``pictures``: with
        ``overlay_alpha``, the uint8 [H, W, 3] device tensor of every item that the maps are laid over.  ``token_maps``:
        per item, the prompt-token maps [n_tok, side, side] or None -- one more group per item in the same launch;
        ``tokens``: per item, the token strings.  ``extras``: per item, name -> further maps [n, side, side] (the word maps,
        the query-row maps of every kind): one more group each, behind the token groups, in the same call."""
        import PIL.Image
        ho = concept_heatmaps.to(torch.float32).contiguous()
        hc = cross_attention_maps.to(torch.float32).contiguous()
        B, C, side = ho.shape[0], ho.shape[1], ho.shape[-1]
        if overlay_alpha is not None:
            size = tuple(pictures[0].shape[:2]) if heatmap_size is None else heatmap_size
        else:
            size = (side, side) if heatmap_size is None else heatmap_size
        H, W = (int(size), int(size)) if isinstance(size, int) else (int(v) for v in size)
        if overlay_alpha is not None and any(tuple(p.shape[:2]) != (H, W) for p in pictures):
            raise ValueError(f"overlay_alpha: heatmap_size = {H} x {W} is not the picture's size "
                             f"{tuple(pictures[0].shape[:2])}")
        with_tok = [k for k in range(B) if token_maps is not None and token_maps[k] is not None]
        n_tok = [token_maps[k].shape[0] for k in with_tok]
        more = [(k, name, m.to(torch.float32).contiguous()) for k in range(B) for name, m in (extras[k] if extras else {}).items()
                if m.shape[0]]
        n_more = [m.shape[0] for _, _, m in more]
        # one allocation: the 2 B groups of C planes, then the token groups (n_tok planes each), then the extra groups
        flat = torch.empty((2 * B * C + sum(n_tok) + sum(n_more)) * H * W * 3, dtype=torch.uint8, device=self.device)
        buf = flat[:2 * B * C * H * W * 3].view(2 * B, C, H, W, 3)
        tok_out, o = [], 2 * B * C
        for n in n_tok + n_more:
            tok_out.append(flat[o * H * W * 3:(o + n) * H * W * 3].view(n, H, W, 3))
            o += n
        ops.heatmap_render([ho[k] for k in range(B)] + [hc[k] for k in range(B)] +
                           [token_maps[k].to(torch.float32).contiguous() for k in with_tok] + [m for _, _, m in more],
                           ops.colormap_lut(cmap, self.device),
                           size=(H, W), bilinear=heatmap_interpolation == "bilinear",
                           images=None if overlay_alpha is None else list(pictures) * 2 + [pictures[k] for k in with_tok] +
                           [pictures[k] for k, _, _ in more],
                           alpha=overlay_alpha, out=list(buf) + tok_out)
        host = flat.cpu().numpy()                      # the one download of the chunk
        planes = host.reshape(-1, H, W, 3)
        first = {k: 2 * B * C + sum(n_tok[:i]) for i, k in enumerate(with_tok)}
        outs = self._device_outputs(images, planes, B, C, first, token_maps, tokens)
        o = 2 * B * C + sum(n_tok)
        for k in range(B):                               # (a set without a plane, a prompt without a word: an empty list)
            for name, m in (extras[k] if extras else {}).items():
                if not m.shape[0]:
                    self._set_extra(outs[k], name, [])
        for (k, name, m), n in zip(more, n_more):
            self._set_extra(outs[k], name, [PIL.Image.fromarray(planes[o + t]) for t in range(n)])
            o += n
        return outs

    @staticmethod
    def _device_outputs(images, planes, B, C, first, token_maps, tokens) -> list:
        import PIL.Image
        return [ConceptAttentionPipelineOutput(
            image=images[k], concept_heatmaps=[PIL.Image.fromarray(planes[k * C + c]) for c in range(C)],
            cross_attention_maps=[PIL.Image.fromarray(planes[(B + k) * C + c]) for c in range(C)],
            token_heatmaps=[PIL.Image.fromarray(planes[first[k] + t]) for t in range(token_maps[k].shape[0])]
            if k in first else None,
            tokens=None if tokens is None else tokens[k]) for k in range(B)]

    def _decode(self, x: torch.Tensor, height: int, width: int, with_bytes: bool):
        """(the images of the B items of ``x``, None), or with ``with_bytes`` (PIL images, their uint8 [B, H, W, 3] bytes
        still on the device) for an overlay: one decode either way."""
        if not with_bytes:
            return self.flux_generator.decode_many(x, height, width), None
        import PIL.Image
        pix = self.flux_generator.decode_pixels(x, height, width)
        host = pix.cpu().numpy()
        return [PIL.Image.fromarray(host[k]) for k in range(host.shape[0])], pix

    def _stream_models(self, n_streams: int):
        """One model (activation set on self.model's weights) and one HIP stream per slot, every replica with
        self.model's current settings: a work item computes the same whichever stream it lands on."""
        while len(self._replicas) < n_streams:
            self._replicas.append(HipFluxDiT(self.params, self.device, weights=self.model.weights))
        for r in self._replicas[1:]:
            for name in HipFluxDiT.ROUTE_SETTINGS:
                setattr(r, name, getattr(self.model, name))
        while len(self._streams) < n_streams:
            self._streams.append(torch.cuda.Stream(device=self.device))

    # ------------------------------------------------------------------ generate_image (:115-202)
    @torch.no_grad()
    @on_own_device
    def generate_image(self, prompt: str, concepts: list, width: int = 1024, height: int = 1024,
                       return_cross_attention=False, layer_indices=list(range(15, 19)),
                       return_pil_heatmaps=True, seed: int = 0, num_inference_steps: int = 4,
                       guidance: float = 0.0, timesteps=None, softmax: bool = True,
                       attention_norm: str = "sparsemax", cmap="plasma", latent: Optional[torch.Tensor] = None,
                       fused: bool = True, heatmap_renderer: str = "host", heatmap_size=None,
                       heatmap_interpolation: str = "nearest", overlay_alpha=None,
                       token_maps=None, keep_trace: bool = False, head_maps=None, head_norm=None,
                       head_normalize_concepts: bool = False, query_maps=None, propagate=None,
                       propagate_steps: int = 1) -> ConceptAttentionPipelineOutput:
        """``latent`` (1,16,h/8,w/8) overrides get_noise (device RNG differs between platforms);
        ``fused=False`` takes the reference's route (stack the per-layer vectors, then reduce).
        ``heatmap_renderer="device"`` makes the PIL heat maps on the device (ops.heatmap_render; the same bytes as
        "host", one download of bytes); only with it: ``heatmap_size`` (an int or (H, W)), ``heatmap_interpolation``
        ("nearest" or "bilinear") and ``overlay_alpha`` (the maps blended over the decoded picture with that weight,
        which needs the HIP autoencoder).
        ``token_maps``: True -> ``token_heatmaps`` holds one map per token of the prompt (``tokens``: the tokenizer's
        strings, the end-of-string token excluded): the attention the image tokens give that token's key in the double
        blocks ``layer_indices``, mean over heads, layers and ``timesteps`` (DAAM; ops.token_maps); an int n -> the first
        n text rows, ``tokens`` None.  Needs the fused route.
        ``keep_trace=True``: ``out.trace`` (an ``ImageTrace``) keeps the image side of the steps in ``timesteps`` for
        ``requery``; needs the fused route, bf16 precision and the default ``capture_independent_image``.
        ``head_maps``: "output", "cross" or "value" (or a tuple of them) -> ``out.head_maps[space]`` is the head-resolved
        fp32 device tensor (num_heads, C, h, w) of that space and ``out.raw_heatmaps[space]`` (C, h, w) its mean over the
        heads, both means over ``layer_indices`` and ``timesteps`` (ops.head_maps; the raw-space baselines' maps).
        ``head_norm``: None (the logits themselves), "softmax", "sparsemax" or "entmax15", across the concepts PER HEAD; a
        sequence of several of them computes all in the same forwards and keys both dicts by (space, norm name);
        ``head_normalize_concepts``: heatmaps.linear_normalization across the concepts of the concept rows first.  Needs
        the fused route; "output" makes the forwards take the fp32 image rows' route, as ``keep_trace`` does.
        ``query_maps``: "tokens", "concepts" or both -> ``out.query_heatmaps[kind]``: where the prompt tokens' / the
        concept tokens' own query rows look in the image, the softmax probability each row puts on every image key in the
        double blocks ``layer_indices``, mean over heads, layers and ``timesteps`` (ops.query_maps).  "tokens" needs
        ``token_maps`` to say which tokens; with the token strings ``query_heatmaps["words"]`` holds the words' sums.
        Needs the fused route."""
        if self._query_kinds(query_maps) and not fused:
            raise ValueError("query_maps needs the fused route (fused=True)")
        if keep_trace and not fused:
            raise ValueError("keep_trace needs the fused route: fused=False stacks the vectors and keeps no image side")
        if head_maps and not fused:
            raise ValueError("head_maps needs the fused route (fused=True)")
        if self._propagate_spaces(propagate) and not fused:
            raise ValueError("propagate needs the fused route (fused=True)")
        if fused:   # (repeated timestep or layer indices still end on the stacked route: _generate_steps_inner)
            return self.generate_images(
                [prompt], [concepts], seeds=[seed], latents=None if latent is None else [latent], width=width, height=height,
                return_cross_attention=return_cross_attention, layer_indices=layer_indices, cmap=cmap, timesteps=timesteps,
                return_pil_heatmaps=return_pil_heatmaps, num_inference_steps=num_inference_steps, guidance=guidance,
                softmax=softmax, attention_norm=attention_norm, heatmap_renderer=heatmap_renderer, heatmap_size=heatmap_size,
                heatmap_interpolation=heatmap_interpolation, overlay_alpha=overlay_alpha, token_maps=token_maps,
                keep_trace=keep_trace, head_maps=head_maps, head_norm=head_norm,
                head_normalize_concepts=head_normalize_concepts, query_maps=query_maps, propagate=propagate,
                propagate_steps=propagate_steps)[0]
        norm = self._generate_norm(return_cross_attention, layer_indices, height, width, softmax, attention_norm)
        check_concept_count(norm, len(concepts))
        show = self._device_renderer(return_pil_heatmaps, cmap, heatmap_renderer, heatmap_size, heatmap_interpolation,
                                     overlay_alpha)
        if self._token_request(prompt, token_maps)[0]:
            raise ValueError("token_maps needs the fused route (fused=True)")
        x = latent if latent is not None else sampling.get_noise(1, height, width, self.device, torch.bfloat16, seed)
        txt, vec, con, con_ids, con_vec = self._embed(prompt, concepts)
        img, concept_heatmaps, cross_attention_maps = self.generate_on_device(
            x, txt, vec, con, layer_indices=layer_indices, num_inference_steps=num_inference_steps,
            guidance=guidance, timesteps=timesteps, fused=False, norm=norm)
        images, pix = self._decode(img, height, width, show[0] and overlay_alpha is not None)
        return self._chunk_outputs([0], images, concept_heatmaps, cross_attention_maps, show, pictures=pix)[0]

    def _generate_norm(self, return_cross_attention, layer_indices, height, width, softmax, attention_norm) -> int:
        """The opening checks of a generate call; the resolved norm."""
        assert return_cross_attention is False, "Not supported yet"
        assert all([0 <= li < self.params.depth for li in layer_indices]), "Invalid layer index"
        assert height == width, "Height and width must be the same for now"
        return resolve_norm(softmax, attention_norm)  # ValueError on an unknown name, as the reference (:70-71)

    @torch.no_grad()
    @on_own_device
    def generate_many_on_device(self, items, n_streams: int = 1, batch: int = 1, **kw):
        """Throughput mode for independent work items (dicts with latent/txt/vec/concepts, each with a leading
        batch dimension of 1 and equal shapes).

        ``batch`` items at a time go through ONE forward (one launch per kernel for all of them): the launches then
        hold 5 x 17 = 85 row tiles / 5 x 408 attention workgroups, which fill the 256 CUs to 99.6 % in their last
        round, where a single item leaves 15-20 % of the chip idle in every launch.
        ``n_streams`` groups are kept in flight on separate HIP streams, each with its own activation set and the
        shared weights.  Every item's result is bit-identical to ``generate_on_device`` on that item alone.
        Returns [(img, heat, cross), ...] in item order."""
        groups, n_streams, cur, cat = self._fan_out(items, n_streams, batch)
        results = [None] * len(items)
        for w0 in range(0, len(groups), n_streams):
            wave = groups[w0:w0 + n_streams]
            gens = {}
            for slot, idx in enumerate(wave):
                st = self._streams[slot] if n_streams > 1 else cur
                if n_streams > 1:
                    st.wait_stream(cur)
                with torch.cuda.stream(st):
                    gens[slot] = self._generate_steps(self._replicas[slot], cat(idx, "latent"), cat(idx, "txt"),
                                                      cat(idx, "vec"), cat(idx, "concepts"), **kw)
            alive = dict(gens)
            done = {}
            while alive:
                for slot in list(alive):
                    with torch.cuda.stream(self._streams[slot] if n_streams > 1 else cur):
                        try:
                            next(alive[slot])
                        except StopIteration as stop:
                            done[slot] = stop.value
                            del alive[slot]
            for slot, idx in enumerate(wave):
                img, hm, cm = done[slot]
                if n_streams > 1:
                    self._hand_back(cur, [self._streams[slot]], (img, hm, cm))
                for k, i in enumerate(idx):
                    results[i] = (img[k:k + 1], hm[k:k + 1], cm[k:k + 1])
        return results

    def _fan_out(self, items, n_streams: int, batch: int):
        """The prologue of the two throughput calls: (groups, n_streams, cur, cat) -- the item indices of every forward
        (``batch`` items, at most MAX_ITEMS_PER_FORWARD), the number of streams in use with their models ready
        (``_stream_models``), the caller's stream, and cat(idx, key): the items' ``key`` tensors along the item axis."""
        batch = items_per_forward(batch)
        groups = [list(range(g0, min(g0 + batch, len(items)))) for g0 in range(0, len(items), batch)]
        n_streams = max(1, min(n_streams, len(groups)))
        self._stream_models(n_streams)
        cur = torch.cuda.current_stream(self.device)
        self.model.materialize()  # shared fp8 weight images: built on `cur`, which every side stream waits on
        return groups, n_streams, cur, lambda idx, key: _cat(items[i][key] for i in idx)

    @staticmethod
    def _hand_back(cur, streams, tensors):
        """``cur`` waits for the side ``streams``; the result tensors were allocated there and are consumed on ``cur``."""
        for st in streams:
            cur.wait_stream(st)
        for t in tensors:
            t.record_stream(cur)

    @torch.no_grad()
    @on_own_device
    def generate_on_device(self, latent, txt, vec, concept_embeddings, layer_indices=list(range(15, 19)),
                           num_inference_steps: int = 4, guidance: float = 0.0, timesteps=None, fused: bool = True,
                           norm: int = 0, token_acc=None, traces: Optional[dict] = None, head_acc=None, query_acc=None,
                           prop_acc=None):
        """``token_acc``: per item, an fp32 [n_tok, patches] accumulator of the caller's for the prompt-token maps (zeroed
        by the caller; None, or None for an item: no token maps).  ``traces``: a dict of the caller's that receives step
        index -> the ``StepTrace`` of every step in ``timesteps`` (fused route only).  ``head_acc``: per item, the
        caller's ``HeadMapAccumulators`` (or None).  ``query_acc``: per item, a dict kind ("tokens" | "concepts") -> the caller's
        zeroed fp32 [n, patches] accumulator of that kind's query-row maps (or None).  ``prop_acc``: per item, (dict space
        ("output" | "cross") -> the caller's zeroed fp32 [C, patches] accumulator of that space's propagated maps, steps), or
        None.  The return tuple is the same with and without any of them."""
        gen = self._generate_steps(self.model, latent, txt, vec, concept_embeddings, layer_indices,
                                   num_inference_steps, guidance, timesteps, fused, norm, token_acc, traces, head_acc,
                                   query_acc, prop_acc)
        while True:
            try:
                next(gen)
            except StopIteration as stop:
                return stop.value

    def _generate_steps(self, model, latent, txt, vec, concept_embeddings, layer_indices=list(range(15, 19)),
                        num_inference_steps: int = 4, guidance: float = 0.0, timesteps=None, fused: bool = True,
                        norm: int = 0, token_acc=None, traces: Optional[dict] = None, head_acc=None, query_acc=None,
                        prop_acc=None):
        """The device-resident core of generate_image for B work items at once (B = 1 from the public API):
        latent (B,16,h/8,w/8), txt (B,T,4096), vec (B,768), concept_embeddings (B,C,4096) already in HBM ->
        (final latent tokens, concept heat maps fp32 [B,C,side,side], cross-attention maps fp32
        [B,C,side,side]) on the device, no host synchronisation."""
        if timesteps is None:
            timesteps = list(range(num_inference_steps))
        x = latent.to(self.device, torch.bfloat16)
        schedule = sampling.get_schedule(num_inference_steps, x.shape[-1] * x.shape[-2] // 4,
                                         shift=(not self.is_schnell))
        con, con_ids, con_vec = sampling.concept_inputs(concept_embeddings, vec)
        inp = sampling.prepare_from_embeddings(x, txt, vec)
        C, n_patches = con.shape[1], inp["img"].shape[1]
        # the reference indexes the stacked maps with `timesteps` (concept_attention_pipeline.py:76): an index
        # outside [-steps, steps) is an IndexError there too; negative indices count from the end
        ts = []
        for t in timesteps:
            t = int(t)
            if not -num_inference_steps <= t < num_inference_steps:
                raise IndexError(f"timestep index {t} is out of range for {num_inference_steps} inference steps")
            ts.append(t % num_inference_steps)
        ls = [int(l) for l in layer_indices]
        keep_before = model.keep_bf16_layers
        if model.precision == "fp8" and self.fp8_keep_heatmap_layers:
            # the double blocks whose attention outputs become heat maps stay in bf16: 4 of 57 blocks, no
            # measurable cost, and the maps move from 1.1e-2 to 1.8e-3 of the bf16 path
            model.set_precision("fp8", keep_bf16_layers=ls)
        try:
            return (yield from self._generate_steps_inner(model, x, inp, con, con_ids, con_vec, schedule, ts, ls,
                                                          C, n_patches, guidance, layer_indices, timesteps, fused,
                                                          norm, token_acc, traces, head_acc, query_acc, prop_acc))
        finally:
            model.keep_bf16_layers = keep_before  # this call's choice does not leak into later sweeps / encodes

    def _generate_steps_inner(self, model, x, inp, con, con_ids, con_vec, schedule, ts, ls, C, n_patches, guidance,
                              layer_indices, timesteps, fused, norm=0, token_acc=None, traces=None, head_acc=None,
                              query_acc=None, prop_acc=None):
        names = {v: k for k, v in _lib.NORMS.items()}
        # repeated indices weigh a (step, layer) pair repeatedly in the reference's fancy indexing
        # (concept_attention_pipeline.py:76-77); the fused accumulation covers distinct pairs only
        if fused and (len(set(ts)) != len(ts) or len(set(ls)) != len(ls)):
            fused = False
        if traces is not None and not fused:
            raise ValueError("keep_trace needs the fused route (fused=True, distinct timesteps and layer indices)")
        B = x.shape[0]
        if token_acc is not None and any(t is not None for t in token_acc):
            if not fused:
                raise ValueError("token_maps needs the fused route (fused=True, distinct timesteps and layer indices)")
            if len(token_acc) != B:
                raise ValueError("token_acc: one accumulator (or None) per work item")
        if head_acc is not None:
            if not fused:
                raise ValueError("head_maps needs the fused route (fused=True, distinct timesteps and layer indices)")
            if len(head_acc) != B:
                raise ValueError("head_acc: one HeadMapAccumulators (or None) per work item")
        if query_acc is not None and any(query_acc):
            if not fused:
                raise ValueError("query_maps needs the fused route (fused=True, distinct timesteps and layer indices)")
            if len(query_acc) != B:
                raise ValueError("query_acc: one dict of accumulators (or None) per work item")
        if prop_acc is not None and any(prop_acc):
            if not fused:
                raise ValueError("propagate needs the fused route (fused=True, distinct timesteps and layer indices)")
            if len(prop_acc) != B:
                raise ValueError("prop_acc: one (dict of accumulators, steps) (or None) per work item")
        if fused:
            acc_o = torch.zeros(B, C, n_patches, device=self.device)
            acc_c = torch.zeros(B, C, n_patches, device=self.device)
            reqs = [HeatmapRequest(tuple(ls), 1.0 / (len(ts) * len(ls)), acc_o[j], acc_c[j], norm=norm,
                                   token_space=None if token_acc is None else token_acc[j],
                                   **head_request_fields(head_acc, j), **query_request_fields(query_acc, j),
                                   **propagate_request_fields(prop_acc, j))
                    for j in range(B)]
            img, _, _ = yield from sampling.denoise_steps(
                model, **inp, timesteps=schedule, guidance=guidance, concepts=con, concept_ids=con_ids,
                concept_vec=con_vec, return_intermediate_images=False, return_vectors=False, heatmaps=reqs,
                heatmap_timesteps=ts, traces=traces)
            side = int(round(n_patches ** 0.5))
            return img, acc_o.view(B, C, side, side), acc_c.view(B, C, side, side)
        if B != 1:
            raise NotImplementedError("the stacked (fused=False) route takes one work item at a time")
        img, _, d = yield from sampling.denoise_steps(
            model, **inp, timesteps=schedule, guidance=guidance, concepts=con, concept_ids=con_ids,
            concept_vec=con_vec, return_intermediate_images=False)
        cross_attention_maps = compute_heatmaps_from_vectors(
            d["cross_attention_image_vectors"], d["cross_attention_concept_vectors"],
            layer_indices=layer_indices, timesteps=timesteps, softmax=False, attention_norm=names[norm])
        concept_heatmaps = compute_heatmaps_from_vectors(
            d["output_space_image_vectors"], d["output_space_concept_vectors"],
            layer_indices=layer_indices, timesteps=timesteps, softmax=False, attention_norm=names[norm])
        return img, concept_heatmaps, cross_attention_maps

    # ------------------------------------------------------------------ per-layer x per-noise-level tables
    @torch.no_grad()
    @on_own_device
    def layer_noise_sweep_on_device(self, latent, txt, vec, concept_embeddings, noise_levels, num_steps: int = 50,
                                    layer_indices=None, seed: int = 0, num_samples: int = 1,
                                    rank: int = 0, world: int = 1, batch: int = 1):
        """Concept maps per (noise level, double block): the workload of the reference's per-layer /
        per-timestep segmentation sweeps (experiments/per_layer_segmentation/test_segmentations_per_layer.py:
        104-114,164-189; experiments/per_timestep_segmentation/test_segmentations_per_time.py:75-104) without
        ever materialising the vector stacks.  Every noise level is an independent forward of the 19 double
        blocks from x = t*noise + (1-t)*latent (concept_attention/segmentation.py:85-113), so the levels shard
        over ranks: this rank computes levels rank, rank+world, ...; rows of other ranks stay
        zero and one all_reduce(sum) (distributed.allreduce_sum_) or all_gather completes the table.
        ``batch`` levels at a time share one forward (each level is a work item with its own timestep; per level
        bit-identical to batch = 1).
        noise_levels: indices into get_schedule(num_steps).  Returns (out_space, cross_space), each
        fp32 [len(noise_levels), len(layer_indices), C, side, side]."""
        layer_indices = list(range(self.params.depth)) if layer_indices is None else [int(l) for l in layer_indices]
        latent = latent.to(self.device, torch.bfloat16)
        n_patches = (latent.shape[-1] // 2) * (latent.shape[-2] // 2)
        side = int(round(n_patches ** 0.5))
        con, con_ids, con_vec = sampling.concept_inputs(concept_embeddings, vec)
        C = con.shape[1]
        schedule = sampling.get_schedule(num_steps, n_patches, shift=(not self.is_schnell))
        nl, nlay = len(noise_levels), len(layer_indices)
        out = torch.zeros(nl, nlay, C, n_patches, device=self.device)
        cross = torch.zeros(nl, nlay, C, n_patches, device=self.device)
        height, width = latent.shape[-2] * 8, latent.shape[-1] * 8
        batch = items_per_forward(batch)
        mine = list(range(rank, nl, world))
        for g0 in range(0, len(mine), batch):
            grp = mine[g0:g0 + batch]
            B = len(grp)
            ts = [schedule[int(noise_levels[li])] for li in grp]
            reqs = [HeatmapRequest(tuple(layer_indices), 0.0, None, None, per_layer_out=out[li],
                                   per_layer_cross=cross[li], per_layer_weight=1.0 / num_samples) for li in grp]

            def rep(t):   # the B levels are B work items of the same image
                return t if B == 1 else t.expand(B, *t.shape[1:]).contiguous()
            for s_i in range(num_samples):
                noise = sampling.get_noise(1, height, width, self.device, torch.bfloat16, seed + s_i)
                x = torch.cat([(t * noise.float() + (1.0 - t) * latent.float()).to(torch.bfloat16) for t in ts], 0)
                inp = sampling.prepare_from_embeddings(x, rep(txt), rep(vec))
                cB, idB, vB = sampling.concept_inputs(rep(con), rep(vec))
                self.model(img=inp["img"], img_ids=inp["img_ids"], txt=inp["txt"], txt_ids=inp["txt_ids"],
                           concepts=cB, concept_ids=idB, concept_vec=vB, y=vB,
                           timesteps=ops.host_values(ts, self.device),
                           guidance=torch.zeros(B, device=self.device), stop_after_multimodal_attentions=True,
                           return_vectors=False, heatmaps=reqs)
        return out.view(nl, nlay, C, side, side), cross.view(nl, nlay, C, side, side)

    @torch.no_grad()
    @on_own_device
    def layer_noise_sweep(self, image, concepts: list, prompt: str, noise_levels, num_steps: int = 50, layer_indices=None,
                          num_samples: int = 1, seed: int = 0, width: int = 1024, height: int = 1024, batch: int = 5,
                          vae_noise=None, query_maps=None, propagate=None):
        """``layer_noise_sweep_on_device`` from an image and strings: ``image`` is a latent tensor (1,16,h/8,w/8) or, with
        an autoencoder in the pipeline, a PIL image (``vae_noise`` (1,16,h/8,w/8): its sampling noise, drawn on the
        device when not given); ``concepts`` and ``prompt`` go through the text encoders as in ``encode_image``.
        Returns the two DEVICE tables (out_space, cross_space), fp32 [len(noise_levels), len(layer_indices), C, side,
        side]; ``batch`` levels share one forward.  ``query_maps`` / ``propagate``: refused (the tables hold the concept maps only)."""
        if self._query_kinds(query_maps):
            raise ValueError("layer_noise_sweep: query_maps are not part of the sweep tables (ask encode_image for them)")
        if self._propagate_spaces(propagate):
            raise ValueError("layer_noise_sweep: propagated maps are not part of the sweep tables (the tables take the "
                             "heat-map launch's second accumulator; ask encode_image for them)")
        assert height == width, "Height and width must be the same for now"
        latent = image.to(self.device, torch.bfloat16) if isinstance(image, torch.Tensor) else \
            self._encode_pixels([image], height, width, vae_noise)
        txt, vec, con, _, _ = self._embed(prompt, concepts)
        return self.layer_noise_sweep_on_device(latent, txt, vec, con, [int(v) for v in noise_levels], num_steps=num_steps,
                                                layer_indices=layer_indices, seed=seed, num_samples=num_samples,
                                                batch=batch)

    # ------------------------------------------------------------------ encode_image (:204-357)
    @torch.no_grad()
    @on_own_device
    def encode_image(self, image, concepts: list, prompt: str = "", width: int = 1024, height: int = 1024,
                     layer_indices=list(range(15, 19)), num_samples: int = 1, num_steps: int = 4,
                     noise_timestep: int = 2, device: str = "cuda:0", return_pil_heatmaps: bool = True,
                     seed: int = 0, cmap="plasma", stop_after_multi_modal_attentions=True,
                     attention_norm: str = "sparsemax", softmax=True,
                     joint_attention_kwargs=None, noise=None, vae_noise=None, heatmap_renderer: str = "host",
                     heatmap_size=None, heatmap_interpolation: str = "nearest",
                     overlay_alpha=None, token_maps=None, keep_trace: bool = False, head_maps=None, head_norm=None,
                     head_normalize_concepts: bool = False, query_maps=None, propagate=None,
                       propagate_steps: int = 1) -> ConceptAttentionPipelineOutput:
        """``image``: a latent tensor (1,16,h/8,w/8), or a PIL image when the pipeline has an autoencoder
        (``autoencoder="synthetic"``, a ``.safetensors`` path, or an injected object).
        One forward of the 19 double blocks per noise sample (stop_after_multimodal_attentions).
        ``joint_attention_kwargs`` (not in the reference's signature, which hard-codes None at :296) lets the
        segmentation harness select the concept cross/self-attention ablations; ``noise`` (a list of num_samples
        tensors shaped like the latent) overrides get_noise, whose device RNG stream differs between platforms;
        ``vae_noise`` (1,16,h/8,w/8) is the autoencoder's sampling noise for a PIL image (drawn on the device when not
        given), so that a call is reproducible.  ``heatmap_renderer`` and the three keywords behind it: as in
        ``generate_image``; the overlays are laid over the INPUT image's bytes, which must already be height x width.
        ``token_maps``: as in ``generate_image`` (the mean runs over heads, layers and noise samples).
        ``keep_trace=True``: ``out.trace`` keeps the image side of every noise sample's forward for ``requery`` (its
        step keys are the sample indices).
        ``head_maps`` / ``head_norm`` / ``head_normalize_concepts``: as in ``generate_image`` (the mean runs over layers
        and noise samples); not with the ablation ``joint_attention_kwargs``.
        ``query_maps``: as in ``generate_image`` (the mean runs over heads, layers and noise samples); "concepts" not with
        the ablation ``joint_attention_kwargs``."""
        return self.encode_images(
            [image], [concepts], [prompt], width=width, height=height, layer_indices=layer_indices, num_samples=num_samples,
            num_steps=num_steps, noise_timestep=noise_timestep, seed=seed, noise=None if noise is None else [noise],
            vae_noise=None if vae_noise is None else [vae_noise], return_pil_heatmaps=return_pil_heatmaps, cmap=cmap,
            stop_after_multi_modal_attentions=stop_after_multi_modal_attentions, attention_norm=attention_norm,
            softmax=softmax, joint_attention_kwargs=joint_attention_kwargs, heatmap_renderer=heatmap_renderer,
            heatmap_size=heatmap_size, heatmap_interpolation=heatmap_interpolation, overlay_alpha=overlay_alpha,
            token_maps=token_maps, keep_trace=keep_trace, head_maps=head_maps, head_norm=head_norm,
            head_normalize_concepts=head_normalize_concepts, query_maps=query_maps, propagate=propagate,
                propagate_steps=propagate_steps)[0]

    def _encode_pixels(self, images, height: int, width: int, vae_noise=None) -> torch.Tensor:
        """PIL images -> bf16 latents (B,16,h/8,w/8).  The HIP autoencoder takes the bytes (``encode_pixels``: resize,
        scaling and cast in one kernel per image); an injected object with ``encode`` alone gets the reference's fp32
        image tensor.  ``vae_noise`` (B,16,h/8,w/8) comes to the device as fp32 here, for every caller."""
        if self.autoencoder is None:
            raise ValueError("encode_image needs a latent tensor, or a pipeline built with autoencoder=\"synthetic\", a "
                             ".safetensors path or an object with encode / decode")
        if vae_noise is not None:
            vae_noise = vae_noise.to(self.device, torch.float32)
        arrays = [np.asarray(im.convert("RGB")) for im in images]
        if hasattr(self.autoencoder, "encode_pixels"):
            return self.autoencoder.encode_pixels(arrays, height, width, noise=vae_noise).to(torch.bfloat16)
        xs = []
        for a in arrays:
            arr = torch.from_numpy(a).permute(2, 0, 1).float() / 255.0
            xs.append(torch.nn.functional.interpolate((2.0 * arr - 1.0)[None].to(self.device), (height, width)))
        kw = {} if vae_noise is None else {"noise": vae_noise}
        return self.autoencoder.encode(torch.cat(xs), **kw).to(torch.bfloat16)

    def _encode_maps(self, model, latent, txt, vec, con, con_ids, con_vec, settings: EncodeSettings, *, noise=None,
                     token_acc=None, traces: Optional[dict] = None, head_acc=None, query_acc=None, prop_acc=None):
        """Device core of encode_image for B images at once (latent (B,16,h,w), txt (B,T,4096), ...): one forward
        per noise sample on ``model``; returns the two fp32 maps [B, C, side, side].  ``noise``: optional list of
        num_samples tensors (1 or B,16,h,w) used instead of get_noise(seed + i).  ``token_acc``: per item, the caller's
        zeroed fp32 [n_tok, patches] accumulator of the prompt-token maps (or None); ``traces``: a dict of the caller's that
        receives sample index -> the StepTrace of that sample's forward; ``head_acc``: per item, the caller's
        ``HeadMapAccumulators`` (or None); ``query_acc``: per item, a dict kind -> the caller's zeroed accumulator of the
        query-row maps (or None); ``prop_acc``: per item, (dict space -> the caller's zeroed accumulator of the propagated
        maps, steps) (or None); the return tuple stays."""
        layer_indices, num_samples, noise_timestep = settings.layer_indices, settings.num_samples, settings.noise_timestep
        if noise is not None and len(noise) != num_samples:
            raise ValueError("noise: one tensor per noise sample")
        B, C = con.shape[0], con.shape[1]
        if token_acc is not None and len(token_acc) != B:
            raise ValueError("token_acc: one accumulator (or None) per work item")
        if query_acc is not None and len(query_acc) != B:
            raise ValueError("query_acc: one dict of accumulators (or None) per work item")
        if prop_acc is not None and len(prop_acc) != B:
            raise ValueError("prop_acc: one (dict of accumulators, steps) (or None) per work item")
        n_patches = (latent.shape[-1] // 2) * (latent.shape[-2] // 2)
        height, width = latent.shape[-2] * 8, latent.shape[-1] * 8
        # the reference indexes the stacked samples with the float schedule values
        # (concept_attention_pipeline.py:311), which selects sample 0 only unless
        # a value >= 1; here every sample contributes equally (identical at num_samples=1).
        acc_o = torch.zeros(B, C, n_patches, device=self.device)
        acc_c = torch.zeros(B, C, n_patches, device=self.device)
        req = [HeatmapRequest(tuple(int(l) for l in layer_indices), 1.0 / (num_samples * len(layer_indices)),
                              acc_o[j], acc_c[j], norm=settings.norm, token_space=None if token_acc is None else token_acc[j],
                              **head_request_fields(head_acc, j), **query_request_fields(query_acc, j),
                              **propagate_request_fields(prop_acc, j))
               for j in range(B)]
        schedule = sampling.get_schedule(settings.num_steps, n_patches, shift=(not self.is_schnell))
        for i in range(num_samples):
            # add_noise_to_image (concept_attention/segmentation.py:85-113)
            nz = (noise[i].to(self.device, torch.bfloat16) if noise is not None
                  else sampling.get_noise(1, height, width, self.device, torch.bfloat16, settings.seed + i))
            t = schedule[noise_timestep]
            x = (t * nz.float() + (1.0 - t) * latent.float()).to(torch.bfloat16)
            inp = sampling.prepare_from_embeddings(x, txt, vec)
            t_vec = torch.full((B,), schedule[noise_timestep], device=self.device)
            model(img=inp["img"], img_ids=inp["img_ids"], txt=inp["txt"], txt_ids=inp["txt_ids"],
                  concepts=con, concept_ids=con_ids, concept_vec=con_vec, y=con_vec, timesteps=t_vec,
                  guidance=torch.zeros(B, device=self.device),
                  stop_after_multimodal_attentions=settings.stop_after_multi_modal_attentions,
                  joint_attention_kwargs=settings.joint_attention_kwargs, return_vectors=False, heatmaps=req,
                  **({} if traces is None else {"trace": traces.setdefault(i, StepTrace())}))
        side = int(round(n_patches ** 0.5))
        return acc_o.view(B, C, side, side), acc_c.view(B, C, side, side)

    # ------------------------------------------------------------------ batched calls from pixels and text
    def _text_length(self) -> int:
        enc = self.text_encoder
        return int(getattr(enc, "max_length", getattr(enc, "n_tokens", 0)))

    def _embed_chunk(self, prompts, concepts, idx, n_out: int = 5) -> tuple:
        """The first ``n_out`` of (txt, vec, con, con_ids, con_vec) for the items ``idx`` of a call, along the item axis:
        one text-encoder call (``FluxGenerator.embed_many``)."""
        emb = self.flux_generator.embed_many([prompts[i] for i in idx], [concepts[i] for i in idx])
        return tuple(_cat(e[k] for e in emb) for k in range(n_out))

    def _encode_chunks(self, images, concepts, prompts, settings: EncodeSettings, *, noise=None, vae_noise=None,
                       token_acc=None, keep_trace: bool = False, head_acc=None, query_acc=None, prop_acc=None):
        """The forwards of ``encode_images``, one at a time: yields (item indices, acc_o, acc_c) with the two fp32 maps
        [len(indices), C, side, side] of the chunk still on the device (``_encode_maps``).  ``images`` and ``prompts`` are lists;
        ``settings`` was built with the call's largest concept count; ``noise`` / ``vae_noise``: as ``encode_images`` takes them;
        ``token_acc``: per item of the call, the caller's accumulator of the prompt-token maps (or None).  With
        ``keep_trace`` a fourth entry follows: sample index -> the StepTrace of the chunk's forward.  ``head_acc``: per item
        of the call, its ``HeadMapAccumulators`` (or None for the call); ``query_acc``: per item of the call, its dict of
        query-row accumulators (or None for the call); ``prop_acc``: per item of the call, its propagated-map accumulators
        (or None for the call)."""
        n, height, width = len(images), settings.height, settings.width
        concepts = _per_item(concepts, n, "encode_images: concepts")
        for name, v in (("prompts", prompts), ("noise", noise), ("vae_noise", vae_noise)):
            if v is not None and len(v) != n:
                raise ValueError(f"encode_images: {name} has {len(v)} entries for {n} images")
        shapes = [tuple(im.shape[1:]) if isinstance(im, torch.Tensor) else (16, height // 8, width // 8) for im in images]
        for idx in plan_batches([(shapes[i], len(concepts[i]), self._text_length()) for i in range(n)], settings.batch):
            txt, vec, con, con_ids, con_vec = self._embed_chunk(prompts, concepts, idx)
            pil = [i for i in idx if not isinstance(images[i], torch.Tensor)]
            lat = {}
            if pil:
                enc = self._encode_pixels([images[i] for i in pil], height, width,
                                          None if vae_noise is None else _cat(vae_noise[i] for i in pil))
                lat = {i: enc[k:k + 1] for k, i in enumerate(pil)}
            latent = _cat(lat[i] if i in lat else images[i].to(self.device, torch.bfloat16) for i in idx)
            if noise is not None and any(len(noise[i]) != settings.num_samples for i in idx):
                raise ValueError("noise: one tensor per noise sample")
            nz = None if noise is None else [_cat(noise[i][s_].to(self.device, torch.bfloat16) for i in idx)
                                             for s_ in range(settings.num_samples)]
            traces = {} if keep_trace else None
            ho, hc = self._encode_maps(self.model, latent, txt, vec, con, con_ids, con_vec, settings, noise=nz,
                                       token_acc=None if token_acc is None else [token_acc[i] for i in idx], traces=traces,
                                       head_acc=None if head_acc is None else [head_acc[i] for i in idx],
                                       query_acc=None if query_acc is None else [query_acc[i] for i in idx],
                                       prop_acc=None if prop_acc is None else [prop_acc[i] for i in idx])
            yield (idx, ho, hc, traces) if keep_trace else (idx, ho, hc)

    @torch.no_grad()
    @on_own_device
    def encode_images(self, images, concepts, prompts, width: int = 1024, height: int = 1024,
                      layer_indices=list(range(15, 19)), num_samples: int = 1, num_steps: int = 4,
                      noise_timestep: int = 2, seed: int = 0, batch: int = 5, noise=None, vae_noise=None,
                      return_pil_heatmaps: bool = True, cmap="plasma", stop_after_multi_modal_attentions=True,
                      attention_norm: str = "sparsemax", softmax=True, joint_attention_kwargs=None,
                      heatmap_renderer: str = "host", heatmap_size=None, heatmap_interpolation: str = "nearest",
                      overlay_alpha=None, token_maps=None, keep_trace: bool = False, head_maps=None, head_norm=None,
                      head_normalize_concepts: bool = False, query_maps=None, propagate=None,
                       propagate_steps: int = 1) -> list:
        """``encode_image`` for a list of images: a list of ConceptAttentionPipelineOutput in item order, every item with
        the maps of its own ``encode_image`` call.  ``images``: PIL images and / or latents (1,16,h/8,w/8);
        ``concepts``: one list for all items or one list per item; ``prompts``: one string per item (or one for all).
        Items that share a latent shape and a concept count go ``batch`` (at most 5) at a time through one text-encoder
        call (``FluxGenerator.embed_many``), one autoencoder pass (``AutoEncoder.encode_pixels``) and one forward.
        ``noise``: per item, what ``encode_image`` takes (a list of num_samples tensors); ``vae_noise``: per item, a
        tensor (1,16,h/8,w/8) -- without it the autoencoder draws one batch of noise per forward, so PIL items are then
        reproducible per call of this method, not against single calls.  ``heatmap_renderer="device"``: the pictures of
        a chunk come from one launch and one download (``_finish_device``).  ``token_maps``: as in ``encode_image``, for
        every item's own prompt (the items of a chunk may have different numbers of tokens).  ``keep_trace``: as in
        ``encode_image``, per item.  ``head_maps`` / ``head_norm`` / ``head_normalize_concepts``: as in ``encode_image``,
        per item.  ``query_maps``: as in ``encode_image``, per item; one ops.query_maps launch per captured layer and
        forward for all items and kinds."""
        if keep_trace:
            self.model._check_traceable("keep_trace", joint_attention_kwargs)
        images = list(images)
        n = len(images)
        prompts = [prompts] * n if isinstance(prompts, str) else list(prompts)
        concepts = _per_item(concepts, n, "encode_images: concepts")
        settings = EncodeSettings(layer_indices, num_samples, num_steps, noise_timestep, seed, width, height, batch,
                                  stop_after_multi_modal_attentions, joint_attention_kwargs, attention_norm, softmax,
                                  depth=self.params.depth, n_concepts=max((len(c) for c in concepts), default=0))
        show = self._device_renderer(return_pil_heatmaps, cmap, heatmap_renderer, heatmap_size, heatmap_interpolation,
                                     overlay_alpha)
        token_acc, tokens = self._token_plan(prompts, token_maps, [
            (im.shape[-1] // 2) * (im.shape[-2] // 2) if isinstance(im, torch.Tensor) else (height // 16) * (width // 16)
            for im in images])
        pictures = [self._input_picture(im, height, width) for im in images] if show[0] and overlay_alpha is not None \
            else None
        head_acc = self._head_plan(head_maps, head_norm, [len(c) for c in concepts], [
            (im.shape[-1] // 2) * (im.shape[-2] // 2) if isinstance(im, torch.Tensor) else (height // 16) * (width // 16)
            for im in images], head_normalize_concepts)
        query_acc = self._query_plan(query_maps, prompts, token_maps, [len(c) for c in concepts], [
            (im.shape[-1] // 2) * (im.shape[-2] // 2) if isinstance(im, torch.Tensor) else (height // 16) * (width // 16)
            for im in images], joint_attention_kwargs)
        prop_acc = self._propagate_plan(propagate, propagate_steps, [len(c) for c in concepts], [
            (im.shape[-1] // 2) * (im.shape[-2] // 2) if isinstance(im, torch.Tensor) else (height // 16) * (width // 16)
            for im in images])
        results = {}
        for idx, ho, hc, *traces in self._encode_chunks(images, concepts, prompts, settings, noise=noise,
                                                        vae_noise=vae_noise, token_acc=token_acc, keep_trace=keep_trace,
                                                        head_acc=head_acc, query_acc=query_acc, prop_acc=prop_acc):
            outs = self._chunk_outputs(idx, [images[i] for i in idx], ho, hc, show, token_acc, tokens,
                                       None if pictures is None else [pictures[i] for i in idx], head_acc, query_acc,
                                       prop_acc)
            if keep_trace:
                self._attach_traces(outs, traces[0], dict(
                    call="encode_image", width=width, height=height, layer_indices=list(layer_indices),
                    num_samples=num_samples, num_steps=num_steps, noise_timestep=noise_timestep, seed=seed,
                    timesteps=sorted(traces[0])))
            results.update(zip(idx, outs))
        return [results[i] for i in range(n)]

    @torch.no_grad()
    @on_own_device
    def generate_images(self, prompts, concepts, seeds=None, latents=None, width: int = 1024, height: int = 1024,
                        return_cross_attention=False, layer_indices=list(range(15, 19)), return_pil_heatmaps=True,
                        num_inference_steps: int = 4, guidance: float = 0.0, timesteps=None, softmax: bool = True,
                        attention_norm: str = "sparsemax", cmap="plasma", batch: int = 5,
                        heatmap_renderer: str = "host", heatmap_size=None, heatmap_interpolation: str = "nearest",
                        overlay_alpha=None, token_maps=None, keep_trace: bool = False, head_maps=None, head_norm=None,
                        head_normalize_concepts: bool = False, query_maps=None, propagate=None,
                       propagate_steps: int = 1) -> list:
        """``generate_image`` for a list of prompts: a list of ConceptAttentionPipelineOutput in item order, every item
        with the image and maps of its own ``generate_image(prompt, concepts, seed=seeds[i], latent=latents[i])`` call on
        the fused route.  ``concepts``: one list for all items or one list per item; ``seeds``: one per item (default
        0, 1, 2, ...).  Items with one concept count go ``batch`` (at most 5) at a time through one text-encoder call,
        one denoising loop and one autoencoder pass whose bytes are made on the device.  ``token_maps``: as in
        ``generate_image``, for every item's own prompt (the items of a chunk may have different numbers of tokens).
        ``keep_trace``: as in ``generate_image``; every item's ``trace`` is its own view of its forward's storage.
        ``head_maps`` / ``head_norm`` / ``head_normalize_concepts``: as in ``generate_image``, per item.
        ``query_maps``: as in ``generate_image``, per item."""
        norm = self._generate_norm(return_cross_attention, layer_indices, height, width, softmax, attention_norm)
        if keep_trace:
            self.model._check_traceable("keep_trace")
        show = self._device_renderer(return_pil_heatmaps, cmap, heatmap_renderer, heatmap_size, heatmap_interpolation,
                                     overlay_alpha)
        prompts = list(prompts)
        n = len(prompts)
        concepts = _per_item(concepts, n, "generate_images: concepts")
        check_concept_count(norm, max((len(c) for c in concepts), default=0))
        seeds = list(range(n)) if seeds is None else list(seeds)
        for name, v in (("seeds", seeds), ("latents", latents)):
            if v is not None and len(v) != n:
                raise ValueError(f"generate_images: {name} has {len(v)} entries for {n} prompts")
        shapes = [(16, height // 8, width // 8) if latents is None else tuple(latents[i].shape[1:]) for i in range(n)]
        token_acc, tokens = self._token_plan(prompts, token_maps, [(s[1] // 2) * (s[2] // 2) for s in shapes])
        head_acc = self._head_plan(head_maps, head_norm, [len(c) for c in concepts],
                                   [(s[1] // 2) * (s[2] // 2) for s in shapes], head_normalize_concepts)
        query_acc = self._query_plan(query_maps, prompts, token_maps, [len(c) for c in concepts],
                                     [(s[1] // 2) * (s[2] // 2) for s in shapes])
        prop_acc = self._propagate_plan(propagate, propagate_steps, [len(c) for c in concepts],
                                        [(s[1] // 2) * (s[2] // 2) for s in shapes])
        if prop_acc is not None:
            ts = list(range(num_inference_steps)) if timesteps is None else [int(t) % max(num_inference_steps, 1) for t in timesteps]
            if len(set(ts)) != len(ts) or len(set(int(l) for l in layer_indices)) != len(list(layer_indices)):
                raise ValueError("propagate needs the fused route (fused=True, distinct timesteps and layer indices)")
        if query_acc is not None:
            ts = list(range(num_inference_steps)) if timesteps is None else [int(t) % max(num_inference_steps, 1) for t in timesteps]
            if len(set(ts)) != len(ts) or len(set(int(l) for l in layer_indices)) != len(list(layer_indices)):
                raise ValueError("query_maps needs the fused route (fused=True, distinct timesteps and layer indices)")
        results = {}
        for idx in plan_batches([(shapes[i], len(concepts[i]), self._text_length()) for i in range(n)], batch):
            txt, vec, con = self._embed_chunk(prompts, concepts, idx, 3)
            x = _cat(latents[i].to(self.device, torch.bfloat16) if latents is not None else
                     sampling.get_noise(1, height, width, self.device, torch.bfloat16, seeds[i]) for i in idx)
            traces = {} if keep_trace else None
            img, ho, hc = self.generate_on_device(x, txt, vec, con, layer_indices=layer_indices,
                                                  num_inference_steps=num_inference_steps, guidance=guidance,
                                                  timesteps=timesteps, fused=True, norm=norm,
                                                  token_acc=None if token_acc is None else [token_acc[i] for i in idx],
                                                  traces=traces,
                                                  head_acc=None if head_acc is None else [head_acc[i] for i in idx],
                                                  query_acc=None if query_acc is None else [query_acc[i] for i in idx],
                                                  prop_acc=None if prop_acc is None else [prop_acc[i] for i in idx])
            pictures, pix = self._decode(img, height, width, show[0] and overlay_alpha is not None)
            outs = self._chunk_outputs(idx, pictures, ho, hc, show, token_acc, tokens, pix, head_acc, query_acc, prop_acc)
            if keep_trace:
                self._attach_traces(outs, traces, dict(
                    call="generate_image", width=width, height=height, layer_indices=list(layer_indices),
                    num_inference_steps=num_inference_steps, guidance=guidance, timesteps=sorted(traces)))
            results.update(zip(idx, outs))
        return [results[i] for i in range(n)]

    @staticmethod
    def _attach_traces(outs, traces: dict, settings: dict) -> None:
        """``out.trace`` of every item of a chunk: ``traces`` maps a step key to the StepTrace of the chunk's forward."""
        views = {k: t.items() for k, t in traces.items()}
        for j, out in enumerate(outs):
            out.trace = ImageTrace({k: v[j] for k, v in views.items()}, dict(settings), out.image)

    # ------------------------------------------------------------------ concept re-query
    @torch.no_grad()
    @on_own_device
    def requery(self, trace, concepts, layer_indices=None, timesteps=None, softmax: bool = True,
                attention_norm: str = "sparsemax", cmap="plasma", return_pil_heatmaps: bool = True,
                heatmap_renderer: str = "host", heatmap_size=None, heatmap_interpolation: str = "nearest",
                overlay_alpha=None, query_maps=None, propagate=None):
        """Other concepts for a finished ``keep_trace=True`` call, without its image pass: only the concept rows' stream
        through the double blocks runs, against the image keys, values and map operands the trace kept
        (``HipFluxDiT.requery``).  ``trace``: an ``ImageTrace`` (-> one ConceptAttentionPipelineOutput) or a list of them
        (-> a list, in item order); ``concepts``: one list of strings for all items or one list per item, any count
        (sparse norms: at most 32), embedded as ``embed_many`` embeds them.  ``layer_indices`` / ``timesteps``: any subset
        of the traced ones (default: all of them; for an encode trace the steps are its noise-sample indices); the maps
        are the mean over that subset.  The other keywords: as in ``generate_image``; overlays are laid over the trace's
        ``image``.  The output carries the trace's ``image`` and no token maps (the text side has not changed).  Items
        that share a geometry and a concept count go through one pass, at most 5 at a time (``plan_requery``)."""
        if self._query_kinds(query_maps):
            raise ValueError("requery: query_maps are not part of a re-query (the trace keeps no text q rows, and the concept "
                             "rows' query maps are asked for in the forward)")
        if self._propagate_spaces(propagate):
            raise ValueError("requery: propagated maps are not part of a re-query (a trace keeps no image q rows; ask for "
                             "them in the call that makes the image)")
        single = isinstance(trace, ImageTrace)
        traces = [trace] if single else list(trace)
        n = len(traces)
        concepts = _per_item(concepts, n, "requery: concepts")
        norm = resolve_norm(softmax, attention_norm)
        check_concept_count(norm, max((len(c) for c in concepts), default=0))
        show = self._device_renderer(return_pil_heatmaps, cmap, heatmap_renderer, heatmap_size, heatmap_interpolation,
                                     overlay_alpha)
        self.model._check_traceable("requery")
        plans = []
        for i, t in enumerate(traces):
            if t.released or any(s.released for s in t.steps.values()):
                raise ValueError(f"requery: trace {i} has been released")
            if any(s.model is not self.model for s in t.steps.values()):
                raise ValueError(f"requery: trace {i} comes from another model object")
            if not concepts[i]:
                raise ValueError("requery: at least one concept per item")
            ls = t.layer_indices if layer_indices is None else [int(l) for l in layer_indices]
            if any(l not in t.layer_indices for l in ls):
                raise ValueError(f"requery: layer_indices {ls} lie outside trace {i} (traced layers {t.layer_indices})")
            steps = t.settings.get("num_inference_steps")
            ts = t.timesteps if timesteps is None else [int(s) % steps if steps else int(s) for s in timesteps]
            if any(s not in t.steps for s in ts):
                raise ValueError(f"requery: timesteps {ts} lie outside trace {i} (traced steps {t.timesteps})")
            if len(set(ls)) != len(ls) or len(set(ts)) != len(ts) or not ls or not ts:
                raise ValueError("requery: layer_indices and timesteps are non-empty lists of distinct entries")
            s0 = t.steps[ts[0]]
            plans.append((ls, ts, (s0.L, s0.layers, tuple(s0.split), tuple(s0.qk16), tuple(ls), tuple(ts))))
        pictures = None
        if show[0] and overlay_alpha is not None:
            if any(not hasattr(t.image, "convert") for t in traces):
                raise ValueError("overlay_alpha needs traces whose image is a picture (a pipeline with an autoencoder)")
            pictures = [self._input_picture(t.image, *t.image.size[::-1]) for t in traces]
        results = {}
        for idx in plan_requery([p[2] for p in plans], [len(c) for c in concepts]):
            ls, ts, _ = plans[idx[0]]
            emb = self.flux_generator.embed_concepts_many([concepts[i] for i in idx])
            con, con_ids = _cat(e[0] for e in emb), _cat(e[1] for e in emb)
            B, C, n_patches = len(idx), con.shape[1], traces[idx[0]].steps[ts[0]].L
            acc_o = torch.zeros(B, C, n_patches, device=self.device)
            acc_c = torch.zeros(B, C, n_patches, device=self.device)
            reqs = [HeatmapRequest(tuple(ls), 1.0 / (len(ts) * len(ls)), acc_o[j], acc_c[j], norm=norm) for j in range(B)]
            for s in ts:
                self.model.requery([traces[i].steps[s] for i in idx], con, con_ids, reqs)
            side = int(round(n_patches ** 0.5))
            outs = self._chunk_outputs(idx, [traces[i].image for i in idx], acc_o.view(B, C, side, side),
                                       acc_c.view(B, C, side, side), show,
                                       pictures=None if pictures is None else [pictures[i] for i in idx])
            results.update(zip(idx, outs))
        out = [results[i] for i in range(n)]
        return out[0] if single else out

    @torch.no_grad()
    @on_own_device
    def encode_many_on_device(self, items, n_streams: int = 1, batch: int = 1, layer_indices=list(range(15, 19)),
                              num_samples: int = 1, num_steps: int = 4, noise_timestep: int = 2, seed: int = 0,
                              noise=None):
        """Batch form of encode_image for independent images (the loop of
        experiments/imagenet_segmentation/run_experiment.py:137; BASELINE.json configs[3]): ``items`` are dicts with
        latent (1,16,h/8,w/8), txt (1,T,4096), vec (1,768), concepts (1,C,4096) already on the device; they are
        dealt round-robin to ``n_streams`` HIP streams, each with its own activation set (the same throughput
        mode as generate_many_on_device).  Returns [(heat [1,C,s,s], cross [1,C,s,s]), ...], identical to
        encoding the items one by one."""
        settings = EncodeSettings(layer_indices, num_samples, num_steps, noise_timestep, seed)
        groups, n_streams, cur, cat = self._fan_out(items, n_streams, batch)
        for st in self._streams[:n_streams]:
            st.wait_stream(cur)
        results = [None] * len(items)
        for gi, idx in enumerate(groups):   # ``batch`` images share every launch of a forward (see generate_many)
            slot = gi % n_streams
            with torch.cuda.stream(self._streams[slot]):
                latent = cat(idx, "latent").to(self.device, torch.bfloat16)
                con, con_ids, con_vec = sampling.concept_inputs(cat(idx, "concepts"), cat(idx, "vec"))
                ho, hc = self._encode_maps(self._replicas[slot], latent, cat(idx, "txt"), cat(idx, "vec"), con, con_ids,
                                           con_vec, settings, noise=noise)
                for k, i in enumerate(idx):
                    results[i] = (ho[k:k + 1], hc[k:k + 1])
        self._hand_back(cur, self._streams[:n_streams], [t for pair in results for t in pair])
        return results
