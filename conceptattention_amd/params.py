"""Model geometry for the Flux DiT the ConceptAttention path runs on.

Mirrors ``FluxParams`` (reference concept_attention/modified_flux_dit.py:13-26) and the two
``configs[*].params`` entries of concept_attention/flux/src/flux/util.py:28-93.  The only
difference between flux-schnell and flux-dev is ``guidance_embed`` (util.py:46 vs :78).
"""
from __future__ import annotations

from dataclasses import dataclass, replace


@dataclass(frozen=True)
class FluxParams:
    in_channels: int = 64
    vec_in_dim: int = 768
    context_in_dim: int = 4096
    hidden_size: int = 3072
    mlp_ratio: float = 4.0
    num_heads: int = 24
    depth: int = 19
    depth_single_blocks: int = 38
    axes_dim: tuple = (16, 56, 56)
    theta: int = 10_000
    qkv_bias: bool = True
    guidance_embed: bool = False

    def __post_init__(self):
        # same guards as ModifiedFluxDiT.__init__ (modified_flux_dit.py:40-46)
        if self.hidden_size % self.num_heads != 0:
            raise ValueError(
                f"Hidden size {self.hidden_size} must be divisible by num_heads {self.num_heads}")
        pe_dim = self.hidden_size // self.num_heads
        if sum(self.axes_dim) != pe_dim:
            raise ValueError(f"Got {list(self.axes_dim)} but expected positional dim {pe_dim}")

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_heads

    @property
    def mlp_hidden(self) -> int:
        return int(self.hidden_size * self.mlp_ratio)


configs = {
    "flux-schnell": FluxParams(guidance_embed=False),
    "flux-dev": FluxParams(guidance_embed=True),
}


@dataclass(frozen=True)
class AutoEncoderParams:
    """Fields of the reference's AutoEncoderParams (flux/modules/autoencoder.py:8-18)."""
    resolution: int = 256
    in_channels: int = 3
    ch: int = 128
    out_ch: int = 3
    ch_mult: tuple = (1, 2, 4, 4)
    num_res_blocks: int = 2
    z_channels: int = 16
    scale_factor: float = 0.3611
    shift_factor: float = 0.1159


# flux/util.py:49-58,81-90: both models ship the same autoencoder
ae_params = {"flux-schnell": AutoEncoderParams(), "flux-dev": AutoEncoderParams()}

@dataclass(frozen=True)
class T5Params:
    """The encoder-side fields of transformers' T5Config; the defaults are google/t5-v1_1-xxl, the checkpoint the
    reference loads (flux/util.py load_t5, flux/modules/conditioner.py:6-38): gated GELU (tanh form), RMS layer norm
    without bias, no bias in any projection, relative-position buckets shared by all blocks."""
    vocab_size: int = 32128
    d_model: int = 4096
    d_kv: int = 64
    num_heads: int = 64
    d_ff: int = 10240
    num_layers: int = 24
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    layer_norm_epsilon: float = 1e-6

    @property
    def inner_dim(self) -> int:
        return self.num_heads * self.d_kv


t5_params = {"t5-v1_1-xxl": T5Params()}


def tiny_t5_params(**kw) -> T5Params:
    """The smallest geometry that still has every structure of the encoder (two blocks, several heads, d_ff != d_model)
    and meets the GEMM's rules (every projection width a multiple of 256, every depth a multiple of 64)."""
    base = dict(vocab_size=512, d_model=256, num_heads=4, d_ff=512, num_layers=2)
    base.update(kw)
    return replace(T5Params(), **base)


@dataclass(frozen=True)
class ClipTextParams:
    """The text-model fields of transformers' CLIPTextConfig; the defaults are openai/clip-vit-large-patch14, the
    checkpoint the reference loads (flux/util.py load_clip, max_length 77): pre-norm blocks, LayerNorm with bias, a bias
    in every projection, quick_gelu, learned position embeddings, a causal mask.  ``eos_token_id`` is 2 in the published
    config (the end-of-text token is 49407): transformers then pools at the first arg-max of the ids, and at the first
    position equal to ``eos_token_id`` for any other value."""
    vocab_size: int = 49408
    hidden_size: int = 768
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    max_position_embeddings: int = 77
    layer_norm_eps: float = 1e-5
    eos_token_id: int = 2

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads


clip_params = {"clip-vit-large-patch14": ClipTextParams()}


def tiny_clip_params(**kw) -> ClipTextParams:
    """The smallest geometry that still has every structure of the text model (two layers, several heads of 64,
    intermediate != hidden) and meets the GEMM's rules (every projection width a multiple of 256)."""
    base = dict(vocab_size=512, hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=2)
    base.update(kw)
    return replace(ClipTextParams(), **base)


# T5 sequence length per model (reference concept_attention/image_generator.py:57)
T5_TOKENS = {"flux-schnell": 256, "flux-dev": 512}


def tiny_params(**kw) -> FluxParams:
    """Small geometry for CPU-checkable tests; keeps head_dim == sum(axes_dim) == 128, which
    the HIP kernels (and the reference's EmbedND check) require."""
    base = dict(hidden_size=256, num_heads=2, depth=2, depth_single_blocks=2)
    base.update(kw)
    return replace(FluxParams(), **base)
