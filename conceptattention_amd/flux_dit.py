"""HipFluxDiT: the modified Flux DiT forward (concept-token stream included) on MI355X.

Host-side mirror of the reference's model object for this path:
  * ``ModifiedFluxDiT.forward``              concept_attention/modified_flux_dit.py:75-163
  * ``ModifiedDoubleStreamBlock.forward``    concept_attention/modified_double_stream_block.py:69-204
  * ``ModifiedSingleStreamBlock.forward``    concept_attention/modified_single_stream_block.py:43-56
It keeps the call contract ``denoise`` (flux/sampling.py:126-139) and ``encode_image``
(concept_attention_pipeline.py:284-297) rely on -- same keyword names, ``(pred | None, dict)``
return value with the four reference keys stacked over the double blocks -- so it can be passed
wherever the reference takes a ``dit_class`` instance.  All arithmetic runs in the gfx950
kernels of libconceptattn.so (conceptattention_amd.ops); PyTorch provides device memory only.

Data layout in HBM (one resident activation set per model instance, batch 1):
  X    [C+T+L, H]   fp32 residual streams, rows = [concept tokens | text tokens | image tokens]
  XM   [C+T+L, H]   LayerNorm+modulated input of the next projection
  QKV  [C+T+L, 3H]  projection output, q|k|v thirds, head-major inside a third
  ATT  [C+T+L, H]   attention output, head-concatenated
  HID  [C+T+L, 4H]  MLP hidden of the double blocks
  CAT  [T+L, 5H]    single blocks: [attention | gelu(mlp)] input of linear2
With this row order the text-weight projections see [concepts|text] as one contiguous matrix
(the concept stream re-uses the text weights, modified_double_stream_block.py:100-104), the
single blocks see [text|image] as one contiguous matrix (modified_flux_dit.py:149), and the
concept attention reads [concept keys | image keys] as two row segments without any copy.
"""
from __future__ import annotations

import math

from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch

from . import _lib as L
from . import ops
from .heatmaps import check_concept_count, linear_normalization
from .params import FluxParams
from .weights import iter_synthetic_state_dict, state_dict_spec

def on_own_device(fn):
    """Run a method with ``self.device`` as the current HIP device: the kernels launch on the calling thread's
    current device and stream, so an object built for cuda:1 must not depend on the caller's current device."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *a, **k):
        with torch.cuda.device(self.device):
            return fn(self, *a, **k)
    return wrapped


DICT_KEYS = (
    "output_space_concept_vectors",
    "output_space_image_vectors",
    "cross_attention_concept_vectors",
    "cross_attention_image_vectors",
)


class FluxWeights:
    """bf16 device weights under the BFL state-dict names.  The adaLN modulation matrices of all
    blocks live in ONE stacked buffer so a diffusion step computes every block's
    shift/scale/gate with a single weight-streaming launch."""

    def __init__(self, params: FluxParams, device):
        self.params = params
        self.device = torch.device(device)
        H = params.hidden_size
        self.tensors: dict[str, torch.Tensor] = {}
        self.fp8 = None  # name -> (e4m3 bytes, fp32 row scales) of the large projections, built on first fp8 use
        mod_names = []
        for i in range(params.depth):
            mod_names += [(f"double_blocks.{i}.img_mod.lin", 6 * H), (f"double_blocks.{i}.txt_mod.lin", 6 * H)]
        for i in range(params.depth_single_blocks):
            mod_names.append((f"single_blocks.{i}.modulation.lin", 3 * H))
        mod_names.append(("final_layer.adaLN_modulation.1", 2 * H))
        self.mod_offset: dict[str, int] = {}
        off = 0
        for name, n in mod_names:
            self.mod_offset[name] = off
            off += n
        self.mod_rows = off
        self.mod_w = torch.empty(off, H, device=self.device, dtype=torch.bfloat16)
        self.mod_b = torch.empty(off, device=self.device, dtype=torch.bfloat16)
        for name, shape in state_dict_spec(params):
            base, kind = name.rsplit(".", 1)
            if base in self.mod_offset:
                o = self.mod_offset[base]
                src = self.mod_w if kind == "weight" else self.mod_b
                self.tensors[name] = src[o:o + shape[0]]
            else:
                self.tensors[name] = torch.empty(shape, device=self.device, dtype=torch.bfloat16)

    def __getitem__(self, name: str) -> torch.Tensor:
        return self.tensors[name]

    def state_dict(self) -> dict[str, torch.Tensor]:
        return dict(self.tensors)

    def load_state_dict(self, sd, strict: bool = True):
        """Copy tensors in (any float dtype / device).  Same (missing, unexpected) semantics as
        nn.Module.load_state_dict (the reference calls it with strict=False,
        concept_attention/image_generator.py:44)."""
        self.fp8 = None
        missing = [k for k in self.tensors if k not in sd]
        unexpected = [k for k in sd if k not in self.tensors]
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing {missing[:4]}.. unexpected {unexpected[:4]}..")
        for k, t in self.tensors.items():
            if k in sd:
                if tuple(sd[k].shape) != tuple(t.shape):
                    raise RuntimeError(f"load_state_dict: {k} has shape {tuple(sd[k].shape)}, expected {tuple(t.shape)}")
                t.copy_(sd[k])
        return missing, unexpected

    def init_synthetic(self, seed: int = 0, on_device: bool = True):
        """Random-init weights of the right geometry.  on_device=True draws on
        the GPU (fast, 23.8 GB for full Flux); False draws on the CPU generator so the values
        are identical to ``weights.synthetic_state_dict`` (used by the parity tests)."""
        dev = self.device if on_device else "cpu"
        self.fp8 = None
        for name, t in iter_synthetic_state_dict(self.params, seed=seed, device=dev, dtype=torch.float32):
            self.tensors[name].copy_(t)
        return self


@dataclass
class _Geom:
    """Row geometry of one forward: B work items; rows [0, oT) concept, [oT, oI) text, [oI, n) image."""
    B: int
    C: int
    T: int
    L: int

    @property
    def oT(self):
        return self.B * self.C

    @property
    def oI(self):
        return self.B * (self.C + self.T)

    @property
    def n(self):
        return self.B * (self.C + self.T + self.L)


@dataclass
class HeatmapRequest:
    """Fused heat-map accumulation (replaces materialising the 478 MB/step dicts that
    compute_heatmaps_from_vectors later slices, concept_attention_pipeline.py:57-82)."""
    layer_indices: tuple
    weight: float                 # 1 / (|timesteps| * |layers|)
    out_space: Optional[torch.Tensor]     # fp32 [C, L] accumulator (output-space maps), or None (per-layer tables only)
    cross_space: Optional[torch.Tensor]   # fp32 [C, L] accumulator (cross-attention-space maps), or None
    # optional per-layer tables [len(layer_indices), C, L] (row i = layer_indices[i]), accumulated with
    # per_layer_weight: the per-layer x per-noise-level extraction of
    # experiments/per_layer_segmentation/test_segmentations_per_layer.py:104-114 without the vector stacks
    per_layer_out: Optional[torch.Tensor] = None
    per_layer_cross: Optional[torch.Tensor] = None
    per_layer_weight: float = 1.0
    norm: int = L.NORM_SOFTMAX    # weighting across concepts: softmax | sparsemax | entmax15 (_lib.NORM_*)
    # prompt-token maps (ops.token_maps): the probability the image rows' joint [text | image] softmax gives to the first
    # n_tok text keys of the item, averaged over the heads, accumulated over the captured layers with ``weight`` /
    # ``per_layer_weight`` as the concept maps are.  fp32 [n_tok, L] and / or [len(layer_indices), n_tok, L]; n_tok is
    # their first / second dimension (at most the text length); None: no launch
    token_space: Optional[torch.Tensor] = None
    per_layer_token: Optional[torch.Tensor] = None
    # query-row maps (ops.query_maps), the other direction: where the item's first n_tok text rows, and its concept rows,
    # look in the image -- the probability each such query row's own softmax puts on every image key, averaged over the
    # heads, accumulated as the concept maps are.  Text rows: the joint [text | image] problem's; concept rows: their own
    # [concept | image] problem's.  fp32 [n_tok, L] / [C, L] and / or [len(layer_indices), ., L]; None: no launch
    token_query_space: Optional[torch.Tensor] = None
    per_layer_token_query: Optional[torch.Tensor] = None
    concept_query_space: Optional[torch.Tensor] = None
    per_layer_concept_query: Optional[torch.Tensor] = None
    # per-head concept maps and the raw-space baselines (ops.head_maps): per head of 128 the concept rows against the
    # image rows of a space, weighted across the concepts per head with ``head_norm`` (None: the logits themselves, or a
    # _lib.NORM_*), accumulated over the captured layers with ``weight``.  heads_* fp32 [num_heads, C, L] (the
    # head-resolved maps), raw_* fp32 [C, L] (their mean over the heads); None: no launch.  The spaces: "output"
    # (ATT32 / ATTI32, which makes the forward take the fp32 image rows' route), "cross" (QPRE), "value" (the v third of
    # QKV).  ``head_normalize_concepts``: heatmaps.linear_normalization across the concepts of the concept rows first
    heads_out: Optional[torch.Tensor] = None
    heads_cross: Optional[torch.Tensor] = None
    heads_value: Optional[torch.Tensor] = None
    raw_out: Optional[torch.Tensor] = None
    raw_cross: Optional[torch.Tensor] = None
    raw_value: Optional[torch.Tensor] = None
    head_norm: Optional[int] = None
    head_normalize_concepts: bool = False
    # the same spaces under further norms in the same forward: HeatmapRequests of which only these head-map fields are read
    head_more: tuple = ()
    # propagated concept maps (ops.propagate_maps): per captured layer the layer's own concept map of a space -- the map
    # that layer adds, times ``weight``, into out_space / cross_space -- carried ``prop_steps`` times (1 .. 4) through the
    # head mean of the image rows' softmax over the image keys, then added with ``weight``.  fp32 [C, L]; None: no launch
    prop_out: Optional[torch.Tensor] = None
    prop_cross: Optional[torch.Tensor] = None
    prop_steps: int = 1

    def query_kinds(self) -> tuple:
        """The query-row maps this request asks for, as (kind, accumulator, per-layer table)."""
        return tuple((k, a, t) for k, a, t in (("tokens", self.token_query_space, self.per_layer_token_query),
                                               ("concepts", self.concept_query_space, self.per_layer_concept_query))
                     if a is not None or t is not None)

    def head_spaces(self) -> tuple:
        """The spaces this request asks head maps of, as (name, heads tensor, raw tensor)."""
        return tuple((n, h, r) for n, h, r in (("output", self.heads_out, self.raw_out),
                                               ("cross", self.heads_cross, self.raw_cross),
                                               ("value", self.heads_value, self.raw_value))
                     if h is not None or r is not None)

    def prop_spaces(self) -> tuple:
        """The spaces this request asks propagated maps of, as (name, accumulator, the space's per-layer table)."""
        return tuple((n, a, t) for n, a, t in (("output", self.prop_out, self.per_layer_out),
                                               ("cross", self.prop_cross, self.per_layer_cross)) if a is not None)

    def head_requests(self) -> tuple:
        """This request and those of ``head_more`` that ask for head maps: one (spaces, norm, normalisation) each."""
        return tuple(r for r in (self,) + tuple(self.head_more) if r.head_spaces())


def _launch_apart(probs: list, accumulators, launch, limit: Optional[int] = None) -> None:
    """``launch(batch)`` over the map problems ``probs``, in order and in as few batches as this allows: a problem that
    names an accumulator already in the batch (``accumulators(problem)``: its tensors or None; two requests may share
    one) starts a new batch, since within a launch the updates are unordered read-modify-writes, and so does a batch of
    ``limit`` problems (None: the launch splits longer lists itself).  No launch for no problems."""
    batch, seen = [], set()
    for pr in probs + [None]:
        ptrs = set() if pr is None else {t.data_ptr() for t in accumulators(pr) if t is not None}
        if pr is None or len(batch) == limit or (ptrs & seen):
            if batch:
                launch(batch)
            batch, seen = [], set()
        if pr is not None:
            batch.append(pr)
            seen |= ptrs


def modulation_rows(params: FluxParams) -> int:
    """Rows of the stacked adaLN matrix (FluxWeights.mod_rows): 2 x 6H per double block, 3H per single block, 2H for the
    final layer.  One fp32 vector of that length is every block's shift / scale / gate for one conditioning vector."""
    H = params.hidden_size
    return (12 * params.depth + 3 * params.depth_single_blocks + 2) * H


def step_trace_nbytes(params: FluxParams, C: int, T: int, L_img: int, blocks: int, n_layers: int) -> int:
    """Bytes one traced step keeps per work item (INTEGRATION.md "Concept re-query"): the bf16 [C+T+L, 3H] qkv slab of
    each of the first ``blocks`` double blocks, per captured layer the fp32 [T+L, H] attention rows and the fp32
    [C+T+L, H] pre-RoPE q rows, and one fp32 modulation vector.  Pure arithmetic."""
    H, n = params.hidden_size, C + T + L_img
    return blocks * n * 3 * H * 2 + n_layers * ((T + L_img) * H * 4 + n * H * 4) + modulation_rows(params) * 4


class StepTrace:
    """What one forward leaves of its image side for ``HipFluxDiT.requery``, in storage of its own.

    The no-copy form: while a traced double block runs, the model's QKV (and, in a captured layer, ATTI32 and QPRE) ARE
    the tensors kept here, so the rotated image k and v are exactly what the attention launch read and nothing is copied.
    The slabs keep the forward's [C+T+L, 3H] rows -- the concept and text rows and the q third ride along unused (13 % at
    1024 x 1024 against a compact [L, 2H] layout, which would cost a 50 MB row copy per block and item) -- and with them the
    3H row stride, so a re-query's own [C', 3H] concept rows and the kept image rows are two key / value segments of one
    row stride.  Pass an empty ``StepTrace()`` as ``trace=``; the forward fills it.  A forward of B items leaves one
    storage; ``items()`` are the per-item views ``requery`` takes."""

    def __init__(self):
        self.model = None            # the HipFluxDiT whose forward filled the trace
        self.item = None             # index into the forward's items (a view made by items()); None: the storage itself
        self.B = self.C = self.T = self.L = 0
        self.layers = ()             # the captured double blocks (sorted)
        self.qkv = []                # per double block 0 .. max(layers): bf16 [B (C+T+L), 3H]
        self.att_img = {}            # captured layer -> fp32 [B, T+L, H] attention rows of [text | image]
        self.qpre = {}               # captured layer -> fp32 [B (C+T+L), H] post-QKNorm pre-RoPE q
        self.split = []              # per block: q from the unrounded LayerNorm output (LayerRoute.split)
        self.qk16 = []               # per block: rotated q / k stored as IEEE half (LayerRoute.qk16)
        self.mod = None              # fp32 [B, mod_rows]: every block's modulation of the concept rows
        self.released = False

    @property
    def filled(self) -> bool:
        return self.model is not None

    def items(self) -> list:
        """One view per work item of the traced forward, sharing this storage."""
        out = []
        for j in range(self.B):
            v = StepTrace()
            v.__dict__.update(self.__dict__)
            v.item = j
            out.append(v)
        return out

    @property
    def nbytes(self) -> int:
        """Bytes kept per work item (``step_trace_nbytes``); B times that for the storage of a batched forward."""
        if not self.filled or self.released:
            return 0
        per_item = step_trace_nbytes(self.model.params, self.C, self.T, self.L, len(self.qkv), len(self.layers))
        return per_item * (self.B if self.item is None else 1)

    def release(self) -> None:
        """Drop this object's hold on the storage (it is freed once every view of a batched forward has let go)."""
        self.qkv, self.att_img, self.qpre, self.mod, self.released = [], {}, {}, None, True

    def image_kv(self, block: int):
        """The rotated image k and v rows [L, H] (row stride 3H) block ``block``'s attention read for this item."""
        H, j = self.qkv[block].shape[1] // 3, self.item or 0
        r = slice(self.B * (self.C + self.T) + j * self.L, self.B * (self.C + self.T) + (j + 1) * self.L)
        return self.qkv[block][r, H:2 * H], self.qkv[block][r, 2 * H:]

    def image_vectors(self, layer: int):
        """(fp32 attention rows, fp32 pre-RoPE q rows) [L, H] of this item's image tokens in a captured layer."""
        j, o = self.item or 0, self.B * (self.C + self.T)
        return self.att_img[layer][j, self.T:], self.qpre[layer][o + j * self.L:o + (j + 1) * self.L]


class LayerRoute(NamedTuple):
    """What HipFluxDiT._layer_route decides for one double block."""
    capture: bool    # the layer's vectors are returned or turned into heat maps
    fp8: bool        # proj and the MLP on e4m3 operands
    fp8_qkv: bool    # the qkv projection too
    split: bool      # q of the image / concept rows from the unrounded LayerNorm output (low-plane GEMM)
    indep: bool      # that q only in map-side attention problems; what feeds proj is formed as in an uncaptured layer
    qk16: bool       # rotated q / k stored as IEEE half
    use_part: bool   # output-space logits as per-head partials from the attention epilogue (PART)
    f32img: bool     # ... or from an fp32 copy of the [text | image] attention rows (ATTI32)


# what the qkv epilogue multiplies the rotated q by: softmax_scale * log2(e) at head_dim 128, folded into q in fp32
# before its one rounding, so the attention kernel's probability is a bare exp2 (include/conceptattn.h
# CA_ATTN_Q_PRESCALED)
Q_OUT_SCALE = (1.0 / math.sqrt(128.0)) * 1.4426950408889634


class HipFluxDiT:
    """Drop-in for the reference's ``ModifiedFluxDiT`` instance on the hot path (inference only)."""

    def __init__(self, params: FluxParams, device="cuda:0", weights: Optional[FluxWeights] = None,
                 attention_block_class=None, precision: str = "bf16", residual_dtype=torch.float32,
                 bf16_timesteps: bool = False):
        # attention_block_class is accepted for signature compatibility with
        # ModifiedFluxDiT(params, attention_block_class=...) (modified_flux_dit.py:34); the HIP
        # path has exactly one block implementation.
        if params.head_dim != 128:
            raise ValueError("HipFluxDiT: the gfx950 kernels are built for head_dim 128")
        self.params = params
        self.device = torch.device(device)
        self.in_channels = params.in_channels
        self.out_channels = params.in_channels
        self.hidden_size = params.hidden_size
        self.num_heads = params.num_heads
        L.load()
        self.weights = weights if weights is not None else FluxWeights(params, self.device)
        self._ws_key = None
        self._ws_cache = {}
        self._rope_key = None
        self._mod_cur = None
        self._mod_steps = None
        self._traced = {}    # lazy buffers a traced block has pointed at a StepTrace's storage (_traced_block)
        # The residual streams X are kept in fp32 by default: every block adds two gated projections to them, and
        # rounding the running sum to bf16 after each add (as a bf16 activation tensor does, the reference's own
        # bf16 run included) is what makes the heat-map error grow with depth -- 38 roundings by layer 18.
        # Measured (tests/tools/error_budget.py): 5e-3 -> 1.3e-3 max-abs on layers 15..18.
        # Cost: 27 MB more per LayerNorm read / projection write-back per block.  torch.bfloat16 is the layout of the
        # reference's activations.
        if residual_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("residual_dtype must be torch.float32 or torch.bfloat16")
        self.residual_dtype = residual_dtype
        # The reference's production (bf16) run builds t_vec / guidance_vec in the activations' dtype and forms
        # time_factor * t in bf16 (flux/sampling.py:122-125, flux/modules/layers.py:37): at t = 0.75 it embeds 752,
        # and most shifted flux-dev schedule values are rounded twice; the embedding itself is cast to bf16 too.
        # Default False = the fp32 oracle's behaviour (t and 1000 t exact); True reproduces the reference's bf16
        # values (pinned by tests/golden/timestep_embedding_bf16.npz).
        self.bf16_timesteps = bool(bf16_timesteps)
        # sampling.denoise keeps the latent in fp32 between the Euler steps when the model says so (False = bf16, as the
        # reference's loop)
        self.fp32_latent = True
        # The rotated q and k of the attention as IEEE half instead of bf16 (ca_gemm_problem.qk_f16 ->
        # ca_attn_fwd_qk16): their bf16 rounding is one of the two things that bound a single output-space heat map
        # (tests/tools/error_budget.py --out-space2: 9e-4 -> 2.5e-4 per map with 11-bit q / k; v and the probabilities
        # do not matter), and behind an RMS norm the values sit far inside fp16's range.  "captured" (default): the
        # layers whose maps are requested -- where the attention's q is special anyway (_double_block); the chip clocks
        # the f16 MFMA 1.6 % lower than the bf16 one, and with every block in half precision ("all") the maps are no
        # closer to the oracle (profiles/r04_full_depth_parity*.json: 5.6e-4 / 9.6e-4 worst single map against
        # 5.7e-4 / 8.4e-4) at -0.6 % heat maps/s.  "0": bf16 everywhere, as the reference.
        self.qk_f16 = "captured"
        # Exact independence of everything the forward returns from WHICH layers' maps are requested (the reference's
        # property: the concept stream and the capture are read-only side computations, modified_double_stream_block.py:
        # 105-119, 185-191).  False (default): a captured layer's attention uses the accurate q for its image and concept
        # rows and half-precision q / k, so the latent moves at rounding level with layer_indices (bounded:
        # tests/test_full_depth_gpu.py::test_latent_dependence_on_the_captured_layer_set).  True: every layer's attention
        # output that feeds proj / the residual streams is formed exactly as in an uncaptured layer (rounded-operand q,
        # bf16 q / k), and the captured layers' maps come from SEPARATE attention problems of the same launch -- the
        # accurate q of the image rows (and of the concept rows) against the same keys and values, written to scratch
        # rows that only the heat maps read.  Cost: the image rows' attention twice in captured layers (+1.3 % of a
        # generate call with 4 of 57 layers captured; +15 % of a 19-layer sweep forward); single output-space maps then
        # carry k's bf16 rounding again (measured in the same test file).  In fp8 mode the independence is exact only with
        # fp8_bf16_qkv_when_captured = False: a captured layer's bf16 qkv projection forms other k and v than e4m3 operands.
        self.capture_independent_image = False
        # fp8 mode: the qkv projection of a layer whose maps are requested stays bf16 (_layer_route)
        self.fp8_bf16_qkv_when_captured = True
        # the heat-map updates of a captured layer (all work items, both spaces) as ONE ca_heatmap_fused launch; False =
        # logits + weighting launches per item and space (the same bits; the parity reference, and what C > 8 uses)
        self.fused_heatmaps = True
        # The output-space logits of a captured layer from the attention kernel's own accumulators: the concept
        # problems run first (their fp32 rows ATT32 must exist), every main problem's epilogue then forms, per head, the
        # dot products of its image rows (fp32, before their bf16 rounding) with the C concept rows and leaves
        # [heads, L, 8] partial logits (PART, 3 MB per item), which ca_heatmap_fused sums over the heads -- instead of an
        # fp32 copy of every [text | image] row (ATTI32: 53 MB per item, +115 us per captured 5-item attention launch,
        # and 250 MB of reads in the heat-map launch).  The same arithmetic in another summation order (per head, then
        # over the heads).  False = the fp32 rows (the parity reference).  Needs fused_heatmaps.
        self.epilogue_logits = True
        self.set_precision(precision)

    # Every setting above that selects a route or a number format: what a replica on another stream must share with the
    # model it stands in for (pipeline._stream_models copies them before every run).
    ROUTE_SETTINGS = ("precision", "keep_bf16_layers", "residual_dtype", "bf16_timesteps", "fp32_latent", "qk_f16",
                      "capture_independent_image", "fp8_bf16_qkv_when_captured", "fused_heatmaps", "epilogue_logits")

    # ---- reduced-precision mode (BASELINE.json configs[4]; no counterpart in the reference)
    FP8_LINEARS = ("img_attn.qkv", "txt_attn.qkv", "img_attn.proj", "txt_attn.proj", "img_mlp.0", "txt_mlp.0",
                   "img_mlp.2", "txt_mlp.2", "linear1", "linear2")

    def set_precision(self, precision: str, keep_bf16_layers=()):
        """"bf16" (default; the parity path) or "fp8": the six large projections of every block run on e4m3
        operands (weights quantised once per output channel, activations per token by the producing
        kernel), accumulation fp32, everything else unchanged.  ``keep_bf16_layers``: double blocks that stay
        in bf16 even in fp8 mode (e.g. the layers whose attention outputs are turned into heat maps).  See
        DESIGN.md "fp8 mode" for the measured heat-map deviation from the bf16 path."""
        if precision not in ("bf16", "fp8"):
            raise ValueError(f"precision must be 'bf16' or 'fp8', got {precision!r}")
        self.precision = precision
        self.keep_bf16_layers = frozenset(int(l) for l in keep_bf16_layers)
        return self

    def _fp8_weights(self):
        W = self.weights
        if W.fp8 is None:
            W.fp8 = {name: ops.quantize_rows_fp8(t) for name, t in W.tensors.items()
                     if name.endswith(".weight") and name.rsplit(".", 1)[0].split(".", 2)[-1] in self.FP8_LINEARS}
        return W.fp8

    def materialize(self):
        """Build the lazily created state that model instances SHARE (the fp8 weight images live on the common
        FluxWeights object) on the CURRENT stream.  Callers that are about to run replicas on other streams call
        this first and then make those streams wait on the current one; otherwise a replica could launch an fp8
        GEMM on weight images whose quantisation kernels are still queued on another stream."""
        if self.precision == "fp8":
            self._fp8_weights()
        return self

    def _gemm(self, fp8, a, a8, a8s, wname, bias, out, *args, **kw):
        """One problem of a grouped launch in the current precision."""
        if fp8:
            q, sc = self._fp8_weights()[wname]
            return ops.Gemm(a8, q, bias, out, *args, a_scale=a8s, w_scale=sc, **kw)
        return ops.Gemm(a, self.weights[wname], bias, out, *args, **kw)

    # ---- nn.Module-like surface the reference's loader touches (image_generator.py:37-44,183,194)
    def load_state_dict(self, sd, strict: bool = True, assign: bool = False):
        return self.weights.load_state_dict(sd, strict=strict)

    def state_dict(self):
        return self.weights.state_dict()

    def to(self, *a, **k):
        return self

    def cpu(self):  # the reference round-trips 23.8 GB per call (image_generator.py:183,194); we keep it resident
        return self

    def eval(self):
        return self

    # ------------------------------------------------------------------ workspace
    def _workspace(self, L_img: int, T: int, C: int, B: int = 1):
        """Activation set for a batch of B work items.  Rows are ordered
        [concept rows of item 0..B-1 | text rows of item 0..B-1 | image rows of item 0..B-1]: all rows that use
        the text weights are one contiguous matrix, all image rows another, and the single blocks' [text | image]
        rows a third (B = 1: the layout of the module docstring)."""
        key = (L_img, T, C, B, self.precision, self.residual_dtype)
        if self._ws_key == key:
            return
        # A few activation sets stay cached (LRU): callers that alternate shapes -- a ragged last group of a batched
        # run, B = 1 calls between B = 5 groups -- would otherwise free and re-zero gigabytes inside their loop.
        cached = self._ws_cache.pop(key, None)
        if cached is None:
            cached = self._alloc_workspace(L_img, T, C, B)
            while len(self._ws_cache) >= self.WS_CACHE_ENTRIES:
                self._ws_cache.pop(next(iter(self._ws_cache)))
        self._ws_cache[key] = cached
        self.__dict__.update({k: v for k, v in cached.items() if k not in self._LAZY_BUFFERS})
        self._ws_key = key
        self._rope_key = None

    WS_CACHE_ENTRIES = 3

    # Buffers only some forwards need (the captured layers' fp32 vectors: ~0.55 GB per work item at 1024 x 1024; +53 MB
    # where the fp32 rows ATTI32 are used) are allocated on first use, per activation set: a model that never returns
    # maps never pays for them.  An fp8-mode forward WITH captured layers does (their qkv projection stays bf16, so the
    # split-q buffers XML / QPRE are used there too).  name -> (rows, columns..., dtype) of the set's geometry
    _LAZY_BUFFERS = {
        "QPRE": lambda n, B, T, L, H: ((n, H), torch.float32),       # post-QKNorm pre-RoPE q (cross-space vectors)
        "XML": lambda n, B, T, L, H: ((n, H), torch.bfloat16),       # low plane of XM: bf16(y - float(bf16(y)))
        "ATTI32": lambda n, B, T, L, H: ((B, T + L, H), torch.float32),   # fp32 [text | image] attention rows
        # capture_independent_image: the accurate q of the captured layers' image / concept rows (the map-side attention
        # problems' queries) and those problems' bf16 output rows, which nothing but the heat maps reads
        # epilogue_logits: per-head partial output-space logits of every item's image rows [B, heads, L, 8]
        "PART": lambda n, B, T, L, H: ((B, H // 128, L, 8), torch.float32),
        "QACC": lambda n, B, T, L, H: ((n, H), torch.bfloat16),
        "ATTM": lambda n, B, T, L, H: ((n, H), torch.bfloat16),
    }

    def _lazy_buffer(self, name: str) -> torch.Tensor:
        if name in self._traced:     # a traced block: the buffer is the trace's storage (_traced_block)
            return self._traced[name]
        ws = self._ws_cache[self._ws_key]
        t = ws.get(name)
        if t is None:
            L_img, T, C, B = self._ws_key[:4]
            shape, dtype = self._LAZY_BUFFERS[name](B * (C + T + L_img), B, T, L_img, self.params.hidden_size)
            t = ws[name] = torch.zeros(shape, device=self.device, dtype=dtype)
        return t

    QPRE = property(lambda self: self._lazy_buffer("QPRE"))
    XML = property(lambda self: self._lazy_buffer("XML"))
    ATTI32 = property(lambda self: self._lazy_buffer("ATTI32"))
    PART = property(lambda self: self._lazy_buffer("PART"))
    QACC = property(lambda self: self._lazy_buffer("QACC"))
    ATTM = property(lambda self: self._lazy_buffer("ATTM"))

    def clear_workspaces(self) -> None:
        """Drop every cached activation set (up to WS_CACHE_ENTRIES sets stay resident between calls: ~1.6 GB per work
        item at 1024 x 1024 with the capture buffers, 8 GB for a 5-item set); the next forward allocates afresh."""
        for ws in self._ws_cache.values():
            for k in ws:
                self.__dict__.pop(k, None)
        self._ws_cache.clear()
        self._ws_key = None
        self._rope_key = None

    def workspace_bytes(self) -> int:
        """Bytes of HBM the cached activation sets hold right now."""
        return sum(t.numel() * t.element_size() for ws in self._ws_cache.values() for t in ws.values()
                   if isinstance(t, torch.Tensor))

    def _alloc_workspace(self, L_img: int, T: int, C: int, B: int) -> dict:
        p, dev = self.params, self.device
        H, MLP = p.hidden_size, p.mlp_hidden
        n = B * (C + T + L_img)
        bf = dict(device=dev, dtype=torch.bfloat16)
        f32 = dict(device=dev, dtype=torch.float32)
        ws = dict(
            X=torch.zeros(n, H, device=dev, dtype=self.residual_dtype),
            XM=torch.zeros(n, H, **bf),
            QKV=torch.zeros(n, 3 * H, **bf),
            ATT=torch.zeros(n, H, **bf),
            HID=torch.zeros(n, MLP, **bf),
            CAT=torch.zeros(B * (T + L_img), H + MLP, **bf),
            # (QPRE, XML, ATTI32 -- the fp32 vectors of the captured layers -- are allocated on first use: _LAZY_BUFFERS)
            ATT32=torch.zeros(max(B * C, 1), H, **f32),  # fp32 copy of the concept attention rows
            TXT_IN=torch.zeros(B * (C + T), p.context_in_dim, **bf),
            PRED=torch.zeros(B * L_img, p.in_channels, **bf),
            PRED32=torch.zeros(B * L_img, p.in_channels, **f32),
            ROPE=torch.zeros(n, 64, 2, **f32),
            TEMB=torch.zeros(2 * B, 256, **f32),      # rows 2j / 2j+1: item j's vec / concept_vec chain
            TVAL=torch.zeros(2 * B, **f32),
            YIN=torch.zeros(2 * B, p.vec_in_dim, **f32),
            HVEC=torch.zeros(2 * B, H, **f32),
            VEC=torch.zeros(2 * B, H, **f32),
            MOD=torch.zeros(B, 2, self.weights.mod_rows, **f32),
            LOGITS=torch.zeros(max(C, 1), L_img, **f32))
        if self.precision == "fp8":   # e4m3 images of the GEMM inputs + one fp32 scale per row
            u8 = dict(device=dev, dtype=torch.uint8)
            ws.update(XM8=torch.zeros(n, H, **u8), XMS=torch.zeros(n, **f32),
                      ATT8=torch.zeros(n, H, **u8), ATTS=torch.zeros(n, **f32),
                      HID8=torch.zeros(n, MLP, **u8), HIDS=torch.zeros(n, **f32),
                      CAT8=torch.zeros(B * (T + L_img), H + MLP, **u8), CATS=torch.zeros(B * (T + L_img), **f32))
        return ws

    def _rope_table(self, img_ids, txt_ids, concept_ids, C, T):
        """(cos, sin) per row in [concept | text | image] order.  rope(): angles in float64,
        stored fp32 (flux/math.py:15-22); EmbedND concatenates the axes (layers.py:18-25)."""
        # The table is cached only for ids whose CONTENT is known: tensors made by sampling.make_img_ids /
        # sampling.zero_ids carry a tag (what they hold + their version counter at creation).  A pointer/shape
        # key is not content identity (the allocator re-uses addresses: 2048x512 then 512x2048 would hit), so
        # untagged or since-modified ids rebuild the table on every forward (a few tiny kernels).
        def tag(t):
            g = getattr(t, "_ca_ids_tag", None)
            if g is None:
                return None
            try:
                return g[0] if t._version == g[1] else None
            except RuntimeError:  # inference-mode tensors have no version counter
                return None
        key = tuple(tag(t) for t in (img_ids, txt_ids, concept_ids))
        if any(k is None for k in key):
            key = None
        if key is not None and self._rope_key == key:
            return
        self._rope_fill(torch.cat((concept_ids.reshape(-1, 3), txt_ids.reshape(-1, 3), img_ids.reshape(-1, 3)), 0),
                        self.ROPE)
        self._rope_key = key

    def _rope_fill(self, ids, rope) -> None:
        """rope[r] = (cos, sin) of row r's position ids [rows, 3]."""
        ids = ids.to(self.device, torch.float64)
        col = 0
        for a, d in enumerate(self.params.axes_dim):
            scale = torch.arange(0, d, 2, dtype=torch.float64, device=self.device) / d
            omega = 1.0 / (self.params.theta ** scale)
            ang = ids[:, a:a + 1] * omega[None]
            rope[:, col:col + d // 2, 0] = torch.cos(ang).float()
            rope[:, col:col + d // 2, 1] = torch.sin(ang).float()
            col += d // 2

    def _mod(self, name: str, row: int, chunk: int, item: int = 0) -> torch.Tensor:
        """fp32 view of one modulation chunk of work item ``item``: name = '<block>.lin' base, row 0 = vec,
        1 = concept_vec.  Consecutive items are ``self._mod_cur.stride(0)`` floats apart (the gate_stride of the
        GEMM epilogue)."""
        H = self.hidden_size
        o = self.weights.mod_offset[name] + chunk * H
        return self._mod_cur[item, row, o:o + H]

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    @on_own_device
    def __call__(self, img, img_ids, txt, txt_ids, concepts, concept_ids, concept_vec, timesteps, y,
                 guidance=None, stop_after_multimodal_attentions: bool = False, edit_metadata=None,
                 iteration=None, joint_attention_kwargs=None, return_vectors: bool = True,
                 heatmaps=None, cond_slot: Optional[int] = None, trace: Optional[StepTrace] = None, **kwargs):
        """Same keyword contract as ModifiedFluxDiT.forward (modified_flux_dit.py:75-92), for a batch of B
        independent work items (the reference's callers use B = 1): img (B,L,64), txt (B,T,4096), concepts
        (B,C,4096), y / concept_vec (B,768), timesteps / guidance (B,), ids (B,n,3).

        Extra (HIP-path) keywords: ``return_vectors=False`` skips materialising the four
        per-layer vector stacks (the dict is then empty); ``heatmaps`` (one HeatmapRequest, or a list of B)
        accumulates softmax-over-concepts maps for the requested layers inside the forward; ``cond_slot=i``
        uses step i of a preceding ``precompute_conditioning`` call instead of recomputing the
        conditioning vectors from ``timesteps`` / ``y`` / ``guidance``; ``trace`` (an empty StepTrace, with
        ``heatmaps``) keeps the image side of the requested layers for ``requery``: the captured layers then take the fp32
        image rows' route (epilogue_logits = False) and the prediction stays bit for bit what it is without."""
        assert concept_vec is not None, "Concept vectors must be provided for this implementation."
        heads_out = self._check_head_maps(heatmaps, return_vectors, joint_attention_kwargs)
        self._check_query_maps(heatmaps, joint_attention_kwargs)
        self._check_propagated(heatmaps, return_vectors, concepts)
        if trace is not None:
            if trace.filled:
                raise ValueError("trace: an empty StepTrace per forward (this one is already filled)")
            if heatmaps is None or return_vectors:
                raise ValueError("trace: a tracing forward takes heatmaps= and return_vectors=False (the stacked route keeps "
                                 "no fp32 image rows)")
            self._check_traceable("trace", joint_attention_kwargs)
            before = self.epilogue_logits
            self.epilogue_logits = False     # the fp32 image rows must exist: the use_part route never writes them
            try:
                return self._forward(img, img_ids, txt, txt_ids, concepts, concept_ids, concept_vec, timesteps, y, guidance,
                                     stop_after_multimodal_attentions, joint_attention_kwargs, return_vectors, heatmaps,
                                     cond_slot, trace)
            finally:
                self.epilogue_logits = before
                self._end_traced_block()
        if heads_out and self.epilogue_logits:
            # output-space head maps read the fp32 image rows ATTI32, as a trace does: the same route for this forward
            self.epilogue_logits = False
            try:
                return self._forward(img, img_ids, txt, txt_ids, concepts, concept_ids, concept_vec, timesteps, y, guidance,
                                     stop_after_multimodal_attentions, joint_attention_kwargs, return_vectors, heatmaps,
                                     cond_slot)
            finally:
                self.epilogue_logits = True
        return self._forward(img, img_ids, txt, txt_ids, concepts, concept_ids, concept_vec, timesteps, y, guidance,
                             stop_after_multimodal_attentions, joint_attention_kwargs, return_vectors, heatmaps, cond_slot)

    def _check_head_maps(self, heatmaps, return_vectors, joint_attention_kwargs) -> bool:
        """The settings per-head maps do not cover, each named and raised before anything is launched.  Returns whether a
        request asks for the output space (the forward then needs the fp32 image rows)."""
        reqs = () if heatmaps is None else heatmaps if isinstance(heatmaps, (list, tuple)) else [heatmaps]
        reqs = [r for h in reqs for r in h.head_requests()]
        spaces = {n for h in reqs for n, _, _ in h.head_spaces()}
        if not spaces:
            return False
        if return_vectors:
            raise ValueError("head maps: a forward with per-head maps takes return_vectors=False (the stacked route has no "
                             "per-head launch)")
        if "output" in spaces and self.capture_independent_image:
            raise ValueError("head maps: capture_independent_image=True is not covered by the output-space head maps "
                             "(\"cross\" and \"value\" are)")
        jak = joint_attention_kwargs or {}
        if not (jak.get("concept_cross_attention", True) and jak.get("concept_self_attention", True)):
            raise ValueError("head maps: the ablation joint_attention_kwargs (concept_cross_attention / "
                             "concept_self_attention = False) are not covered by the per-head maps")
        for h in reqs:
            if h.head_norm is not None and h.head_norm not in L.NORMS.values():
                raise ValueError(f"head maps: head_norm must be None or one of _lib.NORM_SOFTMAX / NORM_SPARSEMAX / "
                                 f"NORM_ENTMAX15, got {h.head_norm}")
        return "output" in spaces

    def _check_query_maps(self, heatmaps, joint_attention_kwargs) -> None:
        """The settings query-row maps do not cover, raised before anything is launched."""
        reqs = () if heatmaps is None else heatmaps if isinstance(heatmaps, (list, tuple)) else [heatmaps]
        kinds = {k for h in reqs for k, _, _ in h.query_kinds()}
        jak = joint_attention_kwargs or {}
        if "concepts" in kinds and not (jak.get("concept_cross_attention", True) and jak.get("concept_self_attention", True)):
            raise ValueError("query maps: the ablation joint_attention_kwargs (concept_cross_attention / "
                             "concept_self_attention = False) change the concept rows' key set and are not covered by the "
                             "concept rows' query maps")

    def _check_propagated(self, heatmaps, return_vectors, concepts) -> None:
        """The settings propagated maps do not cover, raised before anything is launched."""
        reqs = () if heatmaps is None else heatmaps if isinstance(heatmaps, (list, tuple)) else [heatmaps]
        reqs = [h for h in reqs if h.prop_spaces()]
        if not reqs:
            return
        if return_vectors:
            raise ValueError("propagated maps: a forward with propagated maps takes return_vectors=False (the stacked route "
                             "has no launch for them)")
        C = concepts.shape[1]
        if not 1 <= C <= L.PROPMAP_MAX_CONCEPTS:
            raise ValueError(f"propagated maps: {C} concepts; 1 .. {L.PROPMAP_MAX_CONCEPTS} per item")
        for h in reqs:
            if not isinstance(h.prop_steps, int) or not 1 <= h.prop_steps <= 4:
                raise ValueError(f"propagated maps: prop_steps = {h.prop_steps!r}; an int in 1 .. 4")
            for name, acc, table in h.prop_spaces():
                if (h.out_space if name == "output" else h.cross_space) is None:
                    raise ValueError(f"propagated maps: the {name} space's concept maps are not computed by this request "
                                     "(the propagation starts from the map the layer adds into out_space / cross_space)")
                if table is not None:
                    raise ValueError(f"propagated maps: the {name} space also has a per-layer table (the heat-map launch's "
                                     "second accumulator carries the layer's map to the propagation; the sweeps are not covered)")
                if acc.dtype != torch.float32 or acc.dim() != 2 or acc.shape[0] != C or not acc.is_contiguous():
                    raise ValueError(f"propagated maps: prop_{'out' if name == 'output' else 'cross'} must be contiguous fp32 "
                                     f"[C = {C}, L], got {tuple(acc.shape)} {acc.dtype}")

    def _check_traceable(self, what: str, joint_attention_kwargs=None) -> None:
        """The settings a trace and a re-query do not cover, each named; raised before anything is launched."""
        if self.precision != "bf16":
            raise ValueError(f"{what}: precision=\"fp8\" is not covered by the concept re-query (precision=\"bf16\" only)")
        if self.capture_independent_image:
            raise ValueError(f"{what}: capture_independent_image=True is not covered by the concept re-query")
        jak = joint_attention_kwargs or {}
        if not (jak.get("concept_cross_attention", True) and jak.get("concept_self_attention", True)):
            raise ValueError(f"{what}: the ablation joint_attention_kwargs (concept_cross_attention / "
                             "concept_self_attention = False) are not covered by the concept re-query")

    def _begin_traced_block(self, trace: StepTrace, i: int, captured: bool, n: int, B: int, T: int, Li: int) -> None:
        """Point QKV (and in a captured layer ATTI32 and QPRE) at fresh storage the trace owns, for block ``i``."""
        H, dev = self.hidden_size, self.device
        trace.qkv.append(torch.empty(n, 3 * H, device=dev, dtype=torch.bfloat16))
        self.__dict__["QKV"] = trace.qkv[i]
        self._traced = {}
        if captured:
            trace.att_img[i] = torch.empty(B, T + Li, H, device=dev, dtype=torch.float32)
            trace.qpre[i] = torch.empty(n, H, device=dev, dtype=torch.float32)
            self._traced = {"ATTI32": trace.att_img[i], "QPRE": trace.qpre[i]}

    def _end_traced_block(self) -> None:
        """The model's own reusable buffers again."""
        self._traced = {}
        if self._ws_key is not None:
            self.__dict__["QKV"] = self._ws_cache[self._ws_key]["QKV"]

    def _forward(self, img, img_ids, txt, txt_ids, concepts, concept_ids, concept_vec, timesteps, y, guidance,
                 stop_after_multimodal_attentions, joint_attention_kwargs, return_vectors, heatmaps, cond_slot,
                 trace=None):
        """The forward behind ``__call__`` (its arguments, checked); ``trace``: the StepTrace to fill, or None."""
        if img.ndim != 3 or txt.ndim != 3:
            raise ValueError("Input img and txt tensors must have 3 dimensions.")
        B = img.shape[0]
        if txt.shape[0] != B or concepts.shape[0] != B:
            raise ValueError("img, txt and concepts must have the same batch size")
        if 2 * B > L.ATTN_MAX_PROBLEMS or 3 * B > L.MAX_SEGMENTS:
            raise NotImplementedError(f"HipFluxDiT: at most {min(L.ATTN_MAX_PROBLEMS // 2, L.MAX_SEGMENTS // 3)} work "
                                      "items per forward (attention problems / LayerNorm segments per launch)")
        p, W = self.params, self.weights
        if p.guidance_embed and guidance is None:
            raise ValueError("Didn't get guidance strength for guidance distilled model.")
        Li, T, C = img.shape[1], txt.shape[1], concepts.shape[1]
        for h in () if heatmaps is None else heatmaps if isinstance(heatmaps, (list, tuple)) else [heatmaps]:
            check_concept_count(h.norm, C)   # (before the first launch of the forward)
        self._workspace(Li, T, C, B)
        self._rope_table(img_ids, txt_ids, concept_ids, C, T)
        g = _Geom(B, C, T, Li)
        X, XM = self.X, self.XM
        bf = torch.bfloat16
        if heatmaps is not None and not isinstance(heatmaps, (list, tuple)):
            heatmaps = [heatmaps]
        if heatmaps is not None and len(heatmaps) != B:
            raise ValueError("heatmaps: one HeatmapRequest per work item")

        # ---- input embeddings: img_in, txt_in (text and concept tokens share txt_in, :105,120)
        self.TXT_IN[:g.oT].copy_(concepts.reshape(B * C, -1))
        self.TXT_IN[g.oT:].copy_(txt.reshape(B * T, -1))
        img_flat = img.reshape(B * Li, -1)
        split_in = img.dtype == torch.float32 and self.residual_dtype == torch.float32
        if split_in:
            # an fp32 latent (sampling.denoise keeps the Euler state in fp32 on this path): img_in also sees what the
            # bf16 rounding of its operand drops -- the same weights applied to the low plane, accumulated into the
            # fp32 residual stream (K = 64: the second pass costs microseconds)
            img_in = torch.empty(B * Li, img_flat.shape[1], device=img.device, dtype=bf)
            img_lo = torch.empty_like(img_in)
            ops.split_planes(img_flat.contiguous(), img_in, img_lo)
        else:
            img_in = img_flat.to(bf).contiguous()
        ops.gemm([ops.Gemm(img_in, W["img_in.weight"], W["img_in.bias"], X[g.oI:]),
                           ops.Gemm(self.TXT_IN, W["txt_in.weight"], W["txt_in.bias"], X[:g.oI])])
        if split_in:
            ops.gemm([ops.Gemm(img_lo, W["img_in.weight"], None, X[g.oI:], L.EPI_GATE_RESIDUAL,
                                        resid=X[g.oI:], gate=self._ones_gate(W["img_in.weight"].shape[0]))])

        # ---- conditioning vectors: row 0 = vec (y), row 1 = concept_vec (modified_flux_dit.py:99-119)
        if cond_slot is not None:
            self._mod_cur = self._mod_steps[cond_slot]
            if self._mod_cur.shape[0] != B:
                raise ValueError("precompute_conditioning was run for a different batch size")
        else:
            self._mod_cur = self.MOD
            self._conditioning(timesteps, y, concept_vec, guidance, B)

        out = {k: [] for k in DICT_KEYS} if return_vectors else {}
        if trace is not None:
            trace.layers = tuple(sorted({int(l) for h in heatmaps for l in h.layer_indices}))
            trace.B, trace.C, trace.T, trace.L = B, C, T, Li
            trace.mod = self._mod_cur[:, 1].clone()      # (a copy: MOD is reused, the steps' table is replaced)
            trace.model = self
        for i in range(p.depth):
            if trace is not None and trace.layers and i <= trace.layers[-1]:
                route = self._layer_route(i, C, return_vectors, heatmaps)
                trace.split.append(bool(route.split))
                trace.qk16.append(bool(route.qk16))
                self._begin_traced_block(trace, i, i in trace.layers, g.n, B, T, Li)
            self._double_block(i, g, joint_attention_kwargs, out, return_vectors, heatmaps)
            if trace is not None:
                self._end_traced_block()
        if return_vectors:
            out = {k: torch.stack(v, 0) for k, v in out.items()}
        if stop_after_multimodal_attentions:
            return None, out
        for i in range(p.depth_single_blocks):
            self._single_block(i, g)

        # ---- LastLayer on the image rows (flux/modules/layers.py:242-253)
        fm = "final_layer.adaLN_modulation.1"
        ops.ln_modulate(X[g.oI:], XM[g.oI:], [((j + 1) * Li, self._mod(fm, 0, 0, j), self._mod(fm, 0, 1, j))
                                              for j in range(B)])
        # the prediction has the latent's type: an fp32 latent (sampling.denoise on this path) gets it unrounded
        pred = self.PRED32 if split_in else self.PRED
        ops.gemm([ops.Gemm(XM[g.oI:], W["final_layer.linear.weight"], W["final_layer.linear.bias"], pred)])
        return pred.view(B, Li, -1).clone(), out

    def _vec_chain(self, tv, yin, gv, hv, vecs):
        """vec = time_in(t) (+ guidance_in(g)) + vector_in(y) for every row of tv / yin (MLPEmbedders,
        modified_flux_dit.py:99-119), at most 4 vectors per weight pass."""
        p, W = self.params, self.weights
        n = tv.shape[0]
        temb = torch.empty(n, 256, device=self.device, dtype=torch.float32)
        gemb = torch.empty(n, 256, device=self.device, dtype=torch.float32) if p.guidance_embed else None
        for val, emb in ((tv, temb), (gv, gemb)):
            if emb is None:
                continue
            if self.bf16_timesteps:   # bf16(1000 * bf16(t)) as the kernel's argument, embedding rounded to bf16
                arg = (val.to(torch.bfloat16) * 1000.0).float()
                ops.timestep_embedding(arg, emb, time_factor=1.0)
                emb.copy_(emb.to(torch.bfloat16))
            else:
                ops.timestep_embedding(val, emb)
        for r0 in range(0, n, 4):
            r = slice(r0, min(r0 + 4, n))
            ops.gemv(temb[r], W["time_in.in_layer.weight"], W["time_in.in_layer.bias"], hv[r])
            ops.gemv(hv[r], W["time_in.out_layer.weight"], W["time_in.out_layer.bias"], vecs[r], silu_input=True)
            if p.guidance_embed:
                ops.gemv(gemb[r], W["guidance_in.in_layer.weight"], W["guidance_in.in_layer.bias"], hv[r])
                ops.gemv(hv[r], W["guidance_in.out_layer.weight"], W["guidance_in.out_layer.bias"], vecs[r],
                         silu_input=True, accumulate=True)
            ops.gemv(yin[r], W["vector_in.in_layer.weight"], W["vector_in.in_layer.bias"], hv[r])
            ops.gemv(hv[r], W["vector_in.out_layer.weight"], W["vector_in.out_layer.bias"], vecs[r],
                     silu_input=True, accumulate=True)

    def _conditioning(self, timesteps, y, concept_vec, guidance, B=1):
        """vec / concept_vec of every work item and all modulations for ONE step into self.VEC / self.MOD."""
        p = self.params
        t = timesteps.reshape(-1).float()
        self.TVAL.view(B, 2).copy_((t if t.numel() == B else t[:1].expand(B))[:, None].expand(B, 2))
        self.YIN.view(B, 2, -1)[:, 0].copy_(y.reshape(B, -1))
        self.YIN.view(B, 2, -1)[:, 1].copy_(concept_vec.reshape(B, -1))
        gv = None
        if p.guidance_embed:
            gq = guidance.reshape(-1).float()
            gv = (gq if gq.numel() == B else gq[:1].expand(B))[:, None].expand(B, 2).reshape(-1).contiguous()
        self._vec_chain(self.TVAL, self.YIN, gv, self.HVEC, self.VEC)
        self._modulations()

    @on_own_device
    def precompute_conditioning(self, timesteps, y, concept_vec, guidance=None):
        """Conditioning vectors and every block's adaLN modulation for ALL diffusion steps (and all work items of
        a batch: y / concept_vec (B,768)) up front -- they depend only on (t, guidance, y), never on the
        activations: the 6.4 GB of modulation weights are streamed once per 4 vectors instead of once per step.
        Step i is then selected with ``cond_slot=i`` in the model call.  Same arithmetic as the in-call path
        (modified_flux_dit.py:99-119, flux/modules/layers.py:113-126)."""
        p, W, dev = self.params, self.weights, self.device
        if p.guidance_embed and guidance is None:
            raise ValueError("Didn't get guidance strength for guidance distilled model.")
        n = len(timesteps)
        y = y.reshape(-1, p.vec_in_dim)
        B = y.shape[0]
        H = p.hidden_size
        f32 = dict(device=dev, dtype=torch.float32)
        # row order: step, item, (vec | concept_vec)
        tv = ops.host_values([float(t) for t in timesteps for _ in range(2 * B)], dev)
        hv = torch.empty(2 * B * n, H, **f32)
        vecs = torch.empty(2 * B * n, H, **f32)
        yin = torch.empty(n, B, 2, p.vec_in_dim, **f32)
        yin[:, :, 0] = y.float()
        yin[:, :, 1] = concept_vec.reshape(B, -1).float()
        yin = yin.view(2 * B * n, -1)
        gv = None
        if p.guidance_embed:
            gq = ops.host_values(guidance, dev).reshape(-1)
            gv = (gq if gq.numel() == B else gq[:1].expand(B))[None, :, None].expand(n, B, 2).reshape(-1).contiguous()
        mod = torch.empty(n, B, 2, W.mod_rows, **f32)
        mod2 = mod.view(2 * B * n, W.mod_rows)
        self._vec_chain(tv, yin, gv, hv, vecs)
        self._modulation_rows(vecs, mod2)
        self._mod_steps = mod
        return n

    def _modulation_rows(self, vecs, mod2):
        """mod2[v] = Modulation.lin(silu(vecs[v])) of every block for all vectors v.  As two bf16 MFMA GEMMs over the
        stacked [sum N, H] weights (silu(vec) split into hi + lo bf16 planes: ~16 mantissa bits; ops.modulation_gemm),
        which stream the 6.4 GB of weights twice in all; where the shape does not fit that kernel, by weight-streaming
        GEMV launches of 4 vectors (4 x 3072 fp32 inputs leave room for 3 workgroups per CU in LDS; with 8 the weight
        stream drops from 5.3 to 2.2 TB/s: tools/gemv_bench.py), i.e. once per 4 vectors."""
        W = self.weights
        # (the GEMM for ANY vector count: the per-call and the all-steps path must round alike)
        if getattr(W, "mod_ones", None) is None:
            W.mod_ones = torch.ones(W.mod_rows, device=self.device, dtype=torch.float32)
        if ops.modulation_gemm(vecs, W.mod_w, W.mod_b, mod2, W.mod_ones):
            return
        for r0 in range(0, vecs.shape[0], 4):
            r = slice(r0, min(r0 + 4, vecs.shape[0]))
            ops.gemv(vecs[r], W.mod_w, W.mod_b, mod2[r], silu_input=True)

    def _modulations(self):
        """Every block's adaLN shift/scale/gate from VEC (rows 2j / 2j+1 = vec / concept_vec of item j) by
        weight-streaming launches of at most 4 vectors (Modulation, flux/modules/layers.py:113-126)."""
        mod2 = self.MOD.view(-1, self.weights.mod_rows)
        self._modulation_rows(self.VEC[:mod2.shape[0]], mod2)
        self._mod_cur = self.MOD

    def _ones_gate(self, n: int) -> torch.Tensor:
        g = getattr(self, "_ones_gate_vec", None)
        if g is None or g.shape[0] != n:
            g = self._ones_gate_vec = torch.ones(n, device=self.device, dtype=torch.float32)
        return g

    def _layer_route(self, i, C, return_vectors, heatmaps) -> LayerRoute:
        """The route of double block ``i`` with C concept tokens, from the settings in ROUTE_SETTINGS alone."""
        maps = heatmaps is not None
        capture = bool(return_vectors or (maps and any(i in h.layer_indices for h in heatmaps)))
        fp8 = self.precision == "fp8" and i not in self.keep_bf16_layers
        # fp8 mode: the qkv projection of a layer whose maps are requested stays bf16.  Its q / k / v ARE the vectors of
        # that layer's maps, and e4m3's 3 mantissa bits on their GEMM operands cost a map 2-4e-2 against the fp32 oracle
        # (tests/test_full_depth_gpu.py::test_fp8_forward_full_size_vs_fp32_oracle); proj and the MLP reach a map only
        # through the residual stream.  25 % of a double block's projection FLOPs.
        fp8_qkv = fp8 and not (capture and self.fp8_bf16_qkv_when_captured)
        # The bf16 rounding of the qkv GEMM's operand is ~90 % of the cross-space heat-map error and reaches a single
        # output-space map through q (tests/tools/error_budget.py: 3.3e-3 -> 3.5e-4 per cross-space map; 7.8e-4 ->
        # 2.5e-4 per output-space map, tests/tools/diag_out_space.py): the LayerNorm writes a second bf16 plane with
        # what the rounding drops, and the q weights are applied to it as well (+0.45 % FLOPs per call).
        split = capture and not fp8_qkv and self.residual_dtype == torch.float32 and C > 0
        indep = split and self.capture_independent_image
        qk16 = self.qk_f16 == "all" or (self.qk_f16 == "captured" and capture and not self.capture_independent_image)
        use_part = (capture and maps and not indep and self.epilogue_logits and self.fused_heatmaps
                    and ops.heatmap_fused_fits(C, self.hidden_size))
        return LayerRoute(capture, fp8, fp8_qkv, split, indep, qk16, use_part, f32img=capture and maps and not use_part)

    # ---- the projection problems of a double block over one row range.  ``stream`` / the weight name select the image
    # or the text weights; the concept rows use the text weights, inside the [concept | text] range of a forward or on
    # their own in a re-query.  (a8 / a8s: the e4m3 image of the operand and its row scales, fp8 mode only)
    def _qkv_problem(self, b, stream, xm, qkv, rope, qpre, split, qk16, fp8_qkv=False, a8=None, a8s=None):
        """qkv with QK-RMSNorm and RoPE in the epilogue; ``qpre``: where the pre-RoPE q goes (None: nowhere)."""
        W, a = self.weights, f"{b}{stream}_attn."
        return self._gemm(fp8_qkv, xm, a8, a8s, a + "qkv.weight", W.tensors.get(a + "qkv.bias"), qkv,
                          L.EPI_QKV_NORM_ROPE, n_split=3 * self.hidden_size, norm_q=W[a + "norm.query_norm.scale"],
                          norm_k=W[a + "norm.key_norm.scale"], rope=rope, q_prerope=qpre, q_out_scale=Q_OUT_SCALE,
                          qpre_raw=split, qk_f16=qk16)

    def _q_low_plane_problem(self, b, stream, xml, q_out, rope, qpre, qk16):
        """The q weights applied to the low plane of the LayerNorm output (``split``): added to the raw projection in
        ``qpre``, normalised there, and the rotated, scaled q written to ``q_out``."""
        W, a, H = self.weights, f"{b}{stream}_attn.", self.hidden_size
        return ops.Gemm(xml, W[a + "qkv.weight"][:H], None, q_out, epilogue=L.EPI_QKV_NORM_ROPE, n_split=3 * H,
                        norm_q=W[a + "norm.query_norm.scale"], norm_k=W[a + "norm.key_norm.scale"], rope=rope,
                        q_prerope=qpre, q_out_scale=Q_OUT_SCALE, qpre_add=True, qk_f16=qk16)

    def _gated_problem(self, lin, a, x, fp8=False, a8=None, a8s=None, **gates):
        """x += gate * (a @ W.T + bias): proj and the second MLP matrix."""
        return self._gemm(fp8, a, a8, a8s, lin + ".weight", self.weights[lin + ".bias"], x, L.EPI_GATE_RESIDUAL,
                          resid=x, **gates)

    def _mlp_in_problem(self, lin, xm, hid, fp8=False, a8=None, a8s=None):
        return self._gemm(fp8, xm, a8, a8s, lin + ".weight", self.weights[lin + ".bias"], hid, L.EPI_GELU_TANH)

    def _double_block(self, i, g, joint_attention_kwargs=None, out=None, return_vectors=False, heatmaps=None):
        """ModifiedDoubleStreamBlock.forward (modified_double_stream_block.py:69-204) on the resident X rows
        [concepts | text | image] of all work items; 7 launches."""
        p, W = self.params, self.weights
        H, NH = p.hidden_size, p.num_heads
        B, C, T, Li, oT, oI, n = g.B, g.C, g.T, g.L, g.oT, g.oI, g.n
        X, XM, QKV, ATT, HID = self.X, self.XM, self.QKV, self.ATT, self.HID
        qs, ks, vs = QKV[:, :H], QKV[:, H:2 * H], QKV[:, 2 * H:]
        cross = self_ = True
        if joint_attention_kwargs is not None:
            cross = joint_attention_kwargs.get("concept_cross_attention", True)
            self_ = joint_attention_kwargs.get("concept_self_attention", True)
        b = f"double_blocks.{i}."
        im, tm = b + "img_mod.lin", b + "txt_mod.lin"
        route = self._layer_route(i, C, return_vectors, heatmaps)
        capture, fp8, fp8_qkv, split, indep, qk16, use_part, f32img = route
        if fp8:
            XM8, XMS, ATT8, ATTS, HID8, HIDS = self.XM8, self.XMS, self.ATT8, self.ATTS, self.HID8, self.HIDS
            xm_out = dict(out=XM8, out_scale=XMS)
        else:
            XM8 = XMS = ATT8 = ATTS = HID8 = HIDS = None
            xm_out = dict(out=XM)
        xm_out_qkv = xm_out if fp8_qkv else dict(out=XM)

        def rows(t, lo, hi):
            return None if t is None else t[lo:hi]

        def segs(sh, sc):
            """LayerNorm-modulate segments in row order: concept rows (concept_vec), text rows, image rows of
            every item; sh / sc = chunk index of shift / scale in the block's modulation."""
            return ([((j + 1) * C, self._mod(tm, 1, sh, j), self._mod(tm, 1, sc, j)) for j in range(B)] +
                    [(oT + (j + 1) * T, self._mod(tm, 0, sh, j), self._mod(tm, 0, sc, j)) for j in range(B)] +
                    [(oI + (j + 1) * Li, self._mod(im, 0, sh, j), self._mod(im, 0, sc, j)) for j in range(B)])

        gs = 0 if B == 1 else self._mod_cur.stride(0)   # floats between consecutive items' gate vectors
        # K4: LayerNorm + (1+scale)*x+shift, per row range and item (:88-89,94-95,100-101)
        ops.ln_modulate(X, segments=[sg for sg in segs(0, 1) if sg[0] > 0], **xm_out_qkv,
                        **({"out_lo": self.XML} if split else {}))
        # K5+K6+K7: qkv projections (image stream + [concept|text] stream in one grouped launch) with
        # QK-RMSNorm and RoPE fused into the epilogue; pre-RoPE q kept for the cross-attention maps
        qpre = self.QPRE if capture else None
        ops.gemm([self._qkv_problem(b, "img", XM[oI:], QKV[oI:], self.ROPE[oI:], rows(qpre, oI, n), split, qk16,
                                    fp8_qkv, rows(XM8, oI, n), rows(XMS, oI, n)),
                  self._qkv_problem(b, "txt", XM[:oI], QKV[:oI], self.ROPE[:oI], rows(qpre, 0, oI), split, qk16,
                                    fp8_qkv, rows(XM8, 0, oI), rows(XMS, 0, oI))])
        if split:
            # the q weights applied to the low plane of y -- image rows and concept rows; text rows are not captured --
            # with the correction, the RMS norm, the rotation and the store of the ATTENTION's q fused into that launch's
            # epilogue: the main launch leaves the hi plane's raw q projection in QPRE, this one adds its own product,
            # normalises (QPRE <- the cross-attention-space vectors, fp32) and writes the rotated, scaled q over what the
            # main epilogue formed from bf16(y) -- or, with capture_independent_image, to QACC: q / k / the attention
            # output that feeds proj then stay exactly as in an uncaptured layer.
            # (256 x 256 tiles named: the automatic choice prices the concept rows' problem and lands on 256 x 128,
            # 376 vs 332 us per 5-item launch)
            q_acc = self.QACC if indep else qs
            ops.gemm([self._q_low_plane_problem(b, "img", self.XML[oI:], q_acc[oI:], self.ROPE[oI:], qpre[oI:], qk16),
                      self._q_low_plane_problem(b, "txt", self.XML[:oT], q_acc[:oT], self.ROPE[:oT], qpre[:oT], qk16)],
                     L.TILE_PP_256x256)

        # K8+K9: per item, joint text+image attention and the concept rows; one launch (concept problems first)
        def concept_problem(j, q_rows, out_rows, out32):
            cj, ij = slice(j * C, (j + 1) * C), slice(oI + j * Li, oI + (j + 1) * Li)
            if cross and self_:
                return ops.Attn(q_rows[cj], out_rows[cj], ks[cj], vs[cj], ks[ij], vs[ij], out_f32=out32)
            if cross:   # :129-138 image keys/values only
                return ops.Attn(q_rows[cj], out_rows[cj], ks[ij], vs[ij], out_f32=out32)
            return ops.Attn(q_rows[cj], out_rows[cj], ks[cj], vs[cj], out_f32=out32)   # :139-147 concept keys/values only
        probs = []
        if C > 0 and (cross or self_):
            for j in range(B):   # (independent mode: the rounded-q rows feed proj; the fp32 rows of the maps come below)
                probs.append(concept_problem(j, qs, ATT, None if indep else self.ATT32[j * C:(j + 1) * C]))
        if C > 0 and not (cross or self_):   # :157-159 concept_attn = concept_v
            ATT[:oT].copy_(vs[:oT])
            self.ATT32[:oT].copy_(vs[:oT])
        if use_part and probs:
            # the concept rows first, in their own launch (102 us for a 5-item layer): the main problems' epilogues read
            # ATT32.  (A bandwidth-style kernel for these <= 8-row problems -- keys split over workgroups, fp32 scores --
            # was built and measured at the same 100 us and the same maps: removed again)
            ops.attention(probs, NH, q_prescaled=True, qk_f16=qk16)
            probs = []
        for j in range(B):
            tj, ij = slice(oT + j * T, oT + (j + 1) * T), slice(oI + j * Li, oI + (j + 1) * Li)
            hm_kw = dict(hm_con=self.ATT32[j * C:(j + 1) * C], hm_part=self.PART[j]) if use_part else {}
            probs.append(ops.Attn(qs[tj], ATT[tj], ks[tj], vs[tj], ks[ij], vs[ij], q1=qs[ij], out1=ATT[ij],
                                  out_f32=self.ATTI32[j] if (f32img and not indep) else None, **hm_kw))
        if indep:
            # the maps' side: the accurate q of the image rows against the same keys / values, into rows that only the
            # heat maps read (one more problem per item in this launch) ...
            for j in range(B):
                tj, ij = slice(oT + j * T, oT + (j + 1) * T), slice(oI + j * Li, oI + (j + 1) * Li)
                probs.append(ops.Attn(self.QACC[ij], self.ATTM[ij], ks[tj], vs[tj], ks[ij], vs[ij],
                                      out_f32=self.ATTI32[j, T:] if f32img else None))
        # (at most 3 B <= 15 problems: __call__ admits 5 items)
        ops.attention(probs, NH, q_prescaled=True, qk_f16=qk16)
        if indep and C > 0 and (cross or self_):
            # ... and of the concept rows (B tiny problems: their own launch, the first one is full at 5 items)
            ops.attention([concept_problem(j, self.QACC, self.ATTM, self.ATT32[j * C:(j + 1) * C]) for j in range(B)],
                          NH, q_prescaled=True, qk_f16=qk16)
        if capture:
            self._capture(out, i, g, NH, return_vectors, heatmaps, route)
        if fp8:
            ops.quantize_rows_fp8(ATT, ATT8, ATTS)
        # K12: proj + gated residual (:194,198,201); concept rows use txt weights + concept gate
        img_gate = dict(gate_stride=gs, gate_item_rows=Li)

        def txt_gate(chunk):
            return dict(gate=self._mod(tm, 1, chunk), gate2=self._mod(tm, 0, chunk), gate_rows=oT, gate_stride=gs,
                        gate_item_rows=max(C, 1), gate2_item_rows=T)
        ops.gemm([self._gated_problem(b + "img_attn.proj", ATT[oI:], X[oI:], fp8, rows(ATT8, oI, n), rows(ATTS, oI, n),
                                      gate=self._mod(im, 0, 2), **img_gate),
                  self._gated_problem(b + "txt_attn.proj", ATT[:oI], X[:oI], fp8, rows(ATT8, 0, oI), rows(ATTS, 0, oI),
                                      **txt_gate(2))])
        # K13: LN + modulate + MLP + gated residual (:196,199,202)
        ops.ln_modulate(X, segments=[sg for sg in segs(3, 4) if sg[0] > 0], **xm_out)
        ops.gemm([self._mlp_in_problem(b + "img_mlp.0", XM[oI:], HID[oI:], fp8, rows(XM8, oI, n), rows(XMS, oI, n)),
                  self._mlp_in_problem(b + "txt_mlp.0", XM[:oI], HID[:oI], fp8, rows(XM8, 0, oI), rows(XMS, 0, oI))])
        if fp8:
            ops.quantize_rows_fp8(HID, HID8, HIDS)
        ops.gemm([self._gated_problem(b + "img_mlp.2", HID[oI:], X[oI:], fp8, rows(HID8, oI, n), rows(HIDS, oI, n),
                                      gate=self._mod(im, 0, 5), **img_gate),
                  self._gated_problem(b + "txt_mlp.2", HID[:oI], X[:oI], fp8, rows(HID8, 0, oI), rows(HIDS, 0, oI),
                                      **txt_gate(5))])

    def _single_block(self, i, g):
        """ModifiedSingleStreamBlock.forward (modified_single_stream_block.py:43-56) on the [text | image] rows of
        all work items; 4 launches."""
        p, W = self.params, self.weights
        H, NH = p.hidden_size, p.num_heads
        B, T, Li, oT, oI = g.B, g.T, g.L, g.oT, g.oI
        xs, xms, qkvs, CAT = self.X[oT:], self.XM[oT:], self.QKV[oT:], self.CAT
        nT = B * T                       # rows of xs that are text; image rows follow
        b = f"single_blocks.{i}."
        m = b + "modulation.lin"
        fp8 = self.precision == "fp8"
        G = self._gemm
        segs = ([((j + 1) * T, self._mod(m, 0, 0, j), self._mod(m, 0, 1, j)) for j in range(B)] +
                [(nT + (j + 1) * Li, self._mod(m, 0, 0, j), self._mod(m, 0, 1, j)) for j in range(B)])
        if fp8:
            xm8, xms8 = self.XM8[oT:], self.XMS[oT:]
            ops.ln_modulate(xs, xm8, segs, out_scale=xms8)
        else:
            xm8 = xms8 = None
            ops.ln_modulate(xs, xms, segs)
        ops.gemm([G(fp8, xms, xm8, xms8, b + "linear1.weight", W[b + "linear1.bias"], qkvs,
                             L.EPI_QKV_NORM_ROPE, out2=CAT[:, H:], n_split=3 * H, norm_q=W[b + "norm.query_norm.scale"],
                             norm_k=W[b + "norm.key_norm.scale"], rope=self.ROPE[oT:],
                             q_out_scale=Q_OUT_SCALE, qk_f16=self.qk_f16 == "all")])
        qh, kh, vh, oh = qkvs[:, :H], qkvs[:, H:2 * H], qkvs[:, 2 * H:], CAT[:, :H]
        probs = []
        for j in range(B):
            tj, ij = slice(j * T, (j + 1) * T), slice(nT + j * Li, nT + (j + 1) * Li)
            probs.append(ops.Attn(qh[tj], oh[tj], kh[tj], vh[tj], kh[ij], vh[ij], q1=qh[ij], out1=oh[ij]))
        ops.attention(probs, NH, q_prescaled=True, qk_f16=self.qk_f16 == "all")
        if fp8:
            ops.quantize_rows_fp8(CAT, self.CAT8, self.CATS)
        gate = self._mod(m, 0, 2)
        ops.gemm([G(fp8, CAT, self.CAT8 if fp8 else None, self.CATS if fp8 else None, b + "linear2.weight",
                             W[b + "linear2.bias"], xs, L.EPI_GATE_RESIDUAL, resid=xs, gate=gate, gate2=gate,
                             gate_rows=nT, gate_stride=0 if B == 1 else self._mod_cur.stride(0),
                             gate_item_rows=T, gate2_item_rows=Li)])

    forward = __call__

    def _capture_token_maps(self, layer, g, NH, heatmaps, route):
        """The prompt-token maps of a captured layer: ONE ops.token_maps launch for all items that ask for them, over the
        q and k rows this layer's joint attention problems have just read (QKV still holds them): the attention the image
        is made with, capture_independent_image included.  No launch when no item asks."""
        H, T, Li, oT, oI = self.hidden_size, g.T, g.L, g.oT, g.oI
        qs, ks = self.QKV[:, :H], self.QKV[:, H:2 * H]
        probs = []
        for j in range(g.B if heatmaps is not None else 0):
            hm = heatmaps[j]
            if layer not in hm.layer_indices or (hm.token_space is None and hm.per_layer_token is None):
                continue
            li = hm.layer_indices.index(layer)
            table = None if hm.per_layer_token is None else hm.per_layer_token[li]
            n_tok = (hm.token_space if hm.token_space is not None else table).shape[0]
            tj, ij = slice(oT + j * T, oT + (j + 1) * T), slice(oI + j * Li, oI + (j + 1) * Li)
            probs.append(ops.TokenMaps(qs[ij], ks[tj], ks[ij], n_tok, acc=hm.token_space, weight=hm.weight, acc2=table,
                                       weight2=hm.per_layer_weight))
        _launch_apart(probs, lambda pr: (pr.acc, pr.acc2), lambda batch: ops.token_maps(
            batch, NH, 1.0, qk_f16=route.qk16, workspace=self._token_maps_workspace(batch, NH)))

    def _capture_query_maps(self, layer, g, NH, heatmaps, route):
        """The query-row maps of a captured layer: ONE ops.query_maps call for all items and both kinds that ask, over the
        q and k rows this layer's attention problems have just read (QKV still holds them).  Text rows: the first n_tok q
        rows of the item's joint [text | image] problem against its keys.  Concept rows: the q rows of the concept rows' own
        problem, concept_problem(j, qs, ..) of _double_block, against its [concept | image] keys -- on every route the q
        third of QKV (under the split the low-plane launch has left the accurate q there; under
        capture_independent_image it is the rows whose output feeds proj, as the token maps use the joint problem that
        makes the image).  All these q rows carry Q_OUT_SCALE, so scale_log2 = 1.  No launch when no item asks."""
        H, C, T, Li, oT, oI = self.hidden_size, g.C, g.T, g.L, g.oT, g.oI
        qs, ks = self.QKV[:, :H], self.QKV[:, H:2 * H]
        probs = []
        for j in range(g.B if heatmaps is not None else 0):
            hm = heatmaps[j]
            if layer not in hm.layer_indices:
                continue
            li = hm.layer_indices.index(layer)
            cj, tj, ij = slice(j * C, (j + 1) * C), slice(oT + j * T, oT + (j + 1) * T), slice(oI + j * Li, oI + (j + 1) * Li)
            for kind, acc, tables in hm.query_kinds():
                table = None if tables is None else tables[li]
                if kind == "tokens":
                    n_tok = (acc if acc is not None else table).shape[0]
                    q, k0 = qs[tj][:n_tok], ks[tj]
                else:
                    q, k0 = qs[cj], ks[cj]
                probs.append(ops.QueryMaps(q, k0, ks[ij], acc=acc, weight=hm.weight, acc2=table, weight2=hm.per_layer_weight))
        _launch_apart(probs, lambda pr: (pr.acc, pr.acc2), lambda batch: ops.query_maps(
            batch, NH, 1.0, qk_f16=route.qk16, workspace=self._query_maps_workspace(batch, NH)), L.QUERYMAP_MAX_PROBLEMS)

    def _maps_workspace(self, attr, need):
        """A map launch's scratch memory: the model buffer ``attr``, allocated on first use and grown on demand (None
        while the kernel needs none)."""
        if need == 0:
            return None
        ws = getattr(self, attr, None)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, device=self.device, dtype=torch.uint8)
            setattr(self, attr, ws)
        return ws

    def _query_maps_workspace(self, probs, NH):
        """ops.query_maps' scratch memory (8 bytes per head and query row)."""
        return self._maps_workspace("_querymap_ws", ops.query_maps_workspace_bytes(probs, NH))

    def _capture_head_maps(self, layer, g, NH, heatmaps):
        """The per-head maps of a captured layer: ONE ops.head_maps launch (per norm) for all items and spaces that ask,
        over rows this layer has just written: ATT32 / ATTI32 (output space), QPRE (cross space), the v third of QKV
        (value space).  No launch when no item asks."""
        H, C, T, Li, oI = self.hidden_size, g.C, g.T, g.L, g.oI
        launches = {}   # norm -> problems
        for j in range(g.B if heatmaps is not None and C > 0 else 0):
            hm = heatmaps[j]
            if layer not in hm.layer_indices:
                continue
            cj, ij = slice(j * C, (j + 1) * C), slice(oI + j * Li, oI + (j + 1) * Li)
            for hr, (name, heads, raw) in ((hr, s) for hr in hm.head_requests() for s in hr.head_spaces()):
                if name == "output":
                    img, con = self.ATTI32[j, T:], self.ATT32[cj]
                elif name == "cross":
                    img, con = self.QPRE[ij], self.QPRE[cj]
                else:
                    img, con = self.QKV[ij, 2 * H:], self.QKV[cj, 2 * H:]
                if hr.head_normalize_concepts:
                    # (C x hidden elements with torch: not a hot path; the launch reads a normalised copy)
                    con = linear_normalization(con.float(), dim=0).contiguous()
                launches.setdefault(L.NORM_NONE if hr.head_norm is None else hr.head_norm, []).append(
                    ops.HeadMaps(img, con, heads=heads, weight_h=hm.weight, acc=raw, weight=hm.weight))
        for norm, probs in launches.items():
            _launch_apart(probs, lambda pr: (pr.heads, pr.acc), lambda batch, norm=norm: ops.head_maps(batch, NH, norm),
                          L.HEATMAP_MAX_PROBLEMS)

    def _prop_buffer(self, key, C, Li):
        """One of the propagated maps' fp32 [C, L] model buffers (allocated on first use, kept for the next forward),
        zeroed on the stream."""
        bufs = self.__dict__.setdefault("_prop_bufs", {})
        t = bufs.get(key)
        if t is None or tuple(t.shape) != (C, Li):
            t = bufs[key] = torch.empty(C, Li, device=self.device, dtype=torch.float32)
        return t.zero_()

    def _propagated_sources(self, layer, g, heatmaps) -> dict:
        """{(item, space): zeroed fp32 [C, L] model buffer} for every item and space that asks for propagated maps in this
        layer: _heatmap_updates leaves the layer's own map there.  Empty, and nothing launched, when no item asks."""
        self._prop_layer = {}
        for j in range(g.B if heatmaps is not None else 0):
            hm = heatmaps[j]
            if layer in hm.layer_indices:
                for space, _, _ in hm.prop_spaces():
                    self._prop_layer[j, space] = self._prop_buffer((j, space, "map"), g.C, g.L)
        return self._prop_layer

    def _capture_propagated(self, layer, g, NH, heatmaps, route):
        """The propagated maps of a captured layer: prop += weight * (A^n . map), with map the layer's own concept map
        (_propagated_sources: what _heatmap_updates has just added, times weight, into out_space / cross_space) and A the
        head mean of the image rows' softmax over the image keys ONLY (row-stochastic: a constant map stays constant), over
        the q and k rows this layer's joint attention problems have just read (QKV still holds them; the rows
        _capture_token_maps reads, which carry Q_OUT_SCALE, so scale_log2 = 1).  n = prop_steps launches per item and
        space: step s < n goes into one of two zeroed scratch buffers at weight 1, the last one into prop at hm.weight;
        all items and both spaces of a step share one ops.propagate_maps call.  No launch when no item asks."""
        sources = self._prop_layer
        if not sources:
            return
        H, Li, oI = self.hidden_size, g.L, g.oI
        qs, ks = self.QKV[:, :H], self.QKV[:, H:2 * H]
        steps = max(heatmaps[j].prop_steps for j, _ in sources)
        cur = dict(sources)
        for s in range(steps):
            probs = []
            for (j, space), src in cur.items():
                hm = heatmaps[j]
                if s >= hm.prop_steps:
                    continue
                ij = slice(oI + j * Li, oI + (j + 1) * Li)
                if s == hm.prop_steps - 1:
                    dst, w = (hm.prop_out if space == "output" else hm.prop_cross), hm.weight
                else:
                    dst, w = self._prop_buffer((j, space, s & 1), g.C, Li), 1.0
                    cur[j, space] = dst
                probs.append(ops.PropagateMaps(qs[ij], None, ks[ij], src, acc=dst, weight=w))
            _launch_apart(probs, lambda pr: (pr.acc,), lambda batch: ops.propagate_maps(
                batch, NH, 1.0, qk_f16=route.qk16, workspace=self._maps_workspace(
                    "_propmap_ws", ops.propagate_maps_workspace_bytes(batch, NH))), L.PROPMAP_MAX_PROBLEMS)

    def _token_maps_workspace(self, probs, NH):
        """ops.token_maps' scratch memory (none today: the head sum lives in LDS)."""
        return self._maps_workspace("_tokmap_ws", ops.token_maps_workspace_bytes(probs, NH))

    def _capture(self, out, layer, g, NH, return_vectors, heatmaps, route):
        """Dict capture (modified_double_stream_block.py:185-191) and/or fused heat-map update, per work item;
        ``route``: this layer's LayerRoute, which says where the attention left the output-space logits' inputs."""
        ATT, QPRE = self.ATT, self.QPRE
        B, C, Li, oT, oI = g.B, g.C, g.L, g.oT, g.oI

        def operands(j):
            # output space: the C concept rows come from the fp32 copy the attention kernel wrote
            # (their bf16 rounding, multiplied by the large component all attention outputs share,
            # is the dominant heat-map error otherwise -- DESIGN.md "tolerance")
            cj, ij = slice(j * C, (j + 1) * C), slice(oI + j * Li, oI + (j + 1) * Li)
            img_out = None if route.use_part else self.ATTI32[j, g.T:]   # (a layer with maps has use_part or f32img)
            return ((img_out, self.ATT32[cj], self.PART[j] if route.use_part else None), (QPRE[ij], QPRE[cj], None))
        self._heatmap_updates(layer, C, heatmaps, operands, self.LOGITS, self._propagated_sources(layer, g, heatmaps))
        self._capture_propagated(layer, g, NH, heatmaps, route)
        self._capture_token_maps(layer, g, NH, heatmaps, route)
        self._capture_query_maps(layer, g, NH, heatmaps, route)
        self._capture_head_maps(layer, g, NH, heatmaps)
        if return_vectors:
            H = self.hidden_size
            cf = torch.contiguous_format
            out["output_space_concept_vectors"].append(ATT[:oT].view(B, C, H).clone())
            out["output_space_image_vectors"].append(ATT[oI:].view(B, Li, H).clone())
            # the reference stores post-QKNorm, pre-RoPE q per head: [B, heads, tokens, 128]; in the
            # self-attention-only ablation it rebinds concept_q to the post-RoPE tensor (:140), which
            # for the all-zero concept ids is the same values.  (clone, not .contiguous(): for C = 1 the permuted
            # view already counts as contiguous and would keep aliasing QPRE, which the next block overwrites)
            # (QPRE is fp32 on the device; the dict carries the activations' dtype, as the reference's does)
            out["cross_attention_concept_vectors"].append(
                QPRE[:oT].view(B, C, NH, 128).permute(0, 2, 1, 3).to(torch.bfloat16, memory_format=cf, copy=True))
            out["cross_attention_image_vectors"].append(
                QPRE[oI:].view(B, Li, NH, 128).permute(0, 2, 1, 3).to(torch.bfloat16, memory_format=cf, copy=True))

    def _heatmap_updates(self, layer, C, heatmaps, operands, logits, layer_maps=None):
        """The heat-map updates of one captured layer for every work item whose request names it.  ``operands(j)``: item
        j's (image vectors, concept vectors, per-head partial logits or None) of the output space and of the
        cross-attention space -- the forward's own buffers, or in a re-query the image side a trace kept; ``logits``: fp32
        [>= C, L] scratch of the three-launch form.  ``layer_maps``: {(item, space): zeroed fp32 [C, L]} that receives the
        layer's own map of that space as the launch's second accumulator at weight 1 (fma(1, x, 0) is x: the bits the first
        accumulator is given; such a space has no per-layer table, _check_propagated)."""
        layer_maps = layer_maps or {}
        # one launch per layer: ca_heatmap_fused up to 8 concepts, ca_heatmap_many for 9 .. 32 (the concept vectors through
        # LDS in chunks; its image vectors are the fp32 rows ATTI32, as use_part needs C <= 8); the three-launch form
        # otherwise (fused_heatmaps = False, the parity reference, or more than 32 concepts with the softmax)
        launch = None
        if self.fused_heatmaps and ops.heatmap_fused_fits(C, self.hidden_size):
            launch = ops.heatmap_fused
        elif self.fused_heatmaps and ops.heatmap_many_fits(C, self.hidden_size):
            launch = ops.heatmap_many
        fused = launch is not None
        launches = {}   # norm -> problems of this layer: ONE launch for all work items and both spaces
        for j, hm in enumerate(heatmaps if heatmaps is not None else ()):
            if layer not in hm.layer_indices:
                continue
            li = hm.layer_indices.index(layer)
            (img_out, con_out, part), (img_q, con_q, _) = operands(j)
            for space, img_vec, con_vec, acc, table in (("output", img_out, con_out, hm.out_space, hm.per_layer_out),
                                                        ("cross", img_q, con_q, hm.cross_space, hm.per_layer_cross)):
                if acc is None and table is None:
                    continue
                second, w2 = (None if table is None else table[li]), hm.per_layer_weight
                if (j, space) in layer_maps:
                    second, w2 = layer_maps[j, space], 1.0
                if fused:
                    launches.setdefault(hm.norm, []).append(ops.Heatmap(
                        img_vec, None if img_vec is None else con_vec, acc, hm.weight, second, w2,
                        part=part if img_vec is None else None))
                    continue
                # the three-launch form (more than 32 concepts, or fused_heatmaps = False: the parity reference)
                ops.heatmap_logits(img_vec, con_vec, logits[:C])
                if acc is not None:
                    ops.heatmap_norm_accumulate(logits[:C], acc, hm.weight, hm.norm)
                if second is not None:
                    ops.heatmap_norm_accumulate(logits[:C], second, w2, hm.norm)
        for norm, probs in launches.items():        # one launch per norm
            _launch_apart(probs, lambda pr: (pr.acc, pr.acc2), lambda batch, norm=norm: launch(batch, norm),
                          L.HEATMAP_MAX_PROBLEMS)

    # ------------------------------------------------------------------ concept re-query
    @torch.no_grad()
    @on_own_device
    def requery(self, step_traces, concepts, concept_ids, heatmaps) -> None:
        """New concept rows against the kept image side of B <= 5 traced items of one geometry: the concept stream of
        the double blocks alone (txt_in, then per block LayerNorm, qkv, the concept attention over [own keys | kept image
        keys], the heat-map capture, proj and the MLP with the text weights and the kept concept modulation).  No image
        or text row is computed and no single block runs.

        ``step_traces``: B per-item StepTraces (``StepTrace.items()``; the trace of a one-item forward is its own
        item); ``concepts`` (B, C', 4096), C' >= 1, any C' whatever the traced forward's was; ``concept_ids`` (B, C', 3);
        ``heatmaps``: one HeatmapRequest per item, its layers a subset of the traced ones.  The concept rows take every
        block's route of the tracing forward (a layer it captured keeps the accurate q whether or not this call asks for
        its maps), so a layer's maps do not depend on which other layers are asked for."""
        traces = [t for t in step_traces]
        B = len(traces)
        if not 1 <= B <= min(L.ATTN_MAX_PROBLEMS, L.MAX_SEGMENTS, 5):
            raise ValueError(f"requery: 1 .. 5 traced items per call, got {B}")
        if concepts.ndim != 3 or concepts.shape[0] != B or concepts.shape[1] < 1:
            raise ValueError("requery: concepts must be (B, C' >= 1, context_in_dim), one row set per traced item")
        C = concepts.shape[1]
        if concept_ids.reshape(-1, 3).shape[0] != B * C:
            raise ValueError("requery: concept_ids must be (B, C', 3)")
        heatmaps = list(heatmaps) if isinstance(heatmaps, (list, tuple)) else [heatmaps]
        if len(heatmaps) != B:
            raise ValueError("requery: one HeatmapRequest per traced item")
        self._check_traceable("requery")
        t0 = traces[0]
        for t in traces:
            if t.released:
                raise ValueError("requery: the trace has been released")
            if not t.filled or t.model is not self:
                raise ValueError("requery: the trace comes from another model object (or from no forward at all)")
            if t.item is None and t.B != 1:
                raise ValueError("requery: a batched forward's trace is passed by item (StepTrace.items())")
            if (t.L, t.layers, t.split, t.qk16) != (t0.L, t0.layers, t0.split, t0.qk16):
                raise ValueError("requery: the traced items of one call must share their geometry (image tokens) and "
                                 "layer routes")
        for t, h in zip(traces, heatmaps):
            check_concept_count(h.norm, C)
            if h.token_space is not None or h.per_layer_token is not None:
                raise ValueError("requery: token maps are not part of a re-query (the text side has not changed)")
            if h.query_kinds():
                raise ValueError("requery: query-row maps are not part of a re-query (ask for them in the forward)")
            if h.prop_spaces():
                raise ValueError("requery: propagated maps are not part of a re-query (a trace keeps no image q rows)")
            if h.head_requests():
                raise ValueError("requery: per-head maps are not part of a re-query yet (ask for them in the forward)")
            missing = [l for l in h.layer_indices if l not in t.layers]
            if missing:
                raise ValueError(f"requery: layer_indices {missing} lie outside the trace (traced layers {list(t.layers)})")
        blocks = 1 + max((l for h in heatmaps for l in h.layer_indices), default=-1)
        p, W, H, dev = self.params, self.weights, self.hidden_size, self.device
        N = B * C
        bf = dict(device=dev, dtype=torch.bfloat16)
        f32 = dict(device=dev, dtype=torch.float32)
        # the concept rows' own activation set (a few hundred KB): allocated per call, on the caller's stream
        R = dict(X=torch.empty(N, H, device=dev, dtype=self.residual_dtype), XM=torch.empty(N, H, **bf),
                 XML=torch.empty(N, H, **bf), QKV=torch.empty(N, 3 * H, **bf), ATT=torch.empty(N, H, **bf),
                 ATT32=torch.empty(N, H, **f32), QPRE=torch.empty(N, H, **f32), HID=torch.empty(N, p.mlp_hidden, **bf),
                 ROPE=torch.empty(N, 64, 2, **f32), LOGITS=torch.empty(C, t0.L, **f32),
                 MOD=torch.empty(B, W.mod_rows, **f32))
        txt_in = torch.empty(N, p.context_in_dim, **bf)
        txt_in.copy_(concepts.reshape(N, -1))
        for j, t in enumerate(traces):
            R["MOD"][j].copy_(t.mod[t.item or 0])
        self._rope_fill(concept_ids.reshape(-1, 3), R["ROPE"])
        ops.gemm([ops.Gemm(txt_in, W["txt_in.weight"], W["txt_in.bias"], R["X"])])
        for i in range(blocks):
            self._requery_block(i, B, C, R, traces, heatmaps, last=i == blocks - 1)

    def _requery_block(self, i, B, C, R, traces, heatmaps, last=False) -> None:
        """The concept rows' part of ``_double_block`` for block ``i``: the same problems over the rows R, their second
        key / value segment and the heat maps' image operands from the traces; 7 launches, 9 in a captured layer.
        ``last``: nothing reads the residual stream after this block's maps, so it ends there."""
        H, NH = self.hidden_size, self.params.num_heads
        X, XM, QKV, ATT, ATT32, HID, MOD = R["X"], R["XM"], R["QKV"], R["ATT"], R["ATT32"], R["HID"], R["MOD"]
        qs, ks, vs = QKV[:, :H], QKV[:, H:2 * H], QKV[:, 2 * H:]
        b = f"double_blocks.{i}."
        o = self.weights.mod_offset[b + "txt_mod.lin"]
        captured, split, qk16 = i in traces[0].layers, traces[0].split[i], traces[0].qk16[i]

        def mod(chunk, j=0):
            return MOD[j, o + chunk * H:o + (chunk + 1) * H]

        def segs(sh, sc):
            return [((j + 1) * C, mod(sh, j), mod(sc, j)) for j in range(B)]

        def gate(chunk):
            return dict(gate=mod(chunk), gate_stride=0 if B == 1 else MOD.stride(0), gate_item_rows=C)
        ops.ln_modulate(X, out=XM, segments=segs(0, 1), **({"out_lo": R["XML"]} if split else {}))
        qpre = R["QPRE"] if captured else None
        ops.gemm([self._qkv_problem(b, "txt", XM, QKV, R["ROPE"], qpre, split, qk16)])
        if split:
            ops.gemm([self._q_low_plane_problem(b, "txt", R["XML"], qs, R["ROPE"], qpre, qk16)], L.TILE_PP_256x256)
        probs = []
        for j, t in enumerate(traces):
            cj = slice(j * C, (j + 1) * C)
            probs.append(ops.Attn(qs[cj], ATT[cj], ks[cj], vs[cj], *t.image_kv(i), out_f32=ATT32[cj]))
        ops.attention(probs, NH, q_prescaled=True, qk_f16=qk16)
        if captured:
            def operands(j):
                cj = slice(j * C, (j + 1) * C)
                img_out, img_q = traces[j].image_vectors(i)
                return (img_out, ATT32[cj], None), (img_q, R["QPRE"][cj], None)
            self._heatmap_updates(i, C, heatmaps, operands, R["LOGITS"])
        if last:
            return
        ops.gemm([self._gated_problem(b + "txt_attn.proj", ATT, X, **gate(2))])
        ops.ln_modulate(X, out=XM, segments=segs(3, 4))
        ops.gemm([self._mlp_in_problem(b + "txt_mlp.0", XM, HID)])
        ops.gemm([self._gated_problem(b + "txt_mlp.2", HID, X, **gate(5))])
