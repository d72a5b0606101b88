"""Model-level routes of HipFluxDiT (conceptattention_amd/flux_dit.py) on the tiny geometry: the case table.

Imported by tests/test_model_routes_gpu.py (the forwards) and by tests/test_model_route_cases_cpu.py (coverage of every
reachable LayerRoute by a layer of a case, names against routes, attention problems per launch).  Nothing here touches
torch.cuda at import time.

A case is a whole forward: tiny_params() (H = 256, 2 heads, 2 double blocks, 0 or 1 single block), the settings of
HipFluxDiT.ROUTE_SETTINGS that differ from the defaults, the token counts, the batch, what is returned (vector stacks,
fused heat maps of some layers, both), the concept-attention ablation flags and the norm of the maps.  The shapes are the
smallest at which the wiring can still go wrong:
  side  256 -> 256 image tokens, one full 256-row tile; 208 -> 169 tokens, no full tile: the low-plane GEMM and the
        attention run on ragged rows only
  T     8
  C     1, 3, 8 (the last size of the fused heat maps and of the attention epilogue's partial logits), 9 (the
        three-launch heat maps from fp32 image rows)
  B     1 or 3; the items differ in every input, in the timestep and in the guidance

Weights and inputs are those of test_model_gpu.tiny_case: seeded, rounded to bf16 and held as fp32, so the fp32 oracle
(oracle/flux_oracle.py) and the device path start from the same numbers.

Names are made of tokens joined by "_"; tests/test_model_route_cases_cpu.py holds every token to what route_of says.

Gates against the oracle are the tiny-model gates of tests/test_model_gpu.py for every bf16 route; fp8 routes have no
oracle and are held to the bf16 run of the same case with the gates of test_tiny_model_fp8_mode_tracks_bf16.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from types import SimpleNamespace
from typing import Optional

import torch

from conceptattention_amd import _lib as L
from conceptattention_amd.flux_dit import HipFluxDiT, LayerRoute
from conceptattention_amd.params import tiny_params

DEPTH = 2
HIDDEN = 256
DEFAULTS = dict(precision="bf16", keep_bf16_layers=frozenset(), residual_dtype=torch.float32, bf16_timesteps=False,
                fp32_latent=True, qk_f16="captured", capture_independent_image=False,
                fp8_bf16_qkv_when_captured=True, fused_heatmaps=True, epilogue_logits=True)
# the values the coverage enumeration takes per setting (bf16_timesteps / fp32_latent select no LayerRoute)
SETTING_VALUES = dict(precision=("bf16", "fp8"), keep_bf16_layers=(frozenset(), frozenset({1})),
                      residual_dtype=(torch.float32, torch.bfloat16), bf16_timesteps=(False, True), fp32_latent=(True, False),
                      qk_f16=("captured", "0", "all"), capture_independent_image=(False, True),
                      fp8_bf16_qkv_when_captured=(True, False), fused_heatmaps=(True, False), epilogue_logits=(True, False))
ENUM_C = (1, 8, 9)
MAX_ITEMS = min(L.ATTN_MAX_PROBLEMS // 2, L.MAX_SEGMENTS // 3)   # what HipFluxDiT.__call__ admits: 5

# ---- gates (tests/test_model_gpu.py: test_tiny_model_matches_oracle, test_tiny_stop_after_multimodal_and_fused_heatmaps,
# test_tiny_model_fp8_mode_tracks_bf16); no route needed a measured gate of its own
VEC_GATE = 2e-2          # x max(|oracle|max, 1), each of the four vector stacks
PRED_GATE = 3e-2         # x max(|oracle pred|max, 1)
OUT_MAP_GATE = 3e-3      # fused output-space accumulator, max-abs
CROSS_MAP_GATE = 5e-3    # fused cross-attention-space accumulator, max-abs
FP8_MAP_GATE = 3e-2      # fp8 accumulators against the bf16 run of the same case
FP8_PRED_REL_RMS = 0.10  # 0 < rel-rms(pred) < this

# Measured on MI355X, tests/test_model_routes_gpu.py (largest printed max err / gate per route family, the case and
# output it came from):
#   use_part (default route)   0.905  default_neither_b3, output-space maps: with neither ablation flag the concept
#                                     "attention" rows ARE the bf16 v rows, so the maps carry v's rounding (2.7e-3)
#   indep                      0.734  indep_neither, output-space maps (the same rows)
#   f32img, C <= 8             0.215  noepi_entmax15_c8, output-space maps
#   f32img, C = 9              0.479  c9_neither, output-space maps
#   bf16 residual              0.443  cover_bf16res_qkbf16_noepi, output-space maps
#   vectors only               0.116  cover_qkbf16_vectorsonly, output_space_image_vectors
#   fp8 against the bf16 run   0.726  fp8_fp8qkv_indepoff, cross-space maps (e4m3 qkv operands: 2.2e-2 of 3e-2)
# Every route, bf16 residual and side 208 included, is inside the existing gates: none was measured and widened.

ITEM_SEEDS = (2, 21, 22)
ITEM_TIMESTEPS = (0.75, 0.5, 0.2)
ITEM_GUIDANCE = (3.5, 2.5, 4.0)


@dataclass(frozen=True)
class Case:
    name: str
    settings: dict = field(default_factory=dict)   # over HipFluxDiT.ROUTE_SETTINGS, what differs from DEFAULTS
    C: int = 3
    T: int = 8
    side: int = 256
    B: int = 1
    return_vectors: bool = True
    layers: Optional[tuple] = (1,)                 # layers with fused maps, or None: no HeatmapRequest
    cross: bool = True                             # joint_attention_kwargs["concept_cross_attention"]
    self_: bool = True                             # joint_attention_kwargs["concept_self_attention"]
    guidance_embed: bool = False
    norm: int = L.NORM_SOFTMAX
    singles: int = 1                               # depth_single_blocks

    @property
    def L(self) -> int:
        return (-(-self.side // 16)) ** 2

    @property
    def jak(self):
        if self.cross and self.self_:
            return None
        return {"concept_cross_attention": self.cross, "concept_self_attention": self.self_}

    @property
    def fp8(self) -> bool:
        return self.settings.get("precision", "bf16") == "fp8"

    def full_settings(self) -> dict:
        return {**DEFAULTS, **self.settings}

    def bf16_twin(self) -> "Case":
        """The same case in precision "bf16": what an fp8 case is gated against."""
        s = {k: v for k, v in self.settings.items() if k not in ("precision", "keep_bf16_layers")}
        return replace(self, name=self.name + "~bf16", settings=s)


def params(case: Case):
    return tiny_params(guidance_embed=case.guidance_embed, depth=DEPTH, depth_single_blocks=case.singles)


def route_for(settings: dict, layer: int, C: int, return_vectors: bool, layers) -> LayerRoute:
    """HipFluxDiT._layer_route on a plain namespace (it reads settings only; a model needs a GPU)."""
    model = SimpleNamespace(hidden_size=HIDDEN, **{**DEFAULTS, **settings})
    heatmaps = None if layers is None else [SimpleNamespace(layer_indices=tuple(layers))]
    return LayerRoute(*(bool(v) for v in HipFluxDiT._layer_route(model, layer, C, return_vectors, heatmaps)))


def route_of(case: Case, layer: int) -> LayerRoute:
    return route_for(case.settings, layer, case.C, case.return_vectors, case.layers)


def captured_layer(case: Case) -> int:
    """The layer a case's name speaks about: the last captured one (the last layer if none is)."""
    cap = [i for i in range(DEPTH) if route_of(case, i).capture]
    return cap[-1] if cap else DEPTH - 1


def reachable_routes() -> dict:
    """Every distinct LayerRoute of the last double block over all SETTING_VALUES x ENUM_C x return_vectors x
    {no maps, maps of another layer, maps of this layer} -> one (settings, C, return_vectors, layers) that reaches it.
    (C = 0 is left out: a forward without concepts raises before any route runs.)"""
    import itertools
    seen = {}
    keys = list(SETTING_VALUES)
    for combo in itertools.product(*(SETTING_VALUES[k] for k in keys)):
        s = dict(zip(keys, combo))
        for C in ENUM_C:
            for rv in (False, True):
                for layers in (None, (0,), (1,)):
                    seen.setdefault(route_for(s, 1, C, rv, layers), (s, C, rv, layers))
    return seen


def attention_launches(route: LayerRoute, B: int, cross: bool, self_: bool) -> list:
    """Problems per ops.attention launch of one _double_block call, in launch order (C > 0)."""
    con = B if (cross or self_) else 0
    launches = []
    if route.use_part and con:
        launches.append(con)      # the concept rows first: the main problems' epilogues read ATT32
        con = 0
    launches.append(con + B + (B if route.indep else 0))
    if route.indep and (cross or self_):
        launches.append(B)        # the map side's concept rows
    return launches


def expected_attention_launches(case: Case) -> list:
    out = []
    for i in range(DEPTH):
        out += attention_launches(route_of(case, i), case.B, case.cross, case.self_)
    return out + [case.B] * case.singles


# ---------------------------------------------------------------------------------------------------------- the table
_BF, _F32 = torch.bfloat16, torch.float32
INDEP = dict(capture_independent_image=True)
FP8 = dict(precision="fp8")
NOEPI = dict(epilogue_logits=False)
UNFUSED = dict(fused_heatmaps=False)
BF16RES = dict(residual_dtype=_BF)
ABLATIONS = (("both", True, True), ("crossonly", True, False), ("selfonly", False, True), ("neither", False, False))

CASES = [
    # every setting in turn off its default: maps of layer 1 and the vector stacks
    Case("default"),
    Case("default_guidance", guidance_embed=True),
    Case("indep", INDEP),
    Case("noepi", NOEPI),
    Case("unfused", UNFUSED),
    Case("qkbf16", dict(qk_f16="0")),
    Case("qkall", dict(qk_f16="all")),
    Case("bf16res", BF16RES),
    Case("fp8", FP8),
    Case("fp8_fp8qkv", dict(FP8, fp8_bf16_qkv_when_captured=False)),
    Case("fp8_keep1", dict(FP8, keep_bf16_layers=frozenset({1}))),
    # the pairs that change wiring
    Case("indep_qkall", dict(INDEP, qk_f16="all")),
    Case("indep_c9", INDEP, C=9),
    Case("indep_fp8", dict(INDEP, **FP8)),
    Case("bf16res_indepoff", dict(INDEP, **BF16RES)),    # no split without the fp32 stream: the setting is a no-op
    Case("fp8_c9", FP8, C=9),
    Case("fp8_fp8qkv_indepoff", dict(INDEP, **FP8, fp8_bf16_qkv_when_captured=False)),   # e4m3 qkv: no split either
    Case("noepi_b3", NOEPI, B=3),
    Case("indep_b3", INDEP, B=3),
    Case("c9", C=9),
]
# the four ablation combinations under the default route (use_part), indep, C = 9 and fp8, maps and vectors requested
for _tag, _s, _C in (("default", {}, 3), ("indep", INDEP, 3), ("c9", {}, 9), ("fp8", FP8, 3)):
    for _ab, _cross, _self in ABLATIONS[1:]:             # ("both" is the plain case above)
        CASES.append(Case(f"{_tag}_{_ab}", dict(_s), C=_C, cross=_cross, self_=_self))
# ... and at B = 3, one non-trivial combination per route, all three between them (guidance differs per item too)
CASES += [
    Case("default_neither_b3", {}, B=3, cross=False, self_=False, guidance_embed=True),
    Case("indep_crossonly_b3", INDEP, B=3, cross=True, self_=False, guidance_embed=True),
    Case("c9_selfonly_b3", {}, C=9, B=3, cross=False, self_=True, guidance_embed=True),
    Case("fp8_neither_b3", FP8, B=3, cross=False, self_=False, guidance_embed=True),
    Case("default_b3", {}, B=3),
    Case("fp8_b3", FP8, B=3),
    Case("c9_unfused_b3", UNFUSED, C=9, B=3),
    # what is returned
    Case("mapsonly", return_vectors=False),
    Case("vectorsonly", layers=None),
    Case("layer0only", return_vectors=False, layers=(0,)),        # a captured and an uncaptured route in one forward
    Case("mapsonly_both_layers_c8", return_vectors=False, layers=(0, 1), C=8),
    Case("mapsonly_c1", return_vectors=False, C=1),
    Case("indep_layer0only", INDEP, return_vectors=False, layers=(0,)),
    Case("fp8_layer0only", FP8, return_vectors=False, layers=(0,)),
    # the other norms, on non-default routes
    Case("indep_sparsemax", INDEP, norm=L.NORM_SPARSEMAX),
    Case("c9_entmax15", C=9, norm=L.NORM_ENTMAX15),
    Case("noepi_entmax15_c8", NOEPI, C=8, norm=L.NORM_ENTMAX15),
    # no full row tile
    Case("s208", side=208),
    Case("indep_s208", INDEP, side=208),
    Case("fp8_s208", FP8, side=208),
    Case("c9_b3_s208", C=9, B=3, side=208),
]


def _cover(name, settings, **kw):
    return Case("cover_" + name, settings, **kw)


_VEC = dict(layers=None)                                   # vectors only: capture without logits
_L0 = dict(return_vectors=False, layers=(0,))              # layer 1 uncaptured
# routes none of the cases above reaches (tests/test_model_route_cases_cpu.py recomputes the enumeration)
CASES += [
    _cover("qkall_layer0only", dict(qk_f16="all"), **_L0),                                   # uncaptured, qk16
    _cover("fp8_fp8qkv_qkall_layer0only", dict(FP8, qk_f16="all", fp8_bf16_qkv_when_captured=False), **_L0),
    _cover("bf16res_qkbf16_vectorsonly", dict(BF16RES, qk_f16="0"), **_VEC),
    _cover("bf16res_qkbf16_noepi", dict(BF16RES, qk_f16="0", **NOEPI)),
    _cover("bf16res_vectorsonly", BF16RES, **_VEC),
    _cover("bf16res_c9", BF16RES, C=9),
    _cover("qkbf16_vectorsonly", dict(qk_f16="0"), **_VEC),
    _cover("qkbf16_unfused", dict(qk_f16="0", **UNFUSED)),
    _cover("indep_vectorsonly", INDEP, **_VEC),
    _cover("indep_qkall_vectorsonly", dict(INDEP, qk_f16="all"), **_VEC),
    _cover("fp8_bf16res_qkbf16_vectorsonly", dict(FP8, **BF16RES, qk_f16="0"), **_VEC),
    _cover("fp8_bf16res_qkbf16_c9", dict(FP8, **BF16RES, qk_f16="0"), C=9),
    _cover("fp8_bf16res_qkbf16", dict(FP8, **BF16RES, qk_f16="0")),
    _cover("fp8_bf16res_vectorsonly", dict(FP8, **BF16RES), **_VEC),
    _cover("fp8_bf16res_unfused", dict(FP8, **BF16RES, **UNFUSED)),
    _cover("fp8_bf16res", dict(FP8, **BF16RES)),
    _cover("fp8_qkbf16_vectorsonly", dict(FP8, qk_f16="0"), **_VEC),
    _cover("fp8_qkbf16_noepi", dict(FP8, qk_f16="0", **NOEPI)),
    _cover("fp8_qkbf16", dict(FP8, qk_f16="0")),
    _cover("fp8_vectorsonly", FP8, **_VEC),
    _cover("indep_fp8_vectorsonly", dict(INDEP, **FP8), **_VEC),
    _cover("indep_fp8_qkall_vectorsonly", dict(INDEP, **FP8, qk_f16="all"), **_VEC),
    _cover("indep_fp8_qkall_c8", dict(INDEP, **FP8, qk_f16="all"), C=8),
    _cover("fp8_fp8qkv_qkbf16_vectorsonly", dict(FP8, fp8_bf16_qkv_when_captured=False, qk_f16="0"), **_VEC),
    _cover("fp8_fp8qkv_qkbf16_c9", dict(FP8, fp8_bf16_qkv_when_captured=False, qk_f16="0"), C=9),
    _cover("fp8_fp8qkv_qkbf16", dict(FP8, fp8_bf16_qkv_when_captured=False, qk_f16="0")),
    _cover("fp8_fp8qkv_vectorsonly", dict(FP8, fp8_bf16_qkv_when_captured=False), **_VEC),
    _cover("fp8_fp8qkv_noepi", dict(FP8, fp8_bf16_qkv_when_captured=False, **NOEPI)),
]

BY_NAME = {c.name: c for c in CASES}

# ---- name tokens -> what route_of must say on captured_layer(case) (both ways for the first group)
ROUTE_TOKENS = {
    "indep": lambda c, r: r.indep,
    "fp8": lambda c, r: any(route_of(c, i).fp8 for i in range(DEPTH)),
    "fp8qkv": lambda c, r: r.fp8_qkv,
}
IMPLIED_TOKENS = {   # token in the name => predicate (the converse is not claimed)
    "default": lambda c, r: not c.settings,
    "noepi": lambda c, r: r.capture and not r.use_part,
    "unfused": lambda c, r: not r.use_part and not c.full_settings()["fused_heatmaps"],
    "qkbf16": lambda c, r: not r.qk16,
    "qkall": lambda c, r: all(route_of(c, i).qk16 for i in range(DEPTH)),
    "bf16res": lambda c, r: not r.split,
    "indepoff": lambda c, r: c.full_settings()["capture_independent_image"] and not r.indep,
    "keep1": lambda c, r: route_of(c, 0).fp8 and not route_of(c, 1).fp8,
    "c1": lambda c, r: c.C == 1,
    "c8": lambda c, r: c.C == 8 and (r.use_part or not c.full_settings()["epilogue_logits"] or r.indep or not r.f32img),
    "c9": lambda c, r: c.C == 9 and not r.use_part and (r.f32img or c.layers is None),
    "b3": lambda c, r: c.B == 3,
    "s208": lambda c, r: c.side == 208 and c.L == 169,
    "mapsonly": lambda c, r: not c.return_vectors and r.capture and (r.use_part or r.f32img),
    "vectorsonly": lambda c, r: c.return_vectors and c.layers is None and not r.use_part and not r.f32img,
    "layer0only": lambda c, r: route_of(c, 0).capture and not route_of(c, 1).capture,
    "both": lambda c, r: c.layers == (0, 1), "layers": lambda c, r: True,
    "crossonly": lambda c, r: c.cross and not c.self_,
    "selfonly": lambda c, r: c.self_ and not c.cross,
    "neither": lambda c, r: not c.cross and not c.self_,
    "sparsemax": lambda c, r: c.norm == L.NORM_SPARSEMAX,
    "entmax15": lambda c, r: c.norm == L.NORM_ENTMAX15,
    "guidance": lambda c, r: c.guidance_embed,
    "cover": lambda c, r: True,
}


# ---------------------------------------------------------------------------------------------- weights and inputs
_SD, _ITEMS = {}, {}


def bf(x):
    return x.bfloat16().float()


def state_dict(case: Case) -> dict:
    """test_model_gpu.tiny_case's weights (seed 1, bf16-representable fp32), cached per geometry."""
    from conceptattention_amd.weights import synthetic_state_dict
    key = (case.guidance_embed, case.singles)
    if key not in _SD:
        _SD[key] = {k: bf(v) for k, v in synthetic_state_dict(params(case), seed=1).items()}
    return _SD[key]


def item_inputs(case: Case, j: int) -> dict:
    """Work item j's inputs on the CPU (item 0 = tiny_case's, seed 2), plus ``t`` and ``guidance``."""
    from conceptattention_amd.weights import synthetic_inputs
    key = (case.C, case.T, case.side, j)
    if key not in _ITEMS:
        inp = synthetic_inputs(tiny_params(), case.side, case.side, n_txt=case.T, n_concepts=case.C, seed=ITEM_SEEDS[j])
        _ITEMS[key] = {k: (bf(v) if v.is_floating_point() else v) for k, v in inp.items()}
    return dict(_ITEMS[key], t=ITEM_TIMESTEPS[j], guidance=ITEM_GUIDANCE[j] if case.guidance_embed else None)


def oracle_key(case: Case, j: int) -> tuple:
    """What the fp32 oracle's result depends on: geometry, inputs, ablation (no route setting, no request)."""
    return (case.guidance_embed, case.singles, case.C, case.T, case.side, j, case.cross, case.self_)
