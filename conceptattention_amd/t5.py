"""The T5 encoder on the GPU: ``T5Encoder.encode_ids`` with the arithmetic of transformers' ``T5EncoderModel`` as the
reference calls it (concept_attention/flux/src/flux/modules/conditioner.py:6-38), on the HIP kernels of ca_t5.hip and the
grouped GEMM, and ``HipTextEncoder``, the ``HFEmbedder`` contract on its T5 side.

What the reference does and this file keeps.  ``HFEmbedder`` pads every string to ``max_length`` (256 for schnell, 512
for dev) and passes ``attention_mask=None``: PADDING TOKENS TAKE PART IN ATTENTION, there is no mask anywhere, and the
sequence length is always ``max_length``.  T5 attention has no 1/sqrt(d) scale; its only position signal is a learned
bias per (bucket of key - query, head) that block 0 owns and every block adds to its scores.

Precision.  The residual stream is fp32 (transformers runs it in the checkpoint's bf16); every GEMM operand is bf16,
written by the RMS norm, the attention or the gate product in front of it; accumulation, scores, softmax and norm
statistics are fp32.  ``o`` and ``wo`` add into the stream in the GEMM epilogue (EPI_GATE_RESIDUAL with a ones gate), as
``vae.attention_block`` does.  The final norm writes bf16, the dtype the DiT takes.

Packing.  q, k, v of a block are one ``[3 inner, d_model]`` weight; ``[wi_1 ; wi_0]`` one ``[2 d_ff, d_model]`` weight
whose launch stores ``wi_1 x`` plainly and ``gelu_tanh(wi_0 x)`` through EPI_SPLIT_GELU (``n_split = d_ff`` must be a
multiple of the 256-column tile: 10240 = 40 x 256, the tiny 512 = 2 x 256).  The bias table ``[heads, 2L - 1]`` indexed
by ``key - query + L - 1`` is built on the host per L, with the same fp32 torch operations transformers uses for the
bucket, and cached.

Batching.  All sequences of a call go through every launch together (rows = n_seq * L), in passes of at most
``MAX_ROWS`` rows.  Every GEMM runs on the 256 x 256 tile whatever the row count, and L = 256 and 512 fill whole row
tiles, so a sequence's bits do not depend on what else is in the batch; for another L (a multiple of 64) a sequence
would share a row tile with its neighbour or fall to the thin-row kernel depending on the batch, so those lengths run
one sequence per pass.

fp8 mode (``precision="fp8"``, opt-in; bf16 is the default and its bits are what they were).  The projections named in
``fp8_projections`` (of ``qkv``, ``o``, ``wi``, ``wo``) run on ``ca_gemm_fp8``: e4m3 operands with one fp32 scale per
row on both sides (activation row, weight output row), fp32 accumulation, the same epilogues.  The A operands are
written as e4m3 by their producers: the RMS norm in front of ``qkv`` and ``wi`` (``ca_t5_rmsnorm_f32in_fp8``) and the
gate product in front of ``wo`` (``ca_gated_mul_fp8``) own a whole row per workgroup, so the row never exists in bf16;
the attention output has 64 writers per row and goes through ``ca_quantize_rows_fp8``.  Weights: a checkpoint tensor
that arrives as ``torch.float8_e4m3fn`` is used byte for byte with unit scales; any other is rounded to bf16 as in the
bf16 mode and then quantised per output row (scale = row amax / 448).  Everything else -- the fp32 stream, attention,
the embedding, the norm weights, the bias table, the final norm and the bf16 output -- is unchanged.  A row's scale
depends on that row alone and the tile is the same one, so the batching guarantee above holds in fp8 as well.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Sequence

import torch

from . import _lib as L
from . import ops
from .params import T5Params, t5_params, tiny_t5_params
from .weights import _gen, _read_safetensors, fill_tensors, load_text_weights  # noqa: F401

__all__ = ["T5Encoder", "T5Params", "HipTextEncoder", "ToyByteTokenizer", "load_t5", "synthetic_t5_state_dict",
           "t5_state_dict_spec", "relative_position_bucket", "relative_bias_table", "FP8_PROJECTIONS"]

TIED_EMBEDDING = "encoder.embed_tokens.weight"   # transformers lists the tied input embedding under both names
PRECISIONS = ("bf16", "fp8")
FP8_PROJECTIONS = ("qkv", "o", "wi", "wo")       # the four GEMMs of a block, as packed
SCALE_KEY_SUFFIXES = (".scale_weight", ".weight_scale")   # per-tensor scales of scaled-fp8 checkpoints: not supported


# ---------------------------------------------------------------------------------------------------------- layout
def t5_state_dict_spec(p: T5Params) -> list:
    """[(name, shape)] under transformers' key names (T5EncoderModel.state_dict(), without the tied twin of
    ``shared.weight``); Linear weights are (out, in)."""
    inner = p.inner_dim
    spec = [("shared.weight", (p.vocab_size, p.d_model))]
    for i in range(p.num_layers):
        a = f"encoder.block.{i}.layer.0"
        for n in ("q", "k", "v"):
            spec.append((f"{a}.SelfAttention.{n}.weight", (inner, p.d_model)))
        spec.append((f"{a}.SelfAttention.o.weight", (p.d_model, inner)))
        if i == 0:
            spec.append((f"{a}.SelfAttention.relative_attention_bias.weight", (p.relative_attention_num_buckets, p.num_heads)))
        spec.append((f"{a}.layer_norm.weight", (p.d_model,)))
        f = f"encoder.block.{i}.layer.1"
        spec += [(f"{f}.DenseReluDense.wi_0.weight", (p.d_ff, p.d_model)),
                 (f"{f}.DenseReluDense.wi_1.weight", (p.d_ff, p.d_model)),
                 (f"{f}.DenseReluDense.wo.weight", (p.d_model, p.d_ff)),
                 (f"{f}.layer_norm.weight", (p.d_model,))]
    spec.append(("encoder.final_layer_norm.weight", (p.d_model,)))
    return spec


def synthetic_t5_state_dict(p: T5Params, seed: int = 0) -> dict:
    """Seeded on the CPU generator, one generator per tensor name (the values do not depend on the order), every value
    bf16-representable.  With u ~ U(-1, 1):

    * ``shared``: u (token rows of rms 0.58);  layer norms: 1 + 0.1 u.
    * ``q``, ``k``: u * sqrt(0.75 / d_model): q and k elements of variance ~0.25 on a unit-rms input, so a logit --
      64 products, NO 1/sqrt(d) -- has a standard deviation of about 2 nats.
    * ``relative_attention_bias``: 4 u, spanning 8 nats.  transformers' own init gives the bias d_model^-1/2 and a wrong
      bucket, a transposed table or a dropped bias would change nothing a test could see; here each moves the
      probabilities by factors.
    * ``v``, ``o``, ``wo``: u / sqrt(fan_in) (PyTorch's default bound);  ``wi_0``, ``wi_1``: u * sqrt(3 / d_model), unit
      variance before the GELU, so that its curved part (and the tanh / erf difference) is exercised.
    """
    sd = {}
    for name, shape in t5_state_dict_spec(p):
        u = torch.rand(shape, generator=_gen("t5." + name, seed, "cpu"), dtype=torch.float32) * 2 - 1
        if name.endswith("layer_norm.weight"):
            t = 1 + 0.1 * u
        elif name == "shared.weight":
            t = u
        elif name.endswith("relative_attention_bias.weight"):
            t = 4 * u
        elif ".q." in name or ".k." in name:
            t = u * math.sqrt(0.75 / p.d_model)
        elif ".wi_" in name:
            t = u * math.sqrt(3.0 / p.d_model)
        else:
            t = u / math.sqrt(shape[1])
        sd[name] = t.to(torch.bfloat16).to(torch.float32)
    return sd


# ---------------------------------------------------------------------------------------------------------- bias table
def relative_position_bucket(relative_position: torch.Tensor, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """T5Attention._relative_position_bucket, bidirectional (modeling_t5.py), operation for operation -- the logarithm is
    taken in fp32 and truncated, and which side of an integer it falls on is part of the model."""
    num_buckets //= 2
    buckets = (relative_position > 0).to(torch.long) * num_buckets
    rp = torch.abs(relative_position)
    max_exact = num_buckets // 2
    is_small = rp < max_exact
    large = max_exact + (torch.log(rp.float() / max_exact) / math.log(max_distance / max_exact)
                         * (num_buckets - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, num_buckets - 1))
    return buckets + torch.where(is_small, rp, large)


def relative_bias_table(weight: torch.Tensor, length: int, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """fp32 [heads, 2 length - 1]: entry [h, key - query + length - 1] = weight[bucket(key - query), h]."""
    off = torch.arange(-(length - 1), length, dtype=torch.long)
    b = relative_position_bucket(off, num_buckets, max_distance)
    return weight.to(torch.float32)[b].t().contiguous()


# ---------------------------------------------------------------------------------------------------------- the model
class T5Encoder:
    """``encode_ids(ids[n_seq, L]) -> [n_seq, L, d_model]`` bf16: the ``last_hidden_state`` of T5EncoderModel with
    ``attention_mask=None``.  L a multiple of 64 up to 512.

    ``precision``: "bf16" (default) or "fp8" (the module docstring's fp8 mode).  ``fp8_projections``: which of the four
    projections of a block run in e4m3 in fp8 mode; the others keep the bf16 route and its bf16 producer.  The list
    exists because real T5-XXL is known for large activation outliers in front of ``wo``: a user with real weights can
    keep that projection in bf16 (``("qkv", "o", "wi")``) without giving up the rest.  The accuracy of the fp8 mode has
    been measured on this repository's synthetic weights only; real-weight accuracy is UNMEASURED."""

    MAX_ROWS = 8192   # token rows of one pass: 16 sequences of 512; bounds the workspace and every GEMM operand (< 4 GiB)

    def __init__(self, params: T5Params, device="cuda", precision: str = "bf16",
                 fp8_projections: Sequence[str] = FP8_PROJECTIONS):
        p = params
        if precision not in PRECISIONS:
            raise ValueError(f"T5Encoder: precision must be one of {PRECISIONS}, got {precision!r}")
        if isinstance(fp8_projections, str):
            fp8_projections = (fp8_projections,)
        names = tuple(fp8_projections)
        if not names or any(n not in FP8_PROJECTIONS for n in names):
            raise ValueError(f"T5Encoder: fp8_projections must be a non-empty selection of {FP8_PROJECTIONS}, got {names!r}")
        self.precision = precision
        self.fp8 = frozenset(names) if precision == "fp8" else frozenset()   # the projections that run in e4m3
        if p.d_kv != 64:
            raise ValueError("T5Encoder: d_kv must be 64 (ca_t5_attn_bf16)")
        if p.d_model % 256 or (3 * p.inner_dim) % 256 or p.d_ff % 256:
            raise ValueError("T5Encoder: d_model, 3 * num_heads * 64 and d_ff must be multiples of 256 (the GEMM tile; "
                             "d_ff is also the SPLIT_GELU boundary)")
        if p.vocab_size < 1 or p.num_layers < 1 or p.num_heads < 1:
            raise ValueError("T5Encoder: empty geometry")
        self.params = p
        self.device = torch.device(device)
        self.spec = dict(t5_state_dict_spec(p))
        self.tensors: dict = {}      # name -> fp32 host copy as loaded
        self.e4m3: set = set()       # names that arrived as torch.float8_e4m3fn (their fp32 copy holds e4m3 values exactly)
        self.w: dict = {}            # packed device operands
        self._ws: Optional[dict] = None
        self._bias: dict = {}        # L -> device table
        self.loaded = False

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd, strict: bool = True, assign: bool = False):
        """Same (missing, unexpected) semantics as nn.Module.load_state_dict; a shape mismatch always raises.
        ``encoder.embed_tokens.weight`` is the tied twin of ``shared.weight``: either name (or both) fills it.  The
        operands are packed here, once; ``assign`` is accepted and changes nothing (the tensors are always copied).

        A ``torch.float8_e4m3fn`` tensor is widened exactly (every e4m3 value is a bf16 value) and remembered by name:
        the fp8 mode packs its bytes unchanged with unit scales.  In fp8 mode a per-tensor scale key
        (``*.scale_weight`` / ``*.weight_scale``) next to e4m3 weights is a RuntimeError: such files store
        weight / scale and are not supported; in bf16 mode such a key is an unexpected key like any other."""
        sd = dict(sd)
        if self.precision == "fp8":
            is_e4m3 = any(k in self.spec and getattr(v, "dtype", None) == torch.float8_e4m3fn for k, v in sd.items())
            scaled = [k for k in sd if k.endswith(SCALE_KEY_SUFFIXES)]
            if is_e4m3 and scaled:
                raise RuntimeError(f"load_state_dict: {scaled[0]} is a per-tensor scale next to e4m3 weights; per-tensor-"
                                   "scaled fp8 checkpoints are not supported (the e4m3 bytes are used with unit scales)")
        if TIED_EMBEDDING in sd:
            twin = sd.pop(TIED_EMBEDDING)
            sd.setdefault("shared.weight", twin)
        missing, unexpected = fill_tensors(self.spec, sd, strict, self.tensors)
        found = {k for k in self.spec if k in sd}
        self.e4m3 = (self.e4m3 - found) | {k for k in found if sd[k].dtype == torch.float8_e4m3fn}
        if not missing:
            self._pack()
        return missing, unexpected

    def state_dict(self):
        return dict(self.tensors)

    def _pack(self):
        t, p, dev = self.tensors, self.params, self.device

        def bf(x):
            return x.to(dev, torch.bfloat16).contiguous()

        def e4m3(name):
            """(e4m3 bytes [N, K], fp32 scale [N]) of one checkpoint tensor: its own bytes with unit scales if it
            arrived as e4m3, else the bf16 rounding of the bf16 mode quantised per output row."""
            if name in self.e4m3:
                return (t[name].to(torch.float8_e4m3fn).view(torch.uint8).to(dev).contiguous(),
                        torch.ones(t[name].shape[0], device=dev, dtype=torch.float32))
            return ops.quantize_rows_fp8(bf(t[name]))

        def put(key, names):
            """The packed operand of projection ``key`` from the row concatenation of the tensors ``names``."""
            if key.split(".")[1] not in self.fp8:
                w[key] = bf(torch.cat([t[n] for n in names]))
                return
            parts = [e4m3(n) for n in names]     # per-row scales: piecewise == the quantised concatenation
            w[key] = torch.cat([q for q, _ in parts]).contiguous()
            w[key + ".scale"] = torch.cat([s for _, s in parts]).contiguous()
        w = {"shared": bf(t["shared.weight"]), "ones": torch.ones(p.d_model, device=dev, dtype=torch.float32),
             "final_ln": t["encoder.final_layer_norm.weight"].to(dev)}
        for i in range(p.num_layers):
            a, f = f"encoder.block.{i}.layer.0", f"encoder.block.{i}.layer.1.DenseReluDense"
            put(f"{i}.qkv", [f"{a}.SelfAttention.{n}.weight" for n in ("q", "k", "v")])
            put(f"{i}.o", [f"{a}.SelfAttention.o.weight"])
            w[f"{i}.ln0"] = t[f"{a}.layer_norm.weight"].to(dev)
            put(f"{i}.wi", [f"{f}.wi_1.weight", f"{f}.wi_0.weight"])   # [plain ; GELU]
            put(f"{i}.wo", [f"{f}.wo.weight"])
            w[f"{i}.ln1"] = t[f"encoder.block.{i}.layer.1.layer_norm.weight"].to(dev)
        self.w = w
        self._bias = {}
        self.loaded = True

    def weight_bytes(self, embedding: bool = True) -> int:
        """Device bytes of the packed operands (e4m3 planes and their scale vectors included); ``embedding=False``
        leaves the token table out, which no precision mode changes."""
        return sum(v.numel() * v.element_size() for k, v in self.w.items() if embedding or k != "shared")

    def bias_table(self, length: int) -> torch.Tensor:
        """Host table fp32 [heads, 2 length - 1] of the loaded relative_attention_bias."""
        p = self.params
        return relative_bias_table(self.tensors["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"],
                                   length, p.relative_attention_num_buckets, p.relative_attention_max_distance)

    def _device_bias(self, length: int) -> torch.Tensor:
        if length not in self._bias:
            self._bias[length] = self.bias_table(length).to(self.device)
        return self._bias[length]

    # ------------------------------------------------------------------ workspace
    def _workspace(self, rows: int) -> dict:
        """Resident buffers, sized on first use and grown when a pass has more rows (never beyond MAX_ROWS)."""
        ws = self._ws
        if ws is not None and ws["rows"] >= rows:
            return ws
        p, dev = self.params, self.device
        ws = {"rows": rows,
              "x": torch.empty(rows, p.d_model, device=dev, dtype=torch.float32),
              "qkv": torch.empty(rows, 3 * p.inner_dim, device=dev, dtype=torch.bfloat16),
              "ao": torch.empty(rows, p.inner_dim, device=dev, dtype=torch.bfloat16),
              "u": torch.empty(rows, p.d_ff, device=dev, dtype=torch.bfloat16),
              "g": torch.empty(rows, p.d_ff, device=dev, dtype=torch.bfloat16)}
        if not {"qkv", "wi"} <= self.fp8:     # a bf16 norm output is read only by a bf16 qkv or wi projection
            ws["hn"] = torch.empty(rows, p.d_model, device=dev, dtype=torch.bfloat16)
        # fp8 mode: the e4m3 plane and the row scales in front of each quantised projection (hn8: qkv and wi)
        for key, cols, used in (("hn8", p.d_model, self.fp8 & {"qkv", "wi"}), ("ao8", p.inner_dim, self.fp8 & {"o"}),
                                ("p8", p.d_ff, self.fp8 & {"wo"})):
            if used:
                ws[key] = torch.empty(rows, cols, device=dev, dtype=torch.uint8)
                ws[key + ".scale"] = torch.empty(rows, device=dev, dtype=torch.float32)
        self._ws = ws
        return ws

    def workspace_bytes(self) -> int:
        return 0 if self._ws is None else sum(t.numel() * t.element_size() for t in self._ws.values() if isinstance(t, torch.Tensor))

    # ------------------------------------------------------------------ forward
    def sequences_per_pass(self, length: int) -> int:
        return max(1, self.MAX_ROWS // length) if length % 256 == 0 else 1

    @torch.no_grad()
    def encode_ids(self, ids: torch.Tensor) -> torch.Tensor:
        if not self.loaded:
            raise RuntimeError("T5Encoder: no weights loaded")
        if not isinstance(ids, torch.Tensor) or ids.dim() != 2 or ids.is_floating_point() or ids.shape[0] < 1:
            raise ValueError("encode_ids: ids must be an integer tensor [n_seq, L]")
        n_seq, length = ids.shape
        if length % 64 or not 64 <= length <= 512:
            raise ValueError(f"encode_ids: L = {length} must be a multiple of 64 in 64..512")
        host = ids.detach().to("cpu")
        if int(host.min()) < 0 or int(host.max()) >= self.params.vocab_size:
            raise ValueError(f"encode_ids: token ids outside the vocabulary [0, {self.params.vocab_size})")
        dev_ids = host.to(torch.int32).to(self.device)
        out = torch.empty(n_seq, length, self.params.d_model, device=self.device, dtype=torch.bfloat16)
        n = self.sequences_per_pass(length)
        for s0 in range(0, n_seq, n):
            s1 = min(n_seq, s0 + n)
            self._pass(dev_ids[s0:s1].reshape(-1), s1 - s0, length, out[s0:s1].view(-1, self.params.d_model))
        return out

    def _pass(self, ids, n_seq: int, length: int, out) -> None:
        p, w = self.params, self.w
        rows, inner = n_seq * length, p.inner_dim
        ws = self._workspace(rows)
        x, qkv, ao, u, g = (ws[k][:rows] for k in ("x", "qkv", "ao", "u", "g"))
        bias = self._device_bias(length)
        tile = L.TILE_PP_256x256   # one tile for every row count: a row's bits must not depend on the batch
        eps = p.layer_norm_epsilon

        def planes(key):           # the e4m3 plane and the row scales of an fp8 producer
            return ws[key][:rows], ws[key + ".scale"][:rows]

        def project(name, i, a, out_, **epi):
            """out_ = epi(a @ w[name]^T): ``a`` is the bf16 operand, or (e4m3 plane, row scales) where ``name`` is fp8."""
            key = f"{i}.{name}"
            if name in self.fp8:
                ops.gemm([ops.Gemm(a[0], w[key], None, out_, a_scale=a[1], w_scale=w[key + ".scale"], **epi)], tile)
            else:
                ops.gemm([ops.Gemm(a, w[key], None, out_, **epi)], tile)

        def normed(name, weight):  # the RMS norm of the stream as the A operand of projection ``name``
            if name in self.fp8:
                h8 = planes("hn8")
                ops.t5_rmsnorm_fp8(x, weight, h8[0], h8[1], eps)
                return h8
            hn = ws["hn"][:rows]
            ops.t5_rmsnorm(x, weight, hn, eps)
            return hn
        into_stream = dict(epilogue=L.EPI_GATE_RESIDUAL, resid=x, gate=w["ones"])
        ops.embed_rows(w["shared"], ids, x)
        for i in range(p.num_layers):
            project("qkv", i, normed("qkv", w[f"{i}.ln0"]), qkv)
            ops.t5_attention(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], bias, ao, n_seq, p.num_heads)
            if "o" in self.fp8:    # 64 workgroups (one per head) write a row of ao: no kernel knows its maximum
                a = planes("ao8")
                ops.quantize_rows_fp8(ao, a[0], a[1])
            else:
                a = ao
            project("o", i, a, x, **into_stream)
            project("wi", i, normed("wi", w[f"{i}.ln1"]), u, epilogue=L.EPI_SPLIT_GELU, out2=g, n_split=p.d_ff)
            if "wo" in self.fp8:
                a = planes("p8")
                ops.gated_mul_fp8(g, u, a[0], a[1])
            else:
                ops.gated_mul(g, u, u)
                a = u
            project("wo", i, a, x, **into_stream)
        ops.t5_rmsnorm(x, w["final_ln"], out, eps)

    # the reference's callers move the module around and switch modes; resident here
    def to(self, *a, **k):
        return self

    def eval(self):
        return self


def load_t5(params="t5-v1_1-xxl", device="cuda", weights="synthetic", seed: int = 0, precision: str = "bf16",
            fp8_projections: Sequence[str] = FP8_PROJECTIONS) -> T5Encoder:
    """``params``: a T5Params or a name of ``params.t5_params``.  ``weights``: "synthetic", a state dict, or a local
    ``.safetensors`` file or a directory of shards (transformers' names; a full T5 checkpoint's decoder and lm_head
    keys are ignored, a missing encoder key is an error).  The ``T5`` environment variable names the checkpoint when the
    caller gives none ("synthetic"), as ``AE`` does for the autoencoder; nothing is ever downloaded.
    ``precision``, ``fp8_projections``: as for ``T5Encoder``; an e4m3fn ``.safetensors`` file loads as stored (its bytes
    become the fp8 operands unchanged; in bf16 mode they are widened exactly)."""
    p = t5_params[params] if isinstance(params, str) else params
    enc = T5Encoder(p, device, precision=precision, fp8_projections=fp8_projections)
    return load_text_weights(enc, "load_t5", "T5", weights, lambda: synthetic_t5_state_dict(p, seed), "encoder")


# ---------------------------------------------------------------------------------------------------------- text in
class ToyByteTokenizer:
    """A TOY, not a T5 vocabulary: UTF-8 bytes as tokens (id = 3 + byte), 1 = end of string, 0 = padding, with the call
    contract of a HuggingFace tokenizer as conditioner.py:23-31 uses it.  Deterministic, needs no file; it exists so that
    different strings reach the encoder as different, reproducible ids where no sentencepiece model is available."""

    pad_token_id, eos_token_id, vocab_size = 0, 1, 259

    def __call__(self, text, truncation=True, max_length: int = 256, padding="max_length", return_tensors="pt", **_):
        texts = [text] if isinstance(text, str) else list(text)
        ids = torch.zeros(len(texts), max_length, dtype=torch.long)
        for r, s in enumerate(texts):
            tok = [3 + b for b in s.encode("utf-8")][: max_length - 1] + [self.eos_token_id]
            ids[r, : len(tok)] = torch.tensor(tok, dtype=torch.long)
        return {"input_ids": ids}

    def tokenize(self, text: str) -> list:
        """One string per byte of the text, in order (no end-of-string token), as a HuggingFace tokenizer's ``tokenize``
        returns its pieces: what the prompt-token maps are named by."""
        return [bytes([b]).decode("latin-1") for b in text.encode("utf-8")]


class HipTextEncoder:
    """The ``HFEmbedder`` contract (conditioner.py:6-38) with T5 on the HIP encoder: ``t5(text) -> [1, L, d_model]`` bf16,
    ``t5_many(texts) -> [n, L, d_model]`` in one forward (what ``FluxGenerator.embed`` uses for the prompt and all
    concepts of a call).

    ``tokenizer``: any callable with the HuggingFace call contract (``tokenizer(texts, truncation=True,
    max_length=L, padding="max_length", return_tensors="pt")["input_ids"]``); whatever it returns is padded with id 0
    and truncated to ``max_length`` here as well, because the encoder's sequence length is always ``max_length``.  A
    local directory path builds ``T5Tokenizer.from_pretrained(path)`` on first use; that branch has never been
    exercised, because no sentencepiece vocabulary file is available to this repository's tests.

    ``clip``: ``clip(text)`` delegates to the injected ``clip`` -- a callable ``text -> [1, vec_dim]``, or an object with
    such a ``clip`` method (``clip.HipClipEmbedder``, the CLIP text encoder on HIP; kept as ``clip_embedder``) -- and
    without one to ``SyntheticTextEncoder.clip``: seeded noise keyed by the text, a stand-in."""

    def __init__(self, t5_encoder: T5Encoder, tokenizer, max_length: int = 256, clip=None, vec_dim: int = 768):
        if max_length % 64 or not 64 <= max_length <= 512:
            raise ValueError("HipTextEncoder: max_length must be a multiple of 64 in 64..512")
        self.encoder, self.max_length = t5_encoder, int(max_length)
        self._tokenizer = tokenizer
        self.device = t5_encoder.device
        self.clip_embedder = clip if hasattr(clip, "clip") else None
        if self.clip_embedder is not None:
            clip = self.clip_embedder.clip
        if clip is None:
            from .pipeline import SyntheticTextEncoder
            clip = SyntheticTextEncoder(self.max_length, t5_encoder.params.d_model, vec_dim, self.device).clip
        self._clip = clip

    @property
    def tokenizer(self):
        if isinstance(self._tokenizer, (str, os.PathLike)):
            from transformers import T5Tokenizer
            self._tokenizer = T5Tokenizer.from_pretrained(str(self._tokenizer), local_files_only=True)
        return self._tokenizer

    def token_ids(self, texts: Sequence[str]) -> torch.Tensor:
        """int64 [n, max_length]: the tokenizer's ids, zero-padded and truncated to max_length."""
        got = self.tokenizer(list(texts), truncation=True, max_length=self.max_length, return_length=False,
                             return_overflowing_tokens=False, padding="max_length", return_tensors="pt")["input_ids"]
        got = torch.as_tensor(got, dtype=torch.long)
        if got.dim() == 1:
            got = got[None]
        ids = torch.zeros(got.shape[0], self.max_length, dtype=torch.long)
        n = min(self.max_length, got.shape[1])
        ids[:, :n] = got[:, :n]
        return ids

    def t5_many(self, texts: Sequence[str]) -> torch.Tensor:
        return self.encoder.encode_ids(self.token_ids(texts))

    def t5(self, text: str) -> torch.Tensor:
        return self.t5_many([text])

    def clip(self, text: str) -> torch.Tensor:
        return self._clip(text)


def synthetic_text_encoder(context_dim: int, max_length: int, device, vec_dim: int = 768, seed: int = 0,
                           clip=None, t5_precision: str = "bf16") -> HipTextEncoder:
    """``text_encoder="synthetic-t5"``: a two-block T5Encoder of d_model = ``context_dim`` (4 heads, d_ff 512) with
    synthetic weights behind the toy byte tokenizer.  Real arithmetic on meaningless weights: prompts and concepts reach
    the DiT through the encoder's kernels, and equal strings give equal bits.  ``clip``: as for HipTextEncoder (None: the
    seeded-noise stand-in; "synthetic-t5-clip" passes ``clip.synthetic_clip_embedder``).  ``t5_precision``: the
    T5Encoder's ``precision`` ("fp8": all four projections in e4m3)."""
    p = tiny_t5_params(d_model=context_dim, vocab_size=ToyByteTokenizer.vocab_size + 253)
    return HipTextEncoder(load_t5(p, device, "synthetic", seed, precision=t5_precision), ToyByteTokenizer(), max_length,
                          clip=clip, vec_dim=vec_dim)
