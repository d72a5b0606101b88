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
"""
from __future__ import annotations

import math
import os
from typing import Optional, Sequence

import torch

from . import _lib as L
from . import ops
from .params import T5Params, t5_params, tiny_t5_params
from .weights import _gen

__all__ = ["T5Encoder", "T5Params", "HipTextEncoder", "ToyByteTokenizer", "load_t5", "synthetic_t5_state_dict",
           "t5_state_dict_spec", "relative_position_bucket", "relative_bias_table"]

TIED_EMBEDDING = "encoder.embed_tokens.weight"   # transformers lists the tied input embedding under both names


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
    ``attention_mask=None``.  L a multiple of 64 up to 512."""

    MAX_ROWS = 8192   # token rows of one pass: 16 sequences of 512; bounds the workspace and every GEMM operand (< 4 GiB)

    def __init__(self, params: T5Params, device="cuda"):
        p = params
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
        self.w: dict = {}            # packed device operands
        self._ws: Optional[dict] = None
        self._bias: dict = {}        # L -> device table
        self.loaded = False

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd, strict: bool = True, assign: bool = False):
        """Same (missing, unexpected) semantics as nn.Module.load_state_dict; a shape mismatch always raises.
        ``encoder.embed_tokens.weight`` is the tied twin of ``shared.weight``: either name (or both) fills it.  The
        operands are packed here, once; ``assign`` is accepted and changes nothing (the tensors are always copied)."""
        sd = dict(sd)
        if TIED_EMBEDDING in sd:
            twin = sd.pop(TIED_EMBEDDING)
            sd.setdefault("shared.weight", twin)
        missing = [k for k in self.spec if k not in sd]
        unexpected = [k for k in sd if k not in self.spec]
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing {missing[:4]}.. unexpected {unexpected[:4]}..")
        for k, shape in self.spec.items():
            if k in sd:
                if tuple(sd[k].shape) != tuple(shape):
                    raise RuntimeError(f"load_state_dict: {k} has shape {tuple(sd[k].shape)}, expected {tuple(shape)}")
                self.tensors[k] = sd[k].detach().to("cpu", torch.float32)
        if not missing:
            self._pack()
        return missing, unexpected

    def state_dict(self):
        return dict(self.tensors)

    def _pack(self):
        t, p, dev = self.tensors, self.params, self.device

        def bf(x):
            return x.to(dev, torch.bfloat16).contiguous()
        w = {"shared": bf(t["shared.weight"]), "ones": torch.ones(p.d_model, device=dev, dtype=torch.float32),
             "final_ln": t["encoder.final_layer_norm.weight"].to(dev)}
        for i in range(p.num_layers):
            a, f = f"encoder.block.{i}.layer.0", f"encoder.block.{i}.layer.1.DenseReluDense"
            w[f"{i}.qkv"] = bf(torch.cat([t[f"{a}.SelfAttention.{n}.weight"] for n in ("q", "k", "v")]))
            w[f"{i}.o"] = bf(t[f"{a}.SelfAttention.o.weight"])
            w[f"{i}.ln0"] = t[f"{a}.layer_norm.weight"].to(dev)
            w[f"{i}.wi"] = bf(torch.cat([t[f"{f}.wi_1.weight"], t[f"{f}.wi_0.weight"]]))   # [plain ; GELU]
            w[f"{i}.wo"] = bf(t[f"{f}.wo.weight"])
            w[f"{i}.ln1"] = t[f"encoder.block.{i}.layer.1.layer_norm.weight"].to(dev)
        self.w = w
        self._bias = {}
        self.loaded = True

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
              "hn": torch.empty(rows, p.d_model, device=dev, dtype=torch.bfloat16),
              "qkv": torch.empty(rows, 3 * p.inner_dim, device=dev, dtype=torch.bfloat16),
              "ao": torch.empty(rows, p.inner_dim, device=dev, dtype=torch.bfloat16),
              "u": torch.empty(rows, p.d_ff, device=dev, dtype=torch.bfloat16),
              "g": torch.empty(rows, p.d_ff, device=dev, dtype=torch.bfloat16)}
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
        x, hn, qkv, ao, u, g = (ws[k][:rows] for k in ("x", "hn", "qkv", "ao", "u", "g"))
        bias = self._device_bias(length)
        tile = L.TILE_PP_256x256   # one tile for every row count: a row's bits must not depend on the batch
        ops.embed_rows(w["shared"], ids, x)
        for i in range(p.num_layers):
            ops.t5_rmsnorm(x, w[f"{i}.ln0"], hn, p.layer_norm_epsilon)
            ops.gemm([ops.Gemm(hn, w[f"{i}.qkv"], None, qkv)], tile)
            ops.t5_attention(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], bias, ao, n_seq, p.num_heads)
            ops.gemm([ops.Gemm(ao, w[f"{i}.o"], None, x, epilogue=L.EPI_GATE_RESIDUAL, resid=x, gate=w["ones"])], tile)
            ops.t5_rmsnorm(x, w[f"{i}.ln1"], hn, p.layer_norm_epsilon)
            ops.gemm([ops.Gemm(hn, w[f"{i}.wi"], None, u, epilogue=L.EPI_SPLIT_GELU, out2=g, n_split=p.d_ff)], tile)
            ops.gated_mul(g, u, u)
            ops.gemm([ops.Gemm(u, w[f"{i}.wo"], None, x, epilogue=L.EPI_GATE_RESIDUAL, resid=x, gate=w["ones"])], tile)
        ops.t5_rmsnorm(x, w["final_ln"], out, p.layer_norm_epsilon)

    # the reference's callers move the module around and switch modes; resident here
    def to(self, *a, **k):
        return self

    def eval(self):
        return self


def _read_safetensors(path: str) -> dict:
    from safetensors.torch import load_file
    if os.path.isdir(path):
        files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith(".safetensors"))
        if not files:
            raise FileNotFoundError(f"load_t5: no .safetensors file in {path}")
    else:
        files = [path]
    sd: dict = {}
    for f in files:
        sd.update(load_file(f, device="cpu"))
    return sd


def load_t5(params="t5-v1_1-xxl", device="cuda", weights="synthetic", seed: int = 0) -> T5Encoder:
    """``params``: a T5Params or a name of ``params.t5_params``.  ``weights``: "synthetic", a state dict, or a local
    ``.safetensors`` file or a directory of shards (transformers' names; a full T5 checkpoint's decoder and lm_head
    keys are ignored, a missing encoder key is an error).  The ``T5`` environment variable names the checkpoint when the
    caller gives none ("synthetic"), as ``AE`` does for the autoencoder; nothing is ever downloaded."""
    p = t5_params[params] if isinstance(params, str) else params
    enc = T5Encoder(p, device)
    if isinstance(weights, str) and weights == "synthetic" and os.environ.get("T5"):
        weights = os.environ["T5"]
    if isinstance(weights, dict):
        enc.load_state_dict(weights, strict=True)
    elif weights == "synthetic":
        enc.load_state_dict(synthetic_t5_state_dict(p, seed), strict=True)
    else:
        missing, _ = enc.load_state_dict(_read_safetensors(str(weights)), strict=False)
        if missing:
            raise RuntimeError(f"load_t5: {weights} lacks {len(missing)} encoder tensors: {missing[:4]}..")
    return enc


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
                           clip=None) -> HipTextEncoder:
    """``text_encoder="synthetic-t5"``: a two-block T5Encoder of d_model = ``context_dim`` (4 heads, d_ff 512) with
    synthetic weights behind the toy byte tokenizer.  Real arithmetic on meaningless weights: prompts and concepts reach
    the DiT through the encoder's kernels, and equal strings give equal bits.  ``clip``: as for HipTextEncoder (None: the
    seeded-noise stand-in; "synthetic-t5-clip" passes ``clip.synthetic_clip_embedder``)."""
    p = tiny_t5_params(d_model=context_dim, vocab_size=ToyByteTokenizer.vocab_size + 253)
    return HipTextEncoder(load_t5(p, device, "synthetic", seed), ToyByteTokenizer(), max_length, clip=clip, vec_dim=vec_dim)
