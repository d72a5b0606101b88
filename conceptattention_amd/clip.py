"""The CLIP text encoder on the GPU: ``ClipTextEncoder.encode_ids`` is the ``pooler_output`` of transformers'
``CLIPTextModel`` as the reference calls it (concept_attention/flux/src/flux/modules/conditioner.py, flux/util.py
load_clip: openai/clip-vit-large-patch14, max_length 77), on the HIP kernels of ca_clip.hip and the grouped GEMM, and
``HipClipEmbedder``, the ``HFEmbedder`` contract on its CLIP side: the pooled ``vec`` of the DiT from the prompt text.

What the reference does and this file keeps.  ``HFEmbedder`` pads every string to 77 tokens and passes
``attention_mask=None``: the only mask is the causal one, so PADDING TOKENS ARE KEYS like any other (for the queries
behind them).  Token plus learned position embedding; pre-norm blocks (LayerNorm with mean, bias and eps 1e-5; q k^T
scaled by 64^-1/2; a bias in every projection; quick_gelu); a final LayerNorm; the pooled row is the one at the
end-of-text token -- with ``eos_token_id == 2`` (the published config) the first arg-max of the ids, otherwise the first
position equal to ``eos_token_id``.

Precision, as in t5.py.  The residual stream is fp32 (transformers runs it in the checkpoint's dtype); every GEMM
operand is bf16, written by the LayerNorm, the attention or quick_gelu in front of it; accumulation, scores, softmax and
norm statistics are fp32.  The projection biases are bf16 (the GEMM's bias operand), the norms' weights and biases
fp32.  ``out_proj`` and ``fc2`` add into the stream in the GEMM epilogue (EPI_GATE_RESIDUAL with a ones gate), q | k | v
are one ``[3 hidden, hidden]`` weight under EPI_BIAS, ``fc1`` is EPI_BIAS followed by ``ca_quick_gelu_bf16`` in place.

Batching: up to ``MAX_SEGMENTS`` (16) sequences per pass, every sequence with the bits of its own one-sequence pass.
The sequences of a pass are stacked as rows (sequence s owns rows s * L .. s * L + L - 1).  The row kernels -- embedding,
LayerNorm, quick_gelu -- work row by row, and the attention kernel takes ``n_seq`` and never looks across a sequence's
rows.  Each projection is ONE GEMM problem over the stacked rows, always under the 256 x 256 ping-pong tile: the grouped
launch holds at most ``GEMM_MAX_PROBLEMS`` (2) problems, so one problem per sequence would not fit sixteen of them, and
it is not needed -- the GEMM's contract is one k order per accumulator, whichever way a row is computed (a full 256-row
tile, a thin last row tile inside the walk, or the thin-row kernel that a lone sequence's 77 rows take;
tests/test_kernels_gpu.py::test_gemm_thin_last_row_tile_is_bit_identical pins it for every epilogue used here, and
tests/test_clip_model_gpu.py pins the encoder's bits against one-sequence calls).  A call with more sequences runs in
several passes.  The workspace is resident, sized once for a full pass and reused across calls.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Sequence

import torch

from . import _lib as L
from . import ops
from .params import ClipTextParams, clip_params, tiny_clip_params
from .weights import _gen, fill_tensors, load_text_weights

__all__ = ["ClipTextEncoder", "ClipTextParams", "HipClipEmbedder", "ToyClipTokenizer", "load_clip",
           "synthetic_clip_state_dict", "clip_state_dict_spec", "pooled_positions", "synthetic_clip_embedder"]

PREFIX = "text_model."                         # published checkpoints carry it, transformers 5 lists the keys without
IGNORED_KEYS = ("embeddings.position_ids",)    # a buffer of older checkpoints
IGNORED_PREFIXES = ("vision_model.", "text_projection.", "visual_projection.", "logit_scale")   # a full CLIP checkpoint


# ---------------------------------------------------------------------------------------------------------- layout
def clip_state_dict_spec(p: ClipTextParams) -> list:
    """[(name, shape)] under transformers' key names (CLIPTextModel.state_dict() of transformers 5: no ``text_model.``
    prefix); Linear weights are (out, in)."""
    d, f = p.hidden_size, p.intermediate_size
    spec = [("embeddings.token_embedding.weight", (p.vocab_size, d)),
            ("embeddings.position_embedding.weight", (p.max_position_embeddings, d))]
    for i in range(p.num_hidden_layers):
        b = f"encoder.layers.{i}"
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            spec += [(f"{b}.self_attn.{n}.weight", (d, d)), (f"{b}.self_attn.{n}.bias", (d,))]
        spec += [(f"{b}.layer_norm1.weight", (d,)), (f"{b}.layer_norm1.bias", (d,)),
                 (f"{b}.mlp.fc1.weight", (f, d)), (f"{b}.mlp.fc1.bias", (f,)),
                 (f"{b}.mlp.fc2.weight", (d, f)), (f"{b}.mlp.fc2.bias", (d,)),
                 (f"{b}.layer_norm2.weight", (d,)), (f"{b}.layer_norm2.bias", (d,))]
    spec += [("final_layer_norm.weight", (d,)), ("final_layer_norm.bias", (d,))]
    return spec


def synthetic_clip_state_dict(p: ClipTextParams, seed: int = 0) -> dict:
    """Seeded on the CPU generator, one generator per tensor name (the values do not depend on the order), every value
    bf16-representable.  With u ~ U(-1, 1) (variance 1/3):

    * ``token_embedding``: u;  ``position_embedding``: 0.5 u -- the same order as the tokens, so a position taken from
      the wrong row changes the stream visibly (the real table is two orders smaller than this).
    * LayerNorm weights 1 + 0.1 u, biases 0.1 u.
    * ``q_proj``, ``k_proj``: u * sqrt(6 / hidden): q and k elements of variance ~2 on a unit-variance input, so a logit
      -- 64 products TIMES 1/8 -- has a standard deviation of about 2 nats.  Without the scale it would be 16, with the
      scale applied twice 0.25: either changes the probabilities by factors, as does a mask off by one (the newest key
      is one of few for the early queries).  Their biases: u (variance 1/3): q_bias . k alone moves a logit by ~0.8 nats.
    * ``fc1``: weight u * sqrt(2.75 / hidden), bias 0.5 u: variance 11/12 + 1/12 = 1 before quick_gelu, so its curved
      part is exercised and differs visibly from gelu_tanh (by up to 0.02 around |x| = 2).
    * ``v_proj``, ``out_proj``, ``fc2``: u / sqrt(fan_in) (PyTorch's default bound), biases 0.1 u (``v_proj``: 0.5 u).
    """
    sd = {}
    for name, shape in clip_state_dict_spec(p):
        u = torch.rand(shape, generator=_gen("clip." + name, seed, "cpu"), dtype=torch.float32) * 2 - 1
        bias = name.endswith(".bias")
        if "layer_norm" in name:
            t = 0.1 * u if bias else 1 + 0.1 * u
        elif name.startswith("embeddings.token"):
            t = u
        elif name.startswith("embeddings.position"):
            t = 0.5 * u
        elif ".q_proj." in name or ".k_proj." in name:
            t = u if bias else u * math.sqrt(6.0 / p.hidden_size)
        elif ".fc1." in name:
            t = 0.5 * u if bias else u * math.sqrt(2.75 / p.hidden_size)
        elif bias:
            t = 0.5 * u if ".v_proj." in name else 0.1 * u
        else:
            t = u / math.sqrt(shape[1])
        sd[name] = t.to(torch.bfloat16).to(torch.float32)
    return sd


def pooled_positions(ids: torch.Tensor, eos_token_id: int) -> torch.Tensor:
    """int64 [n]: the row CLIPTextModel pools, per sequence.  ``eos_token_id == 2``: the first arg-max of the ids (the
    end-of-text token has the highest id of the vocabulary); otherwise the first position equal to ``eos_token_id`` (0
    when there is none, as transformers' arg-max of an all-false mask gives)."""
    ids = ids.to(torch.int64)
    if eos_token_id == 2:
        return ids.argmax(dim=-1)
    return (ids == eos_token_id).to(torch.int64).argmax(dim=-1)


# ---------------------------------------------------------------------------------------------------------- the model
class ClipTextEncoder:
    """``encode_ids(ids[n, L]) -> [n, hidden]`` bf16, the ``pooler_output`` of CLIPTextModel with
    ``attention_mask=None``; ``hidden_states(ids) -> [n, L, hidden]`` bf16, its ``last_hidden_state`` (after the final
    norm).  L any value in 1..max_position_embeddings (at most 128, the attention kernel's limit).  Up to SEQS_PER_PASS
    sequences share every launch: see the module docstring."""

    SEQS_PER_PASS = L.MAX_SEGMENTS

    def __init__(self, params: ClipTextParams, device="cuda"):
        p = params
        if p.hidden_size != p.num_attention_heads * 64:
            raise ValueError("ClipTextEncoder: the head dim must be 64 (ca_clip_attn_bf16)")
        if p.hidden_size % 256 or p.intermediate_size % 256:
            raise ValueError("ClipTextEncoder: hidden_size and intermediate_size must be multiples of 256 (the GEMM tile)")
        if p.vocab_size < 1 or p.num_hidden_layers < 1 or not 1 <= p.max_position_embeddings <= 128:
            raise ValueError("ClipTextEncoder: empty geometry, or more than 128 positions")
        self.params = p
        self.device = torch.device(device)
        self.spec = dict(clip_state_dict_spec(p))
        self.tensors: dict = {}      # name -> fp32 host copy as loaded
        self.w: dict = {}            # packed device operands
        self._ws: Optional[dict] = None
        self.loaded = False

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd, strict: bool = True, assign: bool = False):
        """Same (missing, unexpected) semantics as nn.Module.load_state_dict; a shape mismatch always raises.  Keys are
        taken with or without the ``text_model.`` prefix; ``embeddings.position_ids`` and the vision tower, projections
        and ``logit_scale`` of a full CLIP checkpoint are ignored.  The operands are packed here, once; ``assign`` is
        accepted and changes nothing (the tensors are always copied)."""
        own = {}
        for k, v in dict(sd).items():
            if k.startswith(IGNORED_PREFIXES):
                continue
            k = k[len(PREFIX):] if k.startswith(PREFIX) else k
            if k not in IGNORED_KEYS:
                own[k] = v
        missing, unexpected = fill_tensors(self.spec, own, strict, self.tensors)
        if not missing:
            self._pack()
        return missing, unexpected

    def state_dict(self):
        return dict(self.tensors)

    def _pack(self):
        t, p, dev = self.tensors, self.params, self.device

        def bf(x):
            return x.to(dev, torch.bfloat16).contiguous()

        def f32(x):
            return x.to(dev, torch.float32).contiguous()
        w = {"tok": bf(t["embeddings.token_embedding.weight"]), "pos": bf(t["embeddings.position_embedding.weight"]),
             "ones": torch.ones(p.hidden_size, device=dev, dtype=torch.float32),
             "final.w": f32(t["final_layer_norm.weight"]), "final.b": f32(t["final_layer_norm.bias"])}
        for i in range(p.num_hidden_layers):
            b = f"encoder.layers.{i}"
            w[f"{i}.qkv"] = bf(torch.cat([t[f"{b}.self_attn.{n}_proj.weight"] for n in "qkv"]))
            w[f"{i}.qkv.b"] = bf(torch.cat([t[f"{b}.self_attn.{n}_proj.bias"] for n in "qkv"]))
            for ours, theirs in (("o", "self_attn.out_proj"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
                w[f"{i}.{ours}"], w[f"{i}.{ours}.b"] = bf(t[f"{b}.{theirs}.weight"]), bf(t[f"{b}.{theirs}.bias"])
            for n in ("1", "2"):
                w[f"{i}.ln{n}.w"], w[f"{i}.ln{n}.b"] = f32(t[f"{b}.layer_norm{n}.weight"]), f32(t[f"{b}.layer_norm{n}.bias"])
        self.w = w
        self.loaded = True

    # ------------------------------------------------------------------ workspace
    def _workspace(self) -> dict:
        """Resident buffers of one full pass (SEQS_PER_PASS sequences of at most max_position_embeddings rows), made on
        first use: calls of any size share them."""
        if self._ws is None:
            p, dev, rows = self.params, self.device, self.SEQS_PER_PASS * self.params.max_position_embeddings
            self._ws = {"x": torch.empty(rows, p.hidden_size, device=dev, dtype=torch.float32),
                        "hn": torch.empty(rows, p.hidden_size, device=dev, dtype=torch.bfloat16),
                        "qkv": torch.empty(rows, 3 * p.hidden_size, device=dev, dtype=torch.bfloat16),
                        "ao": torch.empty(rows, p.hidden_size, device=dev, dtype=torch.bfloat16),
                        "u": torch.empty(rows, p.intermediate_size, device=dev, dtype=torch.bfloat16)}
        return self._ws

    def workspace_bytes(self) -> int:
        return 0 if self._ws is None else sum(t.numel() * t.element_size() for t in self._ws.values())

    # ------------------------------------------------------------------ forward
    def _check_ids(self, ids, what: str):
        if not self.loaded:
            raise RuntimeError("ClipTextEncoder: no weights loaded")
        if not isinstance(ids, torch.Tensor) or ids.dim() != 2 or ids.is_floating_point() or ids.shape[0] < 1:
            raise ValueError(f"{what}: ids must be an integer tensor [n_seq, L]")
        length = ids.shape[1]
        if not 1 <= length <= self.params.max_position_embeddings:
            raise ValueError(f"{what}: L = {length} must be in 1..{self.params.max_position_embeddings}")
        host = ids.detach().to("cpu", torch.int64)
        if int(host.min()) < 0 or int(host.max()) >= self.params.vocab_size:
            raise ValueError(f"{what}: token ids outside the vocabulary [0, {self.params.vocab_size})")
        return host

    @torch.no_grad()
    def encode_ids(self, ids: torch.Tensor) -> torch.Tensor:
        host = self._check_ids(ids, "encode_ids")
        n, length = host.shape
        # the pooled row of sequence s within its pass: (s - s0) * L + position
        pooled = pooled_positions(host, self.params.eos_token_id).to(torch.int32)
        dev_ids = host.to(torch.int32).to(self.device)
        out = torch.empty(n, self.params.hidden_size, device=self.device, dtype=torch.bfloat16)
        for s0 in range(0, n, self.SEQS_PER_PASS):
            s1 = min(n, s0 + self.SEQS_PER_PASS)
            rows = pooled[s0:s1] + torch.arange(s1 - s0, dtype=torch.int32) * length
            self._pass(dev_ids[s0:s1].reshape(-1), s1 - s0, length, out[s0:s1], rows.contiguous())
        return out

    @torch.no_grad()
    def hidden_states(self, ids: torch.Tensor) -> torch.Tensor:
        host = self._check_ids(ids, "hidden_states")
        n = host.shape[0]
        dev_ids = host.to(torch.int32).to(self.device)
        out = torch.empty(*host.shape, self.params.hidden_size, device=self.device, dtype=torch.bfloat16)
        for s0 in range(0, n, self.SEQS_PER_PASS):
            s1 = min(n, s0 + self.SEQS_PER_PASS)
            self._pass(dev_ids[s0:s1].reshape(-1), s1 - s0, host.shape[1], out[s0:s1].view(-1, self.params.hidden_size), None)
        return out

    def _pass(self, ids, n_seq: int, length: int, out, pooled) -> None:
        """``n_seq`` stacked sequences of ``length`` rows through the network; the final norm on all rows, or on the
        rows ``pooled`` names alone."""
        p, w = self.params, self.w
        rows, d = n_seq * length, p.hidden_size
        ws = self._workspace()
        x, hn, qkv, ao, u = (ws[k][:rows] for k in ("x", "hn", "qkv", "ao", "u"))
        tile = L.TILE_PP_256x256   # one tile for every row count: a row's bits must not depend on the batch
        scale = p.head_dim ** -0.5
        ops.clip_embed(w["tok"], w["pos"], ids, x, length)
        for i in range(p.num_hidden_layers):
            ops.layernorm(x, w[f"{i}.ln1.w"], w[f"{i}.ln1.b"], hn, p.layer_norm_eps)
            ops.gemm([ops.Gemm(hn, w[f"{i}.qkv"], w[f"{i}.qkv.b"], qkv)], tile)
            ops.clip_attention(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], ao, n_seq, p.num_attention_heads, scale)
            ops.gemm([ops.Gemm(ao, w[f"{i}.o"], w[f"{i}.o.b"], x, epilogue=L.EPI_GATE_RESIDUAL, resid=x, gate=w["ones"])], tile)
            ops.layernorm(x, w[f"{i}.ln2.w"], w[f"{i}.ln2.b"], hn, p.layer_norm_eps)
            ops.gemm([ops.Gemm(hn, w[f"{i}.fc1"], w[f"{i}.fc1.b"], u)], tile)
            ops.quick_gelu(u, u)
            ops.gemm([ops.Gemm(u, w[f"{i}.fc2"], w[f"{i}.fc2.b"], x, epilogue=L.EPI_GATE_RESIDUAL, resid=x, gate=w["ones"])], tile)
        ops.layernorm(x, w["final.w"], w["final.b"], out, p.layer_norm_eps, row_idx=pooled)

    # the reference's callers move the module around and switch modes; resident here
    def to(self, *a, **k):
        return self

    def eval(self):
        return self


def load_clip(params="clip-vit-large-patch14", device="cuda", weights="synthetic", seed: int = 0) -> ClipTextEncoder:
    """``params``: a ClipTextParams or a name of ``params.clip_params``.  ``weights``: "synthetic", a state dict, or a
    local ``.safetensors`` file or a directory of shards (transformers' names, with or without ``text_model.``; the
    other keys of a full CLIP checkpoint are ignored, a missing text-model key is an error).  The ``CLIP`` environment
    variable names the checkpoint when the caller gives none ("synthetic"), as ``T5`` does for the T5 encoder; nothing
    is ever downloaded."""
    p = clip_params[params] if isinstance(params, str) else params
    return load_text_weights(ClipTextEncoder(p, device), "load_clip", "CLIP", weights,
                             lambda: synthetic_clip_state_dict(p, seed), "text-model")


# ---------------------------------------------------------------------------------------------------------- text in
class ToyClipTokenizer:
    """A TOY, not CLIP's byte-pair vocabulary: begin-of-text, the UTF-8 bytes as tokens (id = byte), end-of-text, with
    the call contract of a HuggingFace tokenizer.  As CLIP's tokenizer does, it pads with the end-of-text token, which
    is the highest id (so both pooling rules find the first one), and truncates so that the last token is end-of-text.
    Deterministic, needs no file."""

    bos_token_id, eos_token_id, pad_token_id, vocab_size = 256, 257, 257, 258

    def __call__(self, text, truncation=True, max_length: int = 77, padding="max_length", return_tensors="pt", **_):
        texts = [text] if isinstance(text, str) else list(text)
        ids = torch.full((len(texts), max_length), self.pad_token_id, dtype=torch.long)
        for r, s in enumerate(texts):
            tok = [self.bos_token_id] + list(s.encode("utf-8"))[: max(0, max_length - 2)] + [self.eos_token_id]
            ids[r, : len(tok)] = torch.tensor(tok, dtype=torch.long)
        return {"input_ids": ids}


class HipClipEmbedder:
    """The ``HFEmbedder`` contract on its CLIP side: ``clip(text) -> [1, hidden]`` bf16, the pooled ``vec`` of the DiT, and
    ``clip_many(texts) -> [n, hidden]``.

    ``tokenizer``: any callable with the HuggingFace call contract; what it returns is cut to ``max_length`` and, if
    shorter, padded with its ``pad_token_id`` (CLIP pads with end-of-text).  A local directory path builds
    ``CLIPTokenizer.from_pretrained(path, local_files_only=True)`` on first use; that branch has never been exercised,
    because no CLIP vocabulary files are available to this repository's tests (as for the T5 tokenizer)."""

    def __init__(self, encoder: ClipTextEncoder, tokenizer, max_length: int = 77):
        if not 2 <= max_length <= encoder.params.max_position_embeddings:
            raise ValueError(f"HipClipEmbedder: max_length must be in 2..{encoder.params.max_position_embeddings}")
        self.encoder, self.max_length = encoder, int(max_length)
        self._tokenizer = tokenizer
        self.device = encoder.device

    @property
    def tokenizer(self):
        if isinstance(self._tokenizer, (str, os.PathLike)):
            from transformers import CLIPTokenizer
            self._tokenizer = CLIPTokenizer.from_pretrained(str(self._tokenizer), local_files_only=True)
        return self._tokenizer

    def token_ids(self, texts: Sequence[str]) -> torch.Tensor:
        """int64 [n, max_length]."""
        tok = self.tokenizer
        got = tok(list(texts), truncation=True, max_length=self.max_length, return_length=False,
                  return_overflowing_tokens=False, padding="max_length", return_tensors="pt")["input_ids"]
        got = torch.as_tensor(got, dtype=torch.long)
        if got.dim() == 1:
            got = got[None]
        if got.shape[1] >= self.max_length:
            return got[:, : self.max_length].contiguous()
        pad = getattr(tok, "pad_token_id", None)
        if pad is None:
            raise ValueError("HipClipEmbedder: the tokenizer returned fewer than max_length ids and names no pad_token_id")
        ids = torch.full((got.shape[0], self.max_length), int(pad), dtype=torch.long)
        ids[:, : got.shape[1]] = got
        return ids

    def clip_many(self, texts: Sequence[str]) -> torch.Tensor:
        return self.encoder.encode_ids(self.token_ids(texts))

    def clip(self, text: str) -> torch.Tensor:
        return self.clip_many([text])

    __call__ = clip


def synthetic_clip_embedder(vec_dim: int, device, seed: int = 0) -> HipClipEmbedder:
    """The CLIP half of ``text_encoder="synthetic-t5-clip"``: a two-layer ClipTextEncoder of hidden = ``vec_dim``
    (heads of 64, intermediate 512) with synthetic weights behind the toy tokenizer.  Real arithmetic on meaningless
    weights: the prompt reaches ``vec`` through the encoder's kernels, and equal strings give equal bits."""
    p = tiny_clip_params(hidden_size=vec_dim, num_attention_heads=vec_dim // 64, vocab_size=ToyClipTokenizer.vocab_size + 254)
    return HipClipEmbedder(load_clip(p, device, "synthetic", seed), ToyClipTokenizer(), p.max_position_embeddings)
