"""Concept heat maps from stacked vectors: the HIP counterpart of
``compute_heatmaps_from_vectors`` (concept_attention/concept_attention_pipeline.py:29-91).

Semantics kept: optional head merge (:43-51), dot products over the feature axis (:57-61),
softmax / sparsemax / entmax15 ACROSS concepts per patch (:64-71), select timesteps then layers (:76-77), mean (:78-82),
reshape to the patch grid (:85-90).  Differences, both deliberate and documented in DESIGN.md:
the (t, layer) pairs that are not selected are never computed (the reference computes all and
slices), and products/softmax/mean are fp32 (the reference runs them in the activations' bf16).
The grid side is sqrt(patches) instead of the reference's hard-coded 64.
"""
from __future__ import annotations

import math

import torch

from . import _lib as L
from . import ops


def resolve_norm(softmax: bool, attention_norm: str) -> int:
    """The reference's branch order (concept_attention_pipeline.py:64-71): softmax if ``softmax`` or
    attention_norm == "softmax", else entmax15 / sparsemax, else ValueError."""
    if softmax or attention_norm == "softmax":
        return L.NORM_SOFTMAX
    if attention_norm in ("entmax15", "sparsemax"):
        return L.NORMS[attention_norm]
    raise ValueError(f"Unknown attention_norm={attention_norm}")


def check_concept_count(norm: int, n_concepts: int) -> None:
    """Refuse what no route can serve BEFORE anything is launched: the sparse norms sort a patch's logits in registers,
    at most L.HEATMAP_MAX_CONCEPTS of them (the softmax has no bound: beyond the limit it takes the three-launch form)."""
    if norm != L.NORM_SOFTMAX and n_concepts > L.HEATMAP_MAX_CONCEPTS:
        name = {v: k for k, v in L.NORMS.items()}[norm]
        raise ValueError(f"{n_concepts} concepts with attention_norm={name!r}: the sparse norms take at most "
                         f"{L.HEATMAP_MAX_CONCEPTS} concepts (softmax has no limit)")


def linear_normalization(x: torch.Tensor, dim: int) -> torch.Tensor:
    """concept_attention/utils.py:35-44 (host-side, tiny: C x dim)."""
    x_min = torch.min(x, dim=dim, keepdim=True)[0]
    x_shifted = x - x_min
    x_sum = torch.sum(x_shifted, dim=dim, keepdim=True)
    x_sum = torch.where(x_sum == 0, torch.ones_like(x_sum), x_sum)
    return x_shifted / x_sum


WORD_MARK = "\u2581"          # sentencepiece's word-start mark
_PUNCTUATION = "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"


def word_groups(tokens) -> list:
    """[(word, [token indices])] of a prompt's token strings, in order.  Sentencepiece pieces (any token carries the
    word-start mark): a token that begins with the mark opens a word, the pieces behind it belong to it (the first token
    opens one either way); the mark is not part of the word.  One-string-per-byte tokens (t5.ToyByteTokenizer): words
    split at the space byte, which belongs to no word; the bytes are joined and read as UTF-8.  Any other token list:
    every token is its own word.  A word without a character (a lone mark) is left out."""
    tokens = list(tokens)
    groups = []
    if any(t.startswith(WORD_MARK) for t in tokens):
        for i, t in enumerate(tokens):
            if t.startswith(WORD_MARK) or not groups:
                groups.append(["", []])
            groups[-1][0] += t[len(WORD_MARK):] if t.startswith(WORD_MARK) else t
            groups[-1][1].append(i)
    elif tokens and all(len(t) == 1 and ord(t) < 256 for t in tokens):
        open_ = False
        for i, t in enumerate(tokens):
            if t == " ":
                open_ = False
                continue
            if not open_:
                groups.append([b"", []])
                open_ = True
            groups[-1][0] += t.encode("latin-1")
            groups[-1][1].append(i)
        groups = [[w.decode("utf-8", errors="replace"), ix] for w, ix in groups]
    else:
        groups = [[t, [i]] for i, t in enumerate(tokens)]
    return [(w, ix) for w, ix in groups if w]


def normalize_word(word: str) -> str:
    """How words are compared in look-ups: case-insensitive, surrounding punctuation stripped."""
    return word.strip(_PUNCTUATION + " ").lower()


def find_words(groups, phrase: str) -> list:
    """Every occurrence of ``phrase`` (one word or several, split at white space) among the words of ``groups``, as the
    list of its token indices; the comparison is ``normalize_word``'s.  [] when it does not occur."""
    want = [normalize_word(w) for w in phrase.split()]
    want = [w for w in want if w]
    have = [normalize_word(w) for w, _ in groups]
    if not want:
        return []
    return [[i for _, ix in groups[a:a + len(want)] for i in ix]
            for a in range(len(have) - len(want) + 1) if have[a:a + len(want)] == want]


def word_maps(token_maps: torch.Tensor, groups) -> torch.Tensor:
    """[len(groups), ...] from per-token maps [n_tok, ...]: a word's map is the sum of its tokens' maps (DAAM's rule), on
    the maps' device, every word summed in token order."""
    if not groups:
        return token_maps.new_zeros((0,) + tuple(token_maps.shape[1:]))
    return torch.stack([token_maps[list(ix)].sum(0) for _, ix in groups])


def compute_heatmaps_from_vectors(image_vectors, concept_vectors, layer_indices, timesteps=list(range(4)),
                                  softmax: bool = True, normalize_concepts: bool = False,
                                  attention_norm: str = "sparsemax"):
    """image_vectors [t, layers, 1, patches, dim] (or [t, layers, 1, heads, patches, 128]),
    concept_vectors likewise with concepts in place of patches -> fp32 [1, concepts, side, side]."""
    # entmax15 / sparsemax: the reference calls the third-party `entmax` package, which it neither pins nor
    # vendors; the kernels implement the published algorithms (parity with that package UNPINNED)
    norm = resolve_norm(softmax, attention_norm)
    if image_vectors.dim() == 6:
        t, l, b, h, n, d = image_vectors.shape
        image_vectors = image_vectors.permute(0, 1, 2, 4, 3, 5).reshape(t, l, b, n, h * d)
        c = concept_vectors.shape[4]
        concept_vectors = concept_vectors.permute(0, 1, 2, 4, 3, 5).reshape(t, l, b, c, h * d)
    if image_vectors.shape[2] != 1:
        raise NotImplementedError("batch size 1 only")
    if normalize_concepts:
        concept_vectors = linear_normalization(concept_vectors.float(), dim=-2).to(torch.bfloat16)
    # heatmaps[timesteps][:, layer_indices]: python ints index dim 0 / dim 1 (floats truncate as in
    # torch indexing, concept_attention_pipeline.py:76)
    ts = [int(t) for t in timesteps]
    ls = [int(l) for l in layer_indices]
    n_patches, C = image_vectors.shape[3], concept_vectors.shape[3]
    check_concept_count(norm, C)
    dev = image_vectors.device
    acc = torch.zeros(C, n_patches, device=dev, dtype=torch.float32)
    logits = torch.empty(C, n_patches, device=dev, dtype=torch.float32)
    w = 1.0 / (len(ts) * len(ls))
    for t in ts:
        for l in ls:
            iv = image_vectors[t, l, 0].to(torch.bfloat16).contiguous()
            cv = concept_vectors[t, l, 0].to(torch.bfloat16).contiguous()
            ops.heatmap_logits(iv, cv, logits)
            ops.heatmap_norm_accumulate(logits, acc, w, norm)
    side = int(round(math.sqrt(n_patches)))
    if side * side != n_patches:
        raise ValueError(f"{n_patches} patches do not form a square grid")
    return acc.view(1, C, side, side)
