"""The text-encoder entries against the bytes they wrote BEFORE their shared device code moved into csrc/ca_text_core.h.

tests/golden/text_parent_records.npz holds what the thirteen kernels of ca_t5.hip and ca_clip.hip, and the two tiny
encoders on top of them, wrote on an MI355X for seeded inputs, recorded from the commit before the move (``record``
below wrote it; only outputs are stored; 42 567 bytes for 184 outputs).  Per family three arrays: ``<family>.sha`` uint8 [outputs, 32], the SHA-256 of
each output's bytes in the order ``computed`` yields them; ``<family>.len`` int32 [outputs], the byte count of every
output of at most 4 KB (0 for a larger one); ``<family>.bytes``, those outputs' bytes one after the other, so that a
failure can be read.  A NaN compares as a NaN (every NaN is replaced by one pattern before the bytes are taken);
everything else compares by bits.

  ``t5_attn``     ca_t5_attn_bf16 at L = 64 .. 512 in steps of 64 (every instantiation), 2 sequences x 3 heads, q | k | v
                  thirds of one buffer, the std8 family; the far family at L = 64 and 512.
  ``clip_attn``   ca_clip_attn_bf16 at every L of clip_cases.ATTN_LENGTHS, 3 x 2 sliced; L = 77 in four buffers; L = 77
                  with scale 0.1.
  ``nf_attn``     both attentions with one cell of q, of k and of v in turn, in the middle one of three sequences, set to
                  NaN, +inf, -inf, -0.0 and the largest bf16 (T5 L = 64, CLIP L = 17 and 65); for CLIP also a NaN row of
                  v at row 0 of the last sequence, which must not reach the sequence before it.
  ``rows``        the ten row kernels (layernorm plain and gathered) on 1 and 5 rows of the minimum width, 264, 1032 and
                  2056 (one past each thread stride), and on five rows that are zero (the fp8 scale is 1), hold +inf,
                  NaN, FLT_MAX (the largest bf16 for a bf16 input), and plain; quick_gelu also at -inf, -128 and +inf.
  ``wrap_*``      the WRAP_CASES of t5_cases, t5_fp8_cases and clip_cases: the grid wrap of the walker and of the row loop.
  ``models``      the tiny T5 in bf16 and in fp8 (all four projections) on 3 sequences of L = 64 and of L = 256; the tiny
                  CLIP's encode_ids and hidden_states at L = 77 for 3 and for 17 sequences (two passes).

The inputs come from the case modules, generated on the CPU from their seeds.

267 bytes of two outputs have moved since the recording, on purpose (``MOVED``).  The recorded kernels clamped the scaled
row with fminf(fmaxf(z, -448), 448), which returns -448 for a NaN: a NaN element of the fp32 row an e4m3 producer
quantises was stored as the finite byte 0xFE.  The e4m3 value-range contract of include/conceptattn.h stores a NaN byte
there (tests/fp8_edge_cases.py, P2).  In ``t5_rmsnorm_fp8 specials`` these are row 1 column 3 (inf * 0) and all of row 2
(a NaN in x), in ``gated_mul_fp8 specials`` row 1 column 3 (inf under an infinite scale) and row 2 column 132 (the NaN
product).  Those two byte planes are compared with the parent's everywhere else and with 0x7F there; their scales, and
every other output, compare bit for bit as before."""
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_cases as CL  # noqa: E402
import t5_cases as T5  # noqa: E402
import t5_fp8_cases as F8  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_parent_records.npz")
KEEP = 4096                                   # an output of at most this many bytes is stored whole
FLT_MAX, BF16_MAX = 3.4028234663852886e38, 3.3895313892515355e38
NF_VALUES = (NAN, float("inf"), -float("inf"), -0.0, BF16_MAX)
WIDTHS = (264, 1032, 2056)                    # behind each kernel's minimum width
ROWS = (1, 5)
FAMILIES = ("t5_attn", "clip_attn", "nf_attn", "rows", "wrap_t5", "wrap_fp8", "wrap_clip", "models")
# output -> the (row, column) cells of its 5 x 264 e4m3 plane where the fp32 row is not finite: the parent holds 0xFE
# there, the contract a NaN byte (0x7F after canonical_bytes)
MOVED = {"t5_rmsnorm_fp8 specials [0]": [(1, 3)] + [(2, c) for c in range(264)],
         "gated_mul_fp8 specials [0]": [(1, 3), (2, 132)]}


def canonical_bytes(t: torch.Tensor) -> bytes:
    """The bytes of a device tensor with every NaN replaced by one pattern (uint8 holds e4m3: 0x7f and 0xff are its NaNs)."""
    t = t.detach().contiguous()
    if t.dtype == torch.uint8:
        t = torch.where((t & 0x7F) == 0x7F, torch.full_like(t, 0x7F), t)
    elif t.is_floating_point():
        t = torch.where(torch.isnan(t), torch.full_like(t, NAN), t)
    return t.cpu().view(torch.uint8).numpy().tobytes()


# ---------------------------------------------------------------------------------------------------------- launches
def t5_attn(q, k, v, bias, n_seq, heads):
    rows, width = q.shape
    qkv = torch.cat([q, k, v], 1).to(DEV, BF)
    out = torch.full((rows, width), NAN, device=DEV, dtype=BF)
    ops.t5_attention(qkv[:, :width], qkv[:, width:2 * width], qkv[:, 2 * width:], bias.to(DEV), out, n_seq, heads)
    return out


def clip_attn(q, k, v, n_seq, heads, scale=CL.SCALE, apart=False):
    rows, width = q.shape
    if apart:
        dq, dk, dv = (torch.zeros(rows, width + pad, device=DEV, dtype=BF)[:, :width] for pad in (8, 16, 24))
        for d, t in zip((dq, dk, dv), (q, k, v)):
            d.copy_(t.to(DEV, BF))
    else:
        qkv = torch.cat([q, k, v], 1).to(DEV, BF)
        dq, dk, dv = qkv[:, :width], qkv[:, width:2 * width], qkv[:, 2 * width:]
    out = torch.full((rows, width), NAN, device=DEV, dtype=BF)
    ops.clip_attention(dq, dk, dv, out, n_seq, heads, scale)
    return out


def _bf_out(rows, cols):
    return torch.full((rows, cols), NAN, device=DEV, dtype=BF)


def _fp8_out(rows, cols):
    return torch.full((rows, cols), 0xAB, device=DEV, dtype=torch.uint8), torch.full((rows,), NAN, device=DEV)


def k_t5_rmsnorm(x, w):
    out = _bf_out(*x.shape)
    ops.t5_rmsnorm(x.to(DEV), w.to(DEV), out, T5.EPS)
    return [out]


def k_t5_rmsnorm_fp8(x, w):
    out, scale = _fp8_out(*x.shape)
    ops.t5_rmsnorm_fp8(x.to(DEV), w.to(DEV), out, scale, F8.EPS)
    return [out, scale]


def k_layernorm(x, w, b, gather=None):
    idx = None if gather is None else torch.tensor(gather, dtype=torch.int32)
    out = _bf_out(x.shape[0] if idx is None else len(gather), x.shape[1])
    ops.layernorm(x.to(DEV), w.to(DEV), b.to(DEV), out, CL.EPS, row_idx=idx)
    return [out]


def k_gated_mul(g, u):
    out = _bf_out(*g.shape)
    ops.gated_mul(g.to(DEV, BF), u.to(DEV, BF), out)
    return [out]


def k_gated_mul_fp8(g, u):
    out, scale = _fp8_out(*g.shape)
    ops.gated_mul_fp8(g.to(DEV, BF), u.to(DEV, BF), out, scale)
    return [out, scale]


def k_quick_gelu(x):
    out = _bf_out(*x.shape)
    ops.quick_gelu(x.to(DEV, BF), out)
    return [out]


def k_embed_rows(table, ids):
    out = torch.full((ids.shape[0], table.shape[1]), NAN, device=DEV)
    ops.embed_rows(table.to(DEV, BF), ids, out)
    return [out]


def k_clip_embed(tok, pos, ids, length):
    out = torch.full((ids.shape[0], tok.shape[1]), NAN, device=DEV)
    ops.clip_embed(tok.to(DEV, BF), pos.to(DEV, BF), ids, out, length)
    return [out]


def special_rows(x: torch.Tensor, big: float) -> torch.Tensor:
    """x [5, cols] with row 0 zero, +inf, NaN and ``big`` in one cell of rows 1, 2, 3, row 4 as it is."""
    x = x.clone()
    x[0] = 0
    x[1, 3], x[2, x.shape[1] // 2], x[3, x.shape[1] - 1] = float("inf"), NAN, big
    return x


# ---------------------------------------------------------------------------------------------------------- families
def _t5_attn_family():
    for L in range(64, 513, 64):
        q, k, v, bias, _ = T5.attn_inputs(T5.AttnCase(2, 3, L, "sliced", "std8"))
        yield f"t5_attn {L} std8", t5_attn(q, k, v, bias, 2, 3)
    for L in (64, 512):
        q, k, v, bias, _ = T5.attn_inputs(T5.AttnCase(2, 3, L, "sliced", "far"))
        yield f"t5_attn {L} far", t5_attn(q, k, v, bias, 2, 3)


def _clip_attn_family():
    for L in CL.ATTN_LENGTHS:
        yield f"clip_attn {L}", clip_attn(*CL.attn_inputs(CL.AttnCase(3, 2, L, "sliced")), 3, 2)
    q, k, v = CL.attn_inputs(CL.AttnCase(3, 2, 77, "apart"))
    yield "clip_attn 77 apart", clip_attn(q, k, v, 3, 2, apart=True)
    yield "clip_attn 77 scale 0.1", clip_attn(q, k, v, 3, 2, scale=0.1)


def _nf_attn_family():
    """One cell at a time, in the middle sequence: row L / 2 of it, column 5 of head 1."""
    q, k, v, bias, _ = T5.attn_inputs(T5.AttnCase(3, 2, 64, "sliced", "std8"))
    for site in range(3):
        for val in NF_VALUES:
            ops_in = [q.clone(), k.clone(), v.clone()]
            ops_in[site][64 + 32, 64 + 5] = val
            yield f"t5_attn 64 {'qkv'[site]} {val}", t5_attn(*ops_in, bias, 3, 2)
    for L in (17, 65):
        q, k, v = CL.attn_inputs(CL.AttnCase(3, 2, L, "sliced"))
        clean = clip_attn(q, k, v, 3, 2)
        for site in range(3):
            for val in NF_VALUES:
                ops_in = [q.clone(), k.clone(), v.clone()]
                ops_in[site][L + L // 2, 64 + 5] = val
                yield f"clip_attn {L} {'qkv'[site]} {val}", clip_attn(*ops_in, 3, 2)
        poisoned = v.clone()
        poisoned[2 * L] = NAN
        got = clip_attn(q, k, poisoned, 3, 2)
        assert torch.equal(got[:2 * L], clean[:2 * L]), f"L = {L}: the next sequence's row 0 reached the one before it"
        assert torch.isnan(got[2 * L:]).all()
        yield f"clip_attn {L} NaN row of v behind the sequence", got


def _clip_embed_inputs(H, rows):
    tok, pos, ids = CL.embed_inputs(H, L=5, n_seq=1)
    return tok, pos, ids[:rows].contiguous(), rows


def _rows_family():
    for rows in ROWS:
        for H in (4,) + WIDTHS:
            yield f"t5_rmsnorm {rows}x{H}", k_t5_rmsnorm(*T5.row_inputs(H, rows))
            x, w, b = CL.ln_inputs(H, rows)
            yield f"layernorm {rows}x{H}", k_layernorm(x, w, b)
            yield f"layernorm gathered {rows}x{H}", k_layernorm(x, w, b, CL.ln_gather(rows))
        for H in (8,) + WIDTHS:
            yield f"t5_rmsnorm_fp8 {rows}x{H}", k_t5_rmsnorm_fp8(*T5.row_inputs(H, rows))
            yield f"gated_mul {rows}x{H}", k_gated_mul(*T5.gate_inputs(H, rows))
            yield f"gated_mul_fp8 {rows}x{H}", k_gated_mul_fp8(*T5.gate_inputs(H, rows))
            yield f"quick_gelu {rows}x{H}", k_quick_gelu(CL.quick_gelu_inputs(H, rows))
            yield f"embed_rows {rows}x{H}", k_embed_rows(*T5.embed_inputs(H, rows))
            yield f"clip_embed {rows}x{H}", k_clip_embed(*_clip_embed_inputs(H, rows))
    x, w = T5.row_inputs(264, 5)
    yield "t5_rmsnorm specials", k_t5_rmsnorm(special_rows(x, FLT_MAX), w)
    yield "t5_rmsnorm_fp8 specials", k_t5_rmsnorm_fp8(special_rows(x, FLT_MAX), w)
    x, w, b = CL.ln_inputs(264, 5)
    yield "layernorm specials", k_layernorm(special_rows(x, FLT_MAX), w, b)
    yield "layernorm gathered specials", k_layernorm(special_rows(x, FLT_MAX), w, b, CL.ln_gather(5))
    g, u = T5.gate_inputs(264, 5)
    yield "gated_mul specials", k_gated_mul(special_rows(g, BF16_MAX), u)
    yield "gated_mul_fp8 specials", k_gated_mul_fp8(special_rows(g, BF16_MAX), u)
    x = special_rows(CL.quick_gelu_inputs(264, 5), BF16_MAX)
    x[4, :3] = torch.tensor([-float("inf"), -128.0, float("inf")])
    yield "quick_gelu specials", k_quick_gelu(x)


def _wrap_t5_family():
    c = T5.WRAP_CASES["t5_rmsnorm"][3]
    yield "t5_rmsnorm wrap", k_t5_rmsnorm(*T5.row_inputs(c["H"], c["rows"]))
    c = T5.WRAP_CASES["gated_mul"][3]
    yield "gated_mul wrap", k_gated_mul(*T5.gate_inputs(c["C"], c["rows"]))
    c = T5.WRAP_CASES["embed_rows"][3]
    yield "embed_rows wrap", k_embed_rows(*T5.embed_inputs(c["H"], c["rows"]))


def _wrap_fp8_family():
    c = F8.WRAP_CASES["t5_rmsnorm_fp8"][3]
    x, w, _ = F8.rms_inputs(c["H"], c["rows"])
    yield "t5_rmsnorm_fp8 wrap", k_t5_rmsnorm_fp8(x, w)
    c = F8.WRAP_CASES["gated_mul_fp8"][3]
    g, u, _ = F8.gate_inputs(c["C"], c["rows"])
    yield "gated_mul_fp8 wrap", k_gated_mul_fp8(g, u)


def _wrap_clip_family():
    c = CL.WRAP_CASES["layernorm"][3]
    x, w, b = CL.ln_inputs(c["H"], c["rows"])
    yield "layernorm wrap", k_layernorm(x, w, b)
    yield "layernorm gathered wrap", k_layernorm(x, w, b, list(range(c["rows"] - 1, -1, -1)))
    c = CL.WRAP_CASES["quick_gelu"][3]
    yield "quick_gelu wrap", k_quick_gelu(CL.quick_gelu_inputs(c["C"], c["rows"]))
    c = CL.WRAP_CASES["clip_embed"][3]
    tok, pos, _ = CL.embed_inputs(c["H"])
    ids = torch.randint(0, tok.shape[0], (c["rows"],), generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    yield "clip_embed wrap", k_clip_embed(tok, pos, ids, CL.EMBED_L)


def _models_family():
    from conceptattention_amd.clip import load_clip, synthetic_clip_state_dict
    from conceptattention_amd.params import tiny_clip_params, tiny_t5_params
    from conceptattention_amd.t5 import load_t5, synthetic_t5_state_dict
    p = tiny_t5_params()
    for precision in ("bf16", "fp8"):
        enc = load_t5(p, DEV, weights=synthetic_t5_state_dict(p, 0), precision=precision)
        for L in (64, 256):
            ids = torch.randint(0, p.vocab_size, (3, L), generator=torch.Generator().manual_seed(L))
            yield f"t5 {precision} 3x{L}", enc.encode_ids(ids)
    p = tiny_clip_params()
    enc = load_clip(p, DEV, weights=synthetic_clip_state_dict(p, 0))
    for n in (3, 17):
        ids = torch.randint(0, p.vocab_size, (n, 77), generator=torch.Generator().manual_seed(n))
        yield f"clip encode_ids {n}x77", enc.encode_ids(ids)
        yield f"clip hidden_states {n}x77", enc.hidden_states(ids)


GENERATORS = {"t5_attn": _t5_attn_family, "clip_attn": _clip_attn_family, "nf_attn": _nf_attn_family,
              "rows": _rows_family, "wrap_t5": _wrap_t5_family, "wrap_fp8": _wrap_fp8_family,
              "wrap_clip": _wrap_clip_family, "models": _models_family}


@functools.lru_cache(maxsize=None)
def computed(family: str):
    """(names, sha uint8 [n, 32], len int32 [n], bytes uint8) of what the library in this tree writes for one family."""
    names, sha, lens, kept = [], [], [], []
    for name, outs in GENERATORS[family]():
        for i, t in enumerate(outs if isinstance(outs, list) else [outs]):
            raw = canonical_bytes(t)
            names.append(f"{name} [{i}]")
            sha.append(np.frombuffer(hashlib.sha256(raw).digest(), dtype=np.uint8))
            lens.append(len(raw) if len(raw) <= KEEP else 0)
            if len(raw) <= KEEP:
                kept.append(np.frombuffer(raw, dtype=np.uint8))
    return names, np.stack(sha), np.array(lens, dtype=np.int32), np.concatenate(kept) if kept else np.zeros(0, np.uint8)


def record(path: str) -> None:
    """Write the fixture from the library in this tree (run once, on the commit before the move)."""
    arrays = {}
    for f in FAMILIES:
        _, arrays[f + ".sha"], arrays[f + ".len"], arrays[f + ".bytes"] = computed(f)
    np.savez_compressed(path, **arrays)


@pytest.fixture(scope="module")
def parent():
    return np.load(FIXTURE)


@pytest.mark.parametrize("family", FAMILIES)
def test_the_outputs_are_the_parents_bit_for_bit(parent, family):
    names, sha, lens, kept = computed(family)
    print(family, len(names), "outputs,", int((lens > 0).sum()), "stored whole")
    assert sha.shape == parent[family + ".sha"].shape and np.array_equal(lens, parent[family + ".len"]), family
    ends = np.cumsum(lens)
    moved = 0
    for i, name in enumerate(names):
        if name in MOVED:   # the parent's bytes with a NaN byte where it held the laundered -448
            a, b = kept[ends[i] - lens[i]:ends[i]], parent[family + ".bytes"][ends[i] - lens[i]:ends[i]].copy()
            cells = np.array([r * 264 + c for r, c in MOVED[name]])
            assert lens[i] == 5 * 264 and (b[cells] == 0xFE).all(), name
            b[cells] = 0x7F
            moved += len(cells)
            assert np.array_equal(a, b), (name, np.nonzero(a != b)[0][:8], a[a != b][:8], b[a != b][:8])
            continue
        if lens[i]:         # readable: the first bytes that differ
            a, b = kept[ends[i] - lens[i]:ends[i]], parent[family + ".bytes"][ends[i] - lens[i]:ends[i]]
            assert np.array_equal(a, b), (name, np.nonzero(a != b)[0][:8], a[a != b][:8], b[a != b][:8])
        assert np.array_equal(sha[i], parent[family + ".sha"][i]), name
    assert moved == (267 if family == "rows" else 0)
