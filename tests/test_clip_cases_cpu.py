"""CPU checks of tests/clip_cases.py: a faithful bf16 / fp32 emulation of every kernel of ca_clip.hip sits inside its
derived bound on every case the GPU test runs, and each named slip leaves it.  Declaration, export and argument
rejection of the four entry points need no GPU either."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import clip_cases as T
import clip_ref
from conceptattention_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ca_clip_attn_bf16", "ca_layernorm_f32in", "ca_quick_gelu_bf16", "ca_clip_embed_f32")


def _ratio(got, ref, bound):
    return float(((got.double() - ref).abs() / bound).max())


@pytest.mark.parametrize("case", T.ATTN_CASES, ids=lambda c: c.name)
def test_attention_emulation_sits_inside_the_bound(case):
    q, k, v = T.attn_inputs(case)
    ref, bound = T.attn_reference(q, k, v, case.n_seq, case.heads)
    r = _ratio(T.attn_emulated(q, k, v, case.n_seq, case.heads), ref, bound)
    assert r <= 1.0, r
    again = clip_ref.causal_attention(q.double(), k.double(), v.double(), case.n_seq, case.heads, T.SCALE)
    assert torch.allclose(again, ref, rtol=1e-12, atol=1e-12)      # clip_cases' reference == clip_ref's statement


def test_the_attention_lengths_are_the_ones_where_the_indexing_changes():
    assert T.ATTN_LENGTHS == (1, 15, 16, 17, 63, 64, 65, 77, 128)
    assert all(c.n_seq == 3 and c.heads == 2 for c in T.ATTN_CASES)


@pytest.mark.parametrize("slip", T.ATTN_SLIPS)
@pytest.mark.parametrize("length", [17, 65, 77])
def test_every_attention_slip_leaves_the_bound(slip, length):
    """key <= query + 1, no mask, the scale missing, the rows behind the sequence counted as keys."""
    case = T.AttnCase(3, 2, length, "sliced")
    q, k, v = T.attn_inputs(case)
    ref, bound = T.attn_reference(q, k, v, case.n_seq, case.heads)
    assert _ratio(T.attn_emulated(q, k, v, case.n_seq, case.heads, slip=slip), ref, bound) > 4.0


def test_query_zero_returns_value_zero_and_the_sequences_have_their_own_v():
    case = T.AttnCase(3, 2, 77, "sliced")
    q, k, v = T.attn_inputs(case)
    ref, _ = T.attn_reference(q, k, v, 3, 2)
    for s in range(3):
        assert torch.allclose(ref[s * 77], v[s * 77].double(), atol=1e-12)        # one visible key: its value, exactly
    assert not torch.equal(v[:77], v[77:154])


@pytest.mark.parametrize("H,rows,strided", T.LN_CASES, ids=[T.ln_id(c) for c in T.LN_CASES])
def test_layernorm_emulation_sits_inside_the_bound_and_the_slips_leave_it(H, rows, strided):
    x, w, b = T.ln_inputs(H, rows)
    ref, bound = T.layernorm_reference(x, w, b)
    assert _ratio(T.layernorm_emulated(x, w, b), ref, bound) <= 1.0
    assert _ratio(T.layernorm_emulated(x, w, b, slip="no_mean"), ref, bound) > 4.0
    assert _ratio(T.layernorm_emulated(x, w, b, slip="no_bias"), ref, bound) > 4.0
    if rows != T.LN_ROWS:      # (the statements below are about the nine-row table)
        return
    odd = x[1::2].double()                                            # the rows with a large mean
    assert (odd.mean(-1).abs() > 50 * odd.std(-1)).all()
    # the one-pass variance, in fp32, is NOT inside the bound on those rows: the bound tells the two forms apart
    xf = x[1::2]
    m = xf.sum(-1, keepdim=True) / H
    var = ((xf * xf).sum(-1, keepdim=True) / H - m * m).clamp_min(0)
    onepass = T.bf16r((xf - m) / torch.sqrt(var + T.EPS) * w + b)
    assert _ratio(onepass, ref[1::2], bound[1::2]) > 1.0


def test_the_ragged_and_minimum_widths_are_cases_and_the_wrap_cases_exceed_their_caps():
    for rows in T.WIDTH_ROWS:
        for s in (False, True):
            assert {(1032, rows, s), (4, rows, s)} <= set(T.LN_CASES) and {(2056, rows, s), (8, rows, s)} <= set(T.QG_CASES)
    assert 8 in T.EMBED_H and [T.ln_id(c) for c in T.LN_CASES][:2] == ["64-False", "64-True"]
    assert all(max(T.ln_gather(r)) == r - 1 and len(T.ln_gather(r)) == 6 for r in (1, 7, 9)) and T.ln_gather(9) == T.LN_GATHER
    src = open(os.path.join(ROOT, "conceptattention_amd", "csrc", "ca_clip.hip")).read()      # the caps, as the source has them:
    core = open(os.path.join(ROOT, "conceptattention_amd", "csrc", "ca_text_core.h")).read()  # stated once, used by every launch
    assert core.count("rows < 65536 ? rows : 65536") == 1 and core.count("if (blocks > 65536) blocks = 65536;") == 1
    assert src.count("dim3(tx_row_blocks(rows))") == 1 and src.count("dim3(tx_walk8_blocks(rows, ") == 2 and "65536" not in src
    assert T.ROW_GRID_CAP == 65536 and T.ELEM_GRID_CAP == 65536 * 256
    assert set(T.WRAP_CASES) == {"layernorm", "quick_gelu", "clip_embed"}
    for op, (units, cap, per_wg, case) in T.WRAP_CASES.items():
        assert cap + per_wg <= units < cap + cap // 4, (op, units, cap)
    assert (43692 - 1) * 384 < T.ELEM_GRID_CAP + 256                      # the smallest row count that wraps by a workgroup
    assert T.WRAP_CASES["clip_embed"][3]["rows"] % 77 == 0 and 77 * 2269 * 96 < T.ELEM_GRID_CAP + 256


@pytest.mark.parametrize("C,rows,strided", T.QG_CASES)
def test_quick_gelu_emulation_sits_inside_the_bound_and_gelu_tanh_leaves(C, rows, strided):
    x = T.quick_gelu_inputs(C, rows)
    assert float(x.min()) == -40.0 and float(x.max()) == 40.0
    ref, bound = T.quick_gelu_reference(x)
    assert _ratio(T.quick_gelu_emulated(x), ref, bound) <= 1.0
    assert _ratio(T.quick_gelu_emulated(x, slip="gelu_tanh"), ref, bound) > 4.0
    assert torch.isfinite(T.quick_gelu_emulated(x)).all()


@pytest.mark.parametrize("H", T.EMBED_H)
def test_embedding_emulation_sits_inside_the_bound_and_the_global_row_position_leaves(H):
    tok, pos, ids = T.embed_inputs(H)
    assert ids.shape[0] == 3 * 77 and int(ids.min()) == 0 and int(ids.max()) == tok.shape[0] - 1
    ref, bound = T.embed_reference(tok, pos, ids)
    assert _ratio(T.embed_emulated(tok, pos, ids), ref, bound) <= 1.0
    assert _ratio(T.embed_emulated(tok, pos, ids, slip="position_of_the_global_row"), ref, bound) > 4.0


@pytest.mark.parametrize("name", list(clip_ref.CASES))
def test_pooling_the_last_row_leaves_the_model_bound(name):
    from conceptattention_amd.clip import synthetic_clip_state_dict
    from conceptattention_amd.params import tiny_clip_params
    geo, length, eos_pos, eos_token_id, _ = clip_ref.CASES[name]
    p = tiny_clip_params(**geo)
    g = np.load(os.path.join(ROOT, "tests", "golden", f"clip_{name}.npz"))
    with torch.no_grad():
        last, pooled = clip_ref.text_model(synthetic_clip_state_dict(p, 0), clip_ref.case_ids(name), p.num_attention_heads,
                                           p.num_hidden_layers, eos_token_id)
    assert clip_ref.rel_rms(pooled.numpy(), g["pooler_f32"]) < 1e-5
    assert clip_ref.rel_rms(last[:, -1].numpy(), g["pooler_f32"]) > 4 * T.MODEL_REL_RMS      # the slip
    assert max(g["bf16_err"]) < T.MODEL_REL_RMS


def test_projection_widths_are_multiples_of_the_gemm_tile_for_both_geometries():
    from conceptattention_amd.params import ClipTextParams, tiny_clip_params
    for p in (ClipTextParams(), tiny_clip_params()):
        assert p.hidden_size % 256 == 0 and p.intermediate_size % 256 == 0 and p.head_dim == 64
        assert p.max_position_embeddings == 77 <= 128      # one thin-row pass of the GEMM, one launch of the attention


# ---------------------------------------------------------------------------------------------------------- the ABI
@pytest.fixture(scope="module")
def lib():
    entry.build()
    return L.load()


def test_the_four_entries_are_declared_bound_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "conceptattn.h")).read()
    declared = set(re.findall(r"\b(ca_[a-z0-9_]+)\s*\(", text))
    for name in ENTRIES:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    src = open(os.path.join(ROOT, "conceptattention_amd", "csrc", "ca_clip.hip")).read()
    assert sorted(re.findall(r'extern "C" int (ca_\w+)\(', src)) == sorted(ENTRIES)      # all four live in the new unit
    from conceptattention_amd.csrc import build
    assert "ca_clip.hip" in build.SOURCES and "-save-temps=obj" in build.EXTRA_FLAGS["ca_clip.hip"]


def test_argument_rejection_of_the_four_entries_needs_no_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15            # a 16-byte aligned non-null address; nothing is ever launched

    def attn(**kw):
        a = dict(q=p, k=p, v=p, out=p, ldq=64, ldk=64, ldv=64, ldo=64, n_seq=1, heads=1, L=77, scale=0.125)
        a.update(kw)
        return lib.ca_clip_attn_bf16(a["q"], a["k"], a["v"], a["out"], a["ldq"], a["ldk"], a["ldv"], a["ldo"], a["n_seq"],
                                     a["heads"], a["L"], a["scale"], None)
    for bad in (dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(L=0), dict(L=129), dict(L=-1), dict(heads=0),
                dict(n_seq=0), dict(ldq=63), dict(ldk=72, heads=2), dict(ldv=56), dict(ldo=68), dict(q=p + 2),
                dict(out=p + 8), dict(scale=0.0), dict(scale=float("nan")), dict(scale=float("inf")),
                dict(n_seq=2 ** 31 - 1, heads=64, L=128)):
        assert attn(**bad) == -1, bad
        assert b"ca_clip_attn_bf16" in lib.ca_last_error()

    def ln(**kw):
        a = dict(x=p, ldx=256, idx=None, w=p, b=p, out=p, ldo=256, rows=1, H=256, eps=1e-5)
        a.update(kw)
        return lib.ca_layernorm_f32in(a["x"], a["ldx"], a["idx"], a["w"], a["b"], a["out"], a["ldo"], a["rows"], a["H"],
                                      a["eps"], None)
    for bad in (dict(x=None), dict(w=None), dict(b=None), dict(out=None), dict(rows=0), dict(H=0), dict(H=254),
                dict(ldx=252), dict(ldo=128), dict(ldo=258), dict(eps=0.0), dict(x=p + 4), dict(b=p + 8), dict(out=p + 2),
                dict(idx=p + 2)):
        assert ln(**bad) == -1, bad
        assert b"ca_layernorm_f32in" in lib.ca_last_error()

    def gelu(**kw):
        a = dict(x=p, ldx=512, out=p, ldo=512, rows=1, C=512)
        a.update(kw)
        return lib.ca_quick_gelu_bf16(a["x"], a["ldx"], a["out"], a["ldo"], a["rows"], a["C"], None)
    for bad in (dict(x=None), dict(out=None), dict(rows=0), dict(C=0), dict(C=508), dict(ldx=504), dict(ldo=8),
                dict(ldo=516), dict(x=p + 8)):
        assert gelu(**bad) == -1, bad
        assert b"ca_quick_gelu_bf16" in lib.ca_last_error()

    def embed(**kw):
        a = dict(tok=p, ldt=256, pos=p, ldp=256, ids=p, out=p, ldo=256, rows=1, L=77, H=256)
        a.update(kw)
        return lib.ca_clip_embed_f32(a["tok"], a["ldt"], a["pos"], a["ldp"], a["ids"], a["out"], a["ldo"], a["rows"],
                                     a["L"], a["H"], None)
    for bad in (dict(tok=None), dict(pos=None), dict(ids=None), dict(out=None), dict(rows=0), dict(L=0), dict(L=129),
                dict(H=4), dict(H=260), dict(ldt=128), dict(ldp=252), dict(ldo=254), dict(ids=p + 2), dict(out=p + 4),
                dict(pos=p + 8)):
        assert embed(**bad) == -1, bad
        assert b"ca_clip_embed_f32" in lib.ca_last_error()


def test_wrappers_reject_bad_tensors_before_any_launch():
    from conceptattention_amd import ops
    t = torch.zeros(77, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.clip_attention(t, t, t, t, 1, 1)                              # not on the device
    with pytest.raises(ValueError):
        ops.layernorm(torch.zeros(4, 256), torch.ones(256), torch.zeros(256), torch.zeros(4, 256, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.quick_gelu(t, t)
    with pytest.raises(ValueError):
        ops.clip_embed(t, t, torch.zeros(4, dtype=torch.int32), torch.zeros(4, 64), 4)
