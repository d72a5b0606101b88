"""CPU checks of tests/t5_cases.py: a faithful bf16 / fp32 emulation of every kernel of ca_t5.hip sits inside its
derived bound on every case the GPU test runs, and each named slip leaves it.  Argument rejection of the four entry
points needs no GPU either."""
import ctypes

import pytest
import torch

import __graft_entry__ as entry
import t5_cases as T
import t5_ref
from conceptattention_amd import _lib as L


def _ratio(got, ref, bound):
    return float(((got.double() - ref).abs() / bound).max())


@pytest.mark.parametrize("case", T.ATTN_CASES, ids=lambda c: c.name)
def test_attention_emulation_sits_inside_the_bound(case):
    q, k, v, bias, _ = T.attn_inputs(case)
    ref, bound = T.attn_reference(q, k, v, bias, case.n_seq, case.heads)
    r = _ratio(T.attn_emulated(q, k, v, bias, case.n_seq, case.heads), ref, bound)
    assert r <= 1.0, r
    again = t5_ref.attention(q.double(), k.double(), v.double(), bias, case.n_seq, case.heads)
    assert torch.allclose(again, ref, rtol=1e-12, atol=1e-12)      # t5_cases' reference == t5_ref's statement


@pytest.mark.parametrize("slip", T.ATTN_SLIPS)
@pytest.mark.parametrize("shape", [(5, 4, 256), (1, 2, 512)])
@pytest.mark.parametrize("family", ["std1", "std8"])
def test_every_attention_slip_leaves_the_bound(slip, shape, family):
    case = T.AttnCase(*shape, "contig", family)
    q, k, v, bias, weight = T.attn_inputs(case)
    ref, bound = T.attn_reference(q, k, v, bias, case.n_seq, case.heads)
    got = T.attn_emulated(q, k, v, bias, case.n_seq, case.heads, slip=slip, weight=weight, n_real=case.L // 2)
    assert _ratio(got, ref, bound) > 4.0


def test_far_key_rows_are_dominated_by_their_far_key():
    case = T.AttnCase(1, 2, 512, "contig", "far")
    q, k, v, bias, _ = T.attn_inputs(case)
    ref, _ = T.attn_reference(q, k, v, bias, 1, 2)
    assert torch.allclose(ref[0, :64], v[511, :64].double(), atol=1e-6)       # query 0 sees key L - 1: offset +511
    assert torch.allclose(ref[511, :64], v[0, :64].double(), atol=1e-6)       # and the reverse: offset -511


@pytest.mark.parametrize("H,rows,strided", T.ROW_CASES)
def test_rmsnorm_emulation_sits_inside_the_bound_and_the_slips_leave_it(H, rows, strided):
    x, w = T.row_inputs(H, rows)
    ref, bound = T.rmsnorm_reference(x, w)
    assert _ratio(T.rmsnorm_emulated(x, w), ref, bound) <= 1.0
    assert _ratio(T.rmsnorm_emulated(x, w, slip="mean_subtracted"), ref, bound) > 4.0
    if rows > 1:     # (row 1 is the small one: eps is a visible share of its mean square)
        assert _ratio(T.rmsnorm_emulated(x, w, slip="eps_1e-5"), ref, bound) > 4.0


@pytest.mark.parametrize("C,rows", [(512, 7), (10240, 3)] + [(C, rows) for C in (2056, 8) for rows in T.WIDTH_ROWS])
def test_gate_emulations_sit_inside_their_bounds_and_erf_gelu_leaves(C, rows):
    g, u = T.gate_inputs(C, rows)
    ref, bound = T.gated_mul_reference(g, u)
    assert _ratio(T.gated_mul_emulated(g, u), ref, bound) <= 1.0
    ref, bound = T.gate_path_reference(g, u)        # the same values as fp32 pre-activations
    assert _ratio(T.gate_path_emulated(g, u), ref, bound) <= 1.0
    if C >= 512:     # (a row of 8 values need not hold one where the two GELUs differ by more than a bf16 step)
        assert _ratio(T.gate_path_emulated(g, u, slip="erf_gelu"), ref, bound) > 4.0


def test_every_attention_instantiation_and_the_ragged_and_minimum_widths_are_cases():
    assert {c.L for c in T.ATTN_CASES} == {64 * n for n in range(1, 9)}        # NT = 4, 8, ..., 32
    for L in (320, 384, 448):
        assert {(c.layout, c.family) for c in T.ATTN_CASES if c.L == L} == \
            {(lay, fam) for lay in ("contig", "sliced") for fam in ("std1", "std8", "far")}
    for rows in T.WIDTH_ROWS:
        for s in (False, True):
            assert {(1032, rows, s), (4, rows, s)} <= set(T.ROW_CASES) and (8, rows, s) in T.EMBED_CASES
            assert {(2056, rows, s), (8, rows, s)} <= set(T.GATE_CASES)
    assert 1032 % 1024 == 8 and 1032 > 1024 and min(H for H, _, _ in T.ROW_CASES) == 4       # a partial second pass; the minimum


def test_wrap_cases_exceed_their_caps_by_a_workgroup_and_by_less_than_a_quarter():
    """The caps are restated from ca_text_core.h, where ca_t5.hip's launches take them from; the source must still hold
    them."""
    import os
    csrc = os.path.join(os.path.dirname(os.path.abspath(entry.__file__)), "conceptattention_amd", "csrc")
    src, core = open(os.path.join(csrc, "ca_t5.hip")).read(), open(os.path.join(csrc, "ca_text_core.h")).read()
    assert core.count("rows < 65536 ? rows : 65536") == 1 and core.count("if (blocks > 65536) blocks = 65536;") == 1
    assert src.count("dim3(tx_row_blocks(rows))") == 3 and src.count("dim3(tx_walk8_blocks(rows, ") == 2
    assert src.count("dim3(256)") == 6 and "65536" not in src
    assert T.ROW_GRID_CAP == 65536 and T.ELEM_GRID_CAP == 65536 * 256
    assert set(T.WRAP_CASES) == {"t5_rmsnorm", "gated_mul", "embed_rows"}
    for op, (units, cap, per_wg, case) in T.WRAP_CASES.items():
        assert cap + per_wg <= units < cap + cap // 4, (op, units, cap)
    assert T.WRAP_CASES["gated_mul"][0] == 13108 * 1280 and (13108 - 1) * 1280 < T.ELEM_GRID_CAP + 256    # the smallest row count
    assert T.WRAP_CASES["embed_rows"][0] == 32769 * 512 and (32769 - 1) * 512 < T.ELEM_GRID_CAP + 256


def test_split_gelu_boundary_is_a_multiple_of_the_tile_for_both_geometries():
    from conceptattention_amd.params import T5Params, tiny_t5_params
    for p in (T5Params(), tiny_t5_params()):
        assert p.d_ff % 256 == 0 and p.d_model % 256 == 0 and (3 * p.inner_dim) % 256 == 0


# ---------------------------------------------------------------------------------------------------------- rejection
@pytest.fixture(scope="module")
def lib():
    entry.build()
    return L.load()


def test_argument_rejection_of_the_four_entries_needs_no_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15            # a 16-byte aligned non-null address; nothing is ever launched

    def attn(**kw):
        a = dict(q=p, k=p, v=p, bias=p, out=p, ldq=64, ldk=64, ldv=64, ldo=64, n_seq=1, heads=1, L=64)
        a.update(kw)
        return lib.ca_t5_attn_bf16(a["q"], a["k"], a["v"], a["bias"], a["out"], a["ldq"], a["ldk"], a["ldv"], a["ldo"],
                                   a["n_seq"], a["heads"], a["L"], None)
    for bad in (dict(q=None), dict(bias=None), dict(out=None), dict(L=0), dict(L=96), dict(L=576), dict(heads=0),
                dict(n_seq=0), dict(ldq=63), dict(ldk=72, heads=2), dict(ldo=68), dict(q=p + 2), dict(out=p + 8),
                dict(n_seq=2 ** 31 - 1, heads=64, L=512)):
        assert attn(**bad) == -1, bad
        assert b"ca_t5_attn_bf16" in lib.ca_last_error()

    def rms(**kw):
        a = dict(x=p, ldx=256, w=p, out=p, ldo=256, rows=1, H=256, eps=1e-6)
        a.update(kw)
        return lib.ca_t5_rmsnorm_f32in(a["x"], a["ldx"], a["w"], a["out"], a["ldo"], a["rows"], a["H"], a["eps"], None)
    for bad in (dict(x=None), dict(w=None), dict(out=None), dict(rows=0), dict(H=0), dict(H=254), dict(ldx=252),
                dict(ldo=128), dict(eps=0.0), dict(x=p + 4), dict(out=p + 2)):
        assert rms(**bad) == -1, bad
        assert b"ca_t5_rmsnorm_f32in" in lib.ca_last_error()

    def gate(**kw):
        a = dict(g=p, ldg=512, u=p, ldu=512, out=p, ldo=512, rows=1, C=512)
        a.update(kw)
        return lib.ca_gated_mul_bf16(a["g"], a["ldg"], a["u"], a["ldu"], a["out"], a["ldo"], a["rows"], a["C"], None)
    for bad in (dict(g=None), dict(u=None), dict(out=None), dict(rows=0), dict(C=0), dict(C=508), dict(ldg=504),
                dict(ldu=516), dict(ldo=8), dict(u=p + 8)):
        assert gate(**bad) == -1, bad
        assert b"ca_gated_mul_bf16" in lib.ca_last_error()

    def embed(**kw):
        a = dict(table=p, ldt=256, ids=p, out=p, ldo=256, rows=1, H=256)
        a.update(kw)
        return lib.ca_embed_rows_f32(a["table"], a["ldt"], a["ids"], a["out"], a["ldo"], a["rows"], a["H"], None)
    for bad in (dict(table=None), dict(ids=None), dict(out=None), dict(rows=0), dict(H=4), dict(H=260), dict(ldt=128),
                dict(ldo=254), dict(ids=p + 2), dict(out=p + 4)):
        assert embed(**bad) == -1, bad
        assert b"ca_embed_rows_f32" in lib.ca_last_error()


def test_wrappers_reject_bad_tensors_before_any_launch():
    from conceptattention_amd import ops
    t = torch.zeros(64, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.t5_attention(t, t, t, torch.zeros(1, 127), t, 1, 1)          # not on the device
    with pytest.raises(ValueError):
        ops.t5_rmsnorm(torch.zeros(4, 256), torch.ones(256), torch.zeros(4, 256, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.gated_mul(t, t, t)
    with pytest.raises(ValueError):
        ops.embed_rows(t, torch.zeros(4, dtype=torch.int32), torch.zeros(4, 64))
