"""The address-range cases (tests/address_range_cases.py, tests/placement.py) without a GPU: every kernel and operand
role of the attention and GEMM case tables has a placement case, the limits DESIGN.md ("Address arithmetic") states
are the ones at which the kernels' 32-bit expressions stop equalling the 64-bit address, the GEMM limit goes through
ca_gemm_plan, and named slips move at least one touched 16-byte access on the chosen placements."""
import ctypes

import numpy as np
import pytest

import address_range_cases as C
import attn_cases as A
import gemm_route_cases as G
import placement as PL
from conceptattention_amd import _lib as L

LINE = 1 << 32

# Roles the audit proves are never dereferenced at a placement of their own: none
NEVER_DEREFERENCED = {}


def test_every_attention_kernel_and_role_has_a_placement_case():
    kernels = {c.kernel for c in A.CASES}
    assert kernels == set(C.ATTN_PLACEMENT), kernels ^ set(C.ATTN_PLACEMENT)
    for kernel, cid in C.ATTN_PLACEMENT.items():
        case = A.BY_ID[cid]
        assert case.kernel == kernel and len(case.probs) == 1
        p = case.probs[0]
        have = {"q", "k0/v0", "out"}
        if p.two_q:
            have |= {"q1", "out1"}
        if p.n1:
            have.add("k1/v1")
        if p.f32:
            have.add("out_f32")
        if p.hm_C:
            have |= {"hm_con", "hm_part"}
        assert have == set(C.ATTN_ROLES[kernel]), (kernel, have ^ set(C.ATTN_ROLES[kernel]))
    all_roles = {"q", "q1", "k0/v0", "k1/v1", "out", "out1", "out_f32", "hm_con", "hm_part"}
    assert set(C.ATTN_ROLES["ca_attn4_kernel"]) == all_roles == set(C.ATTN_ROLES["ca_attn4_qk16_kernel"])
    # the scaling kernel takes no heat-map operands: the validator refuses them ("... and the pre-scaled-q kernel")
    assert all_roles - set(C.ATTN_ROLES["ca_attn_kernel<8>"]) == {"hm_con", "hm_part"}
    assert not any(p.hm_C for c in A.CASES if c.form == "scale" for p in c.probs)
    assert set(C.ATTN_PAST) == {"q", "out", "out_f32"}
    assert {f for f in A.FORMS} == {"scale", "pre", "qk16"} and len(C.ATTN_FAR) == 4       # far rows: every form x 4


def test_every_gemm_route_and_role_has_a_placement_and_a_far_row_case():
    """The GPU file runs gemm_roles(epi, fp8) for every (route, epi) of gemm_epis_for, and GEMM_FAR for every route."""
    placed = {}
    for route in G.ROUTES:
        epis = C.gemm_epis_for(route)
        assert epis, route
        assert all(G.Case(route, e) in G.CASES for e in epis), route     # existing cases of the table
        placed[C.gemm_kernel_of(route)] = set().union(*(C.gemm_roles(e, G.ROUTES[route].fp8) for e in epis))
    assert len(placed) >= 12, placed            # 4 classic, 3 ping-pong (+ thin tiles in the walk), 4 thin-row, fp8
    for kernel, roles in placed.items():
        want = set(C.GEMM_ISSUE_ROLES)
        if "fp8" not in kernel:
            want -= {"scales"}
        if not any(G.compatible(r, "qkv_single_qpre_f32_f16") for r in G.ROUTES if C.gemm_kernel_of(r) == kernel):
            want -= {"q_prerope", "rope"}       # the qkv epilogue exists under the 256-wide ping-pong tile, NW = 4 only
        assert want <= roles, (kernel, want - roles)
    assert {r for r, _, _ in C.GEMM_FAR} == {"A", "W"} and {n for _, n, _ in C.GEMM_FAR} == {"3GiB", "max"}
    assert C.MOD_CHUNK["K"] == 3072 and LINE - (1 << 21) < C.MOD_CHUNK["N"] * 3072 * 2 < LINE and C.MOD_CHUNK["N"] % 256 == 0
    assert {(e, r) for _, e, r in C.GEMM_PAST} >= {("bias_bf16", "out"), ("bias_f32", "out"), ("gate_items_bf16", "resid"),
                                                   ("split_gelu", "out2"), ("qkv_single_qpre_f32_f16", "q_prerope")}


def test_every_rowop_form_and_plane_has_a_placement_case():
    """The GPU file places every case of rowop_cases.py, once per plane of rowop_roles(case)."""
    import rowop_cases as R
    assert len({c.kernel for c in R.CASES}) == 35
    for c in R.CASES:
        roles = C.rowop_roles(c)
        assert len(roles) == len(set(roles)) >= 2, c.id
    past = {(R.BY_ID[cid].op, role) for cid, role in C.ROWOP_PAST}
    assert past >= {("ln", "x"), ("ln", "out"), ("ln", "out_lo"), ("qk", "qkv"), ("logits", "img"), ("fused", "img")}
    assert R.BY_ID["temb_grid_stride"].shape["nt"] * 128 > 4096 * 256     # a second trip through the grid-stride loop


def test_every_vae_entry_point_and_role_has_a_placement_and_a_far_case():
    """The GPU file places VAE_PLACEMENT's case of every entry point of ca_vae.hip once per role of VAE_ROLES, and
    runs VAE_PAST with one operand's row stride from far_ld."""
    import vae_cases as V
    want = {"ca_conv3x3_nhwc": {"x", "w", "bias", "resid", "out"}, "ca_groupnorm_nhwc": {"x", "gamma", "beta", "y", "part"},
            "ca_softmax_rows_f32": {"s", "p"}, "ca_affine_rows_f32": {"x", "logvar", "noise", "out"}}
    assert {c.entry for c in V.CASES} == set(C.VAE_PLACEMENT) == set(want)
    for entry, cid in C.VAE_PLACEMENT.items():
        case = V.BY_ID[cid]
        assert case.entry == entry
        roles = C.VAE_ROLES[entry]
        assert len(roles) == len(set(roles)) and set(roles) == want[entry] == set(C.vae_roles(case)), entry
        if case.op == "affine":
            assert not case.shape["view"]        # four buffers of their own
        if case.op == "gn":
            assert (case.shape["n_chunks"] or V.groupnorm_chunks(case.shape["HW"])) > 1      # part: more than one chunk
    past = {(V.BY_ID[cid].op, role, V.BY_ID[cid].shape.get("out")) for cid, role in C.VAE_PAST}
    assert past >= {("conv", "x", "f32"), ("conv", "resid", "f32"), ("conv", "out", "f32"), ("conv", "out", "bf16"),
                    ("gn", "x", None), ("gn", "y", None), ("softmax", "s", None), ("softmax", "p", None),
                    ("affine", "x", "bf16"), ("affine", "out", "bf16")}
    assert C.VAE_PAST_OWN_TEST in C.VAE_PAST
    for cid, role in C.VAE_PAST:
        s = V.BY_ID[cid].shape
        assert role in C.vae_roles(V.BY_ID[cid]), (cid, role)
        if V.BY_ID[cid].op == "conv":
            assert (s["B"], s["H"], s["W"]) == (2, 5, 7), cid
        if V.BY_ID[cid].op == "gn":
            assert (s["B"], s["HW"]) == (2, 7), cid
        if V.BY_ID[cid].op in ("softmax", "affine"):
            assert s["rows"] == {"softmax": 5, "affine": 70}[V.BY_ID[cid].op], cid
        rows, item = C.vae_far_rows(cid, role)
        ld = C.far_ld(rows, item, C.PAST_4GIB)
        assert ld < 1 << 31, (cid, role, ld)                       # the entry points take int32_t strides
        assert (rows - 1) * ld * item >= LINE, (cid, role)         # the last row starts 2^32 bytes or more from the base
        assert ((rows - 1) * ld + 1) * item > LINE, (cid, role)    # and the touched extent exceeds 2^32 bytes
        assert rows * ld * item <= C.PAST_4GIB < PL.ARENA_BYTES - 2 * PL.GUARD - 256


def test_every_text_pixel_and_scoring_entry_point_and_role_has_a_placement_and_a_far_case():
    """The GPU file places TEXT_PLACEMENT's case of every entry point of ca_t5.hip, ca_clip.hip, ca_pixels.hip and
    ca_seg.hip once per role of TEXT_ROLES, and runs TEXT_PAST (and the pixel source) with one operand's row stride
    from far_ld."""
    import os
    import re

    import clip_cases as CL
    import pixel_cases as P
    import seg_cases as S
    import t5_cases as T5
    import t5_fp8_cases as F8
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    entries = set()
    for unit in ("ca_t5.hip", "ca_clip.hip", "ca_pixels.hip", "ca_seg.hip"):
        src = open(os.path.join(root, "conceptattention_amd", "csrc", unit)).read()
        entries |= set(re.findall(r'extern "C" int (ca_\w+)\(', src))
    assert entries == set(C.TEXT_PLACEMENT) == set(C.TEXT_ROLES) == set(C.TEXT_FREE_STRIDES), entries ^ set(C.TEXT_PLACEMENT)
    # the roles are the pointer parameters of the entry point (ca_seg_score: the pointers of its problem struct)
    pointers = {name: sum(a is ctypes.c_void_p for a in L.SIGNATURES[name][1]) - 1 for name in entries}     # - the stream
    pointers["ca_seg_score"] = len(L.SegProblem._fields_)
    for name, roles in C.TEXT_ROLES.items():
        assert len(roles) == len(set(roles)) == pointers[name], (name, roles, pointers[name])
    # existing cases of the tables
    assert C.TEXT_PLACEMENT["ca_t5_attn_bf16"] in T5.ATTN_CASES and C.TEXT_PLACEMENT["ca_clip_attn_bf16"] in CL.ATTN_CASES
    assert C.TEXT_PLACEMENT["ca_clip_attn_bf16"].layout == "apart" and C.TEXT_PLACEMENT["ca_t5_attn_bf16"].layout == "contig"
    assert C.TEXT_PLACEMENT["ca_t5_rmsnorm_f32in"] in T5.ROW_CASES and C.TEXT_PLACEMENT["ca_embed_rows_f32"] in T5.EMBED_CASES
    assert C.TEXT_PLACEMENT["ca_gated_mul_bf16"] in T5.GATE_CASES and C.TEXT_PLACEMENT["ca_gated_mul_fp8"] in F8.GATE_CASES
    assert C.TEXT_PLACEMENT["ca_t5_rmsnorm_f32in_fp8"] in F8.RMS_CASES and C.TEXT_PLACEMENT["ca_layernorm_f32in"] in CL.LN_CASES
    assert C.TEXT_PLACEMENT["ca_quick_gelu_bf16"] in CL.QG_CASES and C.TEXT_PLACEMENT["ca_clip_embed_f32"] in CL.EMBED_H
    assert C.TEXT_PLACEMENT["ca_pixels_u8_to_nhwc32_bf16"] in P.RESIZE_CASES
    assert C.TEXT_PLACEMENT["ca_seg_score"] in {c.name for c in S.CASES}
    # far rows: every operand with a free row stride, at a stride the int32_t parameters take
    far = {}
    for entry, case, role, rows, item in C.TEXT_PAST:
        assert role in C.TEXT_ROLES[entry], (entry, role)
        far.setdefault(entry, set()).add(role)
        ld = C.far_ld(rows, item, C.PAST_4GIB)
        assert ld < 1 << 31, (entry, role, ld)
        assert (rows - 1) * ld * item >= LINE, (entry, role)             # the last row starts 2^32 bytes or more from the base
        assert rows * ld * item <= C.PAST_4GIB < PL.ARENA_BYTES - 2 * PL.GUARD - 256
        assert rows == 64 if "attn" in entry else rows in (5, 6, 7, 8, 9, 77, 231), (entry, role, rows)
    far.setdefault(C.TEXT_PAST_OWN_TEST[0], set()).add(C.TEXT_PAST_OWN_TEST[1])
    for entry, roles in C.TEXT_FREE_STRIDES.items():
        assert far.get(entry, set()) == roles, (entry, far.get(entry), roles)
    assert any(e == "ca_layernorm_f32in" and c[2] and r == "x" for e, c, r, _, _ in C.TEXT_PAST)      # the gathered x
    h0 = C.PIXEL_FAR[0]
    assert (h0 - 1) * C.far_ld(h0, 1, C.PAST_4GIB) >= LINE and L.SIGNATURES["ca_pixels_u8_to_nhwc32_bf16"][1][1] is ctypes.c_int64
    assert ctypes.c_int32(C.BAD_STRIDE).value == 256                     # what ctypes would hand the library


def test_no_role_is_left_out():
    assert not NEVER_DEREFERENCED


@pytest.mark.parametrize("base", [0x7F0000000000, 0x7F00C0000000 - 1, 0x7F0040000010, 0x7F00FFFFF000, 0x100000000])
def test_arena_boundary_and_straddle_arithmetic(base):
    b = PL.boundary_in(base)
    assert b % LINE == 0 and b - base >= PL.GIB and base + PL.ARENA_BYTES - b >= PL.GIB
    s = PL.straddle_start(b, PL.mid(40, 30, 3 * 384 + 24, 384, 384), 2, 80 * (3 * 384 + 24) * 2)
    assert s % 16 == 0 and s < b < s + 80 * (3 * 384 + 24) * 2
    lo = max(base, b - 2 * PL.GIB)
    assert (lo >> 31) & 1 and ((b - 1) >> 31) & 1 and (lo >> 32) == ((b - 1) >> 32)


def test_attention_limits_are_where_the_32_bit_offsets_stop_being_exact():
    # accepted far-row extents: the emulated 32-bit arithmetic equals the 64-bit offset for every access
    for name, ((nq, n0, n1, nq0), extent) in C.ATTN_FAR.items():
        ld = C.far_ldkv(n0 + n1, extent)
        assert C.attn_accepts(n0, n1, ld) and ld % 8 == 0, name
        if "max" in name:
            assert LINE - (n0 + n1) * ld * 2 < ld * 2, "the last row ends within one row of 2^32"
        emu, exact = C.attn_offsets_u32(n0, n1, ld)
        assert emu.size and np.array_equal(emu, exact), name
        assert int(exact.max()) + 16 <= (n0 + n1) * ld * 2 < LINE
    for name, (nk, ld_at) in C.ATTN_LIMITS.items():
        assert C.attn_accepts(nk, 0, ld_at - 8) and not C.attn_accepts(nk, 0, ld_at), name
    # at the first limit the scalar tile offset wraps; one tile more of keys and an access is wrong
    nk, ld_at = C.ATTN_LIMITS["(n0 + n1) * ldkv * 2 < 2^32"]
    emu, exact = C.attn_offsets_u32(nk, 0, ld_at - 8)
    assert np.array_equal(emu, exact)
    emu, exact = C.attn_offsets_u32(nk + 64, 0, ld_at)
    assert not np.array_equal(emu, exact)
    # at the second limit koff of row 63 needs 64 * ldkv * 2 > 2^32 - one row: the lane offset itself wraps
    ld2 = C.ATTN_LIMITS["64 * ldkv * 2 < 2^32"][1]
    with np.errstate(over="ignore"):
        koff = (np.arange(64, dtype=np.uint32) * np.uint32(ld2 - 8) + np.uint32(120)) * np.uint32(2)
    assert np.array_equal(koff.astype(np.uint64), (np.arange(64, dtype=np.uint64) * np.uint64(ld2 - 8) + np.uint64(120)) * np.uint64(2))
    with np.errstate(over="ignore"):
        koff = (np.arange(65, dtype=np.uint32) * np.uint32(ld2) + np.uint32(120)) * np.uint32(2)
    assert int(koff[64]) != 64 * ld2 * 2 + 240


def test_gemm_operand_limit_through_the_plan():
    """M * lda * 2 and N * ldw * 2 below 2^32 (ca_gemm.hip plan_gemm), through ca_gemm_plan(n_cu=256): no launch."""
    from conceptattention_amd import ops
    K = 3072

    def plan(M, N, lda, ldw):
        arr = (L.GemmProblem * 1)()
        G._raw_problem(arr[0], M, N, K, L.EPI_BIAS)
        arr[0].lda, arr[0].ldw = lda, ldw
        return ops.gemm_plan(arr, tile=L.TILE_PP_256x256, n_cu=256, fp8=False)

    M, lda = 2048, LINE // (2 * 2048)                 # M * lda * 2 == 2^32 exactly
    assert M * lda * 2 == LINE
    plan(M, 256, lda - 8, K)
    with pytest.raises(ValueError, match="operand larger than 4 GiB"):
        plan(M, 256, lda, K)
    N, ldw = 4096, LINE // (2 * 4096)
    plan(256, N, K, ldw - 8)
    with pytest.raises(ValueError, match="operand larger than 4 GiB"):
        plan(256, N, K, ldw)
    # the 32-bit row offsets of the staging loads equal the 64-bit ones under the limit, and wrap at it
    with np.errstate(over="ignore"):
        off = np.arange(M, dtype=np.uint32) * np.uint32(lda - 8) * np.uint32(2) + np.uint32(112)
        assert np.array_equal(off.astype(np.uint64), np.arange(M, dtype=np.uint64) * np.uint64(lda - 8) * np.uint64(2) + np.uint64(112))
        off = np.arange(M + 1, dtype=np.uint32) * np.uint32(lda) * np.uint32(2)
        assert int(off[M]) != M * lda * 2


@pytest.mark.parametrize("slip", ["sign_extend", "row_ld_i32"])
def test_offset_slips_move_an_access_on_the_far_row_cases(slip):
    for name, ((nq, n0, n1, nq0), extent) in C.ATTN_FAR.items():
        emu, exact = C.attn_offsets_u32(n0, n1, C.far_ldkv(n0 + n1, extent), slip)
        assert int((emu != exact).sum()) >= 1, (slip, name)


def test_base_address_slips_move_an_access_on_the_placements():
    """A sign-extended low half breaks every access of a bit31 buffer; a dropped carry into bit 32 breaks the upper
    part of a straddling one (and nothing of a bit31 buffer: why both placements are run)."""
    B = PL.boundary_in(0x7F0012345000)
    n = 1 << 20
    a, sign, nocarry = C.base_address_slips(B - 3 * n, n)                 # bit31
    assert (a != sign).all() and (a == nocarry).all()
    s = PL.straddle_start(B, n // 4, 2, n)
    a, sign, nocarry = C.base_address_slips(s, n)                          # straddle
    assert (a != nocarry).any() and (a != sign).any()
    assert (a[a >= B] != nocarry[a >= B]).all()
