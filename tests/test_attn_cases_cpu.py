"""The attention kernels' case table without a GPU (tests/attn_cases.py): every launch site of ca_attn.hip and
ca_attn4.hip and every attention entry point of include/conceptattn.h is named by a GPU case, the edges the kernels'
indexing turns on are hit (computed from the case shapes), a faithful fp32 emulation of the kernels' numerics passes
every bound, and every bound rejects a named kernel slip."""
import os
import re

import numpy as np
import pytest

import attn_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conceptattention_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "conceptattn.h")


def launch_sites() -> list:
    sites = []
    for f in ("ca_attn.hip", "ca_attn4.hip"):
        src = open(os.path.join(CSRC, f)).read()
        sites += [re.sub(r"\s+", "", s) for s in
                  re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_]\w*(?:<[^>]*>)?)", src)]
    return sites


def attn_entry_points() -> set:
    return set(re.findall(r"\bint\s+(ca_attn_fwd_\w+)\s*\(", open(HEADER).read()))


def test_launch_sites_are_parsed():
    assert sorted(launch_sites()) == sorted(["ca_attn_kernel<8>", "ca_attn4_qk16_kernel", "ca_attn4_kernel"])


def test_every_launch_site_and_entry_point_has_a_case():
    named = {c.kernel for c in A.CASES}
    assert set(launch_sites()) == named, (set(launch_sites()), named)
    entries = attn_entry_points()
    assert entries == {"ca_attn_fwd_bf16", "ca_attn_fwd_qk16"}, entries
    covered = {c.entry.split("(")[0] for c in A.CASES}
    assert entries == covered
    # ca_attn_fwd_bf16 reaches two kernels: with a scale and with CA_ATTN_Q_PRESCALED
    assert {c.entry for c in A.CASES} == {"ca_attn_fwd_bf16", "ca_attn_fwd_bf16(CA_ATTN_Q_PRESCALED)",
                                         "ca_attn_fwd_qk16"}


def test_case_table_is_consistent():
    assert len(A.BY_ID) == len(A.CASES)
    for c in A.CASES:
        assert 1 <= len(c.probs) <= 16, c.id
        for p in c.probs:
            assert p.nq >= 1 and p.n0 >= 1 and p.n1 >= 0, c.id
            assert p.nq0 == 0 or 0 < p.nq0 < p.nq, c.id
            if p.hm_C:
                assert c.form != "scale" and p.two_q and 1 <= p.hm_C <= 8, c.id
            for (h, row, key, octv) in p.spikes:
                assert h < c.heads and row < p.nq and key < p.nk, c.id
        st = A.strides(c.heads)
        D = c.heads * 128
        assert min(st.values()) > D and len(set(st.values())) == 5


def test_probe_scale_log2_is_exactly_one():
    s = np.float32(A.PROBE_SCALE)
    assert s == np.float32(0.6931472)
    assert np.float32(s * np.float32(1.4426950408889634)) == np.float32(1.0)
    assert A.scale_terms(A.BY_ID["scale_nk40_nq20_h1"])[1] == 1.0


def _kernels(pred):
    return {c.form for c in A.CASES for p in c.probs if pred(c, p)}


ALL = {"scale", "pre", "qk16"}
A4 = {"pre", "qk16"}


def test_key_edges():
    t = A.tiles
    assert _kernels(lambda c, p: p.nk < 64) == ALL                        # nt = 1, ragged (ca_attn4: nt_full = 0)
    assert _kernels(lambda c, p: p.nk == 64) == ALL
    assert _kernels(lambda c, p: p.nk == 65) == ALL
    for rem in range(3):
        for rag in (False, True):
            assert _kernels(lambda c, p: t(p.nk)[1] >= 2 and A.loop_T(p.nk) % 3 == rem and t(p.nk)[2] == rag) >= A4, \
                (rem, rag)
    for par in (0, 1):
        for rag in (False, True):
            assert "scale" in _kernels(lambda c, p: t(p.nk)[1] >= 2 and t(p.nk)[1] % 2 == par and t(p.nk)[2] == rag)


def test_segment_edges():
    ts = A.t_straddle
    assert _kernels(lambda c, p: p.n1 == 0) == ALL
    assert _kernels(lambda c, p: p.n1 > 0 and p.n0 % 64 == 0) == ALL
    assert _kernels(lambda c, p: p.n1 > 0 and p.n0 % 64 != 0) == ALL
    assert _kernels(lambda c, p: p.n1 > 0 and p.n0 < 64) == ALL               # tile 0 straddles
    assert _kernels(lambda c, p: ts(p.n0, p.nk) == A.tiles(p.nk)[0] - 1 and A.tiles(p.nk)[2]) == ALL
    assert _kernels(lambda c, p: 0 < p.n1 < 64) == ALL
    assert _kernels(lambda c, p: p.n0 == p.nk - 1) == ALL
    # segment 1 never adjacent to segment 0: make_inputs puts it first, with junk rows between
    x = A.make_inputs(A.BY_ID["pre_nk192_seg_on_tile"])[0]
    assert x.gk1 + 64 < x.gk0 and x.gq1 + 1 < x.gq0


def test_query_edges():
    assert _kernels(lambda c, p: p.nq < 32) == ALL
    assert _kernels(lambda c, p: 32 < p.nq < 64) == ALL
    assert _kernels(lambda c, p: 0 < p.nq % 256 <= 192) >= A4                  # ca_attn4: waves without rows
    assert "scale" in _kernels(lambda c, p: 0 < p.nq % 256 <= 224)
    assert _kernels(lambda c, p: p.two_q and p.nq0 == 1) == ALL
    assert _kernels(lambda c, p: p.two_q and p.nq0 == p.nq - 1) == ALL
    assert _kernels(lambda c, p: p.two_q and p.nq0 % 32 != 0 and 1 < p.nq0 < p.nq - 1) == ALL
    assert _kernels(lambda c, p: p.two_q and p.f32) == ALL


def test_heads_problems_and_walk():
    for f in ALL:
        assert {c.heads for c in A.CASES if c.form == f} >= {1, 3, 8, 9, 24}, f
        assert {len(c.probs) for c in A.CASES if c.form == f} >= {1, 2, 16}, f
    for c in A.CASES:
        if len(c.probs) == 16:
            assert len({(p.nq, p.n0, p.n1, p.nq0) for p in c.probs}) == 16
    walking = [c for c in A.CASES if A.walks(c)]
    assert {c.form for c in walking} == A4
    for c in walking:
        total, us = A.units(c)

        def state(u):
            i, _, _ = us[u]
            p = c.probs[i]
            return (i, A.tiles(p.nk)[2], A.t_straddle(p.n0, p.nk) >= 0, p.n1 > 0, p.two_q)
        # one workgroup's successive units belong to different problems with different tile / segment state
        crossing = [w for w in range(A.N_CU) if w + A.N_CU < total and us[w] and us[w + A.N_CU]
                    and state(w)[0] != state(w + A.N_CU)[0] and state(w)[1:] != state(w + A.N_CU)[1:]]
        assert len(crossing) >= 8, c.id


def test_heatmap_and_rare_path_edges():
    for f in A4:
        hm = [p for c in A.CASES if c.form == f for p in c.probs if p.hm_C]
        assert {p.hm_C for p in hm} >= {1, 5, 8}, f
        assert all(p.nq0 % 32 for p in hm), f
    # redo (ca_attn_kernel): a spike whose tile sum passes 2^30, later than tile 0
    sc = [(p, s) for c in A.CASES if c.form == "scale" for p in c.probs for s in p.spikes]
    assert any(s[2] >= 64 and 2.0 ** s[3] > A.REDO_LIMIT for _, s in sc)
    assert any(A.tiles(p.nk)[2] and s[2] >= 64 * (A.tiles(p.nk)[0] - 1) for p, s in sc)     # masked tail tile
    assert any(s[2] // 64 == A.t_straddle(p.n0, p.nk) for p, s in sc)                        # straddling tile
    a4 = [(c, p, s) for c in A.CASES if c.form != "scale" for p in c.probs for s in p.spikes]
    assert any(s[2] // 64 == A.t_straddle(p.n0, p.nk) and 64 <= s[3] < 100 for _, p, s in a4)
    assert any(A.tiles(p.nk)[2] and s[2] >= 64 * (A.tiles(p.nk)[0] - 1) for _, p, s in a4)
    stats = {c.id: A.expected_stats(c) for c, _, _ in a4}
    assert any(st[1] and st[1] > 0 and st[0] == 0 for st in stats.values()), stats          # in-place re-reference
    assert any(st[0] and st[0] > 0 for st in stats.values()), stats                         # classical recomputation
    assert any(s[3] >= 128 for _, _, s in a4)                                               # exp2 overflow


def test_expected_counters_are_fixed_where_the_design_fixes_them():
    for c in A.CASES:
        if c.form == "scale":
            continue
        st = A.expected_stats(c)
        if c.family in ("probe", "rnd") and not any(p.spikes for p in c.probs):
            assert st == (0, 0), c.id
        assert st[0] is not None, c.id


@pytest.mark.parametrize("case", [c for c in A.CASES if c.exact], ids=lambda c: c.id)
def test_exact_probe_sums_fit_fp32(case):
    assert A.probe_bits(case, A.make_inputs(case)) <= 24


SMALL = [c for c in A.CASES
         if sum(p.nq * p.nk for p in c.probs) * c.heads <= 3_000_000 and not any(p.spikes for p in c.probs)]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.id)
def test_faithful_emulation_passes_every_bound(case):
    """fp32 scores, the tile-0 maximum as reference, fp32 exp2, P rounded to bf16, fp32 sums in tile order: within
    every bound of the case; on exact probes, equal to the fp64 reference rounded to fp32 (up to the exp's l)."""
    for p, x in zip(case.probs, A.make_inputs(case)):
        ref, pre, hm, hm_pre = A.reference(case, p, x)
        f32, b16, hmg = A.emulate(case, p, x)
        assert A.excess(f32, ref, pre, "f32")[1] == 0, case.id
        assert A.excess(b16, ref, pre, "bf16")[1] == 0, case.id
        if hm is not None:
            assert A.excess(hmg[..., :p.hm_C], hm, hm_pre, "f32")[1] == 0, case.id


@pytest.mark.parametrize("slip", list(A.SLIPS))
def test_bounds_reject_a_named_kernel_slip(slip):
    ok, r, _ = A.discrimination(slip)
    assert ok, f"{slip}: the bound rejects the faithful emulation"
    assert r > 1, f"{slip}: the bound does not see the slip (max err / bound {r:.3g})"


SINGLE = [s for s, (_, _, single) in A.SLIPS.items() if single]


@pytest.mark.parametrize("slip", SINGLE)
def test_single_key_slips_at_the_model_key_count(slip):
    """At nk = 4339 (ragged, straddling tile 4) the exact-probe bound rejects each single-key slip by 10x or more;
    the old close(atol=1e-2, rtol=8e-3) of test_kernels_gpu.py lets the same slip pass on the model-statistics
    inputs (max err / tolerance below 1): the reason the probe family exists."""
    ok, r, _ = A.discrimination(slip, big=True)
    assert ok
    assert r >= 10, f"{slip}: margin {r:.3g}"
    ok, _, old = A.discrimination(slip, big=True, family="rnd")
    assert ok
    print(f"{slip}: probe bound margin {r:.1f}, old tolerance max err / tol {old:.2f}")
    assert old < 1, f"{slip}: the old tolerance already caught it ({old:.2f})"
