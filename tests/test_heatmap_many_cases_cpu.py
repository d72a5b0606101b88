"""ca_heatmap_many's case table without a GPU (tests/heatmap_many_cases.py): the shapes the cases must hit, the fp64
reference against an fp32 emulation of the kernel over the same list, the seeded slips the bounds must reject, and that the
unit's launch sites are the kernels the cases name."""
import os
import re

import pytest
import torch

import heatmap_many_cases as H
import rowop_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "conceptattention_amd", "csrc", "ca_heatmap_many.hip")
MANY = [c for c in H.CASES if c.op == "many"]


def test_the_machinery_is_rowop_cases_own():
    for name in ("Case", "norm_logits", "weighted", "sparse_bound", "logits_reference", "excess"):
        assert getattr(H, name) is getattr(R, name), name


def test_shapes_the_cases_must_hit():
    sh = [c.shape for c in MANY]
    assert {s["C"] for s in sh} >= {1, 8, 9, 16, 17, 24, 25, 31, 32}
    assert {s["L"] for s in sh} >= {1, 2, 3, 257}
    assert {s["dim"] for s in sh} >= {8, 264, 520, 3072, 4096}
    assert any(s["dim"] == 4096 and s["C"] == 32 for s in sh)
    assert {s["n"] for s in sh} == {1, 16}
    assert {s["outs"] for s in sh} == {"acc", "acc2", "logits", "all"}
    assert {s["norm"] for s in sh} == {"softmax", "sparsemax", "entmax15"}
    assert all(s["ldi"] > s["dim"] and s["ldc"] > s["dim"] for s in sh)
    assert any(s["dup"] for s in sh)
    for nch in (1, 2, 3, 4):                                   # every chunk count, with all three norms past one chunk
        assert any(len(H.chunks(s["C"])) == nch for s in sh)
    assert {(s["C"] > 16, s["norm"]) for s in sh if s["C"] > 8} == {(b, n) for b in (False, True)
                                                                   for n in ("softmax", "sparsemax", "entmax15")}
    sparse = [c.shape for c in H.CASES if c.op == "norm"]
    assert {(s["norm"], s["C"]) for s in sparse} == {(n, C) for n in ("sparsemax", "entmax15") for C in (17, 24, 32)}
    assert len(H.BY_ID) == len(H.CASES)


def test_chunks_are_at_most_eight_rows_and_cover_every_concept():
    for C in range(1, 33):
        cks = H.chunks(C)
        assert len(cks) == (C + 7) // 8 and cks[0][0] == 0 and cks[-1][1] == C
        assert all(a1 == b0 for (_, a1), (b0, _) in zip(cks, cks[1:]))
        assert all(1 <= c1 - c0 <= 8 for c0, c1 in cks)
    assert H.chunks(9) == [(0, 5), (5, 9)] and H.chunks(32) == [(0, 8), (8, 16), (16, 24), (24, 32)]


def test_launch_sites_are_the_kernels_the_cases_name():
    src = open(SRC).read()
    host = re.sub(r"//[^\n]*", "", src[src.index("\nint ca_heatmap_sparse32"):])
    assert "__global__" not in host
    forms = {re.sub(r"\s+", "", f) for f in
             re.findall(r"(?<!\(const void \*\))\b(ca_\w+_kernel\b(?:<[^>]*>)?)", host)}
    named = {re.sub(r"\s+", "", c.kernel) for c in H.CASES}
    assert forms == named, (sorted(forms), sorted(named))


@pytest.mark.parametrize("C", [9, 17, 32])
@pytest.mark.parametrize("norm", ["softmax", "sparsemax", "entmax15"])
def test_the_weighting_reference_and_its_bound_are_generic_in_C(C, norm):
    """rowop_cases.weighted on rowop_cases.norm_logits beyond the concept counts rowop_cases.py itself uses."""
    z = H.norm_logits(C, 257, 40 + C).double()
    o, pre = H.weighted(z, None, norm, 1.0, torch.zeros_like(z))
    assert float((o.sum(0) - 1).abs().max()) <= 2e-15
    if norm != "softmax":                                      # the sparse supports: from one concept to all C (the ties)
        sup = (o > 0).sum(0)
        assert int(sup.min()) == 1 and int(sup.max()) == C
    print(f"\n  C = {C} {norm}: bound {float(pre.min()):.3g} .. {float(pre.max()):.3g}")
    # (a sanity limit on the bound itself: three orders below 1 / C, the size of a probability it is there to check)
    assert 0 < float(pre.max()) < 1e-4 / 3 and torch.isfinite(pre).all()


@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c.id)
def test_fp32_emulation_is_inside_every_bound(case):
    inp = H.make_inputs(case)
    ref = H.reference(case, inp)
    if case.op == "norm":                                       # (rowop_cases' own emulation: the reference, stored as fp32)
        got = [{k: R.rounded_like_output(r, kind) for k, (r, _, kind) in ref[0].items()}]
    else:
        got = H.emulate(case, inp)
    worst, n_over = H.over_the_bound(case, inp, got, ref)
    print(f"\n  {case.id}: max err / bound = {worst:.3f}")
    assert n_over == 0, f"{case.id}: {n_over} elements of the fp32 emulation over the bound ({worst:.3g})"


@pytest.mark.parametrize("name", list(H.SLIPS))
def test_a_seeded_slip_fails_the_bound(name):
    cid, slip, which = H.SLIPS[name]
    case = H.BY_ID[cid]
    inp = H.make_inputs(case)
    ref = H.reference(case, inp)
    _, n_good = H.over_the_bound(case, inp, H.emulate(case, inp), ref, only=which)
    _, n_bad = H.over_the_bound(case, inp, H.emulate(case, inp, slip=slip), ref, only=which)
    assert n_good == 0 and n_bad > 0, (name, n_good, n_bad)


def test_the_three_launch_slip_of_rowop_cases_is_caught_at_32_concepts():
    """rowop_cases' own seeded slip (the support one entry too large) against the bounds at C = 32."""
    case = H.BY_ID["sparsemax_C32"]
    inp = H.make_inputs(case)
    ref, pre, kind = R.reference(case, inp)["acc"]
    bad = R.reference(case, inp, mutate={"support_off_by_one": True})["acc"][0]
    assert R.excess(R.rounded_like_output(ref, kind), ref, pre, kind)[1] == 0
    assert R.excess(R.rounded_like_output(bad, kind), ref, pre, kind)[1] > 0
