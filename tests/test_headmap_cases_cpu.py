"""ca_head_maps' case table without a GPU (tests/headmap_cases.py): the shapes the cases must hit, the fp64 reference
against an fp32 emulation of the kernel's summation order over the same list, the seeded slips the bounds must reject, the
identity with the full-width logits at norm = none, and that the unit's launch site is the kernels the cases name."""
import os
import re

import pytest
import torch

import headmap_cases as H
import heatmap_many_cases as M
import rowop_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "conceptattention_amd", "csrc", "ca_headmap.hip")


def test_the_machinery_is_rowop_cases_own():
    for name in ("Case", "weighted", "logits_reference", "excess", "U"):
        assert getattr(H, name) is getattr(R, name), name
    assert H.FORMS is M.FORMS


def test_shapes_the_cases_must_hit():
    sh = [c.shape for c in H.CASES]
    assert {s["NH"] for s in sh} >= {1, 3, 4, 5, 23, 24, 32}
    assert {s["L"] for s in sh} >= {1, 2, 3, 257}
    assert {s["C"] for s in sh} >= {1, 8, 9, 16, 17, 32}
    assert {s["n"] for s in sh} == {1, 16}
    assert {s["outs"] for s in sh} == {"heads", "acc", "acc2", "all"}
    assert {s["norm"] for s in sh} == set(H.NORMS)
    assert all(s["dim"] == s["NH"] * 128 and s["ldi"] > s["dim"] and s["ldc"] > s["dim"] for s in sh)
    assert any(s["dup"] for s in sh)
    assert {pair for s in sh for pair in s["forms"]} == {(a, b) for a in ("bf16", "f32") for b in ("bf16", "f32")}
    # every instantiation with every norm, and more than one pass of 16 (8) patches with a ragged last chunk
    assert {(H.kernel_of(s["C"]), s["norm"]) for s in sh} >= {(H.kernel_of(C), n) for C in (8, 16, 32) for n in H.NORMS}
    assert any(s["NH"] % 4 and s["L"] > 16 for s in sh)
    assert len(H.BY_ID) == len(H.CASES)


def test_two_heads_of_one_patch_fall_into_different_families():
    case = H.BY_ID["heads_NH5_L257_C17_none_n16_all"]
    pr = H.make_inputs(case)["probs"][2]                       # (fp32 rows: the families' exact values survive)
    z, _ = H.head_logits(pr["img"][:, :case.shape["dim"]], pr["con"][:, :case.shape["dim"]], case.shape["NH"])
    p = torch.arange(case.shape["L"])
    for h in range(case.shape["NH"]):
        tied = (p + h) % 7 == 1
        assert bool((z[h][:, tied] == 0.625).all()) and not bool((z[h][:, ~tied] == 0.625).all(0).any())
        assert float(z[h][:, (p + h) % 7 == 4].min()) > 200


def test_launch_site_is_the_kernels_the_cases_name():
    src = open(SRC).read()
    host = re.sub(r"//[^\n]*", "", src[src.index('extern "C" int ca_head_maps'):])
    assert "__global__" not in host
    forms = {re.sub(r"\s+", "", f) for f in re.findall(r"\b(ca_\w+_kernel\b(?:<[^>]*>)?)", host)}
    assert forms == {c.kernel for c in H.CASES}, sorted(forms)
    kernel = src.split("namespace {")[1]
    assert "atomic" not in kernel and "asm" not in src          # no atomics; plain HIP


WORST = {}


@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c.id)
def test_fp32_emulation_is_inside_every_bound(case):
    inp = H.make_inputs(case)
    ref = H.reference(case, inp)
    got = H.emulate(case, inp)
    worst, n_over = H.over_the_bound(got, ref)
    WORST[case.shape["norm"]] = max(WORST.get(case.shape["norm"], 0.0), worst)
    print(f"\n  {case.id}: max err / bound = {worst:.3f}   (per norm so far: "
          + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())) + ")")
    assert n_over == 0, f"{case.id}: {n_over} elements of the fp32 emulation over the bound ({worst:.3g})"


@pytest.mark.parametrize("name", list(H.SLIPS))
def test_a_seeded_slip_fails_the_bound(name):
    slip, cids, which = H.SLIPS[name]
    caught = 0
    for cid in cids:
        case = H.BY_ID[cid]
        inp = H.make_inputs(case)
        ref = H.reference(case, inp)
        _, n_good = H.over_the_bound(H.emulate(case, inp), ref, only=which)
        _, n_bad = H.over_the_bound(H.emulate(case, inp, slip=slip), ref, only=which)
        assert n_good == 0, (name, cid, n_good)
        caught += n_bad > 0
    assert caught > 0, name


@pytest.mark.parametrize("cid", ["heads_NH24_L257_C12_none_n1_acc2", "heads_NH5_L257_C17_none_n16_all",
                                 "heads_NH32_L257_C9_none_n1_all"])
def test_at_norm_none_the_head_sum_is_the_full_width_logit(cid):
    """NH x the reference's mean equals rowop_cases.logits_reference on the same rows, inside the two bounds added."""
    case = H.BY_ID[cid]
    s = case.shape
    inp = H.make_inputs(case)
    for pr, res in zip(inp["probs"], H.reference(case, inp)):
        mean, pre, _ = res["acc2"]
        z, e_z, _ = R.logits_reference(case, pr)["logits"]      # (reads shape["dim"] = NH x 128, img and con)
        err = (s["NH"] * mean - z).abs()
        assert bool((err <= s["NH"] * pre + e_z).all()), float((err / (s["NH"] * pre + e_z)).max())
