"""ca_propagate_maps' case table without a GPU (tests/propmap_cases.py): the fp32 emulation of the kernel's order lies
inside the derived bound of the fp64 reference on every case, every named slip leaves it on at least one, the reference is
the softmax-weighted mean it says it is, and the axes the cases must cover are all hit.  No case is skipped or filtered by
a comparison."""
import pytest
import torch

import propmap_cases as P

WORST = {}


def _over(c, slip=None):
    acc, acc2 = P.emulate_outputs(c, slip)
    return P.check_outputs(c, dict(acc=acc, acc2=acc2))


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c.id)
def test_the_emulation_lies_inside_the_bound(case):
    r = _over(case)
    print(f"\n  {case.id}: max err / bound  maps {r['maps'][0]:.3f}  acc {r['acc'][0]:.3f}")
    old = WORST.get(case.family, (0.0, 0.0))
    WORST[case.family] = tuple(max(o, r[k][0]) for o, k in zip(old, ("maps", "acc")))
    assert all(n_over == 0 for _, n_over in r.values()), (case.id, r)


def test_print_the_largest_ratio_per_family():
    for case in P.CASES:
        if case.family not in WORST:
            test_the_emulation_lies_inside_the_bound(case)
    print()
    for fam in P.FAMILIES:
        print(f"  {fam:14s} emulation, largest max err / bound: maps {WORST[fam][0]:.3f}  acc (non-zero start) {WORST[fam][1]:.3f}")
    assert set(WORST) == set(P.FAMILIES)


@pytest.mark.parametrize("slip", P.SLIPS)
def test_every_slip_leaves_the_bound(slip):
    left = []
    for c in P.CASES:
        if c.nq > 200 or c.heads > 5:
            continue                                  # (the slips are looked for on the quick cases)
        r = _over(c, slip)
        if any(n_over for _, n_over in r.values()):
            left.append((c.id, max(w for w, _ in r.values())))
    print(f"\n  {slip}: leaves the bound on {len(left)} cases")
    assert left, slip
    assert len(P.SLIPS) >= 8


def test_the_reference_is_the_softmax_weighted_mean():
    c = next(c for c in P.CASES if c.family == "cold_text" and c.vkind != "const")
    out, bound = P.reference(c)
    q, k, v = P.operands(c)
    s = torch.einsum("ihd,jhd->hij", q, k) * c.scale_log2 * P.LN2            # nats
    want = torch.einsum("hij,cj->ci", torch.softmax(s, -1)[:, :, c.n0:], v) / c.heads
    assert torch.allclose(out, want, rtol=1e-11, atol=0)
    # the cold block: the valued keys hold about e^-20 of the weight, bounded relatively to what they carry (a kernel that
    # returns zeros there fails)
    carried = torch.einsum("hij,cj->ci", torch.softmax(s, -1)[:, :, c.n0:], v.abs()) / c.heads
    assert float(carried.max()) < 1e-4 and float((bound / carried.clamp_min(1e-300))[carried > 0].max()) < 1e-3


def test_a_constant_map_stays_constant_without_leading_keys():
    hit = 0
    for c in P.CASES:
        if c.vkind == "const":
            out, bound = P.reference(c)
            if c.n0 == 0:
                assert torch.allclose(out, torch.full_like(out, P.CONST), rtol=0, atol=1e-14), c.id
                assert float(bound.max()) < 1e-3 * P.CONST
                hit += 1
            else:
                assert bool((out < P.CONST).all()), c.id
    assert hit >= 1
    one = next(c for c in P.CASES if (c.n0, c.n1) == (0, 1))
    assert torch.equal(P.reference(one)[0], P.operands(one)[2].expand(-1, one.nq))


def test_the_axes_are_all_hit():
    C = P.CASES
    assert {c.heads for c in C} == set(P.HEADS) == {1, 2, 3, 5, 24}
    assert {c.nq for c in C} == set(P.NQ) == {1, 15, 16, 17, 63, 64, 65, 200, 513}
    assert {c.n0 for c in C} == set(P.N0) == {0, 1, 77, 512}
    assert {c.n1 for c in C} == set(P.N1) == {1, 31, 127, 128, 129, 1100}
    assert {c.C for c in C} == set(P.CS) == {1, 5, 16, 17, 32}
    assert {(c.C, c.n1) for c in C} >= {(a, b) for a in P.CS for b in P.N1}
    for fam in P.FAMILIES:
        assert {c.f16 for c in C if c.family == fam} == {False, True}, fam
    assert set(P.FAMILIES) == {"unit", "peaky8", "peaky16", "cold_text", "dominant", "ties", "last_tile_max"}
    assert {c.vkind for c in C} == set(P.VKINDS) == {"softmax", "normal", "onehot", "const"}
    assert {c.vkind for c in C if c.n0 == 0} == set(P.VKINDS)
    assert {c.pad for c in C} == set(range(4)) and len(set(P.PADS)) == 4      # four row strides for q and for k
    assert {c.vpad for c in C} == set(range(len(P.VPADS))) and min(P.VPADS) >= 1      # ldv > n1 everywhere
    assert {c.prescaled for c in C} == {False, True}
    assert any((c.n0 + c.n1) % P.TILE == 0 for c in C) and any((c.n0 + c.n1) % P.TILE for c in C)
    assert any(c.heads == 24 and c.nq % P.ROWS for c in C)
    assert len({c.id for c in C}) == len(C)


def test_nothing_a_launch_may_not_read_is_finite():
    """The operands' slices hold the values; every other element of every buffer is NaN."""
    for c in P.CASES[:6]:
        b = P.make_inputs(c)["buffers"]
        for name in ("q", "k0", "k1", "v"):
            full = b[name] if name == "v" else P.from_bits(b[name], c.f16)
            seen = torch.zeros_like(full, dtype=torch.bool)
            r, w = P.view(c, b, name).shape
            seen[:r, :w] = True
            assert bool(torch.isnan(full[~seen]).all()) and bool((~seen).any())
            assert bool(torch.isfinite(full[seen]).all())
