"""ca_query_maps' case table without a GPU (tests/querymap_cases.py): the fp32 emulation of the kernel's order lies inside
the derived bound of the fp64 reference on every case, every named slip leaves it on at least one, the reference's rows
sum to 1 without leading keys, and the axes the cases must cover are all hit.  No case is skipped or filtered by a
comparison."""
import math

import pytest
import torch

import querymap_cases as Q

WORST = {}


def _over(c, slip=None):
    acc, acc2, lse = Q.emulate_outputs(c, slip)
    return Q.check_outputs(c, dict(acc=acc, acc2=acc2, lse=lse))


@pytest.mark.parametrize("case", Q.CASES, ids=lambda c: c.id)
def test_the_emulation_lies_inside_the_bound(case):
    r = _over(case)
    print(f"\n  {case.id}: max err / bound  maps {r['maps'][0]:.3f}  acc {r['acc'][0]:.3f}  lse {r['lse'][0]:.3f}")
    old = WORST.get(case.family, (0.0, 0.0, 0.0))
    WORST[case.family] = tuple(max(o, r[k][0]) for o, k in zip(old, ("maps", "acc", "lse")))
    assert all(n_over == 0 for _, n_over in r.values()), (case.id, r)


def test_print_the_largest_ratio_per_family():
    for case in Q.CASES:
        if case.family not in WORST:
            test_the_emulation_lies_inside_the_bound(case)
    print()
    for fam in Q.FAMILIES:
        print(f"  {fam:14s} emulation, largest max err / bound: maps {WORST[fam][0]:.3f}  acc (non-zero start) "
              f"{WORST[fam][1]:.3f}  lse {WORST[fam][2]:.3f}")
    assert set(WORST) == set(Q.FAMILIES)


@pytest.mark.parametrize("slip", Q.SLIPS)
def test_every_slip_leaves_the_bound(slip):
    left = []
    for c in Q.CASES:
        if c.nq > 77:
            continue                                  # (the slips are looked for on the quick cases)
        r = _over(c, slip)
        if any(n_over for _, n_over in r.values()):
            left.append((c.id, max(w for w, _ in r.values())))
    print(f"\n  {slip}: leaves the bound on {len(left)} cases")
    assert left, slip


def test_the_reference_is_a_softmax_and_the_bound_is_relative():
    c = next(c for c in Q.CASES if c.family == "cold_text" and not c.f16)
    maps, lse, bound = Q.reference(c)
    q, k = Q.operands(c)
    s = torch.einsum("ihd,jhd->hij", q, k) * c.scale_log2 * Q.LN2            # nats
    want = torch.softmax(s, -1)[:, :, c.n0:].mean(0)
    assert torch.allclose(maps, want, rtol=1e-12, atol=0)
    assert torch.allclose(lse, torch.logsumexp(s, -1), rtol=1e-12, atol=1e-12)
    # the cold block: cells of about e^-20 / n, bounded relatively (a kernel that returns zeros there fails)
    assert float(maps.max()) < 1e-7 and float((bound.maps / maps).max()) < 1e-3
    # the families differ from head to head: the dominant key is another one in every head
    d = next(c for c in Q.CASES if c.family == "dominant" and not c.f16 and c.n0 > 0)
    q, k = Q.operands(d)
    top = (torch.einsum("ihd,jhd->hij", q, k)).argmax(-1)
    assert [int(top[h, 0]) for h in range(d.heads)] == [d.n0 + (d.n1 // 2 + 7 * h) % d.n1 for h in range(d.heads)]
    assert bool((top == top[:, :1]).all())
    m = next(c for c in Q.CASES if c.family == "last_tile_max" and c.n1 % Q.EMIT)
    q, k = Q.operands(m)
    top = torch.einsum("ihd,jhd->hij", q, k).argmax(-1)
    n = m.n0 + m.n1
    assert bool((top >= n - 3).all()) and n - 3 >= m.n0 + m.n1 - m.n1 % Q.EMIT     # in the last, ragged emit block
    t = next(c for c in Q.CASES if c.family == "ties" and not c.f16 and c.n0 > 0)
    mt = Q.reference(t)[0]
    assert torch.equal(mt[:, 0], mt[:, t.n1 - 1])


def test_without_leading_keys_the_rows_sum_to_one():
    hit = 0
    for c in Q.CASES:
        if c.n0 == 0:
            maps = Q.reference(c)[0]
            assert torch.allclose(maps.sum(1), torch.ones(c.nq, dtype=torch.float64), rtol=0, atol=1e-13), c.id
            hit += 1
        elif c.nq <= 77:
            assert bool((Q.reference(c)[0].sum(1) < 1).all()), c.id
    assert hit >= 4
    one = next(c for c in Q.CASES if (c.n0, c.n1) == (0, 1))
    assert bool((Q.reference(one)[0] == 1).all())


def test_the_axes_are_all_hit():
    C = Q.CASES
    assert {c.heads for c in C} == set(Q.HEADS) == {1, 2, 3, 24}
    assert {c.nq for c in C} >= set(Q.NQ) == {1, 4, 15, 16, 17, 32, 33, 77, 512}
    assert {c.n0 for c in C} >= set(Q.N0) == {0, 1, 4, 77, 512}
    assert {c.n1 for c in C} >= set(Q.N1) == {1, 15, 63, 64, 65, 200, 1100}
    for fam in Q.FAMILIES:
        assert {c.f16 for c in C if c.family == fam} == {False, True}, fam
    assert set(Q.FAMILIES) == {"unit", "peaky8", "peaky16", "cold_text", "dominant", "ties", "last_tile_max"}
    assert {c.layout for c in C} == {"qkv", "apart0", "apart1", "apart2"} and {c.prescaled for c in C} == {False, True}
    assert {c.outputs for c in C} == set(Q.OUTPUTS) >= {"acc", "acc2", "acc+acc2", "acc+lse", "acc+acc2+lse"}
    strides = set()
    for c in C:
        inp = Q.make_inputs(c)
        strides |= {b.shape[1] - c.heads * 128 for name, b in inp["buffers"].items() if c.layout != "qkv"}
    assert strides == set(Q.PADS) and len(strides) >= 3          # three row strides per width, beside the shared buffer's
    assert any((c.n0 + c.n1) % Q.TILE == 0 for c in C) and any((c.n0 + c.n1) % Q.TILE for c in C)
    assert any(c.n1 % Q.EMIT == 0 for c in C if c.n1 >= Q.EMIT) or any(c.n1 > Q.EMIT and c.n1 % Q.EMIT for c in C)
    assert len({c.id for c in C}) == len(C)


def test_nothing_a_launch_may_not_read_is_finite():
    """The q / k slices hold the values; every other element of every buffer is NaN in both storage types."""
    for c in (Q.CASES[0], Q.CASES[1], Q.CASES[2], next(c for c in Q.CASES if c.n0 == 0 and c.layout != "qkv")):
        inp = Q.make_inputs(c)
        seen = {name: torch.zeros_like(b, dtype=torch.bool) for name, b in inp["buffers"].items()}
        for name in ("q", "k0", "k1"):
            b, r0, n, c0 = inp["views"][name]
            seen[b][r0:r0 + n, c0:c0 + c.heads * 128] = True
        for name, b in inp["buffers"].items():
            for f16 in (False, True):
                vals = Q.from_bits(b, f16)
                assert bool(torch.isnan(vals[~seen[name]]).all()) and (~seen[name]).any()
            assert bool(torch.isfinite(Q.from_bits(b, c.f16)[seen[name]]).all())
    assert math.isclose(Q.SCALE_LOG2, Q.LOG2E / math.sqrt(128), rel_tol=1e-7)
