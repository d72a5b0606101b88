"""ca_token_maps' case table without a GPU (tests/tokmap_cases.py): the fp32 emulation of the kernel's order lies inside
the derived bound of the fp64 reference on every case, every named slip leaves it on at least one, and the axes the
cases must cover are all hit.  No case is skipped or filtered by a comparison."""
import math

import pytest
import torch

import tokmap_cases as T


def _ratios(c, slip=None):
    maps, lse, bound = T.reference(c)
    got_maps, got_lse = T.emulate(c, slip)
    return T.over_the_bound(got_maps, maps, bound.maps), T.over_the_bound(got_lse, lse, bound.lse)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_the_emulation_lies_inside_the_bound(case):
    (worst, n_over), (worst_lse, n_over_lse) = _ratios(case)
    print(f"\n  {case.id}: maps max err / bound = {worst:.3f}, lse {worst_lse:.3f}")
    assert n_over == 0 and n_over_lse == 0, (case.id, worst, n_over, worst_lse, n_over_lse)
    maps, _, bound = T.reference(case)
    inp = T.make_inputs(case)
    acc = T.emulate_acc(inp["acc0"], T.W1, T.emulate(case)[0])
    worst_acc, n_acc = T.over_the_bound(acc, inp["acc0"].double() + T.W1 * maps, T.acc_bound(T.W1, inp["acc0"], maps, bound.maps))
    assert n_acc == 0, (case.id, worst_acc)


@pytest.mark.parametrize("slip", T.SLIPS)
def test_every_slip_leaves_the_bound(slip):
    left = []
    for c in T.CASES:
        if slip == "half_bits_read_as_bf16" and not c.f16:
            continue                                  # (the slip is the identity on bf16 storage)
        (worst, n_over), _ = _ratios(c, slip)
        if n_over:
            left.append((c.id, worst))
    print(f"\n  {slip}: leaves the bound on {len(left)} of {len(T.CASES)} cases")
    assert left, slip


def test_the_reference_is_a_softmax_and_the_bound_is_relative():
    c = next(c for c in T.CASES if c.family == "cold_text" and not c.f16)
    maps, lse, bound = T.reference(c)
    q, k = T.operands(c)
    s = torch.einsum("ihd,jhd->hij", q, k) * c.scale_log2 * T.LN2            # nats
    want = torch.softmax(s, -1)[:, :, :c.n_tok].mean(0).T
    assert torch.allclose(maps, want, rtol=1e-12, atol=0)
    assert torch.allclose(lse, torch.logsumexp(s, -1), rtol=1e-12, atol=1e-12)
    # the cold block: cells of about e^-20 / n, bounded relatively (a kernel that returns zeros there fails)
    assert float(maps.max()) < 1e-8 and float((bound.maps / maps).max()) < 1e-3
    d = next(c for c in T.CASES if c.family == "dominant" and not c.f16)
    assert float(T.reference(d)[0][d.n_tok // 2].min()) > 1 - 1e-6
    t = next(c for c in T.CASES if c.family == "ties" and c.n1 > 0 and not c.f16)
    mt = T.reference(t)[0]
    assert torch.equal(mt[0], mt[t.n_tok - 1]) and float(mt[0].min()) > 0.24
    m = next(c for c in T.CASES if c.family == "last_tile_max" and not c.f16)
    q, k = T.operands(m)
    s = torch.einsum("ihd,jhd->hij", q, k)
    assert bool((s.argmax(-1) == m.n0 + m.n1 - 1).all())


def test_the_axes_are_all_hit():
    C = T.CASES
    assert {c.heads for c in C} == set(T.HEADS) == {1, 2, 3, 24}
    assert {c.nq for c in C} >= set(T.NQ) == {1, 15, 16, 17, 63, 64, 65, 200}
    assert {c.n1 for c in C} >= set(T.N1) == {0, 1, 63, 64, 65, 1100}
    assert {n0 for n0, _ in T.N0_TOK} == {1, 8, 64, 77, 256, 512}
    for n0 in (1, 8, 64, 77, 256, 512):
        toks = {c.n_tok for c in C if c.n0 == n0}
        assert 1 in toks and n0 in toks and (n0 == 1 or any(1 < t < n0 for t in toks)), (n0, toks)
    for fam in T.FAMILIES:
        assert {c.f16 for c in C if c.family == fam} == {False, True}, fam
    assert set(T.FAMILIES) == {"unit", "peaky8", "peaky16", "cold_text", "dominant", "ties", "last_tile_max"}
    assert {c.layout for c in C} == {"qkv", "apart"} and {c.prescaled for c in C} == {False, True}
    assert any((c.n0 + c.n1) % T.TILE == 0 for c in C) and any((c.n0 + c.n1) % T.TILE for c in C)
    assert any(c.nq > 64 and c.n0 == 512 and c.n1 >= 1100 for c in C)
    assert len({c.id for c in C}) == len(C)


def test_nothing_a_launch_may_not_read_is_finite():
    """The q / k slices hold the values; every other element of every buffer is NaN in both storage types."""
    for c in (T.CASES[0], T.CASES[2], next(c for c in T.CASES if c.n1 == 0)):
        inp = T.make_inputs(c)
        seen = {name: torch.zeros_like(b, dtype=torch.bool) for name, b in inp["buffers"].items()}
        for name in ("q", "k0", "k1"):
            b, r0, n, c0 = inp["views"][name]
            seen[b][r0:r0 + n, c0:c0 + c.heads * 128] = True
        for name, b in inp["buffers"].items():
            for f16 in (False, True):
                vals = T.from_bits(b, f16)
                assert bool(torch.isnan(vals[~seen[name]]).all()) and (~seen[name]).any()
            assert bool(torch.isfinite(T.from_bits(b, c.f16)[seen[name]]).all())
        assert math.isclose(T.SCALE_LOG2, T.LOG2E / math.sqrt(128), rel_tol=1e-7)
