"""ca_query_maps' address arithmetic at the 2 GiB and 4 GiB boundaries (tests/placement.py): a multi-problem launch with
all operands at bit 31, one operand role at a time across a 2^32 line, q and key rows at a row stride that puts the last
row more than 4 GiB from the first, and an accumulator whose last row lies 4 GiB behind its first.  Every run must give
the bits of ordinary allocations."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import address_range_cases as C  # noqa: E402
import placement as PL  # noqa: E402
import querymap_cases as Q  # noqa: E402
import tokmap_cases as T  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from test_querymap_kernels_gpu import DEV, NAN, _bytes, assert_same_bits, run, single  # noqa: E402

POOL = [c for c in Q.CASES if (c.heads, c.f16, c.prescaled) == (2, False, False) and c.nq <= 77]
# one case per kind of layout in which every role exists (leading keys, several row blocks and emit blocks)
ROLE_CASES = [next(c for c in Q.CASES if c.layout.startswith(lay) and c.n0 >= 64 and c.nq > 16 and c.n1 > 128
                   and c.outputs == Q.OUTPUTS[0] and c.nq <= 77) for lay in ("qkv", "apart")]


@pytest.fixture(scope="module")
def arena():
    a = PL.Arena(DEV)
    yield a
    a.buf = None
    torch.cuda.empty_cache()


def test_all_operands_at_bit_31(arena):
    cases = POOL[:5]
    pl = arena.placer()
    ws = pl.full((sum((2 * c.nq * 8 + 15) // 16 * 16 for c in cases),), 0, torch.uint8, {"workspace": None})
    got = run(cases, pl, workspace=ws)
    assert pl.placed
    for start, n in pl.placed.values():
        assert start >> 31 & 1 and (start + n - 1) >> 31 & 1, hex(start)
    for c, g in zip(cases, got):
        assert_same_bits(g, single(c), f"bit-31 placement of {c.id}")


@pytest.mark.parametrize("case", ROLE_CASES, ids=lambda c: c.id)
def test_role_by_role_across_a_4_gib_line(arena, case):
    names = list(Q.make_inputs(case)["buffers"]) + ["acc", "acc2", "lse"]
    for name in names + ["workspace"]:
        role = name if name == "workspace" else name + "[0]"
        pl = arena.placer(role)
        ws = pl.full(((case.heads * case.nq * 8 + 15) // 16 * 16,), 0, torch.uint8, {"workspace": None})
        got = run([case], pl, workspace=ws)[0]
        start, n = pl.placed[role]
        assert start < arena.B < start + n, (role, hex(start), n)
        for r, (s, m) in pl.placed.items():
            assert r == role or (s + m <= arena.B and s >> 31 & 1), (r, hex(s))
        assert_same_bits(got, single(case), f"{role} across the line")


def _far_window(arena, n, ld, width, itemsize):
    """A [n, width] strided view at row stride ld inside the arena, guard bands on both sides."""
    start = (arena.base + PL.GUARD + 255) // 256 * 256
    span = (((n - 1) * ld + width) * itemsize + 255) // 256 * 256
    for g in (start - PL.GUARD, start + span):
        arena.window(g, PL.GUARD).fill_(PL.PATTERN)
    return start, span


@pytest.mark.parametrize("role", ["q", "k"])
def test_rows_more_than_4_gib_apart(arena, role):
    """The operand's rows at the largest stride that keeps its extent inside 5 GiB: its last row starts more than 4 GiB
    behind its first (row index times stride in 64 bits).  Only the rows themselves are written."""
    case = next(c for c in POOL if c.layout.startswith("apart") and c.n0 > 0 and c.nq > 1)
    inp = Q.make_inputs(case)
    W = case.heads * 128
    n = case.nq if role == "q" else case.n0 + case.n1
    ld = C.far_ld(n, 2, C.PAST_4GIB)
    ops._i32(ld, "ld")
    assert (n - 1) * ld * 2 > 1 << 32
    start, span = _far_window(arena, n, ld, W, 2)
    rows = arena.window(start, span).view(torch.int16).as_strided((n, W), (ld, 1))
    dev = {k: Q.view(case, inp["buffers"], k).to(DEV) for k in ("q", "k0", "k1")}
    if role == "q":
        rows.copy_(dev["q"])
        dev["q"] = rows
    else:                                                        # the leading rows, then the emitted rows: one stride
        rows.copy_(torch.cat([dev["k0"], dev["k1"]]))
        dev["k0"], dev["k1"] = rows[:case.n0], rows[case.n0:]
    rows0 = rows.clone()
    acc, acc2 = inp["acc0"].to(DEV), inp["acc20"].to(DEV)
    lse = torch.full((case.heads, case.nq), NAN, device=DEV)
    ops.query_maps([ops.QueryMaps(dev["q"].view(torch.bfloat16), dev["k0"].view(torch.bfloat16), dev["k1"].view(torch.bfloat16),
                                  acc=acc, weight=Q.W1, acc2=acc2, weight2=Q.W2, lse=lse)], case.heads, case.scale_log2)
    torch.cuda.synchronize()
    assert torch.equal(_bytes(rows), _bytes(rows0)), "the far rows changed"
    for g in (start - PL.GUARD, start + span):
        assert bool((arena.window(g, PL.GUARD) == PL.PATTERN).all()), "guard band written"
    assert_same_bits(dict(acc=acc, acc2=acc2, lse=lse), single(case), "far " + role + " rows")


def test_an_accumulator_whose_last_row_lies_4_gib_behind_its_first(arena):
    """acc is contiguous [nq, n1], so a far last row needs many emitted keys: nq = 512 rows of n1 = 514 * 4096 floats put
    row 511 more than 4 GiB behind row 0 (row index times n1 in 64 bits); one head keeps the key rows at 0.5 GiB.  The keys
    are 4096 rows repeated 514 times, so the map repeats bit for bit with that period and is the 4096-key map divided by
    514; q row 511 is q row 0, so the far row holds the near row's bits."""
    heads, nq, P, R = 1, 512, 4096, 514
    W, n1 = 128, P * R
    assert (nq - 1) * n1 * 4 > 1 << 32
    g = T._gen("querymap.far_acc")
    qv, kv = torch.randn(nq, W, generator=g), torch.randn(P, W, generator=g)
    qv[nq - 1] = qv[0]
    qb, kb = Q.to_bits(qv, False), Q.to_bits(kv, False)
    a_start, a_span = _far_window(arena, nq, n1, n1, 4)
    assert a_span > 1 << 32
    acc2 = arena.window(a_start, nq * n1 * 4).view(torch.float32).view(nq, n1)
    acc2.zero_()
    k_start = a_start + a_span + 2 * PL.GUARD
    k1 = arena.window(k_start, n1 * W * 2).view(torch.int16).view(R, P, W)
    arena.window(k_start + n1 * W * 2, PL.GUARD).fill_(PL.PATTERN)
    k1.copy_(kb.to(DEV).expand(R, P, W))
    ops.query_maps([ops.QueryMaps(qb.to(DEV).view(torch.bfloat16), None, k1.view(n1, W).view(torch.bfloat16), acc2=acc2,
                                  weight2=1.0)], heads, Q.SCALE_LOG2)
    torch.cuda.synchronize()
    for gd in (a_start - PL.GUARD, a_start + a_span, k_start + n1 * W * 2):
        assert bool((arena.window(gd, PL.GUARD) == PL.PATTERN).all()), "guard band written"
    per = acc2.view(nq, R, P)
    assert bool((per == per[:, :1]).all()), "the map does not repeat with the keys' period"
    assert torch.equal(_bytes(acc2[nq - 1]), _bytes(acc2[0])) and not torch.equal(acc2[1, :P], acc2[0, :P])
    # the 4096-key reference divided by 514; its bound with n = 514 * 4096 keys in the two terms that count keys and tiles
    maps, _, bound = Q.reference_qk(Q.from_bits(qb, False).reshape(nq, 1, W), Q.from_bits(kb, False).reshape(P, 1, W), 0,
                                    Q.SCALE_LOG2)
    extra = ((n1 - P) * Q.U + (n1 - P) // Q.TILE * (Q.EXP_REL + 2 * Q.U)) * Q.SECOND_ORDER
    worst, n_over = Q.over_the_bound(per[:, 0], maps / R, bound.maps / R + maps / R * extra)
    print(f"\n  far accumulator: max err / bound {worst:.3f}")
    assert n_over == 0, worst
