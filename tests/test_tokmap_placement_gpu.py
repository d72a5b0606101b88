"""ca_token_maps' address arithmetic at the 2 GiB and 4 GiB boundaries (tests/placement.py): a multi-problem launch with
all operands at bit 31, one operand role at a time across a 2^32 line, and q and key rows at a row stride that puts the
last row more than 4 GiB from the first.  Every run must give the bits of ordinary allocations."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import address_range_cases as C  # noqa: E402
import placement as PL  # noqa: E402
import tokmap_cases as T  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from test_tokmap_kernels_gpu import DEV, NAN, _bytes, assert_same_bits, run, single  # noqa: E402

POOL = [c for c in T.CASES if (c.heads, c.f16, c.prescaled) == (2, False, False)]
# one case per layout in which every role exists (image keys, several workgroups)
ROLE_CASES = [next(c for c in T.CASES if c.layout == lay and c.n1 > 0 and c.nq > 64 and c.n0 >= 64) for lay in ("qkv", "apart")]


@pytest.fixture(scope="module")
def arena():
    a = PL.Arena(DEV)
    yield a
    a.buf = None
    torch.cuda.empty_cache()


def test_all_operands_at_bit_31(arena):
    cases = POOL[:5]
    pl = arena.placer()
    got = run(cases, pl)
    assert pl.placed
    for start, n in pl.placed.values():
        assert start >> 31 & 1 and (start + n - 1) >> 31 & 1, hex(start)
    for c, g in zip(cases, got):
        assert_same_bits(g, single(c), f"bit-31 placement of {c.id}")


@pytest.mark.parametrize("case", ROLE_CASES, ids=lambda c: c.id)
def test_role_by_role_across_a_4_gib_line(arena, case):
    names = list(T.make_inputs(case)["buffers"]) + ["acc", "acc2", "lse"]
    for name in names:
        role = name + "[0]"
        pl = arena.placer(role)
        got = run([case], pl)[0]
        start, n = pl.placed[role]
        assert start < arena.B < start + n, (role, hex(start), n)
        for r, (s, m) in pl.placed.items():
            assert r == role or (s + m <= arena.B and s >> 31 & 1), (r, hex(s))
        assert_same_bits(got, single(case), f"{role} across the line")


@pytest.mark.parametrize("role", ["q", "k"])
def test_rows_more_than_4_gib_apart(arena, role):
    """The operand's rows at the largest stride that keeps its extent inside 5 GiB: its last row starts more than 4 GiB
    behind its first (row index times stride in 64 bits).  Only the rows themselves are written."""
    case = next(c for c in POOL if c.layout == "apart" and c.n1 > 0 and c.nq > 1)
    inp = T.make_inputs(case)
    W = case.heads * 128
    n = case.nq if role == "q" else case.n0 + case.n1
    ld = C.far_ld(n, 2, C.PAST_4GIB)
    ops._i32(ld, "ld")
    assert (n - 1) * ld * 2 > 1 << 32
    start = (arena.base + PL.GUARD + 255) // 256 * 256
    span = (((n - 1) * ld + W) * 2 + 255) // 256 * 256
    for g in (start - PL.GUARD, start + span):
        arena.window(g, PL.GUARD).fill_(PL.PATTERN)
    rows = arena.window(start, span).view(torch.int16).as_strided((n, W), (ld, 1))
    dev = {k: T.view(case, inp["buffers"], k).to(DEV) for k in ("q", "k0", "k1")}
    if role == "q":
        rows.copy_(dev["q"])
        dev["q"] = rows
    else:                                                        # the text rows, then the image rows: one stride
        rows.copy_(torch.cat([dev["k0"], dev["k1"]]))
        dev["k0"], dev["k1"] = rows[:case.n0], rows[case.n0:]
    rows0 = rows.clone()
    acc, acc2 = inp["acc0"].to(DEV), inp["acc20"].to(DEV)
    lse = torch.full((case.heads, case.nq), NAN, device=DEV)
    ops.token_maps([ops.TokenMaps(dev["q"].view(torch.bfloat16), dev["k0"].view(torch.bfloat16), dev["k1"].view(torch.bfloat16),
                                  case.n_tok, acc=acc, weight=T.W1, acc2=acc2, weight2=T.W2, lse=lse)], case.heads,
                   case.scale_log2)
    torch.cuda.synchronize()
    assert torch.equal(_bytes(rows), _bytes(rows0)), "the far rows changed"
    for g in (start - PL.GUARD, start + span):
        assert bool((arena.window(g, PL.GUARD) == PL.PATTERN).all()), "guard band written"
    assert_same_bits(dict(acc=acc, acc2=acc2, lse=lse), single(case), f"far {role} rows")
