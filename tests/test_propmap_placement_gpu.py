"""ca_propagate_maps' address arithmetic at the 2 GiB and 4 GiB boundaries (tests/placement.py): a multi-problem launch
with all operands at bit 31, one operand role at a time across a 2^32 line (v and the workspace included), q and key rows
at a row stride that puts the last row more than 4 GiB from the first, a v row and an accumulator row more than 4 GiB
behind the first.  Every run must give the bits of ordinary allocations."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import address_range_cases as C  # noqa: E402
import placement as PL  # noqa: E402
import propmap_cases as P  # noqa: E402
import tokmap_cases as T  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from test_propmap_kernels_gpu import DEV, _bytes, assert_same_bits, run, single  # noqa: E402

POOL = [c for c in P.CASES if (c.heads, c.f16, c.prescaled) == (3, False, False) and c.nq <= 200]
# every role exists (leading keys), several row blocks, several key tiles
ROLE_CASES = [next(c for c in P.CASES if c.n0 >= 64 and c.nq > 64 and c.n1 > 64 and c.nq <= 200 and c.heads <= 5 and c.f16 == f16)
              for f16 in (False, True)]


def _ws_bytes(c):
    return (c.heads * c.C * c.nq * 4 + 15) // 16 * 16


@pytest.fixture(scope="module")
def arena():
    a = PL.Arena(DEV)
    yield a
    a.buf = None
    torch.cuda.empty_cache()


def test_all_operands_at_bit_31(arena):
    cases = POOL[:5]
    assert len(cases) >= 3
    pl = arena.placer()
    ws = pl.full((sum(_ws_bytes(c) for c in cases),), 0, torch.uint8, {"workspace": None})
    got = run(cases, pl, workspace=ws)
    assert pl.placed
    for start, n in pl.placed.values():
        assert start >> 31 & 1 and (start + n - 1) >> 31 & 1, hex(start)
    for c, g in zip(cases, got):
        assert_same_bits(g, single(c), f"bit-31 placement of {c.id}")


@pytest.mark.parametrize("case", ROLE_CASES, ids=lambda c: c.id)
def test_role_by_role_across_a_4_gib_line(arena, case):
    names = list(P.make_inputs(case)["buffers"]) + ["acc", "acc2"]
    assert set(names) == {"q", "k0", "k1", "v", "acc", "acc2"}
    for name in names + ["workspace"]:
        role = name if name == "workspace" else name + "[0]"
        pl = arena.placer(role)
        ws = pl.full((_ws_bytes(case),), 0, torch.uint8, {"workspace": None})
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


@pytest.mark.parametrize("role", ["q", "k", "v"])
def test_rows_more_than_4_gib_apart(arena, role):
    """The operand's rows at the largest stride that keeps its extent inside 5 GiB: its last row starts more than 4 GiB
    behind its first (row index times stride in 64 bits).  Only the rows themselves are written."""
    case = next(c for c in POOL if c.n0 > 0 and c.nq >= 6 and c.C >= 6)     # (six rows reach from 0 to past 4 GiB)
    inp = P.make_inputs(case)
    W = case.heads * 128
    n, width, item = {"q": (case.nq, W, 2), "k": (case.n0 + case.n1, W, 2), "v": (case.C, case.n1, 4)}[role]
    ld = C.far_ld(n, item, C.PAST_4GIB)
    ops._i32(ld, "ld")
    assert (n - 1) * ld * item > 1 << 32
    start, span = _far_window(arena, n, ld, width, item)
    rows = arena.window(start, span).view(torch.float32 if role == "v" else torch.int16).as_strided((n, width), (ld, 1))
    dev = {k: P.view(case, inp["buffers"], k).to(DEV) for k in ("q", "k0", "k1", "v")}
    if role == "k":                                              # the leading rows, then the valued rows: one stride
        rows.copy_(torch.cat([dev["k0"], dev["k1"]]))
        dev["k0"], dev["k1"] = rows[:case.n0], rows[case.n0:]
    else:
        rows.copy_(dev[role])
        dev[role] = rows
    rows0 = rows.clone()
    acc, acc2 = inp["acc0"].to(DEV), inp["acc20"].to(DEV)
    bf = torch.bfloat16
    ops.propagate_maps([ops.PropagateMaps(dev["q"].view(bf), dev["k0"].view(bf), dev["k1"].view(bf), dev["v"], acc=acc,
                                          weight=P.W1, acc2=acc2, weight2=P.W2)], case.heads, case.scale_log2, qk_f16=case.f16)
    torch.cuda.synchronize()
    assert torch.equal(_bytes(rows), _bytes(rows0)), "the far rows changed"
    for g in (start - PL.GUARD, start + span):
        assert bool((arena.window(g, PL.GUARD) == PL.PATTERN).all()), "guard band written"
    assert_same_bits(dict(acc=acc, acc2=acc2), single(case), "far " + role + " rows")


def test_an_accumulator_row_more_than_4_gib_behind_the_first(arena):
    """acc is contiguous [C, nq], so a far last row needs many query rows: C = 32 rows of nq = 541201 * 64 floats put row 31
    more than 4 GiB behind row 0 (row index times nq in 64 bits), and the workspace's last head plane as far behind its
    first.  The q rows are 64 rows repeated, so the output repeats bit for bit with that period and equals the 64-row
    launch's: one head, 40 keys keep the pass short."""
    heads, R, nq, n1, Cc = 1, 64, 541201 * 64, 40, 32
    W = 128
    assert (Cc - 1) * nq * 4 > 1 << 32
    g = T._gen("propmap.far_acc")
    qb = P.to_bits(torch.randn(R, W, generator=g), False).to(DEV)
    kb = P.to_bits(torch.randn(n1, W, generator=g), False).to(DEV).view(torch.bfloat16)
    v = torch.randn(Cc, n1, generator=g).to(DEV)
    near = torch.zeros(Cc, R, device=DEV)
    ops.propagate_maps([ops.PropagateMaps(qb.view(torch.bfloat16), None, kb, v, acc2=near, weight2=1.0)], heads, P.SCALE_LOG2)
    a_start, a_span = _far_window(arena, Cc, nq, nq, 4)
    assert a_span > 1 << 32
    acc2 = arena.window(a_start, Cc * nq * 4).view(torch.float32).view(Cc, nq)
    acc2.zero_()
    q = qb.repeat(nq // R, 1).view(torch.bfloat16)
    ws = torch.empty(heads * Cc * nq * 4, dtype=torch.uint8, device=DEV)
    ops.propagate_maps([ops.PropagateMaps(q, None, kb, v, acc2=acc2, weight2=1.0)], heads, P.SCALE_LOG2, workspace=ws)
    torch.cuda.synchronize()
    for gd in (a_start - PL.GUARD, a_start + a_span):
        assert bool((arena.window(gd, PL.GUARD) == PL.PATTERN).all()), "guard band written"
    per = acc2.view(Cc, nq // R, R)
    assert bool((per == near[:, None, :]).all()), "the far accumulator differs from the 64-row launch"
    assert bool(torch.isfinite(near).all()) and not torch.equal(near[0], near[Cc - 1])
