"""ca_mseg_score with its operands at chosen device addresses (tests/placement.py): one case with every buffer where bit 31
of its addresses is set, then role by role across the 2^32 line.  Bit-identical to ordinary allocations, equal to the
restatement, guard elements and guard bands intact every time."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mseg_cases as T  # noqa: E402
import placement as PL  # noqa: E402
import test_mseg_kernels_gpu as TK  # noqa: E402

DEV = "cuda"
ROLES = ["maps", "label", "counts", "class_out", "index_out"]


@pytest.fixture(scope="module")
def arena():
    a = PL.Arena(DEV)
    yield a
    a.buf = None
    torch.cuda.empty_cache()


def _assert_placed(pl, role, case):
    """The straddling role has the 2^32 line INSIDE its data, at least 16 bytes of it on either side (so the kernel's
    own loads or stores cross it, not only the guard tail); every other buffer lies wholly in the bit-31 region."""
    B = pl.arena.B
    data = T.placement_data_bytes(case)
    assert set(pl.placed) == set(ROLES), set(pl.placed) ^ set(ROLES)
    for r, (start, n) in pl.placed.items():
        item = 4 if r in ("maps", "counts") else 1
        assert n == data[r] + TK.GUARD * item, (r, n)
        if r == role:
            assert start + 16 <= B <= start + data[r] - 16, (r, hex(start), data[r])
        else:
            assert start + n <= B and start >> 31 & 1, (r, hex(start), n)


def test_every_operand_at_bit_31_and_across_the_4_gib_line(arena):
    case = next(c for c in T.CASES if c.name == T.PLACEMENT_CASE)
    assert case.outputs == "both" and case.items == 1
    plain = TK.run_case(case)                                  # ordinary allocations: checked against the restatement
    for role in [None] + ROLES:
        pl = arena.placer(role)
        got = TK.run_case(case, pl)                            # (the restatement and the guard elements again)
        _assert_placed(pl, role, case)
        pl.check_guards()
        for a, b in zip(plain, got):
            assert np.array_equal(a, b), f"{role or 'bit31'} != plain"
