"""ca_head_maps' address arithmetic at the 2 GiB and 4 GiB boundaries (tests/placement.py): a 16-problem launch with all
operands at bit 31, one operand role at a time across a 2^32 line, a `heads` tensor whose last plane lies more than 4 GiB
behind its first, and a row stride beyond int32_t.  Every run must give the bits of ordinary allocations."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import headmap_cases as H  # noqa: E402
import placement as PL  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from test_headmap_kernels_gpu import DEV, Guarded, assert_same_bits, inputs_and_reference, run  # noqa: E402


@pytest.fixture(scope="module")
def arena():
    a = PL.Arena(DEV)
    yield a
    a.buf = None
    torch.cuda.empty_cache()


def test_all_operands_at_bit_31(arena):
    case = H.BY_ID["heads_NH4_L257_C16_sparsemax_n16_all"]
    inp, _ = inputs_and_reference(case)
    plain = run(case, inp, Guarded())
    pl = arena.placer()
    got = run(case, inp, pl)
    assert len(pl.placed) == 16 * 5
    for start, n in pl.placed.values():
        assert start >> 31 & 1 and (start + n - 1) >> 31 & 1, hex(start)
    assert_same_bits(got, plain, "bit-31 placement")


@pytest.mark.parametrize("cid", ["heads_NH3_L257_C9_softmax_n1_all", "heads_NH24_L257_C32_softmax_n1_all"])
def test_role_by_role_across_a_4_gib_line(arena, cid):
    case = H.BY_ID[cid]
    inp, _ = inputs_and_reference(case)
    plain = run(case, inp, Guarded())
    for name in ("img", "con", "heads", "acc", "acc2"):
        role = name + "[0]"
        pl = arena.placer(role)
        got = run(case, inp, pl)
        start, n = pl.placed[role]
        assert start < arena.B < start + n, (role, hex(start), n)
        for r, (s, m) in pl.placed.items():
            assert r == role or (s + m <= arena.B and s >> 31 & 1), (r, hex(s))
        assert_same_bits(got, plain, f"{role} across the line")


def test_a_heads_tensor_whose_last_plane_lies_more_than_4_gib_behind_its_first():
    """[NH, C, L] fp32 with (NH - 1) C L 4 bytes > 2^32: the plane offset (h C + c) L + p in 64 bits.  The smallest such
    launch reads NH L 256 bytes of bf16 image rows, twice the tensor itself; norm = none keeps it short.  Sixteen patches
    at the start, in the middle and at the end are compared, all heads and concepts, with a 16-patch launch over copies of
    their rows (a patch's bits do not depend on its position), and the element behind the tensor stays as it was."""
    NH, C = 32, 32
    Lp = (1 << 32) // ((NH - 1) * C * 4) + 64
    assert (NH - 1) * C * Lp * 4 > 1 << 32
    W = NH * 128
    g = torch.Generator().manual_seed(77)
    block = torch.randn(4096, W, generator=g).bfloat16().to(DEV)
    img = block.repeat(Lp // 4096 + 1, 1)[:Lp]
    for lo in (0, Lp // 2, Lp - 16):                            # rows of their own at the places that are compared
        img[lo:lo + 16] = torch.randn(16, W, generator=g).bfloat16().to(DEV)
    con = (torch.randn(C, W, generator=g) * 0.1).bfloat16().to(DEV)
    whole = torch.zeros(NH * C * Lp + 64, device=DEV)
    whole[-64:] = float("nan")
    heads = whole[:NH * C * Lp].view(NH, C, Lp)
    acc = torch.zeros(C, Lp, device=DEV)
    ops.head_maps([ops.HeadMaps(img, con, heads=heads, weight_h=1.0, acc=acc, weight=1.0)], NH, L.NORM_NONE)
    torch.cuda.synchronize()
    assert bool(torch.isnan(whole[-64:]).all()), "behind the tensor written"
    for lo in (0, Lp // 2, Lp - 16):
        few = dict(heads=torch.zeros(NH, C, 16, device=DEV), acc=torch.zeros(C, 16, device=DEV))
        ops.head_maps([ops.HeadMaps(img[lo:lo + 16], con, heads=few["heads"], weight_h=1.0, acc=few["acc"], weight=1.0)],
                      NH, L.NORM_NONE)
        assert torch.equal(heads[:, :, lo:lo + 16], few["heads"]), lo
        assert torch.equal(acc[:, lo:lo + 16], few["acc"]), lo
        assert bool((few["heads"][-1] != 0).any())
    del whole, heads, img
    torch.cuda.empty_cache()


def test_a_row_stride_beyond_int32_is_a_value_error():
    far = torch.zeros(256, dtype=torch.bfloat16, device=DEV).as_strided((1, 256), (2 ** 31, 1))
    con = torch.zeros(4, 256, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="ldi = 2147483648 does not fit the library's int32_t"):
        ops.head_maps([ops.HeadMaps(far, con, acc=torch.zeros(4, 1, device=DEV))], 2)
    with pytest.raises(ValueError, match="ldc = 2147483648 does not fit the library's int32_t"):
        ops.head_maps([ops.HeadMaps(con, far, acc=torch.zeros(1, 4, device=DEV))], 2)
