"""ca_heatmap_render with its operands at chosen device addresses (tests/placement.py): every buffer where bit 31 of its
addresses is set, then role by role across the 2^32 line, once with the ranges found by the kernel and once with given ones;
and two calls whose second plane lies more than 4 GiB behind the first, for the maps and for the output.  Bit-identical to
ordinary allocations, equal to the restatement, guard elements and guard bands intact every time."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import placement as PL  # noqa: E402
import render_cases as R  # noqa: E402
import test_render_kernels_gpu as TK  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402

DEV = "cuda"
CASES = {
    "own-range": R.Case("placement-own-range", 16, 12, 37, 53, bilinear=True, n_maps=3, groups=4, C=2, family="signed",
                        alpha=0.3, out_pad=5, seed=71),
    "given-range": R.Case("placement-given-range", 16, 12, 37, 53, n_maps=3, groups=4, C=2, family="signed", given="narrow",
                          alpha=0.5, out_pad=5, seed=72),
}
ROLES = {"own-range": ["maps", "lut", "out", "range_out", "image"],
         "given-range": ["maps", "lut", "out", "range_out", "range_in", "image"]}


@pytest.fixture(scope="module")
def arena():
    a = PL.Arena(DEV)
    yield a
    a.buf = None
    torch.cuda.empty_cache()


def _data_bytes(case) -> dict:
    G, n = case.groups, case.n_maps
    return {"maps": (G * n * case.C * case.h * case.w, 4), "lut": (R.LUT_ROWS * 3, 1),
            "out": (G * n * (3 * case.H * case.W + case.out_pad), 1), "range_out": (2 * G, 4), "range_in": (2 * G, 4),
            "image": (G * case.H * (3 * case.W + TK.IMG_PAD), 1)}


def _assert_placed(pl, role, case, roles):
    """The straddling role has the 2^32 line INSIDE its data, at least 16 bytes of it on either side (so the kernels' own
    loads, stores or atomics cross it, not only the guard tail); every other buffer lies wholly in the bit-31 region."""
    B = pl.arena.B
    data = _data_bytes(case)
    assert set(pl.placed) == set(roles), set(pl.placed) ^ set(roles)
    for r, (start, n) in pl.placed.items():
        elems, item = data[r]
        assert n == (elems + TK.GUARD) * item, (r, n)
        if r == role:
            assert start + 16 <= B <= start + elems * item - 16, (r, hex(start), elems * item)
        else:
            assert start + n <= B and start >> 31 & 1, (r, hex(start), n)


@pytest.mark.parametrize("which", list(CASES))
def test_every_operand_at_bit_31_and_across_the_4_gib_line(arena, which):
    case, roles = CASES[which], ROLES[which]
    plain, ranges = TK.run_case(case)                          # ordinary allocations: checked against the restatement
    for role in [None] + roles:
        pl = arena.placer(role)
        got, r2 = TK.run_case(case, pl)                        # (the restatement and the guard elements again)
        _assert_placed(pl, role, case, roles)
        pl.check_guards()
        assert plain.tobytes() == got.tobytes() and ranges.tobytes() == r2.tobytes(), f"{role or 'bit31'} != plain"


def _far_call(maps_ptr, map_stride, out_ptr, out_stride, lut, rng, h, w, H, W, flags):
    arr = (L.RenderProblem * 1)()
    p = arr[0]
    p.maps, p.map_stride, p.n_maps = maps_ptr, map_stride, 2
    p.range_out, p.out, p.out_stride = rng.data_ptr(), out_ptr, out_stride
    L.check(L.load().ca_heatmap_render(arr, 1, h, w, H, W, lut.data_ptr(), 0.0, flags,
                                       torch.cuda.current_stream().cuda_stream), "ca_heatmap_render")
    torch.cuda.synchronize()


def test_a_second_plane_more_than_4_gib_behind_the_first(arena):
    h, w, H, W = 16, 16, 37, 53
    planes = R.planes_of("signed", 2, h, w, seed=80)
    lut = torch.from_numpy(TK.LUT).to(DEV)
    start = (arena.base + PL.GUARD + 255) // 256 * 256
    for bilinear in (False, True):
        ref, (lo, hi) = R.render(planes, TK.LUT, H, W, bilinear)
        flags = L.RENDER_BILINEAR if bilinear else 0
        # the maps: map_stride = 2^30 + 16 elements (4 GiB + 64 bytes), NaN on both sides of either plane
        stride = (1 << 30) + 16
        span = (stride + h * w) * 4
        assert span > PL.LINE and span + 2 * PL.GUARD <= arena.nbytes
        tab = arena.window(start, span).view(torch.float32)
        for m in range(2):
            a, b = max(m * stride - 1024, 0), min(m * stride + h * w + 1024, tab.numel())
            tab[a:b] = float("nan")
            tab[m * stride:m * stride + h * w] = torch.from_numpy(planes[m].reshape(-1)).to(DEV)
        out = torch.full((2 * 3 * H * W + TK.GUARD,), TK.BYTE_GUARD, dtype=torch.uint8, device=DEV)
        rng = torch.full((2 + TK.GUARD,), TK.RANGE_GUARD, dtype=torch.float32, device=DEV)
        _far_call(tab.data_ptr(), stride, out.data_ptr(), 3 * H * W, lut, rng, h, w, H, W, flags)
        o, r = out.cpu().numpy(), rng.cpu().numpy()
        assert (o[2 * 3 * H * W:] == TK.BYTE_GUARD).all() and (r[2:] == np.float32(TK.RANGE_GUARD)).all()
        assert np.array_equal(o[:2 * 3 * H * W].reshape(2, H, W, 3), ref) and r[0] == lo and r[1] == hi
        # the output: out_stride = 2^32 + 69 bytes (the second plane starts at an odd byte), 0x3C around either plane
        step = PL.LINE + 69
        span = step + 3 * H * W
        assert span + 2 * PL.GUARD <= arena.nbytes
        dst = arena.window(start, span)
        for m in range(2):
            a, b = max(m * step - 4096, 0), min(m * step + 3 * H * W + 4096, span)
            dst[a:b] = 0x3C
        md = torch.from_numpy(planes).to(DEV)
        rng.fill_(TK.RANGE_GUARD)
        _far_call(md.data_ptr(), h * w, dst.data_ptr(), step, lut, rng, h, w, H, W, flags)
        for m in range(2):
            a, b = max(m * step - 4096, 0), min(m * step + 3 * H * W + 4096, span)
            around = dst[a:b].cpu().numpy()
            at = m * step - a
            assert np.array_equal(around[at:at + 3 * H * W].reshape(H, W, 3), ref[m]), (bilinear, m)
            assert (around[:at] == 0x3C).all() and (around[at + 3 * H * W:] == 0x3C).all(), (bilinear, m)
        r = rng.cpu().numpy()
        assert r[0] == lo and r[1] == hi and (r[2:] == np.float32(TK.RANGE_GUARD)).all()
