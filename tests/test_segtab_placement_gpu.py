"""ca_segtab_score with its operands at chosen device addresses (tests/placement.py): one case with every buffer where bit
31 of its addresses is set, then role by role across the 2^32 line; and one call whose second map lies more than 4 GiB
behind the first (map_stride = 2^30 + 16 elements).  Bit-identical to ordinary allocations, equal to the restatement, guard
elements and guard bands intact every time."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import placement as PL  # noqa: E402
import segtab_cases as T  # noqa: E402
import test_segtab_kernels_gpu as TK  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402

DEV = "cuda"
ROLES = ["maps", "label", "records", "cells"]
PLACEMENT_CASE = "flags-mean-down-blur"


@pytest.fixture(scope="module")
def arena():
    a = PL.Arena(DEV)
    yield a
    a.buf = None
    torch.cuda.empty_cache()


def _data_bytes(case) -> dict:
    hw = case.h * case.w
    return {"maps": case.n_maps * case.C * hw * 4, "label": case.Hl * case.Wl, "records": case.n_maps * 40,
            "cells": 4 * ((hw + 3) & ~3) * 4}


def _assert_placed(pl, role, case):
    """The straddling role has the 2^32 line INSIDE its data, at least 16 bytes of it on either side (so the kernels' own
    loads, stores or atomics cross it, not only the guard tail); every other buffer lies wholly in the bit-31 region."""
    B = pl.arena.B
    data = _data_bytes(case)
    assert set(pl.placed) == set(ROLES), set(pl.placed) ^ set(ROLES)
    for r, (start, n) in pl.placed.items():
        item = {"maps": 4, "cells": 4, "records": 1, "label": 0}[r]       # (the label has no guard elements of its own)
        assert n == data[r] + TK.GUARD * item, (r, n)
        if r == role:
            assert start + 16 <= B <= start + data[r] - 16, (r, hex(start), data[r])
        else:
            assert start + n <= B and start >> 31 & 1, (r, hex(start), n)


def test_every_operand_at_bit_31_and_across_the_4_gib_line(arena):
    case = next(c for c in T.CASES if c.name == PLACEMENT_CASE)
    assert case.C == 4 and case.flags["downscale_for_eval"] and case.flags["apply_blur"]
    plain, ws, _, _ = TK.run_case(case)                        # ordinary allocations: checked against the restatement
    for role in [None] + ROLES:
        pl = arena.placer(role)
        got, ws2, _, _ = TK.run_case(case, pl)                 # (the restatement and the guard elements again)
        _assert_placed(pl, role, case)
        pl.check_guards()
        assert plain.tobytes() == got.tobytes() and np.array_equal(ws, ws2), f"{role or 'bit31'} != plain"


def test_a_second_map_more_than_4_gib_behind_the_first(arena):
    h, w, Hl, Wl = 16, 16, 64, 64
    stride = (1 << 30) + 16                                    # elements: 4 GiB + 64 bytes
    maps = T.table_maps(h, w, 2, seed=60, kinds=("heat", "signed"))
    label = T.seeded_label(h, w, Hl, Wl, 60)
    span = (stride + h * w) * 4
    assert span > PL.LINE and span + 2 * PL.GUARD <= arena.nbytes
    start = (arena.base + PL.GUARD + 255) // 256 * 256
    tab = arena.window(start, span).view(torch.float32)
    for m in range(2):                                         # NaN on both sides of either map
        lo, hi = max(m * stride - 1024, 0), min(m * stride + h * w + 1024, tab.numel())
        tab[lo:hi] = float("nan")
        tab[m * stride:m * stride + h * w] = torch.from_numpy(maps[m].reshape(-1)).to(DEV)
    ld = torch.from_numpy(label).to(DEV)
    res = torch.full((2 * 40 + TK.GUARD,), TK.REC_GUARD, dtype=torch.uint8, device=DEV)
    cells = torch.full((4 * h * w + TK.GUARD,), TK.CELL_GUARD, dtype=torch.int32, device=DEV)
    lib = L.load()
    L.check(lib.ca_segtab_score(ctypes.cast(tab.data_ptr(), ctypes.POINTER(ctypes.c_float)), stride, 2, ld.data_ptr(),
                                res.data_ptr(), cells.data_ptr(), h, w, Hl, Wl, L.SEGTAB_MEAN_THRESHOLD, None,
                                torch.cuda.current_stream().cuda_stream), "ca_segtab_score")
    torch.cuda.synchronize()
    out = res.cpu().numpy()
    assert (out[80:] == TK.REC_GUARD).all() and bool((cells[4 * h * w:] == TK.CELL_GUARD).all())
    rec = out[:80].copy().view(TK.RECORD)
    for m in range(2):
        TK.check(rec[m], T.reference(maps[m], label), ("stride 2^30 + 16", m))
        assert torch.equal(tab[m * stride:m * stride + h * w].cpu(), torch.from_numpy(maps[m].reshape(-1)))
