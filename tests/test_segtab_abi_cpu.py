"""CPU-only checks of ca_segtab_score's boundary: the entry is declared, bound and exported, its constants are the
binding's, and every limit is enforced with the entry's name and the limit's number in the error text, before any launch."""
import ctypes
import os
import re

import pytest

import __graft_entry__ as entry
from conceptattention_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return L.load()


def _header() -> str:
    return open(os.path.join(ROOT, "include", "conceptattn.h")).read()


def test_entry_is_declared_bound_and_exported(lib):
    assert re.search(r"\bint ca_segtab_score\s*\(", _header())
    assert "ca_segtab_score" in L.SIGNATURES and hasattr(lib, "ca_segtab_score")
    assert lib.ca_version() == L.CA_VERSION >= 134
    res, args = L.SIGNATURES["ca_segtab_score"]
    assert res is ctypes.c_int and len(args) == 13
    assert args[1] is ctypes.c_int64 and args[2] is ctypes.c_int32       # map_stride, n_maps
    assert args[6:11] == [ctypes.c_int32] * 5                            # h, w, Hl, Wl, flags


def test_constants_and_the_build():
    consts = dict((k, int(v)) for k, v in re.findall(r"#define CA_SEGTAB_(\w+) (\d+)", _header()))
    assert consts == {"MAX_MAPS": L.SEGTAB_MAX_MAPS, "MEAN_THRESHOLD": L.SEGTAB_MEAN_THRESHOLD,
                      "DOWNSCALE": L.SEGTAB_DOWNSCALE, "BLUR": L.SEGTAB_BLUR, "RAW": L.SEGTAB_RAW}
    assert (L.SEGTAB_MEAN_THRESHOLD, L.SEGTAB_DOWNSCALE, L.SEGTAB_BLUR) == (L.SEG_MEAN_THRESHOLD, L.SEG_DOWNSCALE, L.SEG_BLUR)
    assert L.SEGTAB_RAW == 8 and L.SEGTAB_MAX_MAPS == 65536
    from conceptattention_amd.csrc import build
    assert "ca_segtab.hip" in build.SOURCES
    assert {"-save-temps=obj", "-ffp-contract=off"} <= set(build.EXTRA_FLAGS["ca_segtab.hip"])
    m = re.search(r"ABI version (\d+)", open(os.path.join(ROOT, "INTEGRATION.md")).read())
    assert m and int(m.group(1)) == L.CA_VERSION


_KEEP = (ctypes.c_double * 64)()                       # a 16-byte aligned host address that is never dereferenced
_ADDR = (ctypes.addressof(_KEEP) + 15) & ~15


def _call(lib, stride=None, n=1, h=16, w=16, Hl=64, Wl=64, flags=1, blur=None, null=None, offset=None):
    """One call with host addresses: every call below must be rejected before a launch."""
    p = {"maps": _ADDR, "label": _ADDR, "records": _ADDR, "cells": _ADDR}
    if null:
        p[null] = None
    if offset:
        p[offset[0]] = _ADDR + offset[1]
    bw = (ctypes.c_float * 9)(*[1.0 / 9] * 9) if blur else None
    stride = max(h, 0) * max(w, 0) if stride is None else stride
    return lib.ca_segtab_score(ctypes.cast(p["maps"], ctypes.POINTER(ctypes.c_float)), stride, n, p["label"], p["records"],
                               p["cells"], h, w, Hl, Wl, flags, bw, None)


# name -> (arguments, what the error text must hold)
BAD = {
    "no-cells": (dict(h=0, w=16), b"4096"),
    "negative-side": (dict(h=-4, w=-4), b"4096"),
    "too-many-cells": (dict(h=64, w=65), b"4096"),
    "cells-overflowing-int32": (dict(h=1 << 16, w=1 << 16, stride=1 << 40), b"4096"),
    "no-label-pixels": (dict(Hl=0, Wl=64), b"2^24"),
    "too-many-label-pixels": (dict(Hl=4096, Wl=4097), b"2^24"),
    "label-overflowing-int32": (dict(Hl=1 << 16, Wl=1 << 16), b"2^24"),
    "no-maps": (dict(n=0), b"65536"),
    "negative-maps": (dict(n=-1), b"65536"),
    "over-the-cap": (dict(n=L.SEGTAB_MAX_MAPS + 1), b"65536"),
    "stride-below-the-map": (dict(stride=255), b"255"),
    "negative-stride": (dict(stride=-256), b"-256"),
    "maps-null": (dict(null="maps"), b"4-byte"),
    "label-null": (dict(null="label"), b"non-null"),
    "records-null": (dict(null="records"), b"8-byte"),
    "cells-null": (dict(null="cells"), b"16-byte"),
    "maps-misaligned": (dict(offset=("maps", 2)), b"4-byte"),
    "records-misaligned": (dict(offset=("records", 4)), b"8-byte"),
    "cells-misaligned": (dict(offset=("cells", 8)), b"16-byte"),
    "blur-one-row": (dict(h=1, w=16, flags=L.SEGTAB_BLUR, blur=True), b">= 2"),
    "blur-one-column": (dict(h=16, w=1, flags=L.SEGTAB_MEAN_THRESHOLD | L.SEGTAB_BLUR, blur=True), b">= 2"),
    "blur-without-weights": (dict(flags=L.SEGTAB_BLUR), b"nine"),
    "unknown-flag": (dict(flags=16), b"1 | 2 | 4 | 8"),
    "unknown-flag-among-known": (dict(flags=15 | 32), b"47"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_arguments_are_rejected_without_a_gpu(lib, name):
    kw, text = BAD[name]
    assert _call(lib, **kw) == -1, name
    err = lib.ca_last_error()
    assert b"ca_segtab_score" in err and text in err, err


def test_seg_score_still_rejects_flag_8(lib):
    arr = (L.SegProblem * 1)()
    arr[0].map = arr[0].label = arr[0].result = _ADDR
    assert lib.ca_seg_score(arr, 1, 16, 16, 64, 64, 8, None, None) == -1 and b"ca_seg_score" in lib.ca_last_error()
