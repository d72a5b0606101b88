"""CPU-only checks of ca_seg_score's boundary: the entry is exported, the binding's structs are the header's field for
field, and every class of bad argument is rejected with the entry's name in the error text, before any launch."""
import ctypes
import os
import re

import pytest

import __graft_entry__ as entry
from conceptattention_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CT = {"ptr": ctypes.c_void_p, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "double": ctypes.c_double}


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return L.load()


def _header() -> str:
    return open(os.path.join(ROOT, "include", "conceptattn.h")).read()


def _header_struct_fields(name):
    """(type, field) pairs of a `typedef struct { ... } name;` of the header, in declaration order (the parsing of
    tests/test_abi_cpu.py, with double added)."""
    text = _header()
    end = re.search(r"\}\s*" + name + r"\s*;", text).start()
    body = text[text.rfind("typedef struct {", 0, end) + len("typedef struct {"):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(void|float|double|int32_t)\s*(\*?)\s*(.*)$", decl, re.S)
        assert m, decl
        ctype = "ptr" if m.group(2) or m.group(3).lstrip().startswith("*") else m.group(1)
        for f in m.group(3).split(","):
            out.append((ctype, f.strip().lstrip("*").strip()))
    return out


def test_entry_is_declared_bound_and_exported(lib):
    assert re.search(r"\bint ca_seg_score\s*\(", _header())
    assert "ca_seg_score" in L.SIGNATURES and hasattr(lib, "ca_seg_score")
    assert lib.ca_version() == L.CA_VERSION >= 132


@pytest.mark.parametrize("name,struct", [("ca_seg_problem", "SegProblem"), ("ca_seg_record", "SegRecord")])
def test_struct_fields_match_the_header(name, struct):
    hdr, binding = _header_struct_fields(name), getattr(L, struct)._fields_
    assert [f for _, f in hdr] == [f for f, _ in binding]
    assert [_CT[t] for t, _ in hdr] == [t for _, t in binding]


def test_sizes_and_constants():
    assert ctypes.sizeof(L.SegProblem) == 5 * 8 and ctypes.sizeof(L.SegRecord) == 40
    assert L.SegRecord.ap.offset == 16 and L.SegRecord.thresholds.offset == 36
    consts = dict((k, int(v)) for k, v in re.findall(r"#define CA_SEG_(\w+) (\d+)", _header()))
    assert consts == {"MAX_PROBLEMS": L.SEG_MAX_PROBLEMS, "MEAN_THRESHOLD": L.SEG_MEAN_THRESHOLD,
                      "DOWNSCALE": L.SEG_DOWNSCALE, "BLUR": L.SEG_BLUR}


def _call(lib, n=1, h=16, w=16, Hl=64, Wl=64, flags=1, blur=None, null=None, problems=True):
    """One call with host addresses that are never dereferenced: every call below must be rejected before a launch."""
    arr = (L.SegProblem * max(n, 1))()
    keep = (ctypes.c_double * 64)()
    for p in arr:
        p.map = p.label = p.result = ctypes.addressof(keep)
        if null:
            setattr(p, null, None)
    bw = (ctypes.c_float * 9)(*[1.0 / 9] * 9) if blur else None
    return lib.ca_seg_score(arr if problems else None, n, h, w, Hl, Wl, flags, bw, None)


BAD = {
    "problems-null": dict(problems=False),
    "map-null": dict(null="map"),
    "label-null": dict(null="label"),
    "result-null": dict(null="result"),
    "no-cells": dict(h=0, w=16),
    "negative-side": dict(h=-4, w=-4),
    "too-many-cells": dict(h=64, w=65),
    "cells-overflowing-int32": dict(h=1 << 16, w=1 << 16),
    "no-label-pixels": dict(Hl=0, Wl=64),
    "too-many-label-pixels": dict(Hl=4096, Wl=4097),
    "label-overflowing-int32": dict(Hl=1 << 16, Wl=1 << 16),
    "no-problems": dict(n=0),
    "negative-problems": dict(n=-1),
    "over-the-cap": dict(n=L.SEG_MAX_PROBLEMS + 1),
    "blur-one-row": dict(h=1, w=16, flags=L.SEG_BLUR, blur=True),
    "blur-one-column": dict(h=16, w=1, flags=L.SEG_MEAN_THRESHOLD | L.SEG_BLUR, blur=True),
    "blur-without-weights": dict(flags=L.SEG_BLUR),
    "unknown-flag": dict(flags=8),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_arguments_are_rejected_without_a_gpu(lib, name):
    assert _call(lib, **BAD[name]) == -1, name
    assert b"ca_seg_score" in lib.ca_last_error()


def test_error_text_names_the_limits(lib):
    assert _call(lib, h=64, w=65) == -1 and b"4096" in lib.ca_last_error()
    assert _call(lib, Hl=4096, Wl=4097) == -1 and b"2^24" in lib.ca_last_error()
    assert _call(lib, n=17) == -1 and b"16" in lib.ca_last_error()
    assert _call(lib, h=1, w=16, flags=L.SEG_BLUR, blur=True) == -1 and b">= 2" in lib.ca_last_error()
