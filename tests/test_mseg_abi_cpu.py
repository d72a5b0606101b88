"""CPU-only checks of ca_mseg_score's boundary (the pattern of tests/test_seg_abi_cpu.py): the entry is declared, bound and
exported, the binding's struct is the header's field for field, and every class of bad argument is rejected with -1 and
the entry's name in the error text, before any launch."""
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
    """(type, field) pairs of a `typedef struct { ... } name;` of the header, in declaration order."""
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
    assert re.search(r"\bint ca_mseg_score\s*\(", _header())
    assert "ca_mseg_score" in L.SIGNATURES and hasattr(lib, "ca_mseg_score")
    assert lib.ca_version() == L.CA_VERSION >= 133
    assert len(L.SIGNATURES["ca_mseg_score"][1]) == 14


def test_struct_fields_sizes_and_constants():
    hdr, binding = _header_struct_fields("ca_mseg_problem"), L.MsegProblem._fields_
    assert [f for _, f in hdr] == [f for f, _ in binding] == ["maps", "label", "counts", "class_out", "index_out"]
    assert [_CT[t] for t, _ in hdr] == [t for _, t in binding]
    assert ctypes.sizeof(L.MsegProblem) == 5 * 8
    consts = dict((k, int(v)) for k, v in re.findall(r"#define CA_MSEG_(\w+) (\d+)", _header()))
    assert consts == {"MAX_PROBLEMS": L.MSEG_MAX_PROBLEMS, "MAX_CONCEPTS": L.MSEG_MAX_CONCEPTS,
                      "MAX_CLASSES": L.MSEG_MAX_CLASSES, "MAX_CELLS": L.MSEG_MAX_CELLS, "BLUR": L.MSEG_BLUR}
    assert consts == {"MAX_PROBLEMS": 16, "MAX_CONCEPTS": 32, "MAX_CLASSES": 256, "MAX_CELLS": 16384, "BLUR": 4}
    assert L.MSEG_MAX_LABEL_PIXELS == 1 << 24


def _call(lib, n=1, K=8, h=16, w=16, Hl=64, Wl=64, nclass=21, ignore=-1, flags=0, blur=None, null=None, problems=True,
          class_of=True, bad_class=None, scale=False, misalign=None):
    """One call with host addresses that are never dereferenced: every call below must be rejected before a launch."""
    arr = (L.MsegProblem * max(n, 1))()
    keep = (ctypes.c_double * 64)()
    for p in arr:
        p.maps = p.label = p.counts = ctypes.addressof(keep)
        if null:
            setattr(p, null, None)
        if misalign:
            setattr(p, misalign, ctypes.addressof(keep) + (2 if misalign == "maps" else 4))
    cells = max(n, 1) * max(K, 1)
    cof = (ctypes.c_uint8 * cells)(*[0] * cells)
    if bad_class is not None:
        cof[cells - 1] = bad_class
    bw = (ctypes.c_float * 9)(*[1.0 / 9] * 9) if blur else None
    sc = (ctypes.c_float * max(K, 1))(*[1.0] * max(K, 1)) if scale else None
    return lib.ca_mseg_score(arr if problems else None, n, K, h, w, Hl, Wl, nclass, ignore, flags,
                             cof if class_of else None, sc, bw, None)


BAD = {
    "problems-null": dict(problems=False),
    "maps-null": dict(null="maps"),
    "label-null": dict(null="label"),
    "counts-null": dict(null="counts"),
    "maps-misaligned": dict(misalign="maps"),
    "counts-misaligned": dict(misalign="counts"),
    "no-concepts": dict(K=0),
    "negative-concepts": dict(K=-3),
    "too-many-concepts": dict(K=33),
    "no-cells": dict(h=0, w=16),
    "negative-side": dict(h=-4, w=-4),
    "too-many-cells": dict(h=128, w=129),
    "cells-overflowing-int32": dict(h=1 << 16, w=1 << 16),
    "no-label-pixels": dict(Hl=0, Wl=64),
    "negative-label-side": dict(Hl=-8, Wl=-8),
    "too-many-label-pixels": dict(Hl=4096, Wl=4097),
    "label-overflowing-int32": dict(Hl=1 << 16, Wl=1 << 16),
    "no-classes": dict(nclass=0),
    "too-many-classes": dict(nclass=257),
    "ignore-index-below": dict(ignore=-2),
    "ignore-index-above": dict(ignore=256),
    "class-of-null": dict(class_of=False),
    "class-of-entry-at-nclass": dict(bad_class=21),
    "class-of-entry-above-nclass-last-item": dict(n=3, bad_class=200, scale=True),
    "no-problems": dict(n=0),
    "negative-problems": dict(n=-1),
    "over-the-cap": dict(n=L.MSEG_MAX_PROBLEMS + 1),
    "blur-one-row": dict(h=1, w=16, flags=L.MSEG_BLUR, blur=True),
    "blur-one-column": dict(h=16, w=1, flags=L.MSEG_BLUR, blur=True),
    "blur-without-weights": dict(flags=L.MSEG_BLUR),
    "unknown-flag-1": dict(flags=1),
    "unknown-flag-2": dict(flags=2 | L.MSEG_BLUR, blur=True),
    "unknown-flag-8": dict(flags=8),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_arguments_are_rejected_without_a_gpu(lib, name):
    assert _call(lib, **BAD[name]) == -1, name
    assert b"ca_mseg_score" in lib.ca_last_error()


def test_error_text_names_the_limits(lib):
    assert _call(lib, h=128, w=129) == -1 and b"16384" in lib.ca_last_error()
    assert _call(lib, Hl=4096, Wl=4097) == -1 and b"2^24" in lib.ca_last_error()
    assert _call(lib, K=33) == -1 and b"32" in lib.ca_last_error() and b"K=33" in lib.ca_last_error()
    assert _call(lib, nclass=257) == -1 and b"256" in lib.ca_last_error()
    assert _call(lib, n=17) == -1 and b"16" in lib.ca_last_error() and b"n_problems=17" in lib.ca_last_error()
    assert _call(lib, h=1, w=16, flags=L.MSEG_BLUR, blur=True) == -1 and b">= 2" in lib.ca_last_error()
    assert _call(lib, bad_class=21) == -1 and b"class_of[0][7]=21" in lib.ca_last_error()
    assert _call(lib, ignore=256) == -1 and b"-1..255" in lib.ca_last_error()
