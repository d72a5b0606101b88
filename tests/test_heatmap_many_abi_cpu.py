"""CPU-only checks of ca_heatmap_many's boundary: the entry is declared, bound and exported, its limit is the binding's,
and every argument error is reported with the entry's name in ca_last_error before anything is launched (the calls below
carry host addresses that are never dereferenced)."""
import ctypes
import os
import re

import pytest
import torch

import __graft_entry__ as entry
from conceptattention_amd import _lib as L
from conceptattention_amd import heatmaps, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return L.load()


def _header() -> str:
    return open(os.path.join(ROOT, "include", "conceptattn.h")).read()


def test_entry_is_declared_bound_and_exported(lib):
    """Exported with C linkage and bound (L.INTERNAL_SIGNATURES); declared in csrc/ca_heatmap_core.h, with the arguments of
    ca_heatmap_fused."""
    core = open(os.path.join(ROOT, "conceptattention_amd", "csrc", "ca_heatmap_core.h")).read()
    m = re.search(r'extern "C" int ca_heatmap_many\s*\((.*?)\);', core, re.S)
    assert m and "ca_heatmap_many" in L.INTERNAL_SIGNATURES and hasattr(lib, "ca_heatmap_many")
    assert not set(L.INTERNAL_SIGNATURES) & set(L.SIGNATURES)
    assert lib.ca_version() == L.CA_VERSION >= 136
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["problems", "n_problems", "L", "C", "dim", "norm", "stream"]
    fused = re.search(r"\bint ca_heatmap_fused\s*\((.*?)\);", _header(), re.S).group(1)
    assert [p.split()[-1].lstrip("*") for p in fused.split(",")] == [p.split()[-1].lstrip("*") for p in params]
    res, args = L.INTERNAL_SIGNATURES["ca_heatmap_many"]
    assert res is ctypes.c_int and args == L.SIGNATURES["ca_heatmap_fused"][1]
    assert args[0] == ctypes.POINTER(L.HeatmapProblem) and args[1:6] == [ctypes.c_int32] * 5
    assert lib.ca_heatmap_many.argtypes == args and lib.ca_heatmap_many.restype is ctypes.c_int


def test_constants_and_the_build():
    text = _header()
    assert int(re.search(r"#define CA_HEATMAP_MAX_CONCEPTS (\d+)", text).group(1)) == L.HEATMAP_MAX_CONCEPTS == 32
    assert int(re.search(r"#define CA_VERSION (\d+)", text).group(1)) == L.CA_VERSION
    from conceptattention_amd.csrc import build
    assert "ca_heatmap_many.hip" in build.SOURCES and "ca_heatmap_core.h" in build.HEADERS
    flags = build.EXTRA_FLAGS["ca_heatmap_many.hip"]
    assert "-save-temps=obj" in flags and "-ffp-contract=off" not in flags    # (it must round as ca_rowops.hip does)
    assert "-ffp-contract=off" not in build.EXTRA_FLAGS.get("ca_rowops.hip", [])
    assert callable(build.audit_heatmap_many)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "ca_heatmap_many" in doc and "HEATMAP_MAX_CONCEPTS = 32" in doc
    assert L.HEATMAP_SPARSE_MAX_3LAUNCH == 16


_KEEP = (ctypes.c_double * 64)()                       # a 16-byte aligned host address that is never dereferenced
_ADDR = (ctypes.addressof(_KEEP) + 15) & ~15


def _call(lib, n_problems=1, Lp=16, C=12, dim=64, norm=0, null=(), offset=None, **fields):
    arr = (L.HeatmapProblem * max(n_problems, 1))()
    for p in arr:
        p.img_vec = p.con_vec = p.acc = p.acc2 = p.logits = _ADDR
        p.ldi = p.ldc = dim
        p.weight = p.weight2 = 1.0
        for k, v in fields.items():
            setattr(p, k, v)
        for k in null:
            setattr(p, k, None)
        if offset:
            setattr(p, offset[0], _ADDR + offset[1])
    return lib.ca_heatmap_many(arr, n_problems, Lp, C, dim, norm, None)


# name -> (arguments, what the error text must hold)
BAD = {
    "no-concepts": (dict(C=0), b"C=0"),
    "33-concepts": (dict(C=33), b"C <= 32"),
    "per-head-partials": (dict(img_f32=2), b"img_f32=2"),
    "no-accumulator": (dict(null=("acc", "acc2", "logits")), b"at least one of acc / acc2 / logits"),
    "image-vectors-misaligned": (dict(offset=("img_vec", 8)), b"16-byte aligned"),
    "concept-vectors-misaligned": (dict(offset=("con_vec", 4)), b"16-byte aligned"),
    "17-problems": (dict(n_problems=17), b"n_problems <= 16"),
    "no-problems": (dict(n_problems=0), b"n_problems=0"),
    "no-concept-vectors": (dict(null=("con_vec",)), b"invalid"),
    "dim-not-a-multiple-of-8": (dict(dim=68), b"dim % 8"),
    "dim-above-4096": (dict(dim=4104), b"dim <= 4096"),
    "unknown-norm": (dict(norm=3), b"norm=3"),
    "row-stride-below-dim": (dict(ldi=56), b"ldi=56"),
    "no-patches": (dict(Lp=0), b"L=0"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_arguments_are_rejected_without_a_gpu(lib, name):
    kw, text = BAD[name]
    assert _call(lib, **kw) == -1, name
    err = lib.ca_last_error()
    assert err.startswith(b"ca_heatmap_many: ") and text in err, err
    assert lib.ca_heatmap_many(None, 1, 16, 12, 64, 0, None) == -1


def test_the_sparse_norms_limit_is_reported_without_a_gpu(lib):
    assert lib.ca_heatmap_norm_accumulate(_ADDR, 33, 16, L.NORM_SPARSEMAX, 1.0, _ADDR, None) == -1
    err = lib.ca_last_error()
    assert err.startswith(b"ca_heatmap_norm_accumulate: ") and b"C <= 32" in err, err


def test_the_concept_count_check_of_the_public_calls():
    for norm in (L.NORM_SPARSEMAX, L.NORM_ENTMAX15):
        heatmaps.check_concept_count(norm, 32)
        with pytest.raises(ValueError, match=r"33 concepts.*at most 32"):
            heatmaps.check_concept_count(norm, 33)
    heatmaps.check_concept_count(L.NORM_SOFTMAX, 500)
    assert ops.heatmap_many_fits(9, 3072) and ops.heatmap_many_fits(32, 4096) and not ops.heatmap_many_fits(33, 3072)
    assert ops.heatmap_fused_fits(8, 3072) and not ops.heatmap_fused_fits(9, 3072)
    z = torch.zeros(17, 8)
    with pytest.raises(ValueError, match="C = 17"):                      # (the limit this call always had; no device needed)
        ops.heatmap_softmax_accumulate(z, z.clone(), 1.0, L.NORM_SPARSEMAX)
    with pytest.raises(ValueError, match="1..16 problems"):
        ops.heatmap_many([])
    with pytest.raises(ValueError, match="CUDA"):
        ops.heatmap_many([ops.Heatmap(torch.zeros(4, 8), torch.zeros(2, 8), acc=torch.zeros(2, 4))])
