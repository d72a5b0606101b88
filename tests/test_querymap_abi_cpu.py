"""CPU-only checks of ca_query_maps' boundary: the entry is declared, bound and exported, the ctypes struct matches the
header field for field, every argument rule is reported with the entry's name in ca_last_error before anything is
launched (the calls below carry host addresses that are never dereferenced), ops.query_maps raises for each Python-side
rule, and the source is part of the build with the no-spill audit."""
import ctypes
import os
import re

import pytest
import torch

import __graft_entry__ as entry
from conceptattention_amd import _lib as L
from conceptattention_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conceptattention_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return L.load()


def _decl() -> str:
    return open(os.path.join(CSRC, "ca_querymap.h")).read()


def test_entry_is_declared_bound_and_exported(lib):
    text = _decl()
    m = re.search(r"\bint ca_query_maps\s*\((.*?)\);", text, re.S)
    assert m and "ca_query_maps" in L.INTERNAL_SIGNATURES and hasattr(lib, "ca_query_maps")
    params = [p.strip().split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert params == ["problems", "n_problems", "num_heads", "scale_log2", "flags", "workspace", "workspace_bytes", "stream"]
    res, args = L.INTERNAL_SIGNATURES["ca_query_maps"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(L.QuerymapProblem), ctypes.c_int32, ctypes.c_int32, ctypes.c_float,
                                            ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert lib.ca_query_maps.argtypes == args and lib.ca_query_maps.restype is ctypes.c_int
    assert re.search(r"\bint64_t ca_query_maps_workspace_bytes\s*\(", text) and hasattr(lib, "ca_query_maps_workspace_bytes")
    assert L.INTERNAL_SIGNATURES["ca_query_maps_workspace_bytes"][0] is ctypes.c_int64
    assert not set(L.INTERNAL_SIGNATURES) & set(L.SIGNATURES)
    # not part of the public header, whose version stays
    public = open(os.path.join(ROOT, "include", "conceptattn.h")).read()
    assert "ca_query_maps" not in public
    assert int(re.search(r"#define CA_VERSION (\d+)", public).group(1)) == L.CA_VERSION == lib.ca_version()


def test_the_struct_matches_the_header_field_for_field():
    body = re.search(r"typedef struct ca_querymap_problem \{(.*?)\} ca_querymap_problem;", _decl(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        head, names = re.match(r"(const void|float|int32_t)\s+(.*)", stmt, re.S).groups()
        for n in names.split(","):
            n = n.strip()
            if n.startswith("*"):
                fields.append((n[1:], ctypes.c_void_p))
            else:
                fields.append((n, ctypes.c_float if head == "float" else ctypes.c_int32))
    assert fields == [(n, t) for n, t in L.QuerymapProblem._fields_], fields
    assert ctypes.sizeof(L.QuerymapProblem) == 6 * 8 + 8 * 4
    for name, value in (("CA_QUERYMAP_MAX_PROBLEMS", L.QUERYMAP_MAX_PROBLEMS), ("CA_QUERYMAP_MAX_QUERIES", L.QUERYMAP_MAX_QUERIES),
                        ("CA_QUERYMAP_QK_F16", L.QUERYMAP_QK_F16), ("CA_QUERYMAP_MAX_ROWS", L.QUERYMAP_MAX_ROWS)):
        assert int(re.search(rf"#define {name} (\d+)", _decl()).group(1)) == value
    assert (L.QUERYMAP_MAX_PROBLEMS, L.QUERYMAP_MAX_QUERIES, L.QUERYMAP_MAX_ROWS) == (16, 512, 2 ** 31 - 128)


def test_the_build_and_the_source():
    from conceptattention_amd.csrc import build
    assert "ca_querymap.hip" in build.SOURCES and "ca_querymap.h" in build.HEADERS
    assert "-save-temps=obj" in build.EXTRA_FLAGS["ca_querymap.hip"]
    assert callable(build.audit_querymap)
    src = open(os.path.join(CSRC, "build.py")).read()
    assert '_audit_no_spill("ca_querymap", asm_path)' in src
    assert re.search(r'audit_querymap\(os\.path\.join\(HERE, "ca_querymap-hip-amdgcn-amd-amdhsa-gfx950\.s"\)\)', src)
    # (the unit together with the header that holds the device code it shares with ca_tokmap.hip)
    unit, core = (open(os.path.join(CSRC, name)).read() for name in ("ca_querymap.hip", "ca_qkmap_core.h"))
    assert '#include "ca_qkmap_core.h"' in unit
    kernel = core + unit
    assert "__builtin_amdgcn_mfma_f32_16x16x32_bf16" in kernel and "__builtin_amdgcn_mfma_f32_16x16x32_f16" in kernel
    code = core + unit.split("namespace {")[1]
    assert "atomic" not in code and "asm" not in code             # plain HIP with builtins, no atomics


_KEEP = (ctypes.c_double * 64)()                       # a 16-byte aligned host address that is never dereferenced
_ADDR = (ctypes.addressof(_KEEP) + 15) & ~15


def _problems(n_problems=1, null=(), offset=None, **fields):
    arr = (L.QuerymapProblem * max(n_problems, 1))()
    for p in arr:
        p.q = p.k0 = p.k1 = p.acc = p.acc2 = p.lse = _ADDR
        p.nq, p.ldq, p.n0, p.n1, p.ldk = 4, 256, 8, 64, 256
        p.weight = p.weight2 = 1.0
        for k, v in fields.items():
            setattr(p, k, v)
        for k in null:
            setattr(p, k, None)
        if offset:
            setattr(p, offset[0], _ADDR + offset[1])
    return arr


def _call(lib, n_problems=1, num_heads=2, scale_log2=1.0, flags=0, workspace=_ADDR, workspace_bytes=1 << 20, array=True, **kw):
    arr = _problems(n_problems, **kw)
    return lib.ca_query_maps(arr if array else None, n_problems, num_heads, scale_log2, flags, workspace, workspace_bytes, None)


# name -> (arguments, what the error text must hold); one violation at a time
BAD = {
    "no-array": (dict(array=False), b"bad arguments"),
    "no-problems": (dict(n_problems=0), b"n_problems=0"),
    "17-problems": (dict(n_problems=17), b"n_problems <= 16"),
    "no-heads": (dict(num_heads=0), b"num_heads=0"),
    "scale-not-finite": (dict(scale_log2=float("inf")), b"finite scale_log2"),
    "scale-nan": (dict(scale_log2=float("nan")), b"finite scale_log2"),
    "unknown-flag": (dict(flags=2), b"flags=2"),
    "workspace-too-small": (dict(workspace_bytes=2 * 4 * 8 - 1), b"workspace too small"),
    "negative-workspace": (dict(workspace_bytes=-1), b"workspace too small"),
    "no-workspace": (dict(workspace=None), b"workspace too small"),
    "workspace-misaligned": (dict(workspace=_ADDR + 8), b"16-byte aligned"),
    "no-query-rows": (dict(nq=0), b"nq=0"),
    "513-query-rows": (dict(nq=513), b"nq <= 512"),
    "no-emitted-keys": (dict(n1=0), b"n1=0"),
    "negative-leading-keys": (dict(n0=-1), b"n0=-1"),
    "keys-within-a-block-of-2^31": (dict(n1=2 ** 31 - 135), b"n0 + n1 <= 2147483520"),
    "no-q": (dict(null=("q",)), b"rows invalid"),
    "no-k1": (dict(null=("k1",)), b"rows invalid"),
    "no-k0-with-leading-keys": (dict(null=("k0",)), b"with n0 > 0, k0 non-null"),
    "q-misaligned": (dict(offset=("q", 8)), b"16-byte aligned"),
    "k0-misaligned": (dict(offset=("k0", 2)), b"16-byte aligned"),
    "k1-misaligned": (dict(offset=("k1", 4)), b"16-byte aligned"),
    "q-stride-below-the-width": (dict(ldq=248), b"ldq=248"),
    "k-stride-below-the-width": (dict(ldk=248), b"ldk=248"),
    "q-stride-not-a-multiple-of-8": (dict(ldq=260), b"ldq=260"),
    "k-stride-not-a-multiple-of-8": (dict(ldk=257), b"ldk=257"),
    "no-accumulator": (dict(null=("acc", "acc2")), b"at least one of acc / acc2"),
    "acc-misaligned": (dict(offset=("acc", 2)), b"4-byte aligned"),
    "lse-misaligned": (dict(offset=("lse", 1)), b"4-byte aligned"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_arguments_are_rejected_without_a_gpu(lib, name):
    kw, text = BAD[name]
    assert _call(lib, **kw) == -1, name
    err = lib.ca_last_error()
    assert err.startswith(b"ca_query_maps: ") and text in err, err


def test_the_workspace_size_needs_no_gpu(lib):
    arr = _problems(2, nq=512, ldq=9216, n0=512, n1=4096, ldk=9216)
    arr[1].nq = 3
    assert lib.ca_query_maps_workspace_bytes(arr, 1, 24) == 24 * 512 * 8
    assert lib.ca_query_maps_workspace_bytes(arr, 2, 24) == 24 * 512 * 8 + 24 * 3 * 8
    assert lib.ca_query_maps_workspace_bytes(_problems(1, nq=3), 1, 1) == 32      # (a problem's share is rounded up to 16)
    assert lib.ca_query_maps_workspace_bytes(_problems(1, null=("k0",), n0=0), 1, 2) == 64   # (no leading keys: k0 may be NULL)
    assert lib.ca_query_maps_workspace_bytes(_problems(1, nq=513), 1, 24) == -1
    assert lib.ca_last_error().startswith(b"ca_query_maps_workspace_bytes: ")


def _bf(rows, cols=256):
    return torch.zeros(rows, cols, dtype=torch.bfloat16)


def test_the_python_side_rules_are_checked_before_the_device_is_asked_for():
    """ops.query_maps' own ValueErrors.  The operands are host tensors: a rule that passed would end in _chk's "expected a
    CUDA(HIP) tensor", so each rule is checked on a _chk that lets host tensors through."""
    real = ops._chk
    ops._chk = ops._chk_host
    try:
        q, k0, k1 = _bf(4), _bf(8), _bf(64)
        acc = torch.zeros(4, 64)

        def qm(**kw):
            base = dict(q=q, k0=k0, k1=k1, acc=acc, weight=1.0)
            base.update(kw)
            return ops._query_maps_array([ops.QueryMaps(**base)], 2)
        arr = qm()
        assert (arr[0].nq, arr[0].n0, arr[0].n1, arr[0].ldq, arr[0].ldk) == (4, 8, 64, 256, 256)
        assert qm(k0=None)[0].n0 == 0 and qm(k0=None)[0].k0 is None
        assert qm(k0=_bf(0))[0].n0 == 0
        one = qm(q=_bf(1), acc=torch.zeros(1, 64))
        assert (one[0].nq, one[0].ldq) == (1, 256)
        with pytest.raises(ValueError, match="k1, the emitted key rows, is required"):
            qm(k1=None)
        with pytest.raises(ValueError, match="dtype"):
            qm(q=q.float())
        with pytest.raises(ValueError, match="dtype"):
            qm(acc=acc.double())
        with pytest.raises(ValueError, match="num_heads\\*128 = 256 columns"):
            qm(q=_bf(4, 128))
        with pytest.raises(ValueError, match="num_heads\\*128 = 256 columns"):
            qm(k1=_bf(64, 384))
        with pytest.raises(ValueError, match="share one row stride"):
            qm(k1=_bf(64, 512)[:, :256])
        with pytest.raises(ValueError, match="innermost dimension must be contiguous"):
            qm(q=torch.zeros(256, 4, dtype=torch.bfloat16).T)
        with pytest.raises(ValueError, match="nq <= 512"):
            qm(q=_bf(513), acc=torch.zeros(513, 64))
        with pytest.raises(ValueError, match="n1 >= 1"):
            qm(k1=_bf(0), acc=torch.zeros(4, 0))
        with pytest.raises(ValueError, match="needs acc or acc2"):
            qm(acc=None)
        with pytest.raises(ValueError, match=r"acc must be contiguous fp32 \[4, 64\]"):
            qm(acc=torch.zeros(64, 4))
        with pytest.raises(ValueError, match=r"acc2 must be contiguous fp32 \[4, 64\]"):
            qm(acc2=torch.zeros(4, 128)[:, :64])
        with pytest.raises(ValueError, match=r"lse must be contiguous fp32 \[2, 4\]"):
            qm(lse=torch.zeros(3, 4))
        with pytest.raises(ValueError, match="does not fit the library's int32_t"):
            qm(q=torch.empty_strided((2, 256), (2 ** 31, 1), dtype=torch.bfloat16, device="meta"), acc=torch.zeros(2, 64))
        with pytest.raises(ValueError, match="also an accumulator of problem 0"):
            ops._query_maps_array([ops.QueryMaps(q, k0, k1, acc=acc), ops.QueryMaps(q, k0, k1, acc2=acc)], 2)
        with pytest.raises(ValueError, match="also an accumulator of problem 0"):
            qm(acc2=acc)
    finally:
        ops._chk = real
    with pytest.raises(ValueError, match="CUDA"):
        ops.query_maps([ops.QueryMaps(q, k0, k1, acc=acc)], 2)
    for bad in (dict(problems=[]), dict(num_heads=0), dict(scale_log2=float("nan"))):
        kw = dict(problems=[ops.QueryMaps(q, k0, k1, acc=acc)], num_heads=2)
        kw.update(bad)
        with pytest.raises(ValueError, match="query_maps: "):
            ops.query_maps(**kw)
