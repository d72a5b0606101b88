"""CPU-only checks of ca_propagate_maps' boundary: the entry is declared, bound and exported, the ctypes struct matches
the header field for field, every argument rule is reported with the entry's name in ca_last_error before anything is
launched (the calls below carry host addresses that are never dereferenced), ops.propagate_maps raises for each
Python-side rule, and the source is part of the build with the no-spill audit."""
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
    return open(os.path.join(CSRC, "ca_propmap.h")).read()


def test_entry_is_declared_bound_and_exported(lib):
    text = _decl()
    m = re.search(r"\bint ca_propagate_maps\s*\((.*?)\);", text, re.S)
    assert m and "ca_propagate_maps" in L.INTERNAL_SIGNATURES and hasattr(lib, "ca_propagate_maps")
    params = [p.strip().split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert params == ["problems", "n_problems", "num_heads", "scale_log2", "flags", "workspace", "workspace_bytes", "stream"]
    res, args = L.INTERNAL_SIGNATURES["ca_propagate_maps"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(L.PropmapProblem), ctypes.c_int32, ctypes.c_int32, ctypes.c_float,
                                            ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert lib.ca_propagate_maps.argtypes == args and lib.ca_propagate_maps.restype is ctypes.c_int
    assert re.search(r"\bint64_t ca_propagate_maps_workspace_bytes\s*\(", text)
    assert hasattr(lib, "ca_propagate_maps_workspace_bytes")
    assert L.INTERNAL_SIGNATURES["ca_propagate_maps_workspace_bytes"] == \
        (ctypes.c_int64, [ctypes.POINTER(L.PropmapProblem), ctypes.c_int32, ctypes.c_int32])
    assert not set(L.INTERNAL_SIGNATURES) & set(L.SIGNATURES)
    assert not [n for n in L.SIGNATURES if "propagate" in n]
    # not part of the public header, whose version stays
    public = open(os.path.join(ROOT, "include", "conceptattn.h")).read()
    assert "ca_propagate_maps" not in public
    assert int(re.search(r"#define CA_VERSION (\d+)", public).group(1)) == L.CA_VERSION == lib.ca_version() == 137


def test_the_struct_matches_the_header_field_for_field():
    body = re.search(r"typedef struct ca_propmap_problem \{(.*?)\} ca_propmap_problem;", _decl(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        head, names = re.match(r"(const void|const float|float|int32_t)\s+(.*)", stmt, re.S).groups()
        for n in names.split(","):
            n = n.strip()
            if n.startswith("*"):
                fields.append((n[1:], ctypes.c_void_p))
            else:
                fields.append((n, ctypes.c_float if head == "float" else ctypes.c_int32))
    assert fields == [(n, t) for n, t in L.PropmapProblem._fields_], fields
    assert ctypes.sizeof(L.PropmapProblem) == 6 * 8 + 8 * 4 + 2 * 4
    for name, value in (("CA_PROPMAP_MAX_PROBLEMS", L.PROPMAP_MAX_PROBLEMS), ("CA_PROPMAP_MAX_CONCEPTS", L.PROPMAP_MAX_CONCEPTS),
                        ("CA_PROPMAP_QK_F16", L.PROPMAP_QK_F16), ("CA_PROPMAP_MAX_ROWS", L.PROPMAP_MAX_ROWS),
                        ("CA_PROPMAP_MAX_HEADS", L.PROPMAP_MAX_HEADS)):
        assert int(re.search(rf"#define {name} (\d+)", _decl()).group(1)) == value
    assert (L.PROPMAP_MAX_PROBLEMS, L.PROPMAP_MAX_CONCEPTS, L.PROPMAP_MAX_ROWS) == (16, L.HEATMAP_MAX_CONCEPTS, 2 ** 31 - 128)
    assert "CA_PROPMAP_MAX_QUERIES" not in _decl()                # no limit on the query rows
    assert "unspecified" in _decl()                               # non-finite v other than NaN


def test_the_build_and_the_source():
    from conceptattention_amd.csrc import build
    assert "ca_propmap.hip" in build.SOURCES and "ca_propmap.h" in build.HEADERS
    assert "-save-temps=obj" in build.EXTRA_FLAGS["ca_propmap.hip"]
    assert callable(build.audit_propmap)
    src = open(os.path.join(CSRC, "build.py")).read()
    assert '_audit_no_spill("ca_propmap", asm_path)' in src
    assert re.search(r'audit_propmap\(os\.path\.join\(HERE, "ca_propmap-hip-amdgcn-amd-amdhsa-gfx950\.s"\)\)', src)
    unit = open(os.path.join(CSRC, "ca_propmap.hip")).read()
    assert "ca_qkmap_core.h" not in unit.split("#include", 1)[1]  # the unit states its own fragment and score steps
    assert "#include \"ca_qkmap_core.h\"" not in unit
    assert "__builtin_amdgcn_mfma_f32_16x16x32_bf16" in unit and "__builtin_amdgcn_mfma_f32_16x16x32_f16" in unit
    assert "__builtin_amdgcn_mfma_f32_16x16x4f32" in unit         # p and v enter the product as fp32
    code = unit.split("namespace {")[1]
    assert "atomic" not in code and "asm" not in code             # plain HIP with builtins, no atomics


_KEEP = (ctypes.c_double * 64)()                       # a 16-byte aligned host address that is never dereferenced
_ADDR = (ctypes.addressof(_KEEP) + 15) & ~15


def _problems(n_problems=1, null=(), offset=None, **fields):
    arr = (L.PropmapProblem * max(n_problems, 1))()
    for p in arr:
        p.q = p.k0 = p.k1 = p.v = p.acc = p.acc2 = _ADDR
        p.nq, p.ldq, p.n0, p.n1, p.ldk, p.C, p.ldv = 4, 256, 8, 64, 256, 5, 64
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
    return lib.ca_propagate_maps(arr if array else None, n_problems, num_heads, scale_log2, flags, workspace, workspace_bytes, None)


# name -> (arguments, what the error text must hold); one violation at a time
BAD = {
    "no-array": (dict(array=False), b"bad arguments"),
    "no-problems": (dict(n_problems=0), b"n_problems=0"),
    "17-problems": (dict(n_problems=17), b"n_problems <= 16"),
    "no-heads": (dict(num_heads=0), b"num_heads=0"),
    "too-many-heads": (dict(num_heads=65536, ldq=65536 * 128, ldk=65536 * 128), b"num_heads <= 65535"),
    "scale-not-finite": (dict(scale_log2=float("inf")), b"finite scale_log2"),
    "scale-nan": (dict(scale_log2=float("nan")), b"finite scale_log2"),
    "unknown-flag": (dict(flags=2), b"flags=2"),
    "workspace-too-small": (dict(workspace_bytes=2 * 5 * 4 * 4 - 1), b"workspace too small"),
    "negative-workspace": (dict(workspace_bytes=-1), b"workspace too small"),
    "no-workspace": (dict(workspace=None), b"workspace too small"),
    "workspace-misaligned": (dict(workspace=_ADDR + 8), b"16-byte aligned"),
    "no-query-rows": (dict(nq=0), b"nq=0"),
    "no-valued-keys": (dict(n1=0), b"n1=0"),
    "negative-leading-keys": (dict(n0=-1), b"n0=-1"),
    "keys-within-a-block-of-2^31": (dict(n1=2 ** 31 - 135, ldv=2 ** 31 - 135), b"n0 + n1 <= 2147483520"),
    "no-map-rows": (dict(C=0), b"C=0"),
    "33-map-rows": (dict(C=33), b"C <= 32"),
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
    "no-v": (dict(null=("v",)), b"maps invalid"),
    "v-misaligned": (dict(offset=("v", 2)), b"4-byte aligned"),
    "v-stride-below-n1": (dict(ldv=63), b"ldv=63"),
    "no-accumulator": (dict(null=("acc", "acc2")), b"at least one of acc / acc2"),
    "acc-misaligned": (dict(offset=("acc", 2)), b"4-byte aligned"),
    "acc2-misaligned": (dict(offset=("acc2", 1)), b"4-byte aligned"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_arguments_are_rejected_without_a_gpu(lib, name):
    kw, text = BAD[name]
    assert _call(lib, **kw) == -1, name
    err = lib.ca_last_error()
    assert err.startswith(b"ca_propagate_maps: ") and text in err, err


def test_the_workspace_size_needs_no_gpu(lib):
    arr = _problems(2, nq=4096, ldq=9216, n0=0, n1=4096, ldk=9216, C=32, ldv=4096)
    arr[1].nq, arr[1].C = 3, 5
    assert lib.ca_propagate_maps_workspace_bytes(arr, 1, 24) == 24 * 32 * 4096 * 4
    assert lib.ca_propagate_maps_workspace_bytes(arr, 2, 24) == 24 * 32 * 4096 * 4 + 24 * 5 * 3 * 4
    assert lib.ca_propagate_maps_workspace_bytes(_problems(1, nq=3, C=1), 1, 1) == 16   # (a problem's share is rounded up to 16)
    assert lib.ca_propagate_maps_workspace_bytes(_problems(1, null=("k0",), n0=0), 1, 2) == 2 * 5 * 4 * 4   # (k0 may be NULL)
    assert lib.ca_propagate_maps_workspace_bytes(_problems(1, nq=513, ldq=3072, ldk=3072), 1, 24) == 24 * 5 * 513 * 4   # (no 512-row limit)
    assert lib.ca_propagate_maps_workspace_bytes(_problems(1, C=33, ldq=3072, ldk=3072), 1, 24) == -1
    assert lib.ca_last_error().startswith(b"ca_propagate_maps: ")


def _bf(rows, cols=256):
    return torch.zeros(rows, cols, dtype=torch.bfloat16)


def test_the_python_side_rules_are_checked_before_the_device_is_asked_for():
    """ops.propagate_maps' own ValueErrors.  The operands are host tensors: a rule that passed would end in _chk's "expected
    a CUDA(HIP) tensor", so each rule is checked on a _chk that lets host tensors through."""
    real = ops._chk
    ops._chk = ops._chk_host
    try:
        q, k0, k1 = _bf(4), _bf(8), _bf(64)
        v = torch.zeros(5, 64)
        acc = torch.zeros(5, 4)

        def pm(**kw):
            base = dict(q=q, k0=k0, k1=k1, v=v, acc=acc, weight=1.0)
            base.update(kw)
            return ops._propagate_maps_array([ops.PropagateMaps(**base)], 2)
        arr = pm()
        assert (arr[0].nq, arr[0].n0, arr[0].n1, arr[0].ldq, arr[0].ldk, arr[0].C, arr[0].ldv) == (4, 8, 64, 256, 256, 5, 64)
        assert arr[0].v == v.data_ptr() and arr[0].acc == acc.data_ptr() and arr[0].acc2 is None
        assert pm(k0=None)[0].n0 == 0 and pm(k0=None)[0].k0 is None
        assert pm(k0=_bf(0))[0].n0 == 0
        one = pm(q=_bf(1), acc=torch.zeros(5, 1))
        assert (one[0].nq, one[0].ldq) == (1, 256)                        # one-row strides
        assert pm(v=torch.zeros(5, 80)[:, :64])[0].ldv == 80              # ldv > n1
        assert pm(v=torch.zeros(1, 64), acc=torch.zeros(1, 4))[0].ldv == 64
        big = pm(q=_bf(513), acc=torch.zeros(5, 513))                     # no 512-row limit
        assert big[0].nq == 513
        with pytest.raises(ValueError, match="k1, the valued key rows, is required"):
            pm(k1=None)
        with pytest.raises(ValueError, match="v, the map rows to propagate, is required"):
            pm(v=None)
        with pytest.raises(ValueError, match="dtype"):
            pm(q=q.float())
        with pytest.raises(ValueError, match="dtype"):
            pm(v=v.double())
        with pytest.raises(ValueError, match="dtype"):
            pm(v=v.bfloat16())
        with pytest.raises(ValueError, match="dtype"):
            pm(acc=acc.double())
        with pytest.raises(ValueError, match="num_heads\\*128 = 256 columns"):
            pm(q=_bf(4, 128))
        with pytest.raises(ValueError, match="num_heads\\*128 = 256 columns"):
            pm(k1=_bf(64, 384))
        with pytest.raises(ValueError, match="share one row stride"):
            pm(k1=_bf(64, 512)[:, :256])
        with pytest.raises(ValueError, match="innermost dimension must be contiguous"):
            pm(q=torch.zeros(256, 4, dtype=torch.bfloat16).T)
        with pytest.raises(ValueError, match="innermost dimension must be contiguous"):
            pm(v=torch.zeros(64, 5).T)
        with pytest.raises(ValueError, match=r"v must be 2-D fp32 \[C, n1 = 64\]"):
            pm(v=torch.zeros(5, 63))
        with pytest.raises(ValueError, match=r"v must be 2-D fp32 \[C, n1 = 64\]"):
            pm(v=torch.zeros(64))
        with pytest.raises(ValueError, match="1 <= C <= 32"):
            pm(v=torch.zeros(33, 64), acc=torch.zeros(33, 4))
        with pytest.raises(ValueError, match="1 <= C <= 32"):
            pm(v=torch.zeros(0, 64), acc=torch.zeros(0, 4))
        with pytest.raises(ValueError, match="n1 >= 1"):
            pm(k1=_bf(0), v=torch.zeros(5, 0))
        with pytest.raises(ValueError, match="needs acc or acc2"):
            pm(acc=None)
        with pytest.raises(ValueError, match=r"acc must be contiguous fp32 \[5, 4\]"):
            pm(acc=torch.zeros(4, 5))
        with pytest.raises(ValueError, match=r"acc2 must be contiguous fp32 \[5, 4\]"):
            pm(acc2=torch.zeros(5, 8)[:, :4])
        with pytest.raises(ValueError, match="does not fit the library's int32_t"):
            pm(q=torch.empty_strided((2, 256), (2 ** 31, 1), dtype=torch.bfloat16, device="meta"), acc=torch.zeros(5, 2))
        with pytest.raises(ValueError, match="does not fit the library's int32_t"):
            pm(v=torch.empty_strided((5, 64), (2 ** 31, 1), dtype=torch.float32, device="meta"))
        with pytest.raises(ValueError, match="also an accumulator of problem 0"):
            ops._propagate_maps_array([ops.PropagateMaps(q, k0, k1, v, acc=acc), ops.PropagateMaps(q, k0, k1, v, acc2=acc)], 2)
        with pytest.raises(ValueError, match="also an accumulator of problem 0"):
            pm(acc2=acc)
        # v may not be, or overlap, an accumulator of any problem of the call
        sq_q, sq_k = _bf(64), _bf(64)
        both = torch.zeros(5, 64)
        with pytest.raises(ValueError, match="v overlaps acc of problem 0"):
            ops._propagate_maps_array([ops.PropagateMaps(sq_q, None, sq_k, both, acc=both)], 2)
        with pytest.raises(ValueError, match="v overlaps acc2 of problem 1"):
            ops._propagate_maps_array([ops.PropagateMaps(sq_q, None, sq_k, both, acc=torch.zeros(5, 64)),
                                       ops.PropagateMaps(sq_q, None, sq_k, torch.zeros(5, 64), acc2=both)], 2)
        pool = torch.zeros(5 * 64 + 5 * 64 - 8)
        with pytest.raises(ValueError, match="v overlaps acc of problem 0"):            # a partial overlap
            ops._propagate_maps_array([ops.PropagateMaps(sq_q, None, sq_k, pool[:320].view(5, 64), acc=pool[312:].view(5, 64))], 2)
    finally:
        ops._chk = real
    with pytest.raises(ValueError, match="CUDA"):
        ops.propagate_maps([ops.PropagateMaps(q, k0, k1, v, acc=acc)], 2)
    for bad in (dict(problems=[]), dict(num_heads=0), dict(scale_log2=float("nan"))):
        kw = dict(problems=[ops.PropagateMaps(q, k0, k1, v, acc=acc)], num_heads=2)
        kw.update(bad)
        with pytest.raises(ValueError, match="propagate_maps: "):
            ops.propagate_maps(**kw)
