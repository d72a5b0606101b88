"""CPU-only checks of ca_token_maps' boundary: the entry is declared, bound and exported, the ctypes struct matches the
header field for field, every argument rule is reported with the entry's name in ca_last_error before anything is
launched (the calls below carry host addresses that are never dereferenced), ops.token_maps raises for each Python-side
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
    return open(os.path.join(CSRC, "ca_tokmap.h")).read()


def test_entry_is_declared_bound_and_exported(lib):
    text = _decl()
    m = re.search(r"\bint ca_token_maps\s*\((.*?)\);", text, re.S)
    assert m and "ca_token_maps" in L.INTERNAL_SIGNATURES and hasattr(lib, "ca_token_maps")
    params = [p.strip().split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert params == ["problems", "n_problems", "num_heads", "scale_log2", "flags", "workspace", "workspace_bytes", "stream"]
    res, args = L.INTERNAL_SIGNATURES["ca_token_maps"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(L.TokmapProblem), ctypes.c_int32, ctypes.c_int32, ctypes.c_float,
                                            ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert lib.ca_token_maps.argtypes == args and lib.ca_token_maps.restype is ctypes.c_int
    assert re.search(r"\bint64_t ca_token_maps_workspace_bytes\s*\(", text) and hasattr(lib, "ca_token_maps_workspace_bytes")
    assert L.INTERNAL_SIGNATURES["ca_token_maps_workspace_bytes"][0] is ctypes.c_int64
    assert not set(L.INTERNAL_SIGNATURES) & set(L.SIGNATURES)
    # not part of the public header, whose version stays
    public = open(os.path.join(ROOT, "include", "conceptattn.h")).read()
    assert "ca_token_maps" not in public
    assert int(re.search(r"#define CA_VERSION (\d+)", public).group(1)) == L.CA_VERSION == lib.ca_version()


def test_the_struct_matches_the_header_field_for_field():
    body = re.search(r"typedef struct ca_tokmap_problem \{(.*?)\} ca_tokmap_problem;", _decl(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        ctype = {"const void": ctypes.c_void_p, "float": None, "int32_t": ctypes.c_int32}
        head, names = re.match(r"(const void|float|int32_t)\s+(.*)", stmt, re.S).groups()
        for n in names.split(","):
            n = n.strip()
            if n.startswith("*"):
                fields.append((n[1:], ctypes.c_void_p))
            else:
                fields.append((n, ctypes.c_float if head == "float" else ctype[head]))
    assert fields == [(n, t) for n, t in L.TokmapProblem._fields_], fields
    assert ctypes.sizeof(L.TokmapProblem) == 6 * 8 + 8 * 4
    for name, value in (("CA_TOKMAP_MAX_PROBLEMS", L.TOKMAP_MAX_PROBLEMS), ("CA_TOKMAP_MAX_TEXT", L.TOKMAP_MAX_TEXT),
                        ("CA_TOKMAP_QK_F16", L.TOKMAP_QK_F16), ("CA_TOKMAP_MAX_ROWS", 2 ** 31 - 128)):
        assert int(re.search(rf"#define {name} (\d+)", _decl()).group(1)) == value
    assert (L.TOKMAP_MAX_PROBLEMS, L.TOKMAP_MAX_TEXT) == (16, 512)


def test_the_build_and_the_documents():
    from conceptattention_amd.csrc import build
    assert "ca_tokmap.hip" in build.SOURCES and "ca_tokmap.h" in build.HEADERS
    assert "-save-temps=obj" in build.EXTRA_FLAGS["ca_tokmap.hip"]
    assert callable(build.audit_tokmap)
    src = open(os.path.join(CSRC, "build.py")).read()
    assert '_audit_no_spill("ca_tokmap", asm_path)' in src
    assert re.search(r'audit_tokmap\(os\.path\.join\(HERE, "ca_tokmap-hip-amdgcn-amd-amdhsa-gfx950\.s"\)\)', src)
    # (the unit together with the header that holds the device code it shares with ca_querymap.hip)
    unit, core = (open(os.path.join(CSRC, name)).read() for name in ("ca_tokmap.hip", "ca_qkmap_core.h"))
    assert '#include "ca_qkmap_core.h"' in unit
    kernel = core + unit
    assert "__builtin_amdgcn_mfma_f32_16x16x32_bf16" in kernel and "__builtin_amdgcn_mfma_f32_16x16x32_f16" in kernel
    assert "atomic" not in re.sub(r"std::atomic<unsigned long long> attr_done", "", core + unit.split("namespace {")[1])
    assert "asm" not in kernel                                     # plain HIP with builtins
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Prompt-token maps" in doc and "ca_token_maps" in doc


_KEEP = (ctypes.c_double * 64)()                       # a 16-byte aligned host address that is never dereferenced
_ADDR = (ctypes.addressof(_KEEP) + 15) & ~15


def _call(lib, n_problems=1, num_heads=2, scale_log2=1.0, flags=0, workspace_bytes=0, null=(), offset=None, array=True,
          **fields):
    arr = (L.TokmapProblem * max(n_problems, 1))()
    for p in arr:
        p.q = p.k0 = p.k1 = p.acc = p.acc2 = p.lse = _ADDR
        p.nq, p.ldq, p.n0, p.n1, p.ldk, p.n_tok = 64, 256, 8, 64, 256, 4
        p.weight = p.weight2 = 1.0
        for k, v in fields.items():
            setattr(p, k, v)
        for k in null:
            setattr(p, k, None)
        if offset:
            setattr(p, offset[0], _ADDR + offset[1])
    return lib.ca_token_maps(arr if array else None, n_problems, num_heads, scale_log2, flags, None, workspace_bytes, None)


# name -> (arguments, what the error text must hold); one violation at a time
BAD = {
    "no-array": (dict(array=False), b"bad arguments"),
    "no-problems": (dict(n_problems=0), b"n_problems=0"),
    "17-problems": (dict(n_problems=17), b"n_problems <= 16"),
    "no-heads": (dict(num_heads=0), b"num_heads=0"),
    "scale-not-finite": (dict(scale_log2=float("inf")), b"finite scale_log2"),
    "scale-nan": (dict(scale_log2=float("nan")), b"finite scale_log2"),
    "unknown-flag": (dict(flags=2), b"flags=2"),
    "negative-workspace": (dict(workspace_bytes=-1), b"workspace too small"),
    "no-query-rows": (dict(nq=0), b"nq=0"),
    "query-rows-within-a-block-of-2^31": (dict(nq=2 ** 31 - 127), b"nq <= 2147483520"),
    "keys-within-a-tile-of-2^31": (dict(n1=2 ** 31 - 127), b"n0 + n1 <= 2147483520"),
    "no-text-keys": (dict(n0=0, n_tok=0), b"n0=0"),
    "513-text-keys": (dict(n0=513), b"n0 <= 512"),
    "no-tokens": (dict(n_tok=0), b"n_tok=0"),
    "more-tokens-than-text-keys": (dict(n_tok=9), b"n_tok=9"),
    "negative-image-keys": (dict(n1=-1), b"n1=-1"),
    "no-q": (dict(null=("q",)), b"rows invalid"),
    "no-k0": (dict(null=("k0",)), b"rows invalid"),
    "no-k1-with-image-keys": (dict(null=("k1",)), b"with n1 > 0, k1 non-null"),
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
    assert err.startswith(b"ca_token_maps: ") and text in err, err


def test_the_workspace_size_needs_no_gpu(lib):
    arr = (L.TokmapProblem * 1)()
    p = arr[0]
    p.q = p.k0 = p.k1 = p.acc = _ADDR
    p.nq, p.ldq, p.n0, p.n1, p.ldk, p.n_tok = 4096, 9216, 512, 4096, 9216, 512
    assert lib.ca_token_maps_workspace_bytes(arr, 1, 24) == 0      # (the head sum lives in LDS)
    p.n_tok = 513
    assert lib.ca_token_maps_workspace_bytes(arr, 1, 24) == -1
    assert lib.ca_last_error().startswith(b"ca_token_maps_workspace_bytes: ")


def _bf(rows, cols=256):
    return torch.zeros(rows, cols, dtype=torch.bfloat16)


def test_the_python_side_rules_are_checked_before_the_device_is_asked_for():
    """ops.token_maps' own ValueErrors.  The operands are host tensors: a rule that passed would end in _chk's "expected a
    CUDA(HIP) tensor", so each rule is checked on a _chk that lets host tensors through."""
    real = ops._chk
    ops._chk = ops._chk_host
    try:
        q, k0, k1 = _bf(64), _bf(8), _bf(64)
        acc = torch.zeros(4, 64)

        def tm(**kw):
            base = dict(q=q, k0=k0, k1=k1, n_tok=4, acc=acc, weight=1.0)
            base.update(kw)
            return ops._token_maps_array([ops.TokenMaps(**base)], 2)
        arr = tm()
        assert (arr[0].nq, arr[0].n0, arr[0].n1, arr[0].n_tok, arr[0].ldq, arr[0].ldk) == (64, 8, 64, 4, 256, 256)
        assert tm(k1=None)[0].n1 == 0 and tm(k1=None)[0].k1 is None
        assert tm(n_tok=None, acc=torch.zeros(8, 64))[0].n_tok == 8
        with pytest.raises(ValueError, match="dtype"):
            tm(q=q.float())
        with pytest.raises(ValueError, match="dtype"):
            tm(acc=acc.double())
        with pytest.raises(ValueError, match="num_heads\\*128 = 256 columns"):
            tm(q=_bf(64, 128))
        with pytest.raises(ValueError, match="num_heads\\*128 = 256 columns"):
            tm(k1=_bf(64, 384))
        with pytest.raises(ValueError, match="share one row stride"):
            tm(k1=_bf(64, 512)[:, :256])
        with pytest.raises(ValueError, match="innermost dimension must be contiguous"):
            tm(q=torch.zeros(256, 64, dtype=torch.bfloat16).T)
        with pytest.raises(ValueError, match="n0 <= 512"):
            tm(k0=_bf(513))
        with pytest.raises(ValueError, match="n_tok = 9"):
            tm(n_tok=9, acc=torch.zeros(9, 64))
        with pytest.raises(ValueError, match="n_tok = 0"):
            tm(n_tok=0, acc=torch.zeros(0, 64))
        with pytest.raises(ValueError, match="needs acc or acc2"):
            tm(acc=None)
        with pytest.raises(ValueError, match=r"acc must be contiguous fp32 \[4, 64\]"):
            tm(acc=torch.zeros(64, 4))
        with pytest.raises(ValueError, match=r"acc2 must be contiguous fp32 \[4, 64\]"):
            tm(acc2=torch.zeros(4, 128)[:, :64])
        with pytest.raises(ValueError, match=r"lse must be contiguous fp32 \[2, 64\]"):
            tm(lse=torch.zeros(3, 64))
        with pytest.raises(ValueError, match="does not fit the library's int32_t"):
            tm(q=torch.zeros(256, dtype=torch.bfloat16).as_strided((1, 256), (2 ** 31, 1)), acc=torch.zeros(4, 1))
        with pytest.raises(ValueError, match="also an accumulator of problem 0"):
            ops._token_maps_array([ops.TokenMaps(q, k0, k1, 4, acc=acc), ops.TokenMaps(q, k0, k1, 4, acc2=acc)], 2)
        with pytest.raises(ValueError, match="also an accumulator of problem 0"):
            tm(acc2=acc)
    finally:
        ops._chk = real
    with pytest.raises(ValueError, match="CUDA"):
        ops.token_maps([ops.TokenMaps(q, k0, k1, 4, acc=acc)], 2)
    for bad in (dict(problems=[]), dict(num_heads=0), dict(scale_log2=float("nan"))):
        kw = dict(problems=[ops.TokenMaps(q, k0, k1, 4, acc=acc)], num_heads=2)
        kw.update(bad)
        with pytest.raises(ValueError, match="token_maps: "):
            ops.token_maps(**kw)
