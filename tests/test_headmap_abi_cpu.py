"""CPU-only checks of ca_head_maps' boundary: the entry is declared, bound and exported, the ctypes struct matches the
header field for field, CA_VERSION agrees in the header, the binding and the header's version comment, every argument
rule is reported with the entry's name in ca_last_error before anything is launched (the calls below carry host addresses
that are never dereferenced), ops.head_maps raises for each Python-side rule, and the source is part of the build with the
no-spill audit."""
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
    return open(os.path.join(CSRC, "ca_headmap.h")).read()


def test_entry_is_declared_bound_and_exported(lib):
    m = re.search(r"\bint ca_head_maps\s*\((.*?)\);", _decl(), re.S)
    assert m and "ca_head_maps" in L.INTERNAL_SIGNATURES and hasattr(lib, "ca_head_maps")
    params = [p.strip().split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert params == ["problems", "n_problems", "L", "C", "num_heads", "norm", "stream"]
    res, args = L.INTERNAL_SIGNATURES["ca_head_maps"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(L.HeadmapProblem)] + [ctypes.c_int32] * 5 + [ctypes.c_void_p]
    assert lib.ca_head_maps.argtypes == args and lib.ca_head_maps.restype is ctypes.c_int
    assert not set(L.INTERNAL_SIGNATURES) & set(L.SIGNATURES)
    assert "ca_head_maps" not in open(os.path.join(ROOT, "include", "conceptattn.h")).read()


def test_the_version_agrees_in_all_three_places(lib):
    public = open(os.path.join(ROOT, "include", "conceptattn.h")).read()
    version = int(re.search(r"#define CA_VERSION (\d+)", public).group(1))
    assert version == L.CA_VERSION == lib.ca_version() >= 137
    comment = re.search(r"#define CA_VERSION \d+ /\*(.*?)\*/", public, re.S).group(1)
    last = re.findall(r"\b(1[23]\d):", comment)[-1]
    assert int(last) == version and re.search(rf"{version}: per-head concept maps", comment)


def test_the_struct_matches_the_header_field_for_field():
    body = re.search(r"typedef struct ca_headmap_problem \{(.*?)\} ca_headmap_problem;", _decl(), re.S).group(1)
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
    assert fields == [(n, t) for n, t in L.HeadmapProblem._fields_], fields
    assert ctypes.sizeof(L.HeadmapProblem) == 5 * 8 + 8 * 4
    for name, value in (("CA_NORM_NONE", L.NORM_NONE), ("CA_HEADMAP_MAX_HEADS", L.HEADMAP_MAX_HEADS)):
        assert int(re.search(rf"#define {name} (\d+)", _decl()).group(1)) == value
    assert L.NORM_NONE not in L.NORMS.values() and L.NORM_NONE == 3


def test_the_build_and_the_documents():
    from conceptattention_amd.csrc import build
    assert "ca_headmap.hip" in build.SOURCES and "ca_headmap.h" in build.HEADERS
    assert "-save-temps=obj" in build.EXTRA_FLAGS["ca_headmap.hip"]
    assert callable(build.audit_headmap)
    src = open(os.path.join(CSRC, "build.py")).read()
    assert '_audit_no_spill("ca_headmap", asm_path)' in src
    assert re.search(r'audit_headmap\(os\.path\.join\(HERE, "ca_headmap-hip-amdgcn-amd-amdhsa-gfx950\.s"\)\)', src)
    kernel = open(os.path.join(CSRC, "ca_headmap.hip")).read()
    assert "hm_softmax_terms<" in kernel and "hm_sparse_terms<" in kernel      # the shared weighting, called as it stands
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Per-head maps" in doc and "ca_head_maps" in doc


_KEEP = (ctypes.c_double * 64)()                       # a 16-byte aligned host address that is never dereferenced
_ADDR = (ctypes.addressof(_KEEP) + 15) & ~15


def _call(lib, n_problems=1, Lp=64, Cc=4, num_heads=2, norm=0, null=(), offset=None, array=True, same=None, **fields):
    arr = (L.HeadmapProblem * max(n_problems, 1))()
    for i, p in enumerate(arr):
        p.img = p.con = _ADDR
        p.heads, p.acc, p.acc2 = _ADDR + 64 + 1024 * i, _ADDR + 128 + 1024 * i, _ADDR + 192 + 1024 * i
        p.ldi, p.ldc, p.img_f32, p.con_f32 = 256, 256, 0, 0
        p.weight_h = p.weight = p.weight2 = 1.0
        for k, v in fields.items():
            setattr(p, k, v)
        for k in null:
            setattr(p, k, None)
        if offset:
            setattr(p, offset[0], _ADDR + offset[1])
    if same:                                            # problem 1's `same[1]` is problem 0's `same[0]`
        setattr(arr[1], same[1], getattr(arr[0], same[0]))
    return lib.ca_head_maps(arr if array else None, n_problems, Lp, Cc, num_heads, norm, None)


# name -> (arguments, what the error text must hold); one violation at a time
BAD = {
    "no-array": (dict(array=False), b"bad arguments"),
    "no-problems": (dict(n_problems=0), b"n_problems=0"),
    "17-problems": (dict(n_problems=17), b"n_problems <= 16"),
    "no-patches": (dict(Lp=0), b"L=0"),
    "no-concepts": (dict(Cc=0), b"C=0"),
    "33-concepts": (dict(Cc=33), b"C <= 32"),
    "no-heads": (dict(num_heads=0), b"num_heads=0"),
    "too-many-heads": (dict(num_heads=65537), b"num_heads <= 65536"),
    "unknown-norm": (dict(norm=4), b"norm=4"),
    "negative-norm": (dict(norm=-1), b"norm=-1"),
    "no-img": (dict(null=("img",)), b"rows invalid"),
    "no-con": (dict(null=("con",)), b"rows invalid"),
    "img-misaligned": (dict(offset=("img", 8)), b"16-byte aligned"),
    "con-misaligned": (dict(offset=("con", 4)), b"16-byte aligned"),
    "img-dtype-flag": (dict(img_f32=2), b"img_f32=2"),
    "con-dtype-flag": (dict(con_f32=-1), b"con_f32=-1"),
    "img-stride-below-the-width": (dict(ldi=248), b"ldi=248"),
    "con-stride-below-the-width": (dict(ldc=248), b"ldc=248"),
    "bf16-img-stride-not-a-multiple-of-8": (dict(ldi=260), b"ldi=260"),
    "fp32-con-stride-not-a-multiple-of-4": (dict(ldc=258, con_f32=1), b"ldc=258"),
    "no-output": (dict(null=("heads", "acc", "acc2")), b"at least one of heads / acc / acc2"),
    "heads-misaligned": (dict(offset=("heads", 2)), b"4-byte aligned"),
    "acc2-misaligned": (dict(offset=("acc2", 1)), b"4-byte aligned"),
    "an-accumulator-of-two-problems": (dict(n_problems=2, same=("acc", "acc2")), b"shares an accumulator with problem 0"),
    "heads-of-two-problems": (dict(n_problems=2, same=("heads", "heads")), b"shares an accumulator with problem 0"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_arguments_are_rejected_without_a_gpu(lib, name):
    kw, text = BAD[name]
    assert _call(lib, **kw) == -1, name
    err = lib.ca_last_error()
    assert err.startswith(b"ca_head_maps: ") and text in err, err


def test_one_accumulator_named_twice_by_a_problem_is_rejected(lib):
    arr = (L.HeadmapProblem * 1)()
    p = arr[0]
    p.img = p.con = p.acc = p.acc2 = _ADDR
    p.ldi = p.ldc = 256
    assert lib.ca_head_maps(arr, 1, 64, 4, 2, 0, None) == -1
    assert b"names one accumulator twice" in lib.ca_last_error()


def _rows(rows, cols=256, dtype=torch.bfloat16):
    return torch.zeros(rows, cols, dtype=dtype)


def test_the_python_side_rules_are_checked_before_the_device_is_asked_for():
    """ops.head_maps' own ValueErrors.  The operands are host tensors: a rule that passed would end in _chk's "expected a
    CUDA(HIP) tensor", so each rule is checked on a _chk that lets host tensors through."""
    real = ops._chk
    ops._chk = ops._chk_host
    try:
        img, con = _rows(64), _rows(4)
        acc = torch.zeros(4, 64)

        def hm(num_heads=2, **kw):
            base = dict(img=img, con=con, acc=acc, weight=1.0)
            base.update(kw)
            return ops._head_maps_array([ops.HeadMaps(**base)], num_heads)
        arr, Lp, Cc = hm()
        assert (Lp, Cc, arr[0].ldi, arr[0].ldc, arr[0].img_f32, arr[0].con_f32) == (64, 4, 256, 256, 0, 0)
        arr, _, _ = hm(img=_rows(64, 264, torch.float32)[:, :256], con=_rows(4, dtype=torch.float32))
        assert (arr[0].ldi, arr[0].img_f32, arr[0].con_f32) == (264, 1, 1)
        assert hm(con=_rows(1), acc=torch.zeros(1, 64))[0][0].ldc == 256
        with pytest.raises(ValueError, match="dtype"):
            hm(img=img.half())
        with pytest.raises(ValueError, match="dtype"):
            hm(acc=acc.double())
        with pytest.raises(ValueError, match=r"num_heads\*128 = 256 columns \(hidden % 128 == 0\)"):
            hm(img=_rows(64, 200))
        with pytest.raises(ValueError, match=r"num_heads\*128 = 384 columns"):
            hm(num_heads=3)
        with pytest.raises(ValueError, match="innermost dimension must be contiguous"):
            hm(img=torch.zeros(256, 64, dtype=torch.bfloat16).T)
        with pytest.raises(ValueError, match="row stride 0 is below the width"):
            hm(img=_rows(1).expand(64, 256))                     # (more than one row at a stride below the width)
        with pytest.raises(ValueError, match="16-byte aligned"):
            hm(img=_rows(64, 260)[:, :256])                      # a bf16 row stride that is no multiple of 8
        with pytest.raises(ValueError, match="16-byte aligned"):
            hm(con=_rows(4, 258, torch.float32)[:, :256])        # an fp32 row stride that is no multiple of 4
        with pytest.raises(ValueError, match="16-byte aligned"):
            hm(img=_rows(65, 264).reshape(-1)[4:4 + 64 * 264].view(64, 264)[:, :256])   # the first row 8 bytes off
        with pytest.raises(ValueError, match="1 <= C <= 32"):
            hm(con=_rows(33), acc=torch.zeros(33, 64))
        with pytest.raises(ValueError, match="1 <= C <= 32"):
            hm(con=_rows(0), acc=torch.zeros(0, 64))
        with pytest.raises(ValueError, match="needs heads, acc or acc2"):
            hm(acc=None)
        with pytest.raises(ValueError, match=r"acc must be contiguous fp32 \[4, 64\]"):
            hm(acc=torch.zeros(64, 4))
        with pytest.raises(ValueError, match=r"acc2 must be contiguous fp32 \[4, 64\]"):
            hm(acc2=torch.zeros(4, 128)[:, :64])
        with pytest.raises(ValueError, match=r"heads must be contiguous fp32 \[2, 4, 64\]"):
            hm(heads=torch.zeros(3, 4, 64))
        with pytest.raises(ValueError, match="does not fit the library's int32_t"):
            hm(img=torch.zeros(256, dtype=torch.bfloat16).as_strided((1, 256), (2 ** 31, 1)), acc=torch.zeros(4, 1))
        with pytest.raises(ValueError, match="also an accumulator of problem 0"):
            ops._head_maps_array([ops.HeadMaps(img, con, acc=acc), ops.HeadMaps(img, con, acc2=acc)], 2)
        with pytest.raises(ValueError, match="also an accumulator of problem 0"):
            hm(acc2=acc)
        with pytest.raises(ValueError, match="share L and C"):
            ops._head_maps_array([ops.HeadMaps(img, con, acc=acc), ops.HeadMaps(_rows(32), con, acc=torch.zeros(4, 32))], 2)
    finally:
        ops._chk = real
    with pytest.raises(ValueError, match="CUDA"):
        ops.head_maps([ops.HeadMaps(img, con, acc=acc)], 2)
    for bad in (dict(problems=[]), dict(num_heads=0), dict(norm=7)):
        kw = dict(problems=[ops.HeadMaps(img, con, acc=acc)], num_heads=2, norm=L.NORM_NONE)
        kw.update(bad)
        with pytest.raises(ValueError, match="head_maps: "):
            ops.head_maps(**kw)
