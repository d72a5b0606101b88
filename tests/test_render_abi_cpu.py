"""CPU-only checks of ca_heatmap_render's boundary: the entry and its problem struct are declared, bound and exported field
for field, the limits are the binding's, every limit is enforced with the entry's name in the error text before any launch,
and ops.heatmap_render's own checks raise without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
from conceptattention_amd import _lib as L
from conceptattention_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CT = {"void*": ctypes.c_void_p, "float*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return L.load()


def _header() -> str:
    return open(os.path.join(ROOT, "include", "conceptattn.h")).read()


def test_entry_is_declared_bound_and_exported(lib):
    m = re.search(r"\bint ca_heatmap_render\s*\((.*?)\);", _header(), re.S)
    assert m and "ca_heatmap_render" in L.SIGNATURES and hasattr(lib, "ca_heatmap_render")
    assert lib.ca_version() == L.CA_VERSION >= 135
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    kinds = ["ptr" if "*" in p or p.startswith("ca_stream_t") else p.split()[0] for p in params]
    res, args = L.SIGNATURES["ca_heatmap_render"]
    assert res is ctypes.c_int and len(args) == len(kinds) == 10
    want = {"ptr": (ctypes.c_void_p, ctypes.POINTER(L.RenderProblem)), "int32_t": (ctypes.c_int32,), "float": (ctypes.c_float,)}
    for a, k in zip(args, kinds):
        assert a in want[k], (a, k)


def test_struct_layout_is_the_headers():
    text = _header()
    end = re.search(r"\}\s*ca_render_problem\s*;", text).start()
    body = re.sub(r"/\*.*?\*/", "", text[text.rfind("typedef struct {", 0, end) + len("typedef struct {"):end], flags=re.S)
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            m = re.match(r"(?:const\s+)?(void|float|int32_t|int64_t)\s*(\*?)\s*(\w+)$", decl)
            assert m, decl
            fields.append((m.group(3), _CT[m.group(1) + m.group(2)]))
    assert fields == list(L.RenderProblem._fields_)
    assert ctypes.sizeof(L.RenderProblem) == 72 and L.RenderProblem.range_in.offset == 24   # n_maps padded to 8 bytes


def test_constants_and_the_build():
    consts = dict((k, int(v)) for k, v in re.findall(r"#define CA_RENDER_(\w+) (\d+)", _header()))
    assert consts == {"MAX_PROBLEMS": L.RENDER_MAX_PROBLEMS, "MAX_MAPS": L.RENDER_MAX_MAPS, "MAX_CELLS": L.RENDER_MAX_CELLS,
                      "MAX_SIDE": L.RENDER_MAX_SIDE, "BILINEAR": L.RENDER_BILINEAR, "BLEND": L.RENDER_BLEND}
    assert (L.RENDER_MAX_PROBLEMS, L.RENDER_MAX_MAPS, L.RENDER_MAX_CELLS, L.RENDER_MAX_SIDE) == (16, 65536, 16384, 4096)
    assert L.RENDER_LUT_ROWS == 259
    from conceptattention_amd.csrc import build
    assert "ca_render.hip" in build.SOURCES
    assert {"-save-temps=obj", "-ffp-contract=off"} <= set(build.EXTRA_FLAGS["ca_render.hip"])
    assert callable(build.audit_render)


_KEEP = (ctypes.c_double * 64)()                       # a 16-byte aligned host address that is never dereferenced
_ADDR = (ctypes.addressof(_KEEP) + 15) & ~15


def _call(lib, n_problems=1, h=16, w=16, H=32, W=32, flags=0, alpha=0.5, lut=_ADDR, null=None, offset=None, **fields):
    """One call with host addresses: every call below must be rejected before a launch."""
    arr = (L.RenderProblem * max(n_problems, 1))()
    for p in arr:
        p.maps = p.range_in = p.range_out = p.image = p.out = _ADDR
        p.map_stride, p.n_maps, p.image_stride, p.out_stride = h * w, 2, 3 * W, 3 * H * W
        for k, v in fields.items():
            setattr(p, k, v)
        if null:
            setattr(p, null, None)
        if offset:
            setattr(p, offset[0], _ADDR + offset[1])
    return lib.ca_heatmap_render(arr, n_problems, h, w, H, W, lut, alpha, flags, None)


# name -> (arguments, what the error text must hold)
BAD = {
    "no-problems": (dict(n_problems=0), b"1..16"),
    "too-many-problems": (dict(n_problems=17), b"1..16"),
    "no-cells": (dict(h=0), b"16384"),
    "too-many-cells": (dict(h=128, w=129), b"16384"),
    "cells-overflowing-int32": (dict(h=1 << 16, w=1 << 16), b"16384"),
    "no-rows": (dict(H=0), b"4096"),
    "too-wide": (dict(W=4097), b"4096"),
    "unknown-flag": (dict(flags=4), b"1 | 2"),
    "alpha-above-one": (dict(flags=L.RENDER_BLEND, alpha=1.5), b"alpha"),
    "alpha-negative": (dict(flags=L.RENDER_BLEND, alpha=-0.25), b"alpha"),
    "alpha-nan": (dict(flags=L.RENDER_BLEND, alpha=float("nan")), b"alpha"),
    "no-lut": (dict(lut=None), b"lut"),
    "no-maps": (dict(n_maps=0), b"65536"),
    "too-many-maps": (dict(n_maps=65537), b"65536"),
    "stride-below-the-map": (dict(map_stride=255), b"255"),
    "out-stride-below-the-plane": (dict(out_stride=3071), b"3071"),
    "maps-null": (dict(null="maps"), b"non-null"),
    "range-out-null": (dict(null="range_out"), b"non-null"),
    "out-null": (dict(null="out"), b"non-null"),
    "maps-misaligned": (dict(offset=("maps", 2)), b"4-byte"),
    "range-in-misaligned": (dict(offset=("range_in", 1)), b"4-byte"),
    "range-out-misaligned": (dict(offset=("range_out", 2)), b"4-byte"),
    "blend-without-image": (dict(flags=L.RENDER_BLEND, null="image"), b"image"),
    "image-stride-below-the-row": (dict(flags=L.RENDER_BLEND | L.RENDER_BILINEAR, image_stride=95), b"95"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_arguments_are_rejected_without_a_gpu(lib, name):
    kw, text = BAD[name]
    assert _call(lib, **kw) == -1, name
    err = lib.ca_last_error()
    assert b"ca_heatmap_render" in err and text in err, err
    assert lib.ca_heatmap_render(None, 1, 16, 16, 16, 16, _ADDR, 0.0, 0, None) == -1


def test_the_wrappers_checks_run_without_a_device():
    lut = torch.zeros(259, 3, dtype=torch.uint8)
    ok = torch.zeros(2, 3, 8, 8)
    pic = torch.zeros(8, 8, 3, dtype=torch.uint8)
    bad = [
        (dict(groups=[]), "no groups"),
        (dict(lut=lut[:258]), "259"),
        (dict(lut=lut.float()), "dtype"),
        (dict(groups=[ok[:, 0].double()]), "dtype"),
        (dict(groups=[ok[:, 0, :, ::2]]), "contiguous"),
        (dict(groups=[ok[:, 0, :, :4]]), "contiguous"),
        (dict(groups=[ok[:, 0], torch.zeros(2, 8, 9)]), "groups.1."),
        (dict(groups=[torch.zeros(1, 128, 129)]), "16384"),
        (dict(size=4097), "4096"), (dict(size=(0, 8)), "4096"),
        (dict(images=pic), "alpha"), (dict(alpha=0.5), "alpha"),
        (dict(images=pic, alpha=1.5), "alpha"), (dict(images=pic, alpha=-0.1), "alpha"),
        (dict(images=[pic, pic], alpha=0.5), "2 images"),
        (dict(images=pic.float(), alpha=0.5), "dtype"),
        (dict(images=torch.zeros(8, 9, 3, dtype=torch.uint8), alpha=0.5), "images.0."),
        (dict(images=torch.zeros(8, 8, 4, dtype=torch.uint8)[:, :, :3], alpha=0.5), "images.0."),
        (dict(ranges=torch.zeros(3, 2)), "ranges"), (dict(ranges=torch.zeros(2, dtype=torch.float64)), "dtype"),
        (dict(out=[]), "0 out"),
        (dict(out=[torch.zeros(2, 8, 8, 4, dtype=torch.uint8)[..., :3]]), "out.0."),
        (dict(out=[torch.zeros(3, 8, 8, 3, dtype=torch.uint8)]), "out.0."),
    ]
    for kw, text in bad:
        args = dict(groups=[ok[:, 0]], lut=lut)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            ops.heatmap_render(args.pop("groups"), args.pop("lut"), **args)
    with pytest.raises(ValueError, match="CUDA"):                      # and with nothing else wrong, the device
        ops.heatmap_render([ok[:, 0]], lut)
    with pytest.raises(ValueError, match="65536"):
        ops.heatmap_render([torch.zeros(1, 1, 1).expand(65537, 1, 1)], lut)


def test_colormap_lut_on_the_host():
    import render_cases as R
    for name in ("plasma", "inferno", "jet"):
        t = ops.colormap_lut(name, "cpu")
        assert t.dtype == torch.uint8 and np.array_equal(t.numpy(), R.cmap_lut(name))
        assert ops.colormap_lut(name, "cpu") is t                      # cached per name and device
    import matplotlib
    assert np.array_equal(ops.colormap_lut(matplotlib.colormaps["jet"], "cpu").numpy(), R.cmap_lut("jet"))
    syn = R.synthetic_lut()
    assert np.array_equal(ops.colormap_lut(syn, "cpu").numpy(), syn)
    assert np.array_equal(ops.colormap_lut(torch.from_numpy(syn), "cpu").numpy(), syn)
    with pytest.raises(ValueError):
        ops.colormap_lut(syn[:256], "cpu")
    with pytest.raises(ValueError):
        ops.colormap_lut(syn.astype(np.int32), "cpu")
    with pytest.raises(ValueError):
        ops.colormap_lut(matplotlib.colormaps["jet"].resampled(16), "cpu")
