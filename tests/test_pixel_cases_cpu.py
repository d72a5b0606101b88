"""CPU checks of tests/pixel_cases.py: the numpy restatements of both pixel kernels equal the torch expressions the
kernels are defined by, the nearest-index rule equals torch.nn.functional.interpolate for every size of the table, and
the two entry points are declared, bound, exported and reject bad arguments under their own names."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import pixel_cases as T
from conceptattention_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_table_holds_the_cases_the_kernel_can_go_wrong_at():
    assert T.RESIZE_CASES[:5] == [(16, 16, 16, 16), (5, 7, 16, 24), (33, 17, 16, 8), (1, 1, 8, 8), (3, 1000, 8, 1024)]
    img = T.source_image(16, 16)
    for c in range(3):
        assert sorted(img[:, :, c].reshape(-1).tolist()) == list(range(256))


def test_wrap_cases_exceed_the_cap_by_a_workgroup_and_by_less_than_a_quarter():
    src = open(os.path.join(ROOT, "conceptattention_amd", "csrc", "ca_pixels.hip")).read()
    assert "#define PIX_MAX_BLOCKS 2048" in src and src.count("if (blocks > PIX_MAX_BLOCKS) blocks = PIX_MAX_BLOCKS;") == 2
    assert T.PIXEL_GRID_CAP == 2048 * 256 and set(T.WRAP_CASES) == {"pixels_to_nhwc32", "nhwc_to_pixels"}
    for op, (units, cap, per_wg, case) in T.WRAP_CASES.items():
        assert cap + per_wg <= units < cap + cap // 4, (op, units, cap)
    c = T.WRAP_CASES["pixels_to_nhwc32"][3]
    assert c["h"] * c["w"] > 131072 and c["h"] % c["h0"] and c["w"] % c["w0"]              # a non-integer resize
    n = T.WRAP_CASES["nhwc_to_pixels"][3]["pixels"]
    assert n > 2796203 and (n * 3) % 16 == 9                                                 # a tail behind the last unit
    h0, w0, h, w = T.PRODUCT_RESIZE
    assert h * w * 4 == 8 * T.PIXEL_GRID_CAP


@pytest.mark.parametrize("h0,w0,h,w", T.RESIZE_CASES + [(37, 53, 514, 257), T.PRODUCT_RESIZE])
def test_nearest_index_rule_is_interpolates(h0, w0, h, w):
    """An image that holds its own pixel indices, resized by torch on the CPU, names the source pixel of every
    destination pixel."""
    idx = torch.arange(h0 * w0, dtype=torch.float32).view(1, 1, h0, w0)
    got = torch.nn.functional.interpolate(idx, (h, w))[0, 0].numpy().astype(np.int64)
    want = T.nearest_index(h, h0)[:, None] * w0 + T.nearest_index(w, w0)[None, :]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("h0,w0,h,w", T.RESIZE_CASES)
def test_u8_restatement_equals_the_torch_route(h0, w0, h, w):
    src = T.source_image(h0, w0)
    ref = T.u8_to_nhwc32_reference(src, h, w)
    assert torch.equal(ref[:, :, :3], T.u8_to_nhwc32_torch(src, h, w))
    assert not ref[:, :, 3:].any()


def test_the_division_is_not_a_reciprocal_multiply():
    """What "correctly rounded" buys: x * (1 / 255) differs from x / 255 in fp32 for some bytes, and the difference
    survives into bf16 for none or some of them -- the kernel must not depend on which."""
    b = np.arange(256, dtype=np.float32)
    assert (b / np.float32(255.0) != b * (np.float32(1.0) / np.float32(255.0))).any()


def test_f32_restatement_equals_the_torch_expression_and_the_specials_decide():
    for ld in (3, 32):
        x = T.f32_values(2, 3, 5, ld)
        assert np.array_equal(T.f32_to_u8_reference(x), T.f32_to_u8_torch(torch.from_numpy(x)).numpy())
    one = lambda v: int(T.f32_to_u8_reference(np.array([[v, v, v]], dtype=np.float32))[0, 0])   # noqa: E731
    assert one(1.0) == one(1.0 + T.ULP1) == one(np.inf) == 255 and one(-1.0) == one(-1.0 - T.ULP1) == one(-np.inf) == 0
    assert one(0.0) == one(-0.0) == one(2.0 ** -25) == 127
    assert one(1.0 - 2.0 ** -24) == 255                     # v + 1 rounds up to 2
    assert int(np.trunc(127.5 * (np.float64(np.float32(1.0 - 2.0 ** -24)) + 1.0))) == 254   # exact arithmetic would not
    assert one(1.0 - 2.0 ** -23) == 254
    ramp = T.f32_to_u8_reference(T.f32_values(2, 3, 5, 3)).reshape(-1)[len(T.F32_SPECIALS):]
    assert (np.diff(ramp.astype(np.int64)) >= 0).all() and ramp[0] == 0 and ramp[-1] == 255


# ---------------------------------------------------------------------------------------------------------- the ABI
@pytest.fixture(scope="module")
def lib():
    entry.build()
    return L.load()


def test_both_entries_are_declared_bound_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "conceptattn.h")).read()
    declared = set(re.findall(r"\b(ca_[a-z0-9_]+)\s*\(", text))
    for name in T.ENTRIES:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    src = open(os.path.join(ROOT, "conceptattention_amd", "csrc", "ca_pixels.hip")).read()
    assert sorted(re.findall(r'extern "C" int (ca_\w+)\(', src)) == sorted(T.ENTRIES)      # both live in the new unit
    from conceptattention_amd.csrc import build
    assert "ca_pixels.hip" in build.SOURCES
    assert {"-save-temps=obj", "-ffp-contract=off"} <= set(build.EXTRA_FLAGS["ca_pixels.hip"])
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in T.ENTRIES:
        assert f"lib.{name}.argtypes" in doc, name


def test_a_rejected_call_is_reported_under_its_own_name(lib):
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15            # a 16-byte aligned non-null address; nothing is ever launched

    def to_plane(**kw):
        a = dict(src=p, stride=3 * 7, dst=p, H0=5, W0=7, H=16, W=24)
        a.update(kw)
        return lib.ca_pixels_u8_to_nhwc32_bf16(a["src"], a["stride"], a["dst"], a["H0"], a["W0"], a["H"], a["W"], None)
    for bad in (dict(src=None), dict(dst=None), dict(H0=0), dict(W0=0), dict(H=0), dict(W=-1), dict(stride=20),
                dict(dst=p + 8), dict(dst=p + 2), dict(H=2 ** 24 + 1)):
        assert to_plane(**bad) == -1, bad
        assert b"ca_pixels_u8_to_nhwc32_bf16" in lib.ca_last_error()
    assert to_plane(H0=1, stride=5, src=None) == -1      # (a one-row image's stride is unused: only the null pointer is rejected)

    def to_bytes(**kw):
        a = dict(src=p, ld=3, dst=p, pixels=30)
        a.update(kw)
        return lib.ca_nhwc_f32_to_pixels_u8(a["src"], a["ld"], a["dst"], a["pixels"], None)
    for bad in (dict(src=None), dict(dst=None), dict(ld=2), dict(ld=0), dict(pixels=0), dict(pixels=-4), dict(src=p + 2),
                dict(dst=p + 4), dict(pixels=2 ** 41)):
        assert to_bytes(**bad) == -1, bad
        assert b"ca_nhwc_f32_to_pixels_u8" in lib.ca_last_error()


def test_wrappers_reject_bad_tensors_before_any_launch():
    from conceptattention_amd import ops
    with pytest.raises(ValueError):
        ops.pixels_to_nhwc32(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(8, 8, 32, dtype=torch.bfloat16))   # host
    with pytest.raises(ValueError):
        ops.nhwc_to_pixels(torch.zeros(1, 4, 4, 3), torch.zeros(1, 4, 4, 3, dtype=torch.uint8))                     # host
