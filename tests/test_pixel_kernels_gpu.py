"""The two pixel I/O kernels of ca_pixels.hip on the GPU, bit for bit against the torch expressions they are defined by
(tests/pixel_cases.py): no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pixel_cases as T  # noqa: E402
import placement  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
POISON = -3.0   # bf16-representable; a destination element nobody wrote still holds it


def _run(src_dev, h, w):
    dst = torch.full((h, w, 32), POISON, device=DEV, dtype=torch.bfloat16)
    ops.pixels_to_nhwc32(src_dev, dst)
    return dst.cpu()


def run_to_nhwc32(case, alloc=None):
    """One resize case with its two buffers from an optional allocator (tests/placement.py), checked bit for bit;
    returns a clone of the plane.  tests/test_address_range_gpu.py runs it at chosen addresses."""
    h0, w0, h, w = case
    al = alloc or placement.Plain(DEV)
    src = T.source_image(h0, w0)
    sd = al.to(torch.from_numpy(src), {"src": None})
    dst = al.full((h, w, 32), POISON, torch.bfloat16, {"dst": None})
    ops.pixels_to_nhwc32(sd, dst)
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), T.u8_to_nhwc32_reference(src, h, w)), case
    assert np.array_equal(sd.cpu().numpy(), src), "the source changed"
    return {"dst": dst.clone()}


def run_to_pixels(case, alloc=None):
    """(b, h, w, ld): the decoder's plane to bytes, the buffers from an optional allocator, checked bit for bit."""
    b, h, w, ld = case
    al = alloc or placement.Plain(DEV)
    x = T.f32_values(b, h, w, ld)
    xd = al.to(torch.from_numpy(x), {"src": None})
    out = al.full((b, h, w, 3), 77, torch.uint8, {"dst": None})
    ops.nhwc_to_pixels(xd, out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), T.f32_to_u8_reference(x)), case
    assert np.array_equal(xd.cpu().numpy(), x), "the source changed"
    return {"dst": out.clone()}


@pytest.mark.parametrize("h0,w0,h,w", T.RESIZE_CASES)
def test_u8_to_nhwc32_equals_the_torch_route_bit_for_bit(h0, w0, h, w):
    src = T.source_image(h0, w0)
    got = _run(torch.from_numpy(src).to(DEV), h, w)
    assert torch.equal(got[:, :, :3], T.u8_to_nhwc32_torch(src, h, w, DEV).cpu())      # interpolate on the device, as today
    assert torch.equal(got, T.u8_to_nhwc32_reference(src, h, w))                        # and channels 3..31 are zeros


def test_u8_to_nhwc32_reads_a_source_with_a_padded_row_stride():
    h0, w0, h, w = 5, 7, 16, 24
    src = T.source_image(h0, w0)
    wide = torch.full((h0, w0 + 3, 3), 199, dtype=torch.uint8)     # 9 bytes of padding behind every row
    wide[:, :w0] = torch.from_numpy(src)
    view = wide.to(DEV)[:, :w0]
    assert view.stride(0) == 3 * (w0 + 3) and not view.is_contiguous()
    assert torch.equal(_run(view, h, w), T.u8_to_nhwc32_reference(src, h, w))


def test_u8_to_nhwc32_rejects_a_view_whose_channels_are_not_adjacent_and_takes_a_one_row_image():
    dst = torch.zeros(8, 8, 32, device=DEV, dtype=torch.bfloat16)
    gray = torch.arange(16, dtype=torch.uint8, device=DEV).view(4, 4, 1).expand(4, 4, 3)     # channel stride 0
    with pytest.raises(ValueError):
        ops.pixels_to_nhwc32(gray, dst)
    planar = torch.zeros(3, 4, 4, dtype=torch.uint8, device=DEV).permute(1, 2, 0)            # channel stride 16
    with pytest.raises(ValueError):
        ops.pixels_to_nhwc32(planar, dst)
    src = T.source_image(1, 9)
    row = torch.from_numpy(src).to(DEV).as_strided((1, 9, 3), (5, 3, 1))                     # one row, an odd row stride
    assert torch.equal(_run(row, 8, 8), T.u8_to_nhwc32_reference(src, 8, 8))


def test_u8_to_nhwc32_writes_its_slot_of_a_plane_and_nothing_else():
    h0, w0, h, w = 33, 17, 16, 8
    src = T.source_image(h0, w0)
    plane = torch.full((3, h, w, 32), POISON, device=DEV, dtype=torch.bfloat16)
    ops.pixels_to_nhwc32(torch.from_numpy(src).to(DEV), plane[2])
    got = plane.cpu()
    assert (got[:2] == POISON).all()                                 # the neighbours in front are untouched
    assert torch.equal(got[2], T.u8_to_nhwc32_reference(src, h, w))  # (channels 3..31 zero on the poisoned plane)
    plane = torch.full((3, h, w, 32), POISON, device=DEV, dtype=torch.bfloat16)
    ops.pixels_to_nhwc32(torch.from_numpy(src).to(DEV), plane[1])
    got = plane.cpu()
    assert (got[0] == POISON).all() and (got[2] == POISON).all()     # and the one behind


@pytest.mark.parametrize("ld", [3, 32])
def test_f32_to_u8_equals_the_torch_expression_on_the_device_and_on_the_cpu(ld):
    x = T.f32_values(2, 3, 5, ld)
    xd = torch.from_numpy(x).to(DEV)
    out = torch.full((2, 3, 5, 3), 77, device=DEV, dtype=torch.uint8)
    ops.nhwc_to_pixels(xd, out)
    got = out.cpu()
    assert torch.equal(got, T.f32_to_u8_torch(xd).cpu())                     # the expression evaluated on the device
    assert torch.equal(got, T.f32_to_u8_torch(torch.from_numpy(x)))          # and on the CPU
    assert np.array_equal(got.numpy(), T.f32_to_u8_reference(x))


def test_f32_to_u8_full_units_of_sixteen_bytes_and_the_tail_behind_them():
    """The kernel's unit is 16 output bytes.  30 pixels above are 5 units and a tail of 10 bytes; 149 pixels = 447 bytes are
    27 units and 15 bytes, 16 pixels = 48 bytes are 3 units and no tail, 5 pixels a tail alone; the bytes behind the last
    pixel stay as they were.  A source that is not 16-byte aligned takes the pixel-by-pixel walk at ld = 3 as well."""
    for n in (16 * 9 + 5, 16, 5):
        x = np.linspace(-1.1, 1.1, n * 3, dtype=np.float32).reshape(n, 3)
        for shift in (0, 1):
            src = torch.zeros(n * 3 + 4, device=DEV)
            src[shift:shift + n * 3] = torch.from_numpy(x).to(DEV).view(-1)
            buf = torch.full((n * 3 + 16,), 77, device=DEV, dtype=torch.uint8)
            ops.nhwc_to_pixels(src[shift:shift + n * 3].view(n, 3), buf[: n * 3].view(n, 3))
            got = buf.cpu().numpy()
            assert np.array_equal(got[: n * 3].reshape(n, 3), T.f32_to_u8_reference(x)), (n, shift)
            assert (got[n * 3:] == 77).all(), (n, shift)


def test_u8_to_nhwc32_grid_wrap_between_two_poisoned_neighbours():
    """514 x 257 pixels are 16 workgroups more than the 2048 of the capped grid: their threads take a second 16-byte unit.
    37 x 53 -> 514 x 257 are non-integer factors both ways.  The slot in the middle of three: the wrap writes nothing of
    the neighbours."""
    c = T.WRAP_CASES["pixels_to_nhwc32"][3]
    h0, w0, h, w = c["h0"], c["w0"], c["h"], c["w"]
    src = T.source_image(h0, w0)
    ref = T.u8_to_nhwc32_reference(src, h, w)
    assert torch.equal(_run(torch.from_numpy(src).to(DEV), h, w), ref)
    plane = torch.full((3, h, w, 32), POISON, device=DEV, dtype=torch.bfloat16)
    ops.pixels_to_nhwc32(torch.from_numpy(src).to(DEV), plane[1])
    assert (plane[0] == POISON).all() and (plane[2] == POISON).all()
    assert torch.equal(plane[1].cpu(), ref)


def test_u8_to_nhwc32_at_the_products_size():
    """375 x 500 into 1024 x 1024: every thread walks the loop eight times."""
    h0, w0, h, w = T.PRODUCT_RESIZE
    run_to_nhwc32((h0, w0, h, w))


@pytest.mark.parametrize("ld", [3, 32])
def test_f32_to_u8_grid_wrap(ld):
    """2 797 571 pixels are 524 545 units of 16 bytes, 257 more than the capped grid's threads, and 9 bytes behind the
    last unit.  ld = 3 and an aligned source: the packed kernel; ld = 32: the pixel-by-pixel walk.  The bytes behind the
    last pixel stay as they were."""
    n = T.WRAP_CASES["nhwc_to_pixels"][3]["pixels"]
    x = T.f32_values(1, 1, n, 3).reshape(n, 3)
    src = torch.full((n, ld), 0.123, device=DEV)
    src[:, :3] = torch.from_numpy(x).to(DEV)
    assert src.data_ptr() % 16 == 0
    buf = torch.full((n * 3 + 16,), 77, device=DEV, dtype=torch.uint8)
    ops.nhwc_to_pixels(src, buf[: n * 3].view(n, 3))
    got = buf.cpu().numpy()
    assert np.array_equal(got[: n * 3].reshape(n, 3), T.f32_to_u8_reference(x))
    assert (got[n * 3:] == 77).all()
