"""The two pixel I/O kernels of ca_pixels.hip on the GPU, bit for bit against the torch expressions they are defined by
(tests/pixel_cases.py): no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pixel_cases as T  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
POISON = -3.0   # bf16-representable; a destination element nobody wrote still holds it


def _run(src_dev, h, w):
    dst = torch.full((h, w, 32), POISON, device=DEV, dtype=torch.bfloat16)
    ops.pixels_to_nhwc32(src_dev, dst)
    return dst.cpu()


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
