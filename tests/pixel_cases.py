"""Cases and restatements of the two pixel I/O kernels of ca_pixels.hip (no GPU needed to import).

Both kernels are DEFINED by a torch expression and compared bit for bit, so there is no tolerance here: the numpy
restatements below spell the same fp32 operations out one rounding at a time, tests/test_pixel_cases_cpu.py checks them
against torch on the CPU, and tests/test_pixel_kernels_gpu.py checks the kernels against torch.

ca_pixels_u8_to_nhwc32_bf16:  f = float(byte) / 255 (an IEEE division), v = 2 f - 1 (2 f is exact, one rounding in the
subtraction), bf16 round-to-nearest-even; the source pixel is the one torch's interpolate(mode="nearest") reads:
min(int(floor(y * scale)), n_in - 1) with scale = float32(n_in) / float32(n_out) and the product in fp32.

ca_nhwc_f32_to_pixels_u8:  v = min(max(x, -1), 1); s = v + 1 (rounded); p = 127.5 s (rounded); byte = trunc(p).  The values
of F32_SPECIALS are those where one of the two roundings decides the byte.
"""
import numpy as np
import torch

ENTRIES = ("ca_pixels_u8_to_nhwc32_bf16", "ca_nhwc_f32_to_pixels_u8")

# (H0, W0, H, W): source and destination sizes
RESIZE_CASES = [
    (16, 16, 16, 16),      # identity
    (5, 7, 16, 24),        # upsample by non-integer factors (5/16 exact, 7/24 not representable)
    (33, 17, 16, 8),       # downsample
    (1, 1, 8, 8),          # a single source pixel
    (3, 1000, 8, 1024),    # a long row: an index where the fp32 product matters
    (7, 9, 8, 30),         # 9/30 = 0.3 is not representable: x * 0.3f lands on both sides of integers
]


# ---- grid wrap: both kernels launch at most PIX_MAX_BLOCKS = 2048 workgroups (ca_pixels.hip:8, 54, 124) of 256 threads and
# walk the rest with the grid's stride.  A thread of the input kernel owns a quarter of a pixel (one 16-byte store), a
# thread of the output kernel 16 output bytes.
PIXEL_GRID_CAP = 2048 * 256
# op -> (threads' worth of work, the cap in threads, threads per workgroup, the case itself)
WRAP_CASES = {
    "pixels_to_nhwc32": (514 * 257 * 4, PIXEL_GRID_CAP, 256, dict(h0=37, w0=53, h=514, w=257)),     # non-integer factors
    "nhwc_to_pixels": ((2797571 * 3 + 15) // 16, PIXEL_GRID_CAP, 256, dict(pixels=2797571)),         # 9 bytes behind the last unit
}
PRODUCT_RESIZE = (375, 500, 1024, 1024)      # an evaluation image into the product's size: eight trips through the loop


def nearest_index(n_out: int, n_in: int) -> np.ndarray:
    """int64 [n_out]: the source index of every destination index, in fp32 as torch computes it."""
    scale = np.float32(n_in) / np.float32(n_out)
    prod = np.arange(n_out, dtype=np.float32) * scale            # one fp32 multiply
    return np.minimum(np.floor(prod).astype(np.int64), n_in - 1)


def source_image(h0: int, w0: int, seed: int = 0) -> np.ndarray:
    """uint8 [h0, w0, 3]; the 16 x 16 one holds all 256 byte values in every channel (in three different orders)."""
    if (h0, w0) == (16, 16):
        a = np.arange(256, dtype=np.int64)
        return np.stack([a, 255 - a, (a * 7 + 3) % 256], -1).reshape(16, 16, 3).astype(np.uint8)
    rng = np.random.default_rng(1000 * h0 + w0 + seed)
    return rng.integers(0, 256, size=(h0, w0, 3), dtype=np.uint8)


def u8_to_nhwc32_reference(src: np.ndarray, h: int, w: int) -> torch.Tensor:
    """bf16 [h, w, 32], one rounding per line."""
    f = src.astype(np.float32) / np.float32(255.0)
    v = np.float32(2.0) * f - np.float32(1.0)
    v = v[nearest_index(h, src.shape[0])][:, nearest_index(w, src.shape[1])]
    out = torch.zeros(h, w, 32, dtype=torch.bfloat16)
    out[:, :, :3] = torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16)
    return out


def u8_to_nhwc32_torch(src: np.ndarray, h: int, w: int, device="cpu") -> torch.Tensor:
    """bf16 [h, w, 3]: the route the kernel replaces -- the conversion on the host, interpolate on ``device``, the cast."""
    arr = torch.from_numpy(src).permute(2, 0, 1).float() / 255.0
    arr = torch.nn.functional.interpolate((2.0 * arr - 1.0)[None].to(device), (h, w))
    return arr[0].permute(1, 2, 0).to(torch.bfloat16)


ULP1 = float(np.spacing(np.float32(1.0)))   # 2^-23
F32_SPECIALS = [
    1.0, -1.0, 1.0 + ULP1, -1.0 - ULP1, 3.5, -7.0, float("inf"), float("-inf"),     # the clamp
    -0.0, 0.0,                                                                      # 127.5 -> 127
    2.0 ** -25, -(2.0 ** -25),              # v + 1 rounds to 1 (a tie, to even) / is 1 - 2^-25 exactly: 127 both
    1.0 - 2.0 ** -24,                       # v + 1 = 2 - 2^-24 is a tie and rounds to 2: 255, where exact arithmetic gives 254
    1.0 - 2.0 ** -23,                       # v + 1 = 2 - 2^-23 exactly: 127.5 * that rounds to 255 - 2^-16: 254
    2.0 / 255.0 - 1.0, 4.0 / 255.0 - 1.0,   # around byte boundaries
    1.0 / 127.5 - 1.0, 0.00392156862, 0.0039215689, 0.5, -0.5, 0.99607843, 0.9960785,
]


def f32_values(b: int, h: int, w: int, ld: int) -> np.ndarray:
    """fp32 [b, h, w, ld]: the specials, then an ascending ramp over [-1.25, 1.25]; columns >= 3 hold a poison value that
    would show in the bytes if it were read."""
    n = b * h * w * 3
    vals = np.empty(n, dtype=np.float32)
    k = len(F32_SPECIALS)
    assert n > k + 16
    vals[:k] = np.array(F32_SPECIALS, dtype=np.float32)
    vals[k:] = np.linspace(-1.25, 1.25, n - k, dtype=np.float32)
    x = np.full((b, h, w, ld), 0.123, dtype=np.float32)
    x[..., :3] = vals.reshape(b, h, w, 3)
    return x


def f32_to_u8_reference(x: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] of fp32 [..., ld >= 3], one rounding per line."""
    v = np.minimum(np.maximum(x[..., :3].astype(np.float32), np.float32(-1.0)), np.float32(1.0))
    s = v + np.float32(1.0)
    p = np.float32(127.5) * s
    return np.trunc(p).astype(np.uint8)


def f32_to_u8_torch(x: torch.Tensor) -> torch.Tensor:
    """The expression the kernel replaces, on x's device."""
    return (127.5 * (x[..., :3].clamp(-1, 1) + 1.0)).byte()
