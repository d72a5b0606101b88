"""ca_heatmap_render restated in numpy, one fp32 operation at a time (include/conceptattn.h states the same steps), and the
case lists the CPU twin (tests/test_render_cases_cpu.py) and the GPU test (tests/test_render_kernels_gpu.py) both run.

Every array below is float32 and every numpy operation on float32 arrays rounds once, as the kernel's operations do
(the unit is built with -ffp-contract=off); the bilinear source coordinate is the kernel's one fused operation (``fmaf``).
Nothing here needs a GPU or matplotlib, except ``cmap_lut``."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

F = np.float32
LUT_ROWS, ROW_UNDER, ROW_OVER, ROW_BAD = 259, 256, 257, 258


def synthetic_lut() -> np.ndarray:
    """259 distinct rows: an index that is off by one, or an under / over / bad mix-up, shows in the bytes (plasma has equal
    neighbouring rows)."""
    i = np.arange(LUT_ROWS)
    return np.stack([i & 255, i >> 8, 255 - (i & 255)], 1).astype(np.uint8)


def cmap_lut(name: str) -> np.ndarray:
    """What ops.colormap_lut uploads for a matplotlib name."""
    import matplotlib.pyplot as plt
    cmap = plt.get_cmap(name)
    rows = [cmap(np.arange(256))[:, :3]] + [np.asarray(cmap(v)).reshape(1, 4)[:, :3] for v in (-np.inf, np.inf, np.nan)]
    return (np.concatenate(rows) * 255).astype(np.uint8)


def group_range(planes: np.ndarray):
    """lo, hi over all cells of the group; both NaN if any cell is (ndarray.min / max propagate a NaN)."""
    with np.errstate(all="ignore"):
        lo, hi = F(planes.min()), F(planes.max())
    if np.isnan(lo) or np.isnan(hi):
        return F(np.nan), F(np.nan)
    return lo, hi


def fmaf(a, b, c) -> np.ndarray:
    """fp32 a * b + c in one rounding, for the bilinear source coordinate.  The product of two fp32 numbers is exact in fp64
    (48 bits).  Here a = h / H <= 2^14, so the product's last bit is at or below 2^-1 and adding c = -0.5 lengthens it by
    one bit at the most: the sum is exact in fp64 too, and the cast is the only rounding."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.float64(c)).astype(F)


def values(plane: np.ndarray, H: int, W: int, bilinear: bool) -> np.ndarray:
    """The fp32 value at every output pixel [H, W]."""
    h, w = plane.shape
    plane = plane.astype(F, copy=False)
    sy, sx = F(h) / F(H), F(w) / F(W)
    y, x = np.arange(H, dtype=F), np.arange(W, dtype=F)
    with np.errstate(all="ignore"):
        if not bilinear:
            iy = np.minimum(np.floor(y * sy).astype(np.int64), h - 1)
            ix = np.minimum(np.floor(x * sx).astype(np.int64), w - 1)
            return plane[iy[:, None], ix[None, :]]
        fy = np.maximum(fmaf(sy, y + F(0.5), F(-0.5)), F(0))
        fx = np.maximum(fmaf(sx, x + F(0.5), F(-0.5)), F(0))
        y0, x0 = fy.astype(np.int64), fx.astype(np.int64)
        assert y0.max() <= h - 1 and x0.max() <= w - 1
        y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
        ly, lx = (fy - y0.astype(F))[:, None], (fx - x0.astype(F))[None, :]
        hy, hx = F(1) - ly, F(1) - lx
        a00, a01 = plane[y0[:, None], x0[None, :]], plane[y0[:, None], x1[None, :]]
        a10, a11 = plane[y1[:, None], x0[None, :]], plane[y1[:, None], x1[None, :]]
        top = hx * a00 + lx * a01
        bot = hx * a10 + lx * a11
        v = hy * top + ly * bot
    assert v.dtype == F
    return v


def lut_rows(v: np.ndarray, lo, hi) -> np.ndarray:
    """matplotlib's Colormap._get_rgba_and_mask for a float array, as indices into the 259-row table."""
    with np.errstate(all="ignore"):
        t = (v - F(lo)) / (F(hi) - F(lo))
        xa = t * F(256)
    assert xa.dtype == F
    nan = np.isnan(xa)
    safe = np.where(nan | (xa < 0) | (xa >= 256), F(0), xa)
    row = safe.astype(np.int64)
    row = np.where(xa >= 256, ROW_OVER, row)
    row = np.where(xa == 256, 255, row)
    row = np.where(xa < 0, ROW_UNDER, row)
    return np.where(nan, ROW_BAD, row)


def blend(col: np.ndarray, img: np.ndarray, rows: np.ndarray, alpha: float) -> np.ndarray:
    a = F(alpha)
    b = F(1) - a
    f = col.astype(F) * a + img.astype(F) * b + F(0.5)
    assert f.dtype == F
    return np.where((rows == ROW_BAD)[..., None], img, f.astype(np.int32).astype(np.uint8))


def render(planes: np.ndarray, lut: np.ndarray, H: Optional[int] = None, W: Optional[int] = None, bilinear: bool = False,
           image: Optional[np.ndarray] = None, alpha: Optional[float] = None, given=None):
    """One group: (uint8 [n, H, W, 3], (lo, hi)).  ``given``: the {lo, hi} to use instead of the group's own range."""
    n, h, w = planes.shape
    H, W = (h if H is None else H), (w if W is None else W)
    lo, hi = group_range(planes) if given is None else (F(given[0]), F(given[1]))
    out = np.empty((n, H, W, 3), dtype=np.uint8)
    for k in range(n):
        rows = lut_rows(values(planes[k], H, W, bilinear), lo, hi)
        col = lut[rows]
        out[k] = col if image is None else blend(col, image, rows, alpha)
    return out, (lo, hi)


# ---- inputs.  A family is how the cells of a group are drawn; every one is seeded.
FAMILIES = ("heat", "signed", "distinct", "two", "constant", "nan", "inf", "negzero")


def planes_of(family: str, n: int, h: int, w: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if family == "heat":               # softmax-like: positive, a few large cells
        x = np.exp(rng.normal(size=(n, h * w)) * 2.0)
        p = (x / x.sum(1, keepdims=True)).astype(F).reshape(n, h, w)
    elif family == "signed":
        p = rng.normal(size=(n, h, w)).astype(F)
    elif family == "distinct":
        p = (rng.permutation(n * h * w).astype(F) - F(n * h * w // 3)).reshape(n, h, w)
    elif family == "two":
        p = np.where(rng.random((n, h, w)) < 0.5, F(-1.5), F(2.25)).astype(F)
        p.reshape(-1)[0], p.reshape(-1)[-1] = F(-1.5), F(2.25)
    elif family == "constant":
        p = np.full((n, h, w), 0.375, dtype=F)
    elif family == "nan":              # one NaN cell in the last plane: the whole group is bad
        p = rng.normal(size=(n, h, w)).astype(F)
        p[n - 1, h // 2, w // 2] = np.nan
    elif family == "inf":
        p = rng.normal(size=(n, h, w)).astype(F)
        flat = p.reshape(-1)
        flat[0] = np.inf
        if flat.size > 1:
            flat[-1] = -np.inf
    elif family == "negzero":          # zeros of both signs at the bottom of the range
        p = np.abs(rng.normal(size=(n, h, w))).astype(F)
        flat = p.reshape(-1)
        flat[::3] = F(-0.0)
        flat[1::7] = F(0.0)
    else:
        raise KeyError(family)
    return np.ascontiguousarray(p, dtype=F)


def picture(H: int, W: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


GIVEN = ("data", "narrow", "reversed", "equal")


def given_range(kind: str, planes: np.ndarray):
    """A range handed in: the data's own, a narrower one (under and over rows appear), lo > hi, lo == hi."""
    lo, hi = (F(v) for v in (np.nanmin(planes[np.isfinite(planes)]), np.nanmax(planes[np.isfinite(planes)])))
    mid, q = (lo + hi) / F(2), (hi - lo) / F(4)
    return {"data": (lo, hi), "narrow": (mid - q, mid + q), "reversed": (hi, lo), "equal": (mid, mid)}[kind]


@dataclass(frozen=True)
class Case:
    name: str
    h: int
    w: int
    H: int
    W: int
    bilinear: bool = False
    n_maps: int = 1
    groups: int = 1
    C: int = 1                     # the planes are plane 1 of C (C > 1) or the only one; the others are NaN
    family: str = "heat"
    out_pad: int = 0               # out_stride = 3 H W + out_pad
    given: Optional[str] = None    # one of GIVEN, or None: the group's own range
    alpha: Optional[float] = None  # blend over a random picture whose row stride is 3 W + 7
    seed: int = 0

    def __repr__(self):
        return self.name

    def inputs(self):
        """(planes per group, ranges per group or None, picture per group or None)."""
        planes = [planes_of(self.family, self.n_maps, self.h, self.w, 1000 * self.seed + g) for g in range(self.groups)]
        given = None if self.given is None else [given_range(self.given, p) for p in planes]
        pics = None if self.alpha is None else [picture(self.H, self.W, 77 + g) for g in range(self.groups)]
        return planes, given, pics

    def references(self, lut, inputs=None):
        planes, given, pics = inputs or self.inputs()
        return [render(planes[g], lut, self.H, self.W, self.bilinear, None if pics is None else pics[g], self.alpha,
                       None if given is None else given[g]) for g in range(self.groups)]


def _cases() -> list:
    out, seed = [], 0

    def add(name, *a, **kw):
        nonlocal seed
        seed += 1
        out.append(Case(name, *a, seed=seed, **kw))
    # geometry: every map size at its own size, the up / down / mixed scalings, both interpolations
    geo = [(1, 1, 1, 1), (1, 3, 1, 3), (2, 2, 2, 2), (37, 53, 37, 53), (64, 64, 64, 64), (128, 128, 128, 128),
           (64, 64, 224, 224), (37, 53, 100, 75), (128, 128, 1, 1), (1, 1, 17, 5)]
    for h, w, H, W in geo:
        for bil in (False, True):
            add(f"geo-{h}x{w}-to-{H}x{W}-{'bilinear' if bil else 'nearest'}", h, w, H, W, bilinear=bil, n_maps=2,
                family="signed", out_pad=5 if (h + bil) % 2 else 0)
    add("geo-64x64-to-1024x1024-bilinear-4maps", 64, 64, 1024, 1024, bilinear=True, n_maps=4)
    # groups and strides
    for n in (1, 4, 19, 257):
        for C in (1, 3):
            add(f"maps{n}-C{C}", 16, 16, 16, 16, n_maps=n, C=C, out_pad=5 if C == 3 else 0)
    for g in (1, 10, 16, 17):
        add(f"groups{g}", 9, 11, 20, 13, n_maps=3, groups=g, C=2, bilinear=g % 2 == 0, out_pad=5)
    # value families, both interpolations (0 * inf under bilinear)
    for fam in FAMILIES:
        for bil in (False, True):
            add(f"family-{fam}-{'bilinear' if bil else 'nearest'}", 16, 12, 40, 31, bilinear=bil, n_maps=3, family=fam)
    # given ranges
    for kind in GIVEN:
        add(f"given-{kind}", 16, 16, 24, 24, n_maps=2, groups=2, family="signed", given=kind)
    add("given-data-inf", 16, 16, 16, 16, n_maps=2, family="inf", given="data")
    # blend
    for a in (0.0, 0.5, 1.0, 0.3):
        add(f"blend-alpha{a}", 16, 16, 37, 53, bilinear=a != 0.3, n_maps=2, groups=2, family="signed", alpha=a, out_pad=5)
    add("blend-bad-keeps-picture", 8, 8, 19, 23, n_maps=2, family="constant", alpha=0.5)
    add("blend-nan-bilinear", 8, 8, 19, 23, bilinear=True, n_maps=2, family="inf", alpha=0.3)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
