"""Cases and the numpy restatement of ca_seg_score (csrc/ca_seg.hip); no GPU needed to import.

The kernel scores one heat map against one label image: mask, min-max coefficient, confusion counts and the exact
average precision of the stacked scores (1 - c, c).  ``reference`` below spells the same operations out one rounding per
line.  tests/test_seg_cases_cpu.py pins it against conceptattention_amd.segmentation on the CPU (integer counts equal, AP
to 1e-12), tests/test_seg_kernels_gpu.py pins the kernel against it: counts, thresholds, mean, lo, hi, mask and
coefficient bit for bit, AP to 1e-12.

Why 1e-12 for the AP: it is a sum of at most 2 * 4096 non-negative fp64 terms that add up to at most 1, so two
summation orders differ by at most 8191 * 2^-53 = 9.1e-13; the four roundings inside a term add under 1e-15.

The fp64 sum behind ``mean`` is a FIXED tree, restated here exactly (``mean_tree``): thread t of 1024 adds cells t,
t + 1024, ... in that order, the 64 lanes of a wave are added as a butterfly (partner distance 32, 16, ..., 1) and the 16
wave sums in wave order.  So ``mean`` is compared bit for bit too.
"""
import os

import numpy as np
import torch

ENTRY = "ca_seg_score"
MAX_CELLS = 4096
MAX_PROBLEMS = 16
MAX_LABEL_PIXELS = 1 << 24
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------ pieces
def nearest_index(n_out: int, n_in: int) -> np.ndarray:
    """int64 [n_out]: torch's interpolate(mode="nearest") source index, the product in fp32 (tests/pixel_cases.py)."""
    scale = f32(n_in) / f32(n_out)
    prod = np.arange(n_out, dtype=f32) * scale
    return np.minimum(np.floor(prod).astype(np.int64), n_in - 1)


def blur_weights(sigma: float = 1.0) -> np.ndarray:
    """fp32 [9], row-major: the weights segmentation.gaussian_blur3 forms."""
    k = torch.exp(-0.5 * (torch.tensor([-1.0, 0.0, 1.0]) / sigma) ** 2)
    k = k / k.sum()
    return (k[:, None] * k[None, :]).reshape(-1).numpy().astype(f32)


def blur3(x: np.ndarray, wts: np.ndarray) -> np.ndarray:
    """3x3 blur with reflect padding: nine fp32 products, each rounded, added in row-major order."""
    h, w = x.shape
    xp = np.pad(x.astype(f32), 1, mode="reflect")
    acc = None
    for i in range(3):
        for j in range(3):
            prod = f32(wts[3 * i + j]) * xp[i:i + h, j:j + w]      # one rounding
            acc = prod if acc is None else acc + prod             # one rounding
    return acc.astype(f32)


def mean_tree(x: np.ndarray) -> np.float32:
    """float32(fp64 sum / cells) over the kernel's summation tree (module docstring)."""
    v = np.zeros(4096, dtype=np.float64)
    v[:x.size] = x.reshape(-1).astype(np.float64)
    rows = v.reshape(4, 1024)
    t = rows[0].copy()                                   # thread sums: cells t, t + 1024, ... (adding 0.0 is exact)
    for r in range(1, 4):
        t = t + rows[r]
    t = t.reshape(16, 64)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        t = t + t[:, lanes ^ off]
    s = np.float64(0.0)
    for wave in range(16):
        s = s + t[wave, 0]
    return f32(s / np.float64(x.size))


def reference(amap, label, mean_value_threshold=True, downscale_for_eval=False, apply_blur=False) -> dict:
    """What ca_seg_score returns for one item.  amap fp32 [h, w], label uint8 [Hl, Wl] (nonzero = positive)."""
    amap = np.ascontiguousarray(amap, dtype=f32)
    lab = np.asarray(label) != 0
    h, w = amap.shape
    Hl, Wl = lab.shape
    x = blur3(amap, blur_weights()) if apply_blur else amap
    lo, hi = x.min(), x.max()
    mean = mean_tree(x)
    mask = x > (mean if mean_value_threshold else f32(0.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        num = x - lo                                                  # one rounding
        den = hi - lo                                                 # one rounding
        c = (num / den).astype(f32)                                   # the correctly rounded division
    my, mx = nearest_index(Hl, h), nearest_index(Wl, w)
    cy, cx = my, mx
    if downscale_for_eval:
        cy, cx = nearest_index(14, h)[nearest_index(Hl, 14)], nearest_index(14, w)[nearest_index(Wl, 14)]
    m_px = mask[my][:, mx]
    n11, n10 = int((m_px & lab).sum()), int((m_px & ~lab).sum())
    n01, n00 = int((~m_px & lab).sum()), int((~m_px & ~lab).sum())
    cell = (cy[:, None] * w + cx[None, :]).reshape(-1)
    tot = np.bincount(cell, minlength=h * w).astype(np.int64)
    pos = np.bincount(cell, weights=lab.reshape(-1).astype(np.float64), minlength=h * w).astype(np.int64)
    # the entries: class 1 of a cell scores c, class 0 float32(1 - c); NaN -> 0, -0.0 == 0.0; unread cells dropped
    c1 = c.reshape(-1)
    with np.errstate(invalid="ignore"):
        c0 = (f32(1.0) - c1).astype(f32)                              # one rounding
    score = np.nan_to_num(np.concatenate([c0, c1]), nan=0.0) + f32(0.0)
    n_e = np.concatenate([tot, tot])
    p_e = np.concatenate([tot - pos, pos])
    keep = n_e > 0
    score, n_e, p_e = score[keep], n_e[keep], p_e[keep]
    order = np.argsort(-score.astype(np.float64), kind="stable")
    score, n_e, p_e = score[order], n_e[order], p_e[order]
    last = np.r_[np.nonzero(np.diff(score))[0], score.size - 1]       # the last entry of every run of equal scores
    n_k, tp_k = np.cumsum(n_e)[last], np.cumsum(p_e)[last]            # exact integers
    prec = tp_k.astype(np.float64) / n_k.astype(np.float64)
    rec = tp_k.astype(np.float64) / np.float64(Hl * Wl)
    ap = float(np.sum(np.diff(np.r_[0.0, rec]) * prec))
    return {"n11": n11, "n10": n10, "n01": n01, "n00": n00, "ap": ap, "mean": mean, "lo": f32(lo), "hi": f32(hi),
            "thresholds": int(last.size), "mask": mask.astype(np.uint8), "coeff": c.reshape(h, w), "x": x}


def host_counters(rec: dict, n_pixels: int) -> dict:
    """The counters SegmentationScores.update reports for this record (its (1 - m, m) / (1 - y, y) stacking counts every
    agreeing pixel twice, once per class plane)."""
    agree = rec["n11"] + rec["n00"]
    return {"correct": 2 * agree, "labelled": 2 * n_pixels, "inter": [agree, agree],
            "union": [2 * n_pixels - agree, 2 * n_pixels - agree]}


def mask_margin_ulps(x: np.ndarray, mean) -> float:
    """The smallest distance of a cell from the mean, in fp32 ulps of the mean: the host path thresholds at torch's fp32
    mean, the kernel at float32(fp64 mean); masks can only differ for a cell this close."""
    ulp = float(np.spacing(np.abs(f32(mean)))) or float(np.spacing(f32(0.0)))
    return float(np.min(np.abs(x.astype(np.float64) - np.float64(mean)))) / ulp


# ------------------------------------------------------------------------------------------------------------ inputs
def seeded_map(h: int, w: int, seed: int, kind: str = "heat") -> np.ndarray:
    rng = np.random.default_rng(7919 * seed + 64 * h + w)
    if kind == "heat":            # positive, skewed like an accumulated softmax map
        return (rng.random((h, w), dtype=f32) ** 2 * f32(0.05) + f32(0.01)).astype(f32)
    if kind == "signed":          # negative cells: x > 0 and x > mean differ
        return rng.standard_normal((h, w)).astype(f32)
    if kind == "ties":            # steps of 0.5: few distinct thresholds
        return (np.floor(rng.random((h, w), dtype=f32) * f32(6.0)) * f32(0.5) - f32(1.0)).astype(f32)
    if kind == "const":
        return np.full((h, w), 0.375, dtype=f32)
    if kind == "distinct":        # the cells 0 .. hw-2 and hw-0.5 in a seeded order: c_k + c_j = 1 only for (min, max)
        v = np.arange(h * w, dtype=f32)
        v[-1] = f32(h * w) - f32(0.5)
        return rng.permutation(v).reshape(h, w).astype(f32)
    raise KeyError(kind)


def seeded_label(amap: np.ndarray, Hl: int, Wl: int, seed: int, kind: str = "blob") -> np.ndarray:
    """uint8 [Hl, Wl] of 0 / 1: the resized map plus noise above its median, so that the scores carry signal."""
    if kind == "ones":
        return np.ones((Hl, Wl), dtype=np.uint8)
    if kind == "zeros":
        return np.zeros((Hl, Wl), dtype=np.uint8)
    rng = np.random.default_rng(104729 * seed + 1000 * Hl + Wl)
    big = amap[nearest_index(Hl, amap.shape[0])][:, nearest_index(Wl, amap.shape[1])].astype(np.float64)
    spread = float(big.std()) or 1.0
    noisy = big + 0.7 * spread * rng.standard_normal((Hl, Wl))
    return (noisy > np.median(noisy)).astype(np.uint8)


class Case:
    def __init__(self, name, h, w, Hl, Wl, seed=0, kind="heat", label="blob", mvt=True, down=False, blur=False, gold=None):
        self.name, self.h, self.w, self.Hl, self.Wl, self.seed = name, h, w, Hl, Wl, seed
        self.kind, self.label_kind, self.mvt, self.down, self.blur, self.gold = kind, label, mvt, down, blur, gold

    def __repr__(self):
        return self.name

    @property
    def flags(self) -> dict:
        return dict(mean_value_threshold=self.mvt, downscale_for_eval=self.down, apply_blur=self.blur)

    def inputs(self):
        """(map fp32 [h, w], label uint8 [Hl, Wl])"""
        if self.gold is not None:
            g = np.load(GOLD)
            return (np.ascontiguousarray(g[f"coeff{self.gold}"], dtype=f32),
                    np.ascontiguousarray(g[f"label{self.gold}"] != 0).astype(np.uint8))
        amap = seeded_map(self.h, self.w, self.seed, self.kind)
        return amap, seeded_label(amap, self.Hl, self.Wl, self.seed, self.label_kind)


def _cases() -> list:
    out = [Case("golden1", 64, 64, 64, 64, gold=1), Case("golden2", 17, 9, 17, 9, gold=2)]
    # every map size against every label size: its own, 7, 14, 64, 224 and the rectangular 8 x 30 (9 -> 30 and 64 -> 224
    # are the scales where the fp32 product lands on both sides of integers)
    for h, w in ((2, 2), (3, 3), (5, 5), (16, 16), (31, 31), (64, 64), (17, 9)):
        for Hl, Wl in ((h, w), (7, 7), (14, 14), (64, 64), (224, 224), (8, 30)):
            out.append(Case(f"map{h}x{w}-label{Hl}x{Wl}", h, w, Hl, Wl, seed=1))
    out += [
        Case("downscale-5-to-7", 5, 5, 7, 7, seed=2, down=True),
        Case("downscale-3-to-64", 3, 3, 64, 64, seed=2, down=True),
        Case("downscale-16-to-224", 16, 16, 224, 224, seed=2, down=True),
        Case("downscale-64-to-224", 64, 64, 224, 224, seed=2, down=True),
        Case("downscale-17x9-to-8x30", 17, 9, 8, 30, seed=2, down=True),
        Case("signed-mean-threshold", 16, 16, 64, 64, seed=3, kind="signed"),
        Case("signed-zero-threshold", 16, 16, 64, 64, seed=3, kind="signed", mvt=False),
        Case("signed-zero-threshold-31-to-224", 31, 31, 224, 224, seed=3, kind="signed", mvt=False),
        Case("blur-2-to-7", 2, 2, 7, 7, seed=4, blur=True),
        Case("blur-16-to-64", 16, 16, 64, 64, seed=4, blur=True),
        Case("blur-64-to-224", 64, 64, 224, 224, seed=4, blur=True),
        Case("blur-17x9-to-8x30", 17, 9, 8, 30, seed=4, blur=True),
        Case("blur-downscale-zero-threshold", 31, 31, 224, 224, seed=4, kind="signed", mvt=False, down=True, blur=True),
        Case("ties-16-to-64", 16, 16, 64, 64, seed=5, kind="ties"),
        Case("ties-64-to-224", 64, 64, 224, 224, seed=5, kind="ties"),
        Case("constant-map", 5, 5, 14, 14, seed=6, kind="const"),
        Case("labels-all-positive", 16, 16, 64, 64, seed=7, label="ones"),
        Case("labels-all-negative", 16, 16, 64, 64, seed=7, label="zeros"),
        Case("full-sort-4096-distinct", 64, 64, 224, 224, seed=8, kind="distinct"),
        Case("three-cells", 1, 3, 5, 7, seed=9),
        # label sizes beyond 224 x 224: score_images' own, an ordinary evaluation label, the entry point's limit (2^24
        # pixels on four cells: every count of the record and of the two tables reaches 2^22 .. 2^24)
        Case("map64x64-label1024x1024", 64, 64, 1024, 1024, seed=1),
        Case("map48x64-label375x500", 48, 64, 375, 500, seed=1),      # rectangular; 6144 entries sorted as 8192
        Case("map2x2-label4096x4096", 2, 2, 4096, 4096, seed=1),
        # the dynamic-LDS request crosses 64 KiB where the padded sort size jumps from 4096 to 8192 entries: 2048 cells
        # (57 856 bytes) are the largest launch inside the default limit, 2049 (90 672 bytes) the smallest that raises it
        Case("map32x64-label224x224", 32, 64, 224, 224, seed=1),
        Case("map3x683-label224x224", 3, 683, 224, 224, seed=1),
    ]
    return out


CASES = _cases()
LDS_DEFAULT_LIMIT = 64 * 1024


def lds_bytes(cells: int) -> int:
    """The dynamic LDS ca_seg_score asks for (ca_seg.hip: sort entries, x, tot, pos, scratch)."""
    npad = 2
    while npad < 2 * cells:
        npad <<= 1
    return npad * 8 + (cells + 3) // 4 * 4 * 12 + 512


def cap_launch_inputs():
    """MAX_PROBLEMS items of one geometry (16 x 16 maps, 64 x 64 labels) with different seeds: one launch of the cap."""
    maps = [seeded_map(16, 16, 100 + i) for i in range(MAX_PROBLEMS)]
    return maps, [seeded_label(m, 64, 64, 100 + i) for i, m in enumerate(maps)]
