"""Cases and the numpy restatement of ca_segtab_score (csrc/ca_segtab.hip); no GPU needed to import.

The entry scores a table of heat maps of one geometry against ONE label image and writes the record of ca_seg_score per
map.  The restatement is tests/seg_cases.py's, split the way the kernel splits it:

  ``tables``     what the label pass leaves in the workspace: per map cell the label pixels that read it (tot) and the
                 positive ones among them (pos), for the mask's mapping and for the coefficient's;
  ``score``      one map against those tables: blur, lo, hi, the fixed-tree mean, the mask, the confusion counts as sums
                 over cells, the entries and the threshold walk.  ``normalize=False`` (CA_SEGTAB_RAW) scores the map
                 value itself instead of its min-max coefficient;
  ``reference``  both, for one (map, label).

tests/test_segtab_cases_cpu.py pins ``reference`` against seg_cases.reference (normalised) and against
conceptattention_amd.segmentation on raw maps (counters equal, AP to 1e-12, the bound derived in seg_cases.py: a sum of at
most 2 * 4096 non-negative fp64 terms that add up to at most 1), and the sums over tables against per-pixel counts.

Where this statement says more than seg_cases.reference: lo and hi skip NaN cells (fminf / fmaxf), and both scores of a
cell go through np.nan_to_num's full rule (NaN -> 0, +-inf -> +-FLT_MAX) with -0.0 and 0.0 as one threshold.  A NaN
``mean`` (a NaN cell, or +inf and -inf in one map) compares as NaN: its sign and payload are the adder's own.
"""
import itertools

import numpy as np

import seg_cases as SC

ENTRY = "ca_segtab_score"
MAX_CELLS = 4096
MAX_MAPS = 65536
MAX_LABEL_PIXELS = 1 << 24
f32 = np.float32
KINDS = ("heat", "signed", "ties", "const", "distinct", "special")
FLAG_NAMES = ("mean_value_threshold", "downscale_for_eval", "apply_blur", "normalize")
# every combination of the four flags: (mean threshold, downscale, blur, normalize)
ALL_FLAGS = [dict(zip(FLAG_NAMES, bits)) for bits in itertools.product((True, False), repeat=4)]


def flag_bits(mean_value_threshold=True, downscale_for_eval=False, apply_blur=False, normalize=True) -> int:
    return (1 if mean_value_threshold else 0) | (2 if downscale_for_eval else 0) | (4 if apply_blur else 0) | \
        (0 if normalize else 8)


# ------------------------------------------------------------------------------------------------------------ pieces
def mappings(h, w, Hl, Wl, downscale_for_eval=False):
    """(my, mx, cy, cx): per label row / column the mask's cell row / column and the coefficient's."""
    my, mx = SC.nearest_index(Hl, h), SC.nearest_index(Wl, w)
    cy, cx = my, mx
    if downscale_for_eval:
        cy, cx = SC.nearest_index(14, h)[SC.nearest_index(Hl, 14)], SC.nearest_index(14, w)[SC.nearest_index(Wl, 14)]
    return my, mx, cy, cx


def tables(h, w, label, downscale_for_eval=False) -> np.ndarray:
    """int64 [4, h w]: mask tot, mask pos, coefficient tot, coefficient pos (the workspace after the label pass)."""
    lab = (np.asarray(label) != 0).reshape(-1).astype(np.float64)
    Hl, Wl = np.asarray(label).shape
    my, mx, cy, cx = mappings(h, w, Hl, Wl, downscale_for_eval)
    lab2 = lab.reshape(Hl, Wl)
    out = []
    for ry, rx in ((my, mx), (cy, cx)) if downscale_for_eval else ((my, mx),):
        # pixel (Y, X) reads cell (ry[Y], rx[X]): one-hot row and column selectors, integers in fp64 (exact below 2^53)
        sel_y = (np.arange(h)[:, None] == ry[None, :]).astype(np.float64)          # [h, Hl]
        sel_x = (rx[:, None] == np.arange(w)[None, :]).astype(np.float64)          # [Wl, w]
        out.append(np.outer(sel_y.sum(axis=1), sel_x.sum(axis=0)).reshape(-1).astype(np.int64))
        out.append(((sel_y @ lab2) @ sel_x).reshape(-1).astype(np.int64))
    return np.stack(out if downscale_for_eval else out + out)     # (one mapping without the 14 x 14 round trip)


def nan_to_num_one_zero(s: np.ndarray) -> np.ndarray:
    """np.nan_to_num on fp32 (NaN -> 0, +-inf -> +-FLT_MAX), and -0.0 -> 0.0."""
    return (np.nan_to_num(s.astype(f32)) + f32(0.0)).astype(f32)


def score(amap, tab, n_pixels, mean_value_threshold=True, apply_blur=False, normalize=True) -> dict:
    """The record of one map from the tables of its geometry and label (``tab`` = tables(...))."""
    amap = np.ascontiguousarray(amap, dtype=f32)
    h, w = amap.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = SC.blur3(amap, SC.blur_weights()) if apply_blur else amap
        # fminf / fmaxf from +inf / -inf: NaN cells are skipped
        lo, hi = np.fmin.reduce(x.reshape(-1), initial=np.inf), np.fmax.reduce(x.reshape(-1), initial=-np.inf)
        mean = SC.mean_tree(x)
        mask = x > (mean if mean_value_threshold else f32(0.0))
        if normalize:
            num = x - lo                                                  # one rounding
            den = hi - lo                                                 # one rounding
            c = (num / den).astype(f32)                                   # the correctly rounded division
        else:
            c = x
        mtot, mpos, tot, pos = tab
        mk = mask.reshape(-1)
        n11, n10 = int(mpos[mk].sum()), int((mtot - mpos)[mk].sum())
        n01, n00 = int(mpos[~mk].sum()), int((mtot - mpos)[~mk].sum())
        c1 = c.reshape(-1)
        c0 = (f32(1.0) - c1).astype(f32)                                  # one rounding
        sc = nan_to_num_one_zero(np.concatenate([c0, c1]))
        n_e = np.concatenate([tot, tot])
        p_e = np.concatenate([tot - pos, pos])
        keep = n_e > 0
        sc, n_e, p_e = sc[keep], n_e[keep], p_e[keep]
        order = np.argsort(-sc.astype(np.float64), kind="stable")
        sc, n_e, p_e = sc[order].astype(np.float64), n_e[order], p_e[order]
        last = np.r_[np.nonzero(np.diff(sc))[0], sc.size - 1]             # the last entry of every run of equal scores
        n_k, tp_k = np.cumsum(n_e)[last], np.cumsum(p_e)[last]            # exact integers
        prec = tp_k.astype(np.float64) / n_k.astype(np.float64)
        rec = tp_k.astype(np.float64) / np.float64(n_pixels)
        ap = float(np.sum(np.diff(np.r_[0.0, rec]) * prec))
    return {"n11": n11, "n10": n10, "n01": n01, "n00": n00, "ap": ap, "mean": f32(mean), "lo": f32(lo), "hi": f32(hi),
            "thresholds": int(last.size), "mask": mask.astype(np.uint8), "coeff": c.reshape(h, w), "x": x}


def reference(amap, label, mean_value_threshold=True, downscale_for_eval=False, apply_blur=False, normalize=True) -> dict:
    """What ca_segtab_score writes for one map.  amap fp32 [h, w], label uint8 [Hl, Wl] (nonzero = positive)."""
    h, w = np.asarray(amap).shape
    return score(amap, tables(h, w, label, downscale_for_eval), np.asarray(label).size, mean_value_threshold, apply_blur,
                 normalize)


def pixel_counts(mask, label, h, w, downscale_for_eval=False) -> dict:
    """The per-pixel statement the tables replace: the confusion counts of the resized mask against the label, and per
    coefficient cell the pixels and the positives that read it, pixel by pixel."""
    lab = np.asarray(label) != 0
    Hl, Wl = lab.shape
    my, mx, cy, cx = mappings(h, w, Hl, Wl, downscale_for_eval)
    m_px = np.asarray(mask, dtype=bool)[my][:, mx]
    tot, pos = np.zeros(h * w, dtype=np.int64), np.zeros(h * w, dtype=np.int64)
    np.add.at(tot, (cy[:, None] * w + cx[None, :]).reshape(-1), 1)
    np.add.at(pos, (cy[:, None] * w + cx[None, :]).reshape(-1), lab.reshape(-1).astype(np.int64))
    return {"n11": int((m_px & lab).sum()), "n10": int((m_px & ~lab).sum()), "n01": int((~m_px & lab).sum()),
            "n00": int((~m_px & ~lab).sum()), "tot": tot, "pos": pos}


# ------------------------------------------------------------------------------------------------------------ inputs
def seeded_map(h: int, w: int, seed: int, kind: str = "heat") -> np.ndarray:
    """seg_cases.seeded_map, and ``special``: a signed map with +inf, -inf, NaN, -0.0 and 0.0 cells where it has room."""
    if kind != "special":
        return SC.seeded_map(h, w, seed, kind)
    x = SC.seeded_map(h, w, seed, "signed").reshape(-1).copy()
    cells = np.random.default_rng(seed).permutation(x.size)
    for c, v in zip(cells, (np.inf, -np.inf, np.nan, -0.0, 0.0)):
        x[c] = f32(v)
    return x.reshape(h, w)


def table_maps(h, w, n_maps, seed=0, kinds=KINDS) -> np.ndarray:
    """fp32 [n_maps, h, w]: map m is of kind kinds[m % len(kinds)] with its own seed."""
    return np.stack([seeded_map(h, w, seed + m, kinds[m % len(kinds)]) for m in range(n_maps)])


def seeded_label(h, w, Hl, Wl, seed, kind="blob") -> np.ndarray:
    if kind == "stripes":         # cheap to form at 2^24 pixels: diagonal stripes, 2 of 5 positive
        ys, xs = (np.arange(Hl) * 7 % 5).astype(np.uint8), ((np.arange(Wl) * 13 + seed) % 5).astype(np.uint8)
        return ((ys[:, None] + xs[None, :]) % np.uint8(5) < 2).astype(np.uint8)
    return SC.seeded_label(SC.seeded_map(h, w, seed, "heat"), Hl, Wl, seed, kind)


class Case:
    """One call: n_maps maps of h x w (plane ``target`` of C) against one Hl x Wl label."""

    def __init__(self, name, h, w, Hl, Wl, n_maps=1, C=1, target=0, seed=0, label="blob", kinds=KINDS, **flags):
        self.name, self.h, self.w, self.Hl, self.Wl, self.n_maps, self.C, self.target = name, h, w, Hl, Wl, n_maps, C, target
        self.seed, self.label_kind, self.kinds = seed, label, kinds
        self.flags = dict(mean_value_threshold=True, downscale_for_eval=False, apply_blur=False, normalize=True)
        self.flags.update(flags)

    def __repr__(self):
        return self.name

    def inputs(self):
        """(maps fp32 [n_maps, h, w], label uint8 [Hl, Wl])"""
        return table_maps(self.h, self.w, self.n_maps, self.seed, self.kinds), \
            seeded_label(self.h, self.w, self.Hl, self.Wl, self.seed, self.label_kind)

    def references(self, maps, label) -> list:
        tab = tables(self.h, self.w, label, self.flags["downscale_for_eval"])
        return [score(m, tab, label.size, self.flags["mean_value_threshold"], self.flags["apply_blur"],
                      self.flags["normalize"]) for m in maps]


def _flag_name(f) -> str:
    return "-".join(n for n, on in (("mean", f["mean_value_threshold"]), ("down", f["downscale_for_eval"]),
                                    ("blur", f["apply_blur"]), ("raw", not f["normalize"])) if on) or "none"


def _cases() -> list:
    out = [
        # geometry: every map size, label size, map count and stride of the kernel's paths
        Case("map1x1-label1x1", 1, 1, 1, 1, n_maps=1, kinds=("heat", "special")),
        Case("map2x2-label7x7-blur", 2, 2, 7, 7, n_maps=2, C=4, target=2, seed=1, apply_blur=True),
        Case("map1x3-label7x7-19maps", 1, 3, 7, 7, n_maps=19, seed=2),
        Case("map37x53-label375x500", 37, 53, 375, 500, n_maps=2, C=4, target=3, seed=3),
        Case("map32x64-label224x224", 32, 64, 224, 224, n_maps=2, seed=4),               # 2048 cells: the default LDS limit
        Case("map3x683-label224x224-raw", 3, 683, 224, 224, n_maps=2, C=4, target=1, seed=5, normalize=False),   # 2049
        Case("map64x64-label224x224-19maps", 64, 64, 224, 224, n_maps=19, C=4, target=0, seed=6),
        Case("map64x64-label224x224-raw-down", 64, 64, 224, 224, n_maps=6, seed=7, normalize=False,
             downscale_for_eval=True),
        Case("map16x16-label64x64-257maps", 16, 16, 64, 64, n_maps=257, C=4, target=1, seed=8),      # one more than the CUs
        Case("map5x7-label7x7-950maps-raw", 5, 7, 7, 7, n_maps=950, seed=9, normalize=False),        # 50 levels x 19 layers
        Case("map2x2-label4096x4096", 2, 2, 4096, 4096, n_maps=2, seed=10, label="stripes"),              # counts up to 2^24
        Case("map16x16-label7x7-unread-cells", 16, 16, 7, 7, n_maps=6, C=4, target=2, seed=11),
        Case("labels-all-positive", 16, 16, 64, 64, n_maps=6, seed=12, label="ones"),
        Case("labels-all-negative-raw", 16, 16, 64, 64, n_maps=6, seed=13, label="zeros", normalize=False),
    ]
    # every flag combination on one small rectangular geometry, one map of every kind
    for f in ALL_FLAGS:
        out.append(Case("flags-" + _flag_name(f), 17, 9, 30, 40, n_maps=len(KINDS), C=4, target=1, seed=20, **f))
    return out


CASES = _cases()
FLAG_CASES = [c for c in CASES if c.name.startswith("flags-")]
# the size pairs of the table / per-pixel check: (h, w, Hl, Wl); the last has a label smaller than the map
TABLE_SIZES = [(5, 5, 7, 7), (64, 64, 224, 224), (17, 9, 8, 30), (16, 16, 7, 7)]
