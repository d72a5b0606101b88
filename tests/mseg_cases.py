"""Cases and the numpy restatement of ca_mseg_score (csrc/ca_mseg.hip); no GPU needed to import.

The kernel takes an item's K accumulated maps, forms torch.argmax over the concepts per map cell, looks the winning
concept's class up in the item's table and counts the class map, read through the nearest rule, against a label image of
class ids.  ``reference`` below spells the same operations out one rounding per line; every output is an integer, so
tests/test_mseg_kernels_gpu.py compares counts, class map and index map bit for bit.

What of the reference's harness is restated here (experiments/pascal_voc_segmentation; its two files cannot be imported:
they fetch a corpus at import and depend on modules that are gone, so no golden made by the harness itself exists -- the
pins are torch.argmax / interpolate on the CPU and the transcription below, see tests/test_mseg_cases_cpu.py):
  multi_class_segmentation.py:71-77      optional 3x3 blur of the maps, then argmax over the concepts
  run_multi_class_seg_experiment.py:25-37    concept index -> class id (background concepts -> 0)
  run_multi_class_seg_experiment.py:195-200  nearest resize of the class map to the label
  run_multi_class_seg_experiment.py:207-222  correct / labelled of batch_pix_accuracy (every label counts as labelled),
                                             then per class the pixels with mask == c and label == c, mask == c or label == c
  run_multi_class_seg_experiment.py:225-233  mIoU = sum of inter / union over classes with union > 0, / (their number + 1e-6)
"""
import numpy as np

from seg_cases import blur3, blur_weights, nearest_index

ENTRY = "ca_mseg_score"
MAX_PROBLEMS = 16
MAX_CONCEPTS = 32
MAX_CLASSES = 256
MAX_CELLS = 16384
MAX_LABEL_PIXELS = 1 << 24
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------ pieces
def argmax_first(s: np.ndarray) -> np.ndarray:
    """int64 [h, w]: torch.argmax over axis 0.  Plane k replaces the running best iff s_k > best, or s_k is NaN and best
    is not: the first index of the maximum wins, -0.0 == 0.0, the first NaN beats every number."""
    best = s[0].copy()
    index = np.zeros(s.shape[1:], dtype=np.int64)
    for k in range(1, s.shape[0]):
        with np.errstate(invalid="ignore"):
            take = (s[k] > best) | (np.isnan(s[k]) & ~np.isnan(best))
        best = np.where(take, s[k], best)
        index = np.where(take, k, index)
    return index


def scaled_planes(maps, scale=None, apply_blur=False) -> np.ndarray:
    """fp32 [K, h, w]: s_k of the header."""
    x = np.ascontiguousarray(maps, dtype=f32)
    if apply_blur:
        wts = blur_weights()
        with np.errstate(invalid="ignore", over="ignore"):
            x = np.stack([blur3(p, wts) for p in x])                      # nine rounded products, eight rounded sums
    if scale is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            x = (np.asarray(scale, dtype=f32)[:, None, None] * x).astype(f32)   # one rounding
    return x


def counts_of(pred: np.ndarray, label: np.ndarray, nclass: int, ignore_index=None) -> np.ndarray:
    """int64 [2 + 2 nclass]: correct, labelled, inter[nclass], union[nclass] of a class map at label resolution."""
    p, y = pred.reshape(-1).astype(np.int64), label.reshape(-1).astype(np.int64)
    if ignore_index is not None and ignore_index >= 0:
        keep = y != ignore_index
        p, y = p[keep], y[keep]
    hit = p == y
    inter = np.bincount(p[hit], minlength=nclass)[:nclass]
    union = np.bincount(p, minlength=nclass)[:nclass] + np.bincount(y[y < nclass], minlength=nclass)[:nclass] - inter
    return np.concatenate([[int(hit.sum()), int(y.size)], inter, union]).astype(np.int64)


def reference(maps, label, class_of, nclass, ignore_index=None, scale=None, apply_blur=False) -> dict:
    """What ca_mseg_score returns for one item.  maps fp32 [K, h, w], label uint8 [Hl, Wl], class_of K class ids."""
    s = scaled_planes(maps, scale, apply_blur)
    index = argmax_first(s)
    klass = np.asarray(class_of, dtype=np.int64)[index]
    Hl, Wl = label.shape
    my, mx = nearest_index(Hl, s.shape[1]), nearest_index(Wl, s.shape[2])
    pred = klass[my][:, mx]
    return {"counts": counts_of(pred, np.asarray(label), nclass, ignore_index).astype(np.int32),
            "class": klass.astype(np.uint8), "index": index.astype(np.uint8), "s": s, "pred": pred}


def harness_counts(mask: np.ndarray, labels: np.ndarray, nclass: int):
    """Lines 207-222 of run_multi_class_seg_experiment.py, transcribed: (correct, labelled, inter[nclass], union[nclass])
    of one image; ``mask`` and ``labels`` float arrays of class ids (the harness has no ignore_index)."""
    predict, target = mask + 1, labels + 1                                 # batch_pix_accuracy (utils.py:66-80)
    labelled = np.sum(target > 0)
    correct = np.sum((predict == target) * (target > 0))
    inter, union = np.zeros(nclass), np.zeros(nclass)
    for class_index in range(nclass):
        intersection = (mask == class_index) & (labels == class_index)
        un = (mask == class_index) | (labels == class_index)
        inter[class_index] += intersection.sum()
        union[class_index] += un.sum()
    return int(correct), int(labelled), inter.astype(np.int64), union.astype(np.int64)


def harness_miou(total_inter, total_union) -> float:
    """Lines 225-233, transcribed."""
    miou, num_nonzero_classes = 0.0, 0
    for class_index in range(len(total_union)):
        if total_union[class_index] == 0:
            continue
        num_nonzero_classes += 1
        miou += total_inter[class_index] / total_union[class_index]
    return miou / (num_nonzero_classes + 1e-6)


def top2_gap_ulps(s: np.ndarray) -> float:
    """The smallest gap between a cell's largest and second largest value, in fp32 ulps of the largest: two roundings of
    the blur can only move the argmax of a cell this close (inf when K = 1)."""
    if s.shape[0] < 2:
        return float("inf")
    top = np.sort(s.astype(np.float64), axis=0)[-2:]
    ulp = np.spacing(np.abs(top[1]).astype(f32)).astype(np.float64)
    return float(np.min((top[1] - top[0]) / ulp))


# ------------------------------------------------------------------------------------------------------------ inputs
def seeded_maps(K, h, w, seed, kind="heat") -> np.ndarray:
    rng = np.random.default_rng(7919 * seed + 4096 * K + 64 * h + w)
    m = (rng.random((K, h, w), dtype=f32) ** 2 * f32(0.05) + f32(0.01)).astype(f32)
    if kind == "heat":
        return m
    if kind == "quant":            # four distinct values: most cells tie, the first maximum must win
        return (np.floor(rng.random((K, h, w), dtype=f32) * f32(4.0)) * f32(0.25)).astype(f32)
    if kind == "dup":              # every plane is a copy of plane 0 or 1: ties between exact duplicates
        return np.ascontiguousarray(m[np.arange(K) % 2])
    if kind == "special":          # NaN in one plane, NaN in all planes, +-0 everywhere, +-inf
        m = rng.standard_normal((K, h, w)).astype(f32)
        cells = rng.permutation(h * w)
        q = max(1, h * w // 8)
        flat = m.reshape(K, -1)
        for c in cells[:q]:                                       # NaN in one plane (not always the first)
            flat[rng.integers(0, K), c] = np.nan
        flat[:, cells[q:2 * q]] = np.nan                         # NaN in all planes
        for c in cells[2 * q:3 * q]:                              # only zeros of both signs
            flat[:, c] = np.where(rng.random(K) < 0.5, f32(0.0), f32(-0.0))
        for c in cells[3 * q:4 * q]:                              # +inf twice, -inf elsewhere
            flat[:, c] = -np.inf
            flat[rng.integers(0, K, size=2), c] = np.inf
        for c in cells[4 * q:5 * q]:                              # all -inf
            flat[:, c] = -np.inf
        return m
    raise KeyError(kind)


def seeded_class_of(K, nclass, seed) -> list:
    """K class ids: the first concepts are background (0), the others any class below nclass."""
    rng = np.random.default_rng(31337 * seed + K + 7 * nclass)
    n_bg = min(K - 1, 5) if K > 1 else 0
    return [0] * n_bg + [int(v) for v in rng.integers(0, nclass, size=K - n_bg)]


def seeded_label(maps, class_of, Hl, Wl, nclass, seed, border=True, top=None) -> np.ndarray:
    """uint8 [Hl, Wl]: where a coarse coin says so the class of the (NaN-free) argmax, else a coarse random class id below
    ``top`` (default nclass); with ``border`` a frame and a stripe of 255, VOC's void label."""
    rng = np.random.default_rng(104729 * seed + 1000 * Hl + Wl)
    K, h, w = maps.shape
    base = np.asarray(class_of)[np.argmax(np.nan_to_num(maps, nan=0.0, posinf=1e30, neginf=-1e30), axis=0)]
    base = base[nearest_index(Hl, h)][:, nearest_index(Wl, w)]
    gy, gx = nearest_index(Hl, 9), nearest_index(Wl, 7)
    coin = (rng.random((9, 7)) < 0.5)[gy][:, gx]
    other = rng.integers(0, top or nclass, size=(9, 7))[gy][:, gx]
    y = np.where(coin, base, other).astype(np.uint8)
    if border and Hl >= 4 and Wl >= 4:
        t = max(1, min(Hl, Wl) // 32)
        y[:t], y[-t:], y[:, :t], y[:, -t:] = 255, 255, 255, 255
        y[Hl // 2:Hl // 2 + t, Wl // 3:2 * Wl // 3] = 255
    return y


class Case:
    def __init__(self, name, K, h, w, Hl, Wl, nclass, ignore=None, seed=0, kind="heat", scale=None, blur=False, items=1,
                 outputs="both", border=True, top=None):
        self.name, self.K, self.h, self.w, self.Hl, self.Wl, self.nclass = name, K, h, w, Hl, Wl, nclass
        self.ignore, self.seed, self.kind, self.scale, self.blur, self.items = ignore, seed, kind, scale, blur, items
        self.outputs, self.border, self.top = outputs, border, top

    def __repr__(self):
        return self.name

    def inputs(self):
        """(maps [items][K, h, w], labels [items][Hl, Wl], class_of [items][K], scale [K] or None)"""
        maps, labels, tables = [], [], []
        for i in range(self.items):
            m = seeded_maps(self.K, self.h, self.w, self.seed + 101 * i, self.kind)
            t = seeded_class_of(self.K, self.nclass, self.seed + 101 * i)      # a different table per item
            maps.append(m), tables.append(t)
            labels.append(seeded_label(m, t, self.Hl, self.Wl, self.nclass, self.seed + 101 * i, self.border, self.top))
        scale = None
        if self.scale is not None:
            scale = np.linspace(0.5, 2.0, self.K).astype(f32)
            if self.K > 1:
                scale[self.K // 2] = 0.0                   # (0 * inf = NaN, 0 * x = +-0)
            scale[-1] = -1.5                                # (the smallest plane becomes the largest)
        return maps, labels, tables, scale


def _cases() -> list:
    return [
        # ---- K, map and label sizes, nclass, ignore_index
        Case("k1-map1x1-label1x1-nclass1", 1, 1, 1, 1, 1, 1, seed=1, border=False),
        Case("k2-map2x2-label2x2-nclass2-blur", 2, 2, 2, 2, 2, 2, seed=2, blur=True, border=False),
        Case("k2-map16x16-label1x1-nclass2", 2, 16, 16, 1, 1, 2, seed=3),
        Case("k11-map16x16-label16x16-nclass21", 11, 16, 16, 16, 16, 21, seed=4),
        Case("k11-map16x16-label224x224-nclass21-ignore255", 11, 16, 16, 224, 224, 21, ignore=255, seed=5),
        Case("k11-map16x16-label224x224-nclass21-border-counted", 11, 16, 16, 224, 224, 21, seed=5),   # ids >= nclass
        Case("k32-map37x53-label375x500-nclass21-ignore0", 32, 37, 53, 375, 500, 21, ignore=0, seed=6),
        Case("k11-map37x53-label37x53-nclass256", 11, 37, 53, 37, 53, 256, seed=7),
        Case("k11-map64x64-label1024x1024-nclass21-ignore255", 11, 64, 64, 1024, 1024, 21, ignore=255, seed=8),
        Case("k8-map64x64-label64x64-nclass21-ignore255", 8, 64, 64, 64, 64, 21, ignore=255, seed=9),
        Case("k32-map128x128-label128x128-nclass256-ignore-absent", 32, 128, 128, 128, 128, 256, ignore=250, seed=10,
             border=False, top=200),
        Case("k11-map128x128-label224x224-nclass21", 11, 128, 128, 224, 224, 21, seed=11),
        Case("k2-map2x2-label4096x4096-nclass2", 2, 2, 2, 4096, 4096, 2, seed=12),                       # the label limit
        Case("k1-map16x16-label64x64-nclass2", 1, 16, 16, 64, 64, 2, seed=13),
        # ---- value families
        Case("quantised-k11-map16x16-label64x64", 11, 16, 16, 64, 64, 21, ignore=255, seed=14, kind="quant"),
        Case("quantised-k32-map37x53-label224x224", 32, 37, 53, 224, 224, 21, seed=14, kind="quant"),
        Case("duplicate-planes-k11-map16x16-label64x64", 11, 16, 16, 64, 64, 21, seed=15, kind="dup"),
        Case("special-values-k11-map37x53-label224x224", 11, 37, 53, 224, 224, 21, ignore=255, seed=16, kind="special"),
        Case("special-values-k2-map16x16-label64x64", 2, 16, 16, 64, 64, 2, seed=16, kind="special"),
        Case("special-values-scaled-k11-map16x16-label64x64", 11, 16, 16, 64, 64, 21, seed=17, kind="special", scale=True),
        Case("scaled-k11-map16x16-label224x224", 11, 16, 16, 224, 224, 21, ignore=255, seed=18, scale=True),
        Case("scaled-blur-k8-map37x53-label375x500", 8, 37, 53, 375, 500, 21, ignore=255, seed=18, scale=True, blur=True),
        Case("blur-k11-map16x16-label224x224", 11, 16, 16, 224, 224, 21, ignore=255, seed=19, blur=True),
        Case("blur-k8-map64x64-label224x224", 8, 64, 64, 224, 224, 21, seed=19, blur=True),
        Case("blur-k2-map128x128-label128x128", 2, 128, 128, 128, 128, 21, seed=19, blur=True),
        Case("blur-special-values-k11-map16x16-label64x64", 11, 16, 16, 64, 64, 21, seed=20, kind="special", blur=True),
        # ---- the call: the cap and one more item (two launches), a different class table per item
        Case("items16-k8-map16x16-label64x64", 8, 16, 16, 64, 64, 21, ignore=255, seed=21, items=16),
        Case("items17-k8-map16x16-label64x64", 8, 16, 16, 64, 64, 21, seed=22, items=17),
        # ---- the optional outputs
        Case("outputs-class-only", 11, 16, 16, 64, 64, 21, ignore=255, seed=23, outputs="class"),
        Case("outputs-index-only", 11, 16, 16, 64, 64, 21, ignore=255, seed=23, outputs="index"),
        Case("outputs-none", 11, 16, 16, 64, 64, 21, ignore=255, seed=23, outputs="none"),
    ]


CASES = _cases()
PLACEMENT_CASE = "k11-map16x16-label224x224-nclass21-ignore255"


def placement_data_bytes(case) -> dict:
    """Bytes the kernel reads or writes per operand role of a one-item launch (without any guard elements a launch helper
    appends): what tests/test_mseg_placement_gpu.py must find on both sides of the 2^32 line."""
    cells = case.h * case.w
    return {"maps": case.K * cells * 4, "label": case.Hl * case.Wl, "counts": (2 + 2 * case.nclass) * 4,
            "class_out": cells, "index_out": cells}
