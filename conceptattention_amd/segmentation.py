"""Zero-shot segmentation on top of the concept heat maps, and the scores the reference's evaluation
harness reports for it.

What is mirrored
  * ``add_noise_to_image``        concept_attention/segmentation.py:85-113
  * mean-threshold masks           concept_attention/segmentation.py:55-81 (``SegmentationAbstractClass.__call__``)
  * ``batch_pix_accuracy`` / ``batch_intersection_union`` / ``get_ap_scores``
                                   concept_attention/utils.py:48-108
  * the per-image scoring + running pixAcc / mIoU / mAP of
                                   experiments/imagenet_segmentation/run_experiment.py:166-235
The heat maps themselves come from ``ConceptAttentionFluxPipeline.encode_image`` (one forward of the 19
double blocks on the HIP path); everything in this file is small host-side arithmetic on (C, side, side)
maps -- except ``DeviceSegmentationScores`` and ``ConceptAttentionSegmentationModel.score_images`` (and their multi-class
counterparts ``DeviceMultiClassScores`` / ``score_multiclass_images`` on ca_mseg_score, csrc/ca_mseg.hip), which score the maps
where they are: one ca_seg_score workgroup per image (csrc/ca_seg.hip) computes the mask, the counts and the exact AP from
the device accumulators, and only the 40-byte records come back, once.  ``SweepScores`` / ``DeviceSweepScores`` /
``score_sweep`` do the same for the per-layer x per-noise-level tables of ``pipeline.layer_noise_sweep`` (ca_segtab_score,
csrc/ca_segtab.hip: one record per (level, layer) map, two launches per table).  The image loop of the harness (`run_experiment.py:137`) is the natural multi-GPU shard: every rank
scores its own images and ``SegmentationScores.all_reduce`` sums the five counters once at the end.
"""
from __future__ import annotations

from dataclasses import dataclass, field, fields

import numpy as np
import torch

from . import _lib as L
from . import ops, sampling
from .pipeline import EncodeSettings


# ------------------------------------------------------------------------------------------ noise
def add_noise_to_image(encoded_image: torch.Tensor, num_steps: int = 50, noise_timestep: int = 49, seed: int = 63,
                       width: int = 1024, height: int = 1024, device="cuda", is_schnell: bool = True,
                       noise: torch.Tensor | None = None):
    """x = t*noise + (1-t)*latent at schedule position ``noise_timestep``; returns (x, remaining timesteps).
    ``noise`` overrides get_noise (device RNG streams differ between platforms)."""
    x = noise if noise is not None else sampling.get_noise(1, height, width, device, torch.bfloat16, seed)
    timesteps = sampling.get_schedule(num_steps, x.shape[-1] * x.shape[-2] // 4, shift=(not is_schnell))
    t = timesteps[noise_timestep]
    x = t * x + (1.0 - t) * encoded_image.to(x.dtype)
    return x, timesteps[noise_timestep:]


# ------------------------------------------------------------------------------------------ masks
def mean_threshold_masks(coefficients: torch.Tensor) -> torch.Tensor:
    """(C, h, w) coefficients -> bool masks, each concept thresholded at its own spatial mean."""
    return coefficients > coefficients.mean(dim=(1, 2), keepdim=True)


def target_mask(coefficients: torch.Tensor, index: int, mean_value_threshold: bool = True) -> torch.Tensor:
    c = coefficients[index]
    return c > (c.mean() if mean_value_threshold else 0.0)


def _resize_nearest(x: torch.Tensor, size) -> torch.Tensor:
    return torch.nn.functional.interpolate(x[None, None].float(), size=size, mode="nearest")[0, 0]


def prepare_for_scoring(coefficients, mask, size: int = 224, downscale_for_eval: bool = False):
    """min-max rescale the target concept's map, optional 14x14 round trip, nearest resize of map and mask
    to the label resolution (run_experiment.py:177-204)."""
    c = torch.as_tensor(np.asarray(coefficients), dtype=torch.float32)
    c = (c - c.min()) / (c.max() - c.min())
    if downscale_for_eval:
        c = _resize_nearest(c, (14, 14))
    c = _resize_nearest(c, (size, size))
    m = _resize_nearest(torch.as_tensor(np.asarray(mask), dtype=torch.float32), (size, size))
    return c, m


# ------------------------------------------------------------------------------------------ metrics
def _np(x) -> np.ndarray:
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def batch_pix_accuracy(predict, target):
    """(correct, labelled) pixel counts; labels < 0 are unlabelled."""
    p, t = _np(predict) + 1, _np(target) + 1
    labelled = int(np.sum(t > 0))
    correct = int(np.sum((p == t) & (t > 0)))
    assert correct <= labelled, "Correct area should be smaller than Labeled"
    return correct, labelled


def batch_intersection_union(predict, target, nclass: int):
    """per-class (intersection, union) areas, classes 0..nclass-1, labels < 0 ignored."""
    p, t = _np(predict) + 1, _np(target) + 1
    p = p * (t > 0).astype(p.dtype)
    hit = p * (p == t)
    rng = (1, nclass)
    inter, _ = np.histogram(hit, bins=nclass, range=rng)
    a_p, _ = np.histogram(p, bins=nclass, range=rng)
    a_t, _ = np.histogram(t, bins=nclass, range=rng)
    union = a_p + a_t - inter
    assert (inter <= union).all(), "Intersection area should be smaller than Union area"
    return inter, union


def average_precision(y_true: np.ndarray, y_score: np.ndarray) -> float:
    """AP = sum_n (R_n - R_{n-1}) P_n over the distinct score thresholds, descending (the definition
    sklearn.metrics.average_precision_score uses, which utils.py:63 calls)."""
    y_true = np.asarray(y_true).astype(np.float64).ravel()
    y_score = np.asarray(y_score).astype(np.float64).ravel()
    n_pos = y_true.sum()
    if y_true.size == 0 or n_pos == 0:
        return float("nan") if y_true.size == 0 else 0.0
    order = np.argsort(-y_score, kind="stable")
    s, y = y_score[order], y_true[order]
    last_of_run = np.r_[np.nonzero(np.diff(s))[0], s.size - 1]
    tp = np.cumsum(y)[last_of_run]
    precision = tp / (last_of_run + 1.0)
    recall = tp / n_pos
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


def get_ap_scores(predict, target, ignore_index: int = -1):
    """per-sample AP of (K, h, w) class scores against an (h, w) integer label map."""
    out = []
    for pred, tgt in zip(predict, target):
        pred, tgt = _np(pred), _np(tgt)
        k = pred.shape[0]
        lab = np.broadcast_to(tgt[None], pred.shape)
        onehot = (np.arange(k).reshape(k, *([1] * tgt.ndim)) == np.clip(tgt, 0, None).astype(np.int64)[None])
        keep = lab.reshape(-1) != ignore_index
        score = np.nan_to_num(pred.reshape(-1))[keep]
        out.append(float(np.nan_to_num(average_precision(onehot.reshape(-1)[keep], score))))
    return out


def _all_reduce_vector(v: torch.Tensor):
    """The sum of the host vector ``v`` over ranks, on the host in ``v``'s dtype (through the current device under nccl);
    None without an initialised process group of more than one rank: the caller's counters then stay as they are."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return None
    from .distributed import allreduce_sum_
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else v.device
    return allreduce_sum_(v.to(dev)).cpu()


@dataclass
class SegmentationScores:
    """Running pixAcc / mIoU / mAP over images (run_experiment.py:134-232)."""
    correct: float = 0.0
    labelled: float = 0.0
    inter: np.ndarray = field(default_factory=lambda: np.zeros(2))
    union: np.ndarray = field(default_factory=lambda: np.zeros(2))
    ap_sum: float = 0.0
    n: int = 0

    def update(self, mask, coefficients, labels) -> dict:
        """mask, coefficients: (h, w) at the label resolution (see prepare_for_scoring); labels: (h, w) bool."""
        m = torch.as_tensor(_np(mask), dtype=torch.float32)
        y = torch.as_tensor(_np(labels).astype(np.float32))
        c = torch.as_tensor(_np(coefficients), dtype=torch.float32)
        m2, y2 = torch.stack((1 - m, m)), torch.stack((1 - y, y))
        cor, lab = batch_pix_accuracy(m2, y2)
        inter, union = batch_intersection_union(m2, y2, nclass=2)
        ap = get_ap_scores(torch.stack((1 - c, c))[None], y[None])[0]
        self.correct += cor
        self.labelled += lab
        self.inter = self.inter + inter
        self.union = self.union + union
        self.ap_sum += ap
        self.n += 1
        return {"correct": cor, "labelled": lab, "inter": inter, "union": union, "ap": ap}

    def all_reduce(self) -> "SegmentationScores":
        """Sum the counters over ranks (no-op without an initialised process group)."""
        v = _all_reduce_vector(torch.tensor([self.correct, self.labelled, *self.inter, *self.union, self.ap_sum,
                                             float(self.n)], dtype=torch.float64))
        if v is not None:
            self.correct, self.labelled = float(v[0]), float(v[1])
            self.inter, self.union = v[2:4].numpy().copy(), v[4:6].numpy().copy()
            self.ap_sum, self.n = float(v[6]), int(round(float(v[7])))
        return self

    def result(self) -> dict:
        eps = np.spacing(1, dtype=np.float64)
        iou = self.inter / (eps + self.union)
        return {"pixAcc": float(self.correct / (eps + self.labelled)), "mIoU": float(iou.mean()),
                "mAP": float(self.ap_sum / max(self.n, 1)), "n": self.n}


# ------------------------------------------------------------------------------------------ scores on the device
SEG_RECORD = np.dtype([("n11", "<i4"), ("n10", "<i4"), ("n01", "<i4"), ("n00", "<i4"), ("ap", "<f8"), ("mean", "<f4"),
                       ("lo", "<f4"), ("hi", "<f4"), ("thresholds", "<i4")])   # ca_seg_record (include/conceptattn.h)


class _DeviceRows:
    """The rows of a device tensor [*, width] that grows by ``chunk`` rows, and their download: ``n`` rows are taken,
    ``_take`` hands out the next ones, ``_rows`` downloads the rows taken so far ONCE (and not again until new ones were
    taken).  The three ``Device*Scores`` classes keep their records in one."""

    def __init__(self, width: int, dtype, device, chunk: int):
        self.device = torch.device(device)
        self.chunk = max(1, int(chunk))
        self.n = 0
        self._buf = torch.zeros(self.chunk, width, dtype=dtype, device=self.device)
        self._host = None            # (n, rows) of the last download

    def _take(self, n: int) -> torch.Tensor:
        need = self.n + n
        if need > self._buf.shape[0]:
            cap = -(-need // self.chunk) * self.chunk
            grown = torch.zeros(cap, self._buf.shape[1], dtype=self._buf.dtype, device=self.device)
            grown[:self.n] = self._buf[:self.n]      # (stream-ordered behind the launches that wrote them)
            self._buf = grown
        out = self._buf[self.n:need]
        self.n = need
        return out

    def _rows(self) -> np.ndarray:
        if self._host is None or self._host[0] != self.n:
            self._host = (self.n, self._buf[:self.n].cpu().numpy())
        return self._host[1]


class DeviceSegmentationScores(_DeviceRows):
    """``SegmentationScores`` whose per-image records stay on the device until somebody asks: ``reserve`` hands
    ``ops.seg_score`` the next records of a buffer that grows by ``chunk`` records, and ``to_host`` / ``result`` /
    ``all_reduce`` download the records written so far ONCE (and not again until new ones were reserved)."""

    def __init__(self, device="cuda:0", chunk: int = 256):
        super().__init__(SEG_RECORD.itemsize, torch.uint8, device, chunk)
        self._pixels: list = []      # label pixels per item (host)

    def reserve(self, n: int, label_pixels: int) -> torch.Tensor:
        """uint8 [n, 40]: the records of the next n items (each scored against ``label_pixels`` label pixels)."""
        self._pixels += [int(label_pixels)] * n
        return self._take(n)

    def records(self) -> np.ndarray:
        """The n records as a numpy array of SEG_RECORD, in item order: the one download."""
        return self._rows().view(SEG_RECORD).reshape(self.n)

    def to_host(self) -> SegmentationScores:
        """The counters the host path would hold after ``update`` on the same items: its (1 - m, m) against (1 - y, y)
        stacking counts every pixel where mask and label agree once per class plane."""
        rec = self.records()
        out = SegmentationScores()
        for r, n_px in zip(rec, self._pixels):
            agree = int(r["n11"]) + int(r["n00"])
            out.correct += 2 * agree
            out.labelled += 2 * n_px
            out.inter = out.inter + np.array([agree, agree])
            out.union = out.union + np.array([2 * n_px - agree, 2 * n_px - agree])
            out.ap_sum += float(r["ap"])
            out.n += 1
        return out

    def all_reduce(self) -> SegmentationScores:
        return self.to_host().all_reduce()

    def result(self) -> dict:
        return self.to_host().result()


# ------------------------------------------------------------------------------------------ sweep scores
SWEEP_SPACES = ("output", "cross_attention")


class SweepScores:
    """The running tables of the per-layer and per-timestep segmentation sweeps
    (experiments/per_layer_segmentation/test_segmentations_per_layer.py:164-243,
    experiments/per_timestep_segmentation/test_segmentations_per_time.py:75-174): per space (``output``,
    ``cross_attention``) arrays [n_levels, n_columns] of ``correct``, ``labelled``, ``ap_sum`` and ``n`` and
    [n_levels, n_columns, 2] of ``inter`` and ``union``, summed over images.  A column is a layer, or the extra last
    column of a sweep scored with ``layer_mean`` (the per-timestep script's "all layers at this level" row)."""

    def __init__(self, n_levels: int, n_layers: int):
        self.n_levels, self.n_columns = int(n_levels), int(n_layers)
        shape = (self.n_levels, self.n_columns)
        self.tables = {s: {"correct": np.zeros(shape), "labelled": np.zeros(shape), "inter": np.zeros(shape + (2,)),
                           "union": np.zeros(shape + (2,)), "ap_sum": np.zeros(shape), "n": np.zeros(shape, dtype=np.int64)}
                       for s in SWEEP_SPACES}

    def _add(self, space, level, column, cor, lab, inter, union, ap):
        t = self.tables[space]
        t["correct"][level, column] += cor
        t["labelled"][level, column] += lab
        t["inter"][level, column] += inter
        t["union"][level, column] += union
        t["ap_sum"][level, column] += ap
        t["n"][level, column] += 1

    def update(self, space: str, level: int, column: int, mask, coefficients, labels) -> dict:
        """The host route for one map: mask, coefficients (h, w) at the label resolution, labels (h, w) bool; what
        ``SegmentationScores.update`` computes, added to cell (level, column) of ``space``."""
        out = SegmentationScores().update(mask, coefficients, labels)
        self._add(space, level, column, out["correct"], out["labelled"], out["inter"], out["union"], out["ap"])
        return out

    def add_records(self, space: str, records, label_pixels: int, columns=None) -> "SweepScores":
        """ca_seg_record rows [n_levels, len(columns)] of ONE image (``columns``: all of them by default), with the
        (1 - m, m) double counting ``DeviceSegmentationScores.to_host`` documents: a pixel where mask and label agree
        counts once per class plane."""
        rec = np.asarray(records)
        columns = list(range(self.n_columns)) if columns is None else [int(c) for c in columns]
        rec = rec.reshape(self.n_levels, len(columns))
        t, n_px = self.tables[space], int(label_pixels)
        agree = rec["n11"].astype(np.int64) + rec["n00"].astype(np.int64)
        t["correct"][:, columns] += 2 * agree
        t["labelled"][:, columns] += 2 * n_px
        t["inter"][:, columns] += agree[..., None]
        t["union"][:, columns] += (2 * n_px - agree)[..., None]
        t["ap_sum"][:, columns] += rec["ap"]
        t["n"][:, columns] += 1
        return self

    def _vector(self) -> np.ndarray:
        return np.concatenate([np.asarray(self.tables[s][k], dtype=np.float64).reshape(-1) for s in SWEEP_SPACES
                               for k in ("correct", "labelled", "inter", "union", "ap_sum", "n")])

    def all_reduce(self) -> "SweepScores":
        """Sum the tables over ranks (no-op without an initialised process group)."""
        v = _all_reduce_vector(torch.from_numpy(self._vector()))
        if v is not None:
            v, o = v.numpy(), 0
            for s in SWEEP_SPACES:
                for k in ("correct", "labelled", "inter", "union", "ap_sum", "n"):
                    a = self.tables[s][k]
                    part = v[o:o + a.size].reshape(a.shape)
                    self.tables[s][k] = np.rint(part).astype(np.int64) if k == "n" else part.copy()
                    o += a.size
        return self

    def result(self, space: str = "output") -> dict:
        """pixAcc, mIoU, mAP as arrays [n_levels, n_columns] (the formulas of ``SegmentationScores.result``) and n."""
        t = self.tables[space]
        eps = np.spacing(1, dtype=np.float64)
        iou = t["inter"] / (eps + t["union"])
        return {"pixAcc": t["correct"] / (eps + t["labelled"]), "mIoU": iou.mean(axis=-1),
                "mAP": t["ap_sum"] / np.maximum(t["n"], 1), "n": t["n"].copy()}

    def rows(self, space: str = "output"):
        """(level, column, pixAcc, mIoU, mAP) in the scripts' CSV order: level by level, column by column."""
        r = self.result(space)
        for lv in range(self.n_levels):
            for col in range(self.n_columns):
                yield lv, col, float(r["pixAcc"][lv, col]), float(r["mIoU"][lv, col]), float(r["mAP"][lv, col])


class DeviceSweepScores(_DeviceRows):
    """``SweepScores`` whose records stay on the device until somebody asks: ``reserve`` hands ``ops.segtab_score`` the
    [n_levels * len(columns), 40] records of one call, and ``records`` / ``to_host`` / ``result`` / ``all_reduce``
    download everything written so far ONCE (and not again until new records were reserved)."""

    def __init__(self, n_levels: int, n_layers: int, device="cuda:0", chunk: int = 4096):
        super().__init__(SEG_RECORD.itemsize, torch.uint8, device, chunk)
        self.n_levels, self.n_columns = int(n_levels), int(n_layers)
        self._calls: list = []       # (space, first record, columns, label pixels) per reserve

    def reserve(self, space: str, label_pixels: int, columns=None) -> torch.Tensor:
        """uint8 [n_levels * len(columns), 40], level-major: the records of one image's maps in ``space``."""
        if space not in SWEEP_SPACES:
            raise ValueError(f"space: one of {SWEEP_SPACES}")
        columns = list(range(self.n_columns)) if columns is None else [int(c) for c in columns]
        self._calls.append((space, self.n, columns, int(label_pixels)))
        return self._take(self.n_levels * len(columns))

    def records(self) -> list:
        """[(space, columns, records [n_levels, len(columns)] of SEG_RECORD), ...] in reservation order: the one
        download."""
        rec = self._rows().view(SEG_RECORD).reshape(self.n)
        return [(s, cols, rec[o:o + self.n_levels * len(cols)].reshape(self.n_levels, len(cols)))
                for s, o, cols, _ in self._calls]

    def to_host(self) -> SweepScores:
        out = SweepScores(self.n_levels, self.n_columns)
        for (s, cols, rec), (_, _, _, n_px) in zip(self.records(), self._calls):
            out.add_records(s, rec, n_px, cols)
        return out

    def all_reduce(self) -> SweepScores:
        return self.to_host().all_reduce()

    def result(self, space: str = "output") -> dict:
        return self.to_host().result(space)

    def rows(self, space: str = "output"):
        return self.to_host().rows(space)


# ------------------------------------------------------------------------------------------ multi-class scores
def map_predictions_to_class_indices(index_map, class_of):
    """The class id of every cell of an argmax map: ``class_of[index_map]``, one table lookup (``class_of[k]`` is the
    class id of concept k: 0 for the background concepts, ``class_names.index(name)`` for a present class).  The
    reference's ``map_predictions_to_voc_class_indices`` (run_multi_class_seg_experiment.py:25-37) remaps in place, class
    after class, so a cell already mapped to class id v is remapped again when a later concept index equals v; this is
    the one-step table it means.  A tensor gives an int64 tensor, anything else an int64 array."""
    table = np.asarray([int(c) for c in class_of], dtype=np.int64)
    if isinstance(index_map, torch.Tensor):
        return torch.from_numpy(table)[index_map.detach().cpu().long()]
    return table[np.asarray(index_map).astype(np.int64)]


def multiclass_table(background_concepts, target_concepts, class_names) -> list:
    """class_of for the concept list ``background_concepts + target_concepts``: 0 for every background concept,
    ``class_names.index(name)`` for every present class (ValueError for a name ``class_names`` does not hold)."""
    names = list(class_names)
    missing = [c for c in target_concepts if c not in names]
    if missing:
        raise ValueError(f"present classes {missing} are not in class_names")
    return [0] * len(background_concepts) + [names.index(c) for c in target_concepts]


class MultiClassScores:
    """Running pixAcc / mIoU / per-class IoU of the multi-class harness (run_multi_class_seg_experiment.py:137-140,
    207-233): exact integer counters ``correct``, ``labelled``, ``inter[nclass]``, ``union[nclass]`` and ``n``."""

    def __init__(self, nclass: int):
        self.nclass = int(nclass)
        self.correct = 0
        self.labelled = 0
        self.inter = np.zeros(self.nclass, dtype=np.int64)
        self.union = np.zeros(self.nclass, dtype=np.int64)
        self.n = 0

    def update(self, class_map, labels, ignore_index=None) -> dict:
        """class_map, labels: (H, W) class ids at the label resolution.  Over the pixels with ``labels != ignore_index``
        (None: all of them, as the harness behaves): labelled, correct, and per class c < nclass the pixels with
        class == label == c and with class == c or label == c.  A label >= nclass that is not ignored is labelled, never
        correct and in the union of the predicted class only (VOC's 255 border)."""
        p = np.asarray(_np(class_map)).astype(np.int64)
        y = np.asarray(_np(labels)).astype(np.int64)
        if p.shape != y.shape:
            raise ValueError(f"class map {p.shape} and labels {y.shape} differ in shape")
        keep = np.ones(y.shape, dtype=bool) if ignore_index is None else y != int(ignore_index)
        p, y = p[keep], y[keep]
        hit = p == y
        inter = np.bincount(p[hit & (p < self.nclass)], minlength=self.nclass)[:self.nclass]
        union = np.bincount(p[p < self.nclass], minlength=self.nclass)[:self.nclass] + \
            np.bincount(y[y < self.nclass], minlength=self.nclass)[:self.nclass] - inter
        cor, lab = int(hit.sum()), int(y.size)
        self.correct += cor
        self.labelled += lab
        self.inter = self.inter + inter
        self.union = self.union + union
        self.n += 1
        return {"correct": cor, "labelled": lab, "inter": inter, "union": union}

    def add_counts(self, counts) -> "MultiClassScores":
        """One item's int32 [2 + 2 nclass] row of ca_mseg_score: correct, labelled, inter[nclass], union[nclass]."""
        c = np.asarray(counts).astype(np.int64).reshape(-1)
        if c.size != 2 + 2 * self.nclass:
            raise ValueError(f"a row of {c.size} counts for nclass = {self.nclass}")
        self.correct += int(c[0])
        self.labelled += int(c[1])
        self.inter = self.inter + c[2:2 + self.nclass]
        self.union = self.union + c[2 + self.nclass:]
        self.n += 1
        return self

    def all_reduce(self) -> "MultiClassScores":
        """Sum the counters over ranks (no-op without an initialised process group)."""
        v = _all_reduce_vector(torch.tensor([self.correct, self.labelled, self.n, *self.inter, *self.union],
                                            dtype=torch.int64))
        if v is not None:
            v = v.numpy()
            self.correct, self.labelled, self.n = int(v[0]), int(v[1]), int(v[2])
            self.inter, self.union = v[3:3 + self.nclass].copy(), v[3 + self.nclass:].copy()
        return self

    def result(self) -> dict:
        """pixAcc = correct / (spacing(1) + labelled); mIoU = the sum of inter / union over the classes with union > 0,
        divided by (their number + 1e-6) (run_multi_class_seg_experiment.py:225-233); IoU: the per-class vector, NaN for a
        class with an empty union."""
        eps = np.spacing(1, dtype=np.float64)
        seen = self.union > 0
        iou = np.full(self.nclass, np.nan)
        iou[seen] = self.inter[seen].astype(np.float64) / self.union[seen].astype(np.float64)
        miou = 0.0
        for c in range(self.nclass):          # (the harness's loop, in its order)
            if self.union[c] == 0:
                continue
            miou += float(self.inter[c]) / float(self.union[c])
        miou /= (int(seen.sum()) + 1e-6)
        return {"pixAcc": float(np.float64(1.0) * self.correct / (eps + self.labelled)), "mIoU": float(miou), "IoU": iou,
                "n": self.n}


class DeviceMultiClassScores(_DeviceRows):
    """``MultiClassScores`` whose per-image count rows stay on the device until somebody asks: ``reserve`` hands
    ``ops.mseg_score`` the next int32 [2 + 2 nclass] rows of a buffer that grows by ``chunk`` rows, and ``records`` /
    ``to_host`` / ``result`` / ``all_reduce`` download the rows written so far ONCE (and not again until new ones were
    reserved).  ``ids[r]`` is what the caller named row r (``score_multiclass_images``: the image's position in its call,
    since images of different concept counts are scored in different forwards)."""

    def __init__(self, nclass: int, device="cuda:0", chunk: int = 256):
        self.nclass = int(nclass)
        self.width = 2 + 2 * self.nclass
        super().__init__(self.width, torch.int32, device, chunk)
        self.ids: list = []

    def reserve(self, n: int, ids=None) -> torch.Tensor:
        """int32 [n, 2 + 2 nclass]: the rows of the next n items."""
        self.ids += list(range(self.n, self.n + n)) if ids is None else list(ids)
        return self._take(n)

    def records(self) -> np.ndarray:
        """int32 [n, 2 + 2 nclass] in reservation order (``ids``): the one download."""
        return self._rows()

    def to_host(self) -> MultiClassScores:
        out = MultiClassScores(self.nclass)
        for row in self.records():
            out.add_counts(row)
        return out

    def all_reduce(self) -> MultiClassScores:
        return self.to_host().all_reduce()

    def result(self) -> dict:
        return self.to_host().result()


# what score_images and the multi-class methods accept as **encode_kwargs: the settings a caller chooses under the harness's
# names (``layers`` for layer_indices), and the per-call ``noise`` / ``vae_noise``
_ENCODE_KEYS = {"layers", "noise", "vae_noise"} | {f.name for f in fields(EncodeSettings) if f.init} - {
    "layer_indices", "stop_after_multi_modal_attentions"}


def encode_settings(kw: dict, what: str = "encode_settings", pipeline=None, concepts=()) -> EncodeSettings:
    """The settings record of a harness call's keywords ``kw`` (keys of _ENCODE_KEYS; ``noise`` / ``vae_noise`` are not
    settings and stay in ``kw``), with EncodeSettings' defaults and checks: against ``pipeline``'s depth and the per-item
    ``concepts`` lists where they are given.  TypeError, under the name ``what``, for any other key."""
    unknown = set(kw) - _ENCODE_KEYS
    if unknown:
        raise TypeError(f"{what}: unexpected arguments {sorted(unknown)}")
    given = {"layer_indices" if k == "layers" else k: v for k, v in kw.items() if k not in ("noise", "vae_noise")}
    return EncodeSettings(**given, depth=None if pipeline is None else pipeline.params.depth,
                          n_concepts=max((len(c) for c in concepts), default=0))


def _encode_chunks(pipe, images, concepts, captions, settings: EncodeSettings, kw: dict):
    """``pipe._encode_chunks`` for a harness call (``kw``: its encode_kwargs): the accumulators stay on the device."""
    return pipe._encode_chunks(images, concepts, list(captions[:len(images)]), settings, noise=kw.get("noise"),
                               vae_noise=kw.get("vae_noise"))


def _scoring_inputs(concepts, target_concepts, labels, size: int, apply_blur: bool) -> tuple:
    """(per_item, target, lab, blur) of score_images and score_sweep: every item's concept list (``concepts``: one list for
    all items or one per item), the index of its target concept in it (ValueError when missing), its label as a uint8 array
    (size, size), nonzero = positive (ValueError naming ``labels[i]`` otherwise), and the device's blur weights or None."""
    n = len(target_concepts)
    per_item = list(concepts) if concepts and not isinstance(concepts[0], str) else [list(concepts)] * n
    target = [per_item[i].index(target_concepts[i]) for i in range(n)]
    lab = []
    for i, y in enumerate(labels):
        y = np.asarray(_np(y))
        if y.shape != (size, size) or y.dtype not in (np.uint8, np.bool_):
            raise ValueError(f"labels[{i}]: expected a uint8 / bool array ({size}, {size}), got {y.dtype} {y.shape}")
        lab.append(y.astype(np.uint8, copy=False))
    return per_item, target, lab, ops.seg_blur_weights() if apply_blur else None


# ------------------------------------------------------------------------------------------ model wrapper
class ConceptAttentionSegmentationModel:
    """Callable with the reference's segmentation-model contract (segmentation.py:34-81):
    ``model(images, target_concepts, concepts, captions, mean_value_threshold=True, joint_attention_kwargs=None,
    apply_blur=False, **kwargs) -> (all_masks, all_coefficients, reconstructed_images)``.
    ``images`` are latents (1,16,h/8,w/8) or, with an autoencoder injected into the pipeline, PIL images."""

    def __init__(self, pipeline):
        self.pipeline = pipeline

    @torch.no_grad()
    def segment_individual_image(self, image, concepts, caption, layers=list(range(15, 19)), num_samples: int = 1,
                                 num_steps: int = 4, noise_timestep: int = 2, seed: int = 0, height: int = 1024,
                                 width: int = 1024, target_space: str = "output", joint_attention_kwargs=None,
                                 **_unused):
        return self.segment_images([image], [concepts], [caption], layers, num_samples, num_steps, noise_timestep, seed, height,
                                   width, target_space, joint_attention_kwargs)[0]   # (encode_image is encode_images of one)

    @torch.no_grad()
    def segment_images(self, images, concepts, captions, layers=list(range(15, 19)), num_samples: int = 1,
                       num_steps: int = 4, noise_timestep: int = 2, seed: int = 0, height: int = 1024,
                       width: int = 1024, target_space: str = "output", joint_attention_kwargs=None, batch: int = 5,
                       **_unused):
        """``segment_individual_image`` for a list of images through ``pipeline.encode_images``: up to ``batch`` images
        per forward, every image with the coefficients of its own call."""
        kw = dict(layers=layers, num_samples=num_samples, num_steps=num_steps, noise_timestep=noise_timestep, seed=seed,
                  height=height, width=width, joint_attention_kwargs=joint_attention_kwargs, batch=batch)
        return [(maps, None) for maps in self._encoded_maps(images, concepts, captions, encode_settings(kw), kw, target_space)]

    def _encoded_maps(self, images, concepts, captions, settings: EncodeSettings, kw: dict, target_space: str) -> list:
        """Per image the fp32 maps (C, side, side) of ``target_space`` on the host, from ``pipeline.encode_images`` under
        ``settings`` and the ``noise`` / ``vae_noise`` of the encode_kwargs ``kw``."""
        outs = self.pipeline.encode_images(images, concepts, list(captions[:len(images)]), noise=kw.get("noise"),
                                           vae_noise=kw.get("vae_noise"), return_pil_heatmaps=False, **settings.keywords())
        return [torch.as_tensor(np.asarray(o.concept_heatmaps if target_space == "output" else o.cross_attention_maps),
                                dtype=torch.float32) for o in outs]

    @torch.no_grad()
    def score_images(self, images, target_concepts, concepts, captions, labels, scores, size: int = 224,
                     downscale_for_eval: bool = False, apply_blur: bool = False, mean_value_threshold: bool = True,
                     target_space: str = "output", return_masks: bool = False, **encode_kwargs):
        """Encode ``images`` and score every target concept's map against its label without leaving the device: the
        chunks of ``pipeline.encode_images`` (``batch`` images per forward), each chunk's target planes straight from the
        device accumulators into ``ops.seg_score``, the records into ``scores`` (a ``DeviceSegmentationScores``).
        ``labels``: per image a uint8 / bool array (size, size), nonzero = positive (resizing label files stays the
        caller's job, as in the harness).  ``encode_kwargs``: what ``segment_images`` takes (layers, num_samples,
        num_steps, noise_timestep, seed, height, width, batch, joint_attention_kwargs) and ``noise`` / ``vae_noise`` /
        ``attention_norm`` / ``softmax`` of ``encode_images``.  Nothing per image comes back unless ``return_masks``:
        then ``(all_masks, all_coefficients)`` as ``__call__`` returns them, at map resolution (one download at the end).
        Maps of more than 4096 cells raise a ValueError: ``__call__`` + ``prepare_for_scoring`` +
        ``SegmentationScores.update`` remain for them, and for ``target_concepts=None``."""
        if target_concepts is None:
            raise ValueError("score_images scores one target concept per image; multi-class masks go through __call__")
        images = list(images)
        n = len(images)
        if not (len(target_concepts) == len(labels) == n and len(captions) >= n):
            raise ValueError(f"score_images: {n} images need {n} target concepts, labels and captions")
        if target_space not in ("output", "cross_attention"):
            raise ValueError("target_space: 'output' or 'cross_attention'")
        pipe = self.pipeline
        per_item, target, lab, blur = _scoring_inputs(concepts, target_concepts, labels, size, apply_blur)
        settings = encode_settings(encode_kwargs, "score_images", pipe, per_item)
        masks, planes, order = [], [], []
        with torch.cuda.device(pipe.device):
            for idx, acc_o, acc_c in _encode_chunks(pipe, images, concepts, captions, settings, encode_kwargs):
                acc = acc_o if target_space == "output" else acc_c
                maps = [acc[k, target[i]] for k, i in enumerate(idx)]
                y = torch.from_numpy(np.stack([lab[i] for i in idx])).pin_memory().to(pipe.device, non_blocking=True)
                m_out = torch.empty(len(idx), *maps[0].shape, dtype=torch.uint8, device=pipe.device) if return_masks else None
                ops.seg_score(maps, list(y), scores.reserve(len(idx), size * size), mean_value_threshold=mean_value_threshold,
                              downscale_for_eval=downscale_for_eval, blur_weights=blur, mask_out=m_out)
                if return_masks:
                    masks.append(m_out), planes.append(torch.stack(maps)), order.extend(idx)
        if not return_masks:
            return None
        masks, planes = torch.cat(masks).cpu().numpy().astype(bool), torch.cat(planes).cpu()
        if apply_blur:
            planes = gaussian_blur3(planes)      # (what __call__ hands out; the kernel's mask is of its own blur)
        planes = planes.numpy()
        back = {i: k for k, i in enumerate(order)}
        return [masks[back[i]] for i in range(n)], [planes[back[i]] for i in range(n)]

    @torch.no_grad()
    def score_sweep(self, images, target_concepts, concepts, captions, labels, scores, noise_levels,
                    mean_value_threshold: bool = True, downscale_for_eval: bool = False, apply_blur: bool = False,
                    size: int = 224, normalize: bool = True, layer_mean: bool = False, target_space=None, **sweep_kwargs):
        """The per-layer and per-timestep segmentation sweeps without leaving the device: per image the two tables of
        ``pipeline.layer_noise_sweep`` ([levels, layers, C, side, side]), then per space ONE ``ops.segtab_score`` call
        that scores the target concept's levels x layers maps against the image's label; the records go into ``scores``
        (a ``DeviceSweepScores`` of len(noise_levels) levels and as many columns as layers, plus one with
        ``layer_mean``).  ``layer_mean=True`` adds a second call per space on ``table.mean(dim=1)``, formed by torch on
        the device and scored into the extra last column: the per-timestep script's "all layers at this level" row.
        ``normalize=False`` scores the raw coefficients, as the per-layer script does (its call is ``noise_levels=[t]``,
        ``normalize=False``).  ``target_space``: "output", "cross_attention", or None for both.  ``labels``: per image a
        uint8 / bool array (size, size), nonzero = positive.  ``sweep_kwargs``: what ``layer_noise_sweep`` takes
        (num_steps, layer_indices, num_samples, seed, width, height, batch) and ``vae_noise``, one tensor per image.
        Nothing per image comes back.  Maps of more than 4096 cells raise a ValueError: ``SweepScores.update`` remains
        for them, and for the per-timestep script's bilinear resize of the coefficients."""
        images = list(images)
        n = len(images)
        if target_concepts is None or not (len(target_concepts) == len(labels) == n and len(captions) >= n):
            raise ValueError(f"score_sweep: {n} images need {n} target concepts, labels and captions")
        spaces = SWEEP_SPACES if target_space is None else (target_space,)
        if any(s not in SWEEP_SPACES for s in spaces):
            raise ValueError("target_space: 'output', 'cross_attention' or None for both")
        kw = dict(sweep_kwargs)
        if kw.pop("query_maps", None):
            raise ValueError("score_sweep: query_maps are not part of the sweep tables (ask encode_images for them)")
        if kw.pop("propagate", None):
            raise ValueError("score_sweep: propagated maps are not part of the sweep tables (ask encode_images for them)")
        unknown = set(kw) - {"num_steps", "layer_indices", "num_samples", "seed", "width", "height", "batch", "vae_noise"}
        if unknown:
            raise TypeError(f"score_sweep: unexpected arguments {sorted(unknown)}")
        vae_noise = kw.pop("vae_noise", None)
        if vae_noise is not None and len(vae_noise) != n:
            raise ValueError(f"score_sweep: vae_noise has {len(vae_noise)} entries for {n} images")
        pipe = self.pipeline
        side_h, side_w = kw.get("height", 1024) // 16, kw.get("width", 1024) // 16
        if side_h * side_w > L.SEG_MAX_CELLS:
            raise ValueError(f"score_sweep: maps of {side_h} x {side_w} cells; the device route takes up to "
                             f"{L.SEG_MAX_CELLS} (layer_noise_sweep + SweepScores.update remain for larger maps)")
        layer_indices = kw.get("layer_indices")
        n_layers = pipe.params.depth if layer_indices is None else len(layer_indices)
        levels = [int(v) for v in noise_levels]
        if (scores.n_levels, scores.n_columns) != (len(levels), n_layers + int(bool(layer_mean))):
            raise ValueError(f"score_sweep: scores holds {scores.n_levels} x {scores.n_columns} cells; the sweep has "
                             f"{len(levels)} levels and {n_layers} layers" + (" plus the layer mean" if layer_mean else ""))
        per_item, target, lab, blur = _scoring_inputs(concepts, target_concepts, labels, size, apply_blur)
        flags = dict(mean_value_threshold=mean_value_threshold, downscale_for_eval=downscale_for_eval, blur_weights=blur,
                     normalize=normalize)
        with torch.cuda.device(pipe.device):
            cells = ops.segtab_cells(side_h, side_w, pipe.device)
            for i in range(n):
                tabs = pipe.layer_noise_sweep(images[i], per_item[i], captions[i], levels,
                                              vae_noise=None if vae_noise is None else vae_noise[i], **kw)
                y = torch.from_numpy(lab[i]).pin_memory().to(pipe.device, non_blocking=True)
                for space in spaces:
                    table = tabs[SWEEP_SPACES.index(space)]                     # [levels, layers, C, side, side]
                    ops.segtab_score(table.reshape(-1, *table.shape[2:]), target[i], y,
                                     scores.reserve(space, size * size, range(n_layers)), cells, **flags)
                    if layer_mean:
                        ops.segtab_score(table.mean(dim=1), target[i], y, scores.reserve(space, size * size, [n_layers]),
                                         cells, **flags)
        return None

    def _multiclass_arguments(self, what, images, captions, background_concepts, target_concepts, target_space, kw):
        n = len(images)
        if isinstance(captions, str) or len(captions) < n:
            raise ValueError(f"{what}: {n} images need {n} captions")
        if target_concepts is None or len(target_concepts) != n or any(isinstance(t, str) for t in target_concepts):
            raise ValueError(f"{what}: target_concepts is one list of present classes per image ({n} images)")
        if target_space not in ("output", "cross_attention"):
            raise ValueError("target_space: 'output' or 'cross_attention'")
        concepts = [list(background_concepts) + list(t) for t in target_concepts]
        return concepts, encode_settings(kw, what, self.pipeline, concepts)

    @torch.no_grad()
    def segment_multiclass(self, images, captions, background_concepts, target_concepts, apply_blur: bool = False,
                           target_space: str = "output", **encode_kwargs):
        """The reference's ``FluxMultiClassSegmentation.__call__`` (multi_class_segmentation.py:58-79) for a list of
        images, on the host: per image ``(predicted_concepts, concept_heatmaps, None)`` with the fp32 maps
        (K, side, side) of the concepts ``background_concepts + target_concepts[i]`` (blurred with ``apply_blur``) and
        their argmax over the concepts, int64 (side, side).  ``target_concepts``: one list of present classes per image;
        the images go through ``pipeline.encode_images``, those with one concept count ``batch`` at a time.
        ``encode_kwargs``: what ``score_images`` takes."""
        images = list(images)
        concepts, settings = self._multiclass_arguments("segment_multiclass", images, captions, background_concepts,
                                                        target_concepts, target_space, encode_kwargs)
        results = []
        for maps in self._encoded_maps(images, concepts, captions, settings, encode_kwargs, target_space):
            if apply_blur:
                maps = gaussian_blur3(maps)
            results.append((maps.argmax(dim=0), maps, None))
        return results

    @torch.no_grad()
    def score_multiclass_images(self, images, captions, background_concepts, target_concepts, class_names, labels, scores,
                                ignore_index=None, apply_blur: bool = False, concept_scale_values=None,
                                target_space: str = "output", return_predictions: bool = False, **encode_kwargs):
        """The multi-class (Pascal VOC) evaluation loop of the reference (run_multi_class_seg_experiment.py:143-233)
        without leaving the device: the chunks of ``pipeline.encode_images``, each item's (K, side, side) planes straight
        from the device accumulator into ``ops.mseg_score`` (argmax, class table, nearest resize to the label, counts),
        the count rows into ``scores`` (a ``DeviceMultiClassScores`` of ``len(class_names)`` classes; its ``ids`` name
        the image of every row).  ``target_concepts``: one list of present classes per image, each a name of
        ``class_names``; the background concepts count as class 0.  ``labels``: per image a uint8 array of class ids, all
        of one shape (resizing label files stays the caller's job, as in the harness); ``ignore_index``: the label value
        that is skipped, None for none (the harness skips none).  ``concept_scale_values``: per image None or one factor
        per concept, multiplied onto the planes before the argmax (the harness's unimplemented argument).  Nothing per
        image comes back unless ``return_predictions``: then the class maps, uint8 (side, side) per image, in one download
        at the end.  Maps of more than 16384 cells raise a ValueError."""
        images = list(images)
        n = len(images)
        what = "score_multiclass_images"
        concepts, settings = self._multiclass_arguments(what, images, captions, background_concepts, target_concepts,
                                                        target_space, encode_kwargs)
        if len(labels) != n:
            raise ValueError(f"{what}: {n} images need {n} labels")
        class_names = list(class_names)
        if not 1 <= len(class_names) <= L.MSEG_MAX_CLASSES or getattr(scores, "nclass", None) != len(class_names):
            raise ValueError(f"{what}: class_names holds 1..{L.MSEG_MAX_CLASSES} names and scores counts as many classes")
        tables = [multiclass_table(background_concepts, t, class_names) for t in target_concepts]
        if any(not 1 <= len(c) <= L.MSEG_MAX_CONCEPTS for c in concepts):
            raise ValueError(f"{what}: an image takes 1..{L.MSEG_MAX_CONCEPTS} concepts (background and present classes)")
        side_h, side_w = settings.height // 16, settings.width // 16
        if side_h * side_w > L.MSEG_MAX_CELLS:
            raise ValueError(f"{what}: maps of {side_h} x {side_w} cells; the device route takes up to {L.MSEG_MAX_CELLS} "
                             "(segment_multiclass + MultiClassScores.update remain for larger maps)")
        lab = []
        for i, y in enumerate(labels):
            y = np.asarray(_np(y))
            if y.ndim != 2 or y.dtype != np.uint8 or (lab and y.shape != lab[0].shape):
                raise ValueError(f"labels[{i}]: expected a uint8 array of class ids (size, size), all labels of one shape, "
                                 f"got {y.dtype} {y.shape}")
            lab.append(y)
        scales = [None] * n
        if concept_scale_values is not None:
            if len(concept_scale_values) != n:
                raise ValueError(f"{what}: concept_scale_values is one entry per image ({n} images)")
            for i, v in enumerate(concept_scale_values):
                if v is not None:
                    scales[i] = tuple(float(x) for x in v)
                    if len(scales[i]) != len(concepts[i]):
                        raise ValueError(f"{what}: concept_scale_values[{i}] needs one factor per concept ({len(concepts[i])})")
        pipe = self.pipeline
        blur = ops.seg_blur_weights() if apply_blur else None
        preds, order = [], []
        with torch.cuda.device(pipe.device):
            for idx, acc_o, acc_c in _encode_chunks(pipe, images, concepts, captions, settings, encode_kwargs):
                acc = acc_o if target_space == "output" else acc_c
                y = torch.from_numpy(np.stack([lab[i] for i in idx])).pin_memory().to(pipe.device, non_blocking=True)
                groups = {}                      # the items of a launch share one scale
                for k, i in enumerate(idx):
                    groups.setdefault(scales[i], []).append(k)
                for sc, ks in groups.items():
                    c_out = torch.empty(len(ks), *acc.shape[2:], dtype=torch.uint8, device=pipe.device) \
                        if return_predictions else None
                    ops.mseg_score([acc[k] for k in ks], [y[k] for k in ks], scores.reserve(len(ks), [idx[k] for k in ks]),
                                   [tables[idx[k]] for k in ks], len(class_names), ignore_index=ignore_index, scale=sc,
                                   blur_weights=blur, class_out=c_out)
                    if return_predictions:
                        preds.append(c_out), order.extend(idx[k] for k in ks)
        if not return_predictions:
            return None
        preds = torch.cat(preds).cpu().numpy()
        back = {i: k for k, i in enumerate(order)}
        return [preds[back[i]] for i in range(n)]

    def __call__(self, images, target_concepts, concepts, captions, mean_value_threshold: bool = True,
                 joint_attention_kwargs=None, apply_blur: bool = False, **kwargs):
        if not isinstance(images, (list, tuple)):
            images = [images]
        all_masks, all_coefficients, reconstructed = [], [], []
        batched = None
        if len(images) > 1 and hasattr(self.pipeline, "encode_images"):   # several images share every forward
            batched = self.segment_images(images, concepts, captions, joint_attention_kwargs=joint_attention_kwargs,
                                          **kwargs)
        for i, image in enumerate(images):
            coeff, recon = batched[i] if batched is not None else self.segment_individual_image(
                image, concepts, captions[i], joint_attention_kwargs=joint_attention_kwargs, **kwargs)
            if apply_blur:
                coeff = gaussian_blur3(coeff)
            if target_concepts is None:
                all_masks.append(mean_threshold_masks(coeff))
                all_coefficients.append(coeff)
            else:
                k = concepts.index(target_concepts[i])
                all_masks.append(target_mask(coeff, k, mean_value_threshold).numpy())
                all_coefficients.append(coeff[k].numpy())
            reconstructed.append(recon)
        return all_masks, all_coefficients, reconstructed


def gaussian_blur3(x: torch.Tensor, sigma: float = 1.0) -> torch.Tensor:
    """3x3 Gaussian blur with reflect padding of a (C, h, w) map (torchvision's gaussian_blur(kernel_size=3,
    sigma=1.0), used at segmentation.py:61)."""
    k = torch.exp(-0.5 * (torch.tensor([-1.0, 0.0, 1.0]) / sigma) ** 2)
    k = (k / k.sum()).to(x.dtype)
    w = (k[:, None] * k[None, :])[None, None]
    xp = torch.nn.functional.pad(x[:, None], (1, 1, 1, 1), mode="reflect")
    return torch.nn.functional.conv2d(xp, w)[:, 0]
