"""Launch forms of ca_head_maps (conceptattention_amd/csrc/ca_headmap.hip), their fp64 reference and bounds.  Built on
tests/rowop_cases.py as tests/heatmap_many_cases.py is: Case, weighted, logits_reference, excess and U are that module's,
imported and not copied, and no constant of it is widened here.

Imported by tests/test_headmap_kernels_gpu.py (the device) and tests/test_headmap_cases_cpu.py (the fp64 reference against
an fp32 emulation of the kernel's summation order on the CPU, and the seeded slips that the bounds must reject).

A case is ONE launch of n problems that share L, C, NH (heads of 128 columns) and the norm.  Problem i has its own vectors
(seed + 10 i), its own dtypes (heatmap_many_cases.FORMS[i % 3]; two cases name other pairs), row strides above the width
with NaN in the padding, and the outputs the case names.  The vectors are built PER HEAD so that a head's logits fall into rowop_cases.norm_logits'
families by (p + h) % 7 (two heads of one patch differ, so a head mix-up shows): column 0 of every concept row's head is 1,
column 1 a small integer, column 2 uniform in [-1, 1], the rest random, and the image row's head is
  0, 5, 6  unit scale (random);
  1        0.625 e0: all C tied, exactly;
  2        0.5 e0 + e1: partial ties, exactly;
  3        300 e2 plus a random row: spread +-300;
  4        250 e0 plus a random row: a shared offset of +250.
`dup`: concept row 1 repeats row 0.

Bounds, for the kernel's own order (ca_headmap.hip's header comment):
  z      rowop_cases.logits_reference's form, 2 (fmas per lane + butterfly levels + 1) U sum |con img| with 8 fmas per
         lane and the 4-level butterfly of a head's 16 lanes: 26 U S.
  w      rowop_cases.weighted(z, e_z, norm, 1, 0): its bound before the store (it charges the product with the weight and
         the add, 4 U |w|, which the kernel's v * (1 / sum) and the store of w into the head sum are covered by).
         norm "none": w = z, e_w = e_z.
  heads  start + WH w: WH e_w + 2 U |WH w| + 2 U |result|  (weighted's own accumulate terms).
  mean   (1 / NH) sum_h w_h: (1 / NH) (sum_h e_w + (NH - 1 + 2) U sum_h |w_h|) + 2 U |mean|; NH - 1 adds in head order
         inside a lane group and across the chunks, 2 levels of exchange (lanes ^ 16, ^ 32); the last term is the fp32
         1 / NH and the product with it.
  acc    start + W1 mean by one fma: W1 e_mean + 2 U |W1 mean| (the fp32 weight and nothing else) + U |result| (the one
         rounding of the fma on the start value).
  acc2   starts at zero with weight 1, so it holds the mean itself: e_mean + U |mean| alone.
Accumulators start at N(0, 0.5) (acc, heads) and at zero (acc2)."""
from __future__ import annotations

import math

import torch

import heatmap_many_cases as M
import rowop_cases as R
from rowop_cases import Case, U, excess, logits_reference, weighted  # noqa: F401

FORMS = M.FORMS
WH, W1, W2 = 0.8, 0.45, 1.0                     # weight of heads / acc / acc2 (acc2 starts at zero: the map itself)
OUTS = {"heads": ("heads",), "acc": ("acc",), "acc2": ("acc2",), "all": ("heads", "acc", "acc2")}
NORMS = ("none", "softmax", "sparsemax", "entmax15")
FMAS, LEVELS, HEAD_LEVELS = 8, 4, 2             # per lane and head; butterfly levels of a head; exchanges of the head sum
Z_COEF = 2 * (FMAS + LEVELS + 1)


def kernel_of(C: int) -> str:
    return f"ca_headmap_kernel<{8 if C <= 8 else 16 if C <= 16 else 32}>"


def _hd(NH, L, C, norm, n=1, outs="all", pad=(8, 16), dup=False, seed=0, forms=FORMS):
    name = f"heads_NH{NH}_L{L}_C{C}_{norm}_n{n}_{outs}" + ("_dup" if dup else "") + \
        ("" if forms is FORMS else "_" + "+".join(f"{a}.{b}" for a, b in forms))
    W = NH * 128
    return Case(name, "ca_head_maps", kernel_of(C), "headmap",
                dict(NH=NH, L=L, C=C, norm=norm, n=n, outs=outs, dim=W, ldi=W + pad[0], ldc=W + pad[1], dup=dup,
                     forms=forms), seed)


# NH = 1, 3, 4, 5, 23, 24, 32 (one head, a ragged last chunk, chunk boundaries, the model's, hidden 4096); L = 1, 2, 3, 257;
# C = 1, 8, 9, 16, 17, 32; 1 and 16 problems; every subset of outputs and all four norms
CASES = [
    _hd(1, 1, 1, "none", seed=300),
    _hd(1, 257, 8, "softmax", n=16, seed=301),
    _hd(1, 3, 8, "sparsemax", outs="acc", seed=302),
    _hd(1, 257, 8, "entmax15", outs="acc", seed=303),
    _hd(3, 257, 9, "softmax", seed=304),
    _hd(3, 2, 32, "none", n=16, outs="heads", seed=305),
    _hd(4, 257, 16, "sparsemax", n=16, seed=306),
    _hd(4, 3, 17, "entmax15", outs="acc2", seed=307),
    _hd(5, 257, 17, "none", n=16, seed=308),
    _hd(5, 1, 9, "sparsemax", outs="heads", seed=309),
    _hd(23, 257, 16, "entmax15", seed=310),
    _hd(23, 3, 16, "softmax", n=16, outs="acc", seed=311),
    _hd(24, 257, 32, "softmax", seed=312),
    _hd(24, 257, 12, "none", outs="acc2", seed=313),
    _hd(24, 2, 32, "sparsemax", n=16, seed=314),
    _hd(24, 257, 32, "entmax15", outs="acc", seed=315),
    _hd(32, 257, 9, "none", pad=(16, 8), seed=316),
    _hd(32, 3, 1, "softmax", n=16, outs="acc2", seed=317),
    _hd(24, 257, 12, "sparsemax", dup=True, seed=318),
    _hd(5, 257, 16, "softmax", dup=True, outs="heads", seed=319),
    # the fourth dtype pair, fp32 image rows with bf16 concept rows (the entry point takes the two flags independently)
    _hd(3, 257, 8, "sparsemax", forms=(("f32", "bf16"),), seed=320),
    _hd(5, 3, 17, "none", n=16, forms=(("f32", "bf16"), ("bf16", "f32")), seed=321),
]
BY_ID = {c.id: c for c in CASES}


# --------------------------------------------------------------------------------------------------- inputs
def _vectors(C, Lp, NH, seed, dup):
    con = R._randn((C, NH, 128), seed + 1, 1.5 / math.sqrt(128))
    con[:, :, 0] = 1.0
    con[:, :, 1] = torch.randint(0, 3, (C, NH), generator=R._gen(seed + 2)).double()
    con[:, :, 2] = torch.rand(C, NH, generator=R._gen(seed + 3), dtype=torch.float64) * 2 - 1
    if dup and C > 1:
        con[1] = con[0]
    img = R._randn((Lp, NH, 128), seed)
    img[:, :, :3] = 0.0
    fam = (torch.arange(Lp)[:, None] + torch.arange(NH)[None, :]) % 7
    img[fam == 1] = 0.0
    img[fam == 2] = 0.0
    e = torch.zeros(128, dtype=torch.float64)
    e1, e2 = e.clone(), e.clone()
    e1[0] = 0.625
    e2[0], e2[1] = 0.5, 1.0
    img[fam == 1] = e1
    img[fam == 2] = e2
    img[..., 2] = torch.where(fam == 3, torch.full_like(img[..., 2], 300.0), img[..., 2])
    img[..., 0] = torch.where(fam == 4, torch.full_like(img[..., 0], 250.0), img[..., 0])
    return img.reshape(Lp, NH * 128), con.reshape(C, NH * 128)


def make_inputs(case: Case) -> dict:
    """Host tensors of one case: a list of per-problem dicts (img / con row-strided with NaN padding, heads0 / acc0 /
    acc20 the accumulators' contents before the launch)."""
    s = case.shape
    probs = []
    for i in range(s["n"]):
        sd = case.seed + 10 * i
        it, ct = s["forms"][i % len(s["forms"])]
        img, con = _vectors(s["C"], s["L"], s["NH"], sd, s["dup"])
        probs.append(dict(img=R._padded(img.float() if it == "f32" else img.bfloat16(), s["ldi"]),
                          con=R._padded(con.float() if ct == "f32" else con.bfloat16(), s["ldc"]),
                          heads0=R._randn((s["NH"], s["C"], s["L"]), sd + 4, 0.5).float(),
                          acc0=R._randn((s["C"], s["L"]), sd + 5, 0.5).float(),
                          acc20=torch.zeros(s["C"], s["L"])))
    return dict(probs=probs)


# --------------------------------------------------------------------------------------------------- reference
def head_logits(img, con, NH):
    """fp64 z [NH, C, L] and S = sum |con img| of the same shape, from [L, NH*128] / [C, NH*128] rows."""
    i3 = img.double().reshape(img.shape[0], NH, 128)
    c3 = con.double().reshape(con.shape[0], NH, 128)
    z = torch.einsum("chd,phd->hcp", c3, i3)
    S = torch.einsum("chd,phd->hcp", c3.abs(), i3.abs())
    return z, S


def head_weights(z, e_z, norm):
    """fp64 w [NH, C, L] = norm over the concepts per head and patch, and its bound e_w (rowop_cases.weighted per head,
    all heads in one call: the concept axis first, heads and patches side by side)."""
    if norm == "none":
        return z, e_z
    NH, C, Lp = z.shape
    zz = z.permute(1, 0, 2).reshape(C, NH * Lp)
    ee = e_z.permute(1, 0, 2).reshape(C, NH * Lp)
    w, e_w = weighted(zz, ee, norm, 1.0, torch.zeros_like(zz))
    return w.reshape(C, NH, Lp).permute(1, 0, 2), e_w.reshape(C, NH, Lp).permute(1, 0, 2)


def mean_and_bound(w, e_w):
    NH = w.shape[0]
    mean = w.sum(0) / NH
    e_mean = (e_w.sum(0) + (NH - 1 + HEAD_LEVELS) * U * w.abs().sum(0)) / NH + 2 * U * mean.abs()
    return mean, e_mean


def f32(w: float) -> float:
    """A weight as the library receives it (a C float)."""
    return float(torch.tensor(w, dtype=torch.float32))


def reference(case: Case, inp: dict, dev="cpu") -> list:
    """fp64 reference of every output of every problem: [ {name: (ref, bound before the fp32 store, "f32")} ]."""
    s = case.shape
    out = []
    for pr in inp["probs"]:
        z, S = head_logits(pr["img"].to(dev)[:, :s["dim"]], pr["con"].to(dev)[:, :s["dim"]], s["NH"])
        e_z = Z_COEF * U * S
        w, e_w = head_weights(z, e_z, s["norm"])
        res = {}
        if "heads" in OUTS[s["outs"]]:
            o = pr["heads0"].to(dev).double() + WH * w
            res["heads"] = (o, WH * e_w + 2 * U * (WH * w).abs() + 2 * U * o.abs(), "f32")
        mean, e_mean = mean_and_bound(w, e_w)
        if "acc" in OUTS[s["outs"]]:
            o = pr["acc0"].to(dev).double() + W1 * mean
            res["acc"] = (o, W1 * e_mean + 2 * U * (W1 * mean).abs() + U * o.abs(), "f32")
        if "acc2" in OUTS[s["outs"]]:
            res["acc2"] = (mean, e_mean + U * mean.abs(), "f32")
        out.append(res)
    return out


# ----------------------------------------------------------------------------------- fp32 emulation (CPU)
def _fma(a, b, c):
    """fp32 fma(a, b, c): the product of two floats is exact in fp64; the add rounds to fp64 and then to fp32 (a double
    rounding that can differ from the fused one by one fp32 ulp in rare ties; the emulation is held to bounds, not bits)."""
    return (a.double() * b.double() + c.double()).float()


def emulate_logits(img, con, NH):
    """z [NH, C, L] in fp32 in the kernel's order: lane t of a head chains its 8 columns by fma, then the 4-level
    butterfly over the head's 16 lanes."""
    Lp, C = img.shape[0], con.shape[0]
    x = img.float().reshape(Lp, NH, 16, 8).permute(1, 0, 2, 3)[:, None]      # [NH, 1, L, 16, 8]
    b = con.float().reshape(C, NH, 16, 8).permute(1, 0, 2, 3)[:, :, None]    # [NH, C, 1, 16, 8]
    a = torch.zeros(NH, C, Lp, 16, dtype=torch.float32)
    for k in range(8):
        a = _fma(x[..., k].expand(NH, C, Lp, 16), b[..., k].expand(NH, C, Lp, 16), a)
    lane = torch.arange(16)
    for o in (1, 2, 4, 8):
        a = a + a[..., lane ^ o]
    return a[..., 0]


def _f32_weights(z, norm, slip=None):
    """fp32 weights over axis 0 of z [C, X]: the kernel's softmax is exp / sum as v * (1 / sum); the sparse norms are
    heatmap_many_cases' fp32 sort-and-threshold."""
    if norm == "none":
        return z
    if norm == "softmax":
        e = torch.exp(z - z.amax(0, keepdim=True))
        s = torch.zeros_like(e[0])
        for c in range(e.shape[0]):
            s = s + e[c]
        return e * (torch.tensor(1.0) / s)
    return M._f32_weighting(z, norm, None)


def emulate(case: Case, inp: dict, slip=None) -> list:
    """What ca_head_maps computes, in fp32 on the CPU, in its summation order.  `slip` seeds a mistake:
      "next head's columns"   head h reads head h + 1's columns (the last one wraps to the first);
      "last head dropped"     the last head takes no part (its plane of `heads` keeps its start value);
      "mean over NH - 1"      the mean divides by NH - 1;
      "norm after the mean"   the logits are averaged over the heads and weighted once;
      "softmax over heads"    the softmax runs across the heads instead of the concepts;
      "weight twice"          acc gets weight * weight, heads weight_h * weight_h;
      "acc2 given weight"     acc2 is updated with acc's weight."""
    s = case.shape
    NH, C, Lp, norm = s["NH"], s["C"], s["L"], s["norm"]
    wh, w1, w2 = (torch.tensor(v, dtype=torch.float32) for v in (WH, W1, W2))
    if slip == "weight twice":
        wh, w1 = wh * wh, w1 * w1
    if slip == "acc2 given weight":
        w2 = w1
    out = []
    for pr in inp["probs"]:
        z = emulate_logits(pr["img"][:, :s["dim"]], pr["con"][:, :s["dim"]], NH)          # [NH, C, L]
        if slip == "next head's columns":
            z = torch.roll(z, -1, 0)
        if slip == "norm after the mean":
            zm = z.sum(0) / NH
            w = _f32_weights(zm, norm)[None].expand(NH, C, Lp)
        elif slip == "softmax over heads":
            w = _f32_weights(z, norm)                                                      # (axis 0 = the heads)
        else:
            w = _f32_weights(z.permute(1, 0, 2).reshape(C, NH * Lp), norm).reshape(C, NH, Lp).permute(1, 0, 2)
        live = NH - 1 if slip == "last head dropped" else NH
        groups = []
        for g in range(4):                                                                 # lane group g: heads 4 j + g
            m = torch.zeros(C, Lp, dtype=torch.float32)
            for h in range(g, live, 4):
                m = m + w[h]
            groups.append(m)
        m = (groups[0] + groups[1]) + (groups[2] + groups[3])
        div = NH - 1 if slip == "mean over NH - 1" else NH
        mean = m * (torch.tensor(1.0) / torch.tensor(float(div)))
        res = {}
        if "heads" in OUTS[s["outs"]]:
            res["heads"] = pr["heads0"].clone()
            res["heads"][:live] = _fma(wh.expand_as(w[:live]), w[:live], pr["heads0"][:live])
        if "acc" in OUTS[s["outs"]]:
            res["acc"] = _fma(w1.expand_as(mean), mean, pr["acc0"])
        if "acc2" in OUTS[s["outs"]]:
            res["acc2"] = _fma(w2.expand_as(mean), mean, pr["acc20"])
        out.append(res)
    return out


SLIPS = {
    # name: (slip, cases to try, output that must expose it on at least one of them)
    "head h reads head h + 1's columns": ("next head's columns", ("heads_NH4_L257_C16_sparsemax_n16_all",
                                                                   "heads_NH5_L257_C17_none_n16_all"), "heads"),
    "the last head dropped": ("last head dropped", ("heads_NH3_L257_C9_softmax_n1_all",
                                                    "heads_NH24_L257_C32_softmax_n1_all"), "acc"),
    "the mean divides by NH - 1": ("mean over NH - 1", ("heads_NH24_L257_C32_softmax_n1_all",
                                                        "heads_NH5_L257_C17_none_n16_all"), "acc2"),
    "the norm applied after the head mean": ("norm after the mean", ("heads_NH3_L257_C9_softmax_n1_all",
                                                                     "heads_NH4_L257_C16_sparsemax_n16_all"), "acc2"),
    "softmax across heads instead of concepts": ("softmax over heads", ("heads_NH3_L257_C9_softmax_n1_all",
                                                                         "heads_NH24_L257_C32_softmax_n1_all"), "acc2"),
    "the weight applied twice": ("weight twice", ("heads_NH4_L257_C16_sparsemax_n16_all",
                                                  "heads_NH24_L257_C32_entmax15_n1_acc"), "acc"),
    "acc2 given weight": ("acc2 given weight", ("heads_NH24_L257_C12_none_n1_acc2",
                                                "heads_NH4_L3_C17_entmax15_n1_acc2"), "acc2"),
}


def over_the_bound(got: list, ref: list, only=None):
    """(largest err / bound, elements over the bound) over all problems and outputs (`only`: that output alone)."""
    worst, n_over = 0.0, 0
    for g, r in zip(got, ref):
        assert set(g) == set(r), (set(g), set(r))
        for name, (rv, pre, kind) in r.items():
            if only is None or name == only:
                ratio, n = excess(g[name], rv, pre, kind)
                worst, n_over = max(worst, ratio), n_over + n
    return worst, n_over
