"""Launch forms of ca_heatmap_many (conceptattention_amd/csrc/ca_heatmap_many.hip) and of the sparse weighting at 17 .. 32
concepts, their fp64 reference and bounds.  Built on tests/rowop_cases.py: Case, norm_logits, weighted, sparse_bound,
logits_reference and excess are that module's, imported and not copied, and so are the bounds (generic in C).

Imported by tests/test_heatmap_many_kernels_gpu.py (the device) and tests/test_heatmap_many_cases_cpu.py (the fp64
reference against an fp32 emulation of the kernel on the CPU, and the seeded slips that the bounds must reject).

A case is ONE launch of n problems that share L, C, dim and the norm.  Problem i has its own vectors (seed + 10 i), its
own dtypes (FORMS[i % 3]: the three pairs the three-launch form takes too), row strides above dim with NaN in the padding,
and the outputs the case names.  The vectors are built so that the logits fall into norm_logits' families by patch index
p % 7 (column 0 of every concept row is 1, column 1 a small integer, column 2 uniform in [-1, 1], the rest random):
  0, 5, 6  unit scale (random image row);
  1        all C tied, exactly (the image row is 0.625 e0);
  2        partial ties, exactly (0.5 e0 + e1: the logit is 0.5 + the concept's integer);
  3        spread +-300 (300 e2 plus a random row);
  4        a shared offset of +250 (250 e0 plus a random row).
`dup`: concept row 1 repeats row 0.

Bounds: the logits carry rowop_cases.logits_reference's bound (dim / 64 fmas per lane, the 6-level butterfly); the
weighting is rowop_cases.weighted with that bound passed in as e_z, as rowop_cases.fused_reference does it.  Checked on the
CPU at C = 9, 17 and 32 for all three norms (tests/test_heatmap_many_cases_cpu.py): the reference's rows sum to 1 within
2e-15, the sparse supports run from 1 to C, the largest weighting bound is 2.2e-5.  No constant of rowop_cases.py is
widened here."""
from __future__ import annotations

import math

import torch

import rowop_cases as R
from rowop_cases import Case, excess, logits_reference, norm_logits, sparse_bound, weighted  # noqa: F401

FORMS = (("bf16", "bf16"), ("bf16", "f32"), ("f32", "f32"))   # (image, concept) vectors of problem i % 3
W1, W2 = 0.45, 1.3                                             # weight of acc / acc2
OUTS = {"acc": ("acc",), "acc2": ("acc2",), "logits": ("logits",), "all": ("acc", "acc2", "logits")}


def kernel_of(C: int) -> str:
    return f"ca_heatmap_many_kernel<{8 if C <= 8 else 16 if C <= 16 else 32}>"


def _many(C, L, dim, norm, n=1, outs="all", pad=(8, 4), dup=False, seed=0):
    name = f"many_C{C}_L{L}_dim{dim}_{norm}_n{n}_{outs}" + ("_dup" if dup else "")
    return Case(name, "ca_heatmap_many", kernel_of(C), "many",
                dict(C=C, L=L, dim=dim, norm=norm, n=n, outs=outs, ldi=dim + pad[0], ldc=dim + pad[1], dup=dup), seed)


# C = 1, 8, 9, 16, 17, 24, 25, 31, 32; L = 1, 2, 3, 257; dim = 8, 264, 520, 3072, and 4096 with C = 32; 1 and 16 problems
CASES = [
    _many(1, 1, 8, "softmax", seed=200),
    _many(1, 257, 264, "entmax15", n=16, seed=201),
    _many(8, 257, 264, "sparsemax", seed=202),
    _many(8, 3, 3072, "softmax", n=16, outs="acc2", seed=203),
    _many(9, 257, 520, "softmax", n=16, seed=204),
    _many(9, 2, 3072, "sparsemax", outs="logits", seed=205),
    _many(16, 3, 264, "entmax15", outs="acc", seed=206),
    _many(16, 257, 520, "sparsemax", n=16, seed=207),
    _many(17, 257, 264, "sparsemax", n=16, seed=208),
    _many(17, 1, 520, "entmax15", seed=209),
    _many(24, 2, 3072, "entmax15", outs="acc2", seed=210),
    _many(24, 257, 8, "softmax", n=16, seed=211),
    _many(25, 257, 3072, "softmax", outs="logits", seed=212),
    _many(25, 3, 520, "sparsemax", n=16, outs="acc", seed=213),
    _many(31, 257, 520, "entmax15", n=16, seed=214),
    _many(32, 257, 4096, "sparsemax", pad=(8, 8), seed=215),            # 2 KB + 8 x 4096 x 4 bytes of LDS: the raised limit
    _many(32, 3, 8, "softmax", n=16, seed=216),
    _many(32, 257, 3072, "entmax15", n=16, seed=217),
    _many(12, 257, 3072, "sparsemax", dup=True, seed=218),
]

# the three-launch weighting at the concept counts ca_heatmap_sparse_kernel<32, .> serves
CASES += [
    Case(f"{norm}_C{C}", "ca_heatmap_norm_accumulate", f"ca_heatmap_sparse_kernel<32,{str(norm == 'entmax15').lower()}>",
         "norm", dict(norm=norm, C=C, L=257, w=w), 230 + C + (100 if norm == "entmax15" else 0))
    for norm in ("sparsemax", "entmax15") for C, w in ((17, 0.7), (24, 1.3), (32, 0.7))
]
BY_ID = {c.id: c for c in CASES}


# --------------------------------------------------------------------------------------------------- inputs
def _vectors(C, Lp, dim, seed, dup):
    con = R._randn((C, dim), seed + 1, 1.5 / math.sqrt(dim))
    con[:, 0] = 1.0
    con[:, 1] = torch.randint(0, 3, (C,), generator=R._gen(seed + 2)).double()
    con[:, 2] = torch.rand(C, generator=R._gen(seed + 3), dtype=torch.float64) * 2 - 1
    if dup and C > 1:
        con[1] = con[0]
    img = R._randn((Lp, dim), seed)
    img[:, :3] = 0.0
    fam = torch.arange(Lp) % 7
    img[fam == 1] = 0.0
    img[fam == 1, 0] = 0.625
    img[fam == 2] = 0.0
    img[fam == 2, 0], img[fam == 2, 1] = 0.5, 1.0
    img[fam == 3, 2] = 300.0
    img[fam == 4, 0] = 250.0
    return img, con


def make_inputs(case: Case) -> dict:
    """Host tensors of one case.  `many`: a list of per-problem dicts (img / con row-strided with NaN padding, acc0 /
    acc20 the accumulators' contents before the launch)."""
    if case.op != "many":
        return R.make_inputs(case)
    s = case.shape
    probs = []
    for i in range(s["n"]):
        sd = case.seed + 10 * i
        it, ct = FORMS[i % 3]
        img, con = _vectors(s["C"], s["L"], s["dim"], sd, s["dup"])
        probs.append(dict(img=R._padded(img.float() if it == "f32" else img.bfloat16(), s["ldi"]),
                          con=R._padded(con.float() if ct == "f32" else con.bfloat16(), s["ldc"]),
                          acc0=R._randn((s["C"], s["L"]), sd + 5, 0.5).float(),
                          acc20=R._randn((s["C"], s["L"]), sd + 6, 0.5).float()))
    return dict(probs=probs)


# --------------------------------------------------------------------------------------------------- reference
def reference(case: Case, inp: dict, dev="cpu", mutate=None) -> list:
    """fp64 reference of every output of every problem: [ {name: (ref, bound before the fp32 store, "f32")} ]."""
    if case.op != "many":
        return [R.reference(case, inp, dev, mutate)]
    s = case.shape
    out = []
    for pr in inp["probs"]:
        z, e_z, _ = logits_reference(case, pr, dev)["logits"]
        res = {}
        if "logits" in OUTS[s["outs"]]:
            res["logits"] = (z, e_z, "f32")
        for name, w, a0 in (("acc", W1, "acc0"), ("acc2", W2, "acc20")):
            if name in OUTS[s["outs"]]:
                o, pre = weighted(z, e_z, s["norm"], w, pr[a0].to(dev).double(), mutate)
                res[name] = (o, pre, "f32")
        out.append(res)
    return out


# ----------------------------------------------------------------------------------- fp32 emulation (CPU)
def chunks(C: int) -> list:
    """The concept rows of every LDS chunk, as the kernel cuts them: ceil(C / 8) chunks of equal height, the last lower."""
    nch = (C + 7) // 8
    h = (C + nch - 1) // nch
    return [(c0, min(c0 + h, C)) for c0 in range(0, C, h)]


def _f32_weighting(z: torch.Tensor, norm: str, slip) -> torch.Tensor:
    """softmax / sparsemax / 1.5-entmax over axis 0 in fp32, the sort-and-threshold algorithms the kernel implements."""
    C = z.shape[0]
    zs = z - z.amax(0, keepdim=True)
    if norm == "softmax":
        e = torch.exp(zs)
        return e / e.sum(0, keepdim=True)
    x = zs * (0.5 if norm == "entmax15" else 1.0)
    srt = torch.sort(x, 0, descending=True).values
    rho = torch.arange(1, C + 1, dtype=torch.float32)[:, None]
    cs = torch.cumsum(srt, 0)
    if norm == "sparsemax":
        tau_j = (cs - 1.0) / rho
        inside = 1.0 + rho * srt > cs
    else:
        mean = cs / rho
        ss = rho * (torch.cumsum(srt * srt, 0) / rho - mean * mean)
        tau_j = mean - torch.sqrt(((1.0 - ss) / rho).clamp(min=0.0))
        inside = tau_j <= srt
    k = inside.sum(0, keepdim=True)
    if slip == "support off by one":
        k = (k + 1).clamp(max=C)
    tau = torch.gather(tau_j, 0, k - 1)
    d = (x - tau).clamp(min=0.0)
    return d * d if norm == "entmax15" else d


def emulate(case: Case, inp: dict, slip=None) -> list:
    """What ca_heatmap_many computes, in fp32 on the CPU: the logits chunk by chunk (each chunk's rows against the image
    rows), parked per patch, then weighted over all C at once and added to the accumulators.  `slip` seeds a mistake:
      "last chunk left out"   the logits of the last chunk keep what the table held (zeros);
      "support off by one"    the sparse support one entry too large."""
    s = case.shape
    out = []
    for pr in inp["probs"]:
        img = pr["img"][:, :s["dim"]].float()
        con = pr["con"][:, :s["dim"]].float()
        z = torch.zeros(s["C"], s["L"], dtype=torch.float32)
        cks = chunks(s["C"])
        for i, (c0, c1) in enumerate(cks):
            if slip == "last chunk left out" and i == len(cks) - 1:
                continue
            z[c0:c1] = con[c0:c1] @ img.T
        p = _f32_weighting(z, s["norm"], slip)
        res = {}
        if "logits" in OUTS[s["outs"]]:
            res["logits"] = z
        if "acc" in OUTS[s["outs"]]:
            res["acc"] = pr["acc0"] + torch.tensor(W1) * p
        if "acc2" in OUTS[s["outs"]]:
            res["acc2"] = pr["acc20"] + torch.tensor(W2) * p
        out.append(res)
    return out


SLIPS = {
    # name: (case, slip, output that must expose it)
    "last chunk left out (C = 9: 5 + 4 rows)": ("many_C9_L257_dim520_softmax_n16_all", "last chunk left out", "acc"),
    "last chunk left out (C = 32: 4 x 8 rows)": ("many_C32_L257_dim4096_sparsemax_n1_all", "last chunk left out", "logits"),
    "last chunk left out (C = 17, weighted only)": ("many_C17_L257_dim264_sparsemax_n16_all", "last chunk left out", "acc2"),
    "sparsemax support off by one (C = 17)": ("many_C17_L257_dim264_sparsemax_n16_all", "support off by one", "acc"),
    "sparsemax support off by one (C = 32)": ("many_C32_L257_dim4096_sparsemax_n1_all", "support off by one", "acc"),
    "entmax15 support off by one (C = 31)": ("many_C31_L257_dim520_entmax15_n16_all", "support off by one", "acc2"),
}


def over_the_bound(case: Case, inp: dict, got: list, ref: list, only=None):
    """(largest err / bound, elements over the bound) over all problems and outputs (`only`: that output alone)."""
    worst, n_over = 0.0, 0
    for g, r in zip(got, ref):
        assert set(g) == set(r), (set(g), set(r))
        for name, (rv, pre, kind) in r.items():
            if only is None or name == only:
                ratio, n = excess(g[name], rv, pre, kind)
                worst, n_over = max(worst, ratio), n_over + n
    return worst, n_over
