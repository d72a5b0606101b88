"""Launch forms of the attention kernels (ca_attn.hip, ca_attn4.hip), their fp64 reference and derived bounds.

Imported by tests/test_attn_routes_gpu.py (the GPU cases) and by tests/test_attn_cases_cpu.py (coverage of every
launch site, entry point and edge by a case; a faithful fp32 emulation of the kernels' numerics; the named kernel
slips each bound rejects).  Nothing here touches torch.cuda at import time; the reference and the bounds run on
whatever device their inputs live on.

Every case names the C entry point, the kernel it reaches (spelled as at its hipLaunchKernelGGL site), its problems
(shapes, key / query segment layout, spikes, seed) and its input family.  Every problem lives in buffers laid out as the
model passes them: q is the first third of a fused [rows, ldq] projection buffer, k and v the second and third thirds of
another [rows, ldkv] one; segment 1 of the keys and of the queries lies BEFORE segment 0 in memory with junk rows
between; out / out1 share an [rows, ldo] buffer, out_f32 has ldo32 and hm_con ldhc.  All five strides exceed
heads * 128 and differ from one another.

Input families:
  probe   exact probes: q rows hold +-1 at two dimensions per head, k rows {-1, 0, 1}, v integers in [-8, 8] (dimensions
          126 and 127 of q and k are kept free for spikes).  A score is an integer in [-2, 2], computed exactly by the
          MFMA chain; p = exp2(s - reference) is a power of two in [2^-4, 2^4], exact in bf16 whatever the last bit of
          v_exp_f32; O^T = sum p v is exact in fp32 in any order (probe_bits <= 24), so the only charged error is the
          exponential's in l, the finish and, for the scaling kernel, the distance of PROBE_SCALE * log2(e) from 1
          (its fp32 scale_log2 is exactly 1.0f).  A lost, duplicated or mis-paired key moves an output by at least
          about p_k |dv| / l >= 1 / (2 nk): at nk = 4352 more than 10x the bound (test_attn_cases_cpu.py).
          Spiked probes (a key `octaves` above its row: the redo, re-reference and recomputation paths) are not exact;
          they use the model bound.
  rnd     model statistics: bf16 q / k / v ~ N(0, 1) (q times Q_SCALE, rounded once, for the pre-scaled kernels; IEEE
          half q / k for ca_attn_fwd_qk16).
  std<s>, structured_far   the logit distributions of test_kernels_gpu._peaky_case (std s nats; a cold tile 0 at -40
          nats and five hot keys at +45 nats: the in-place re-reference).

Bounds (elementwise, u = 2^-24; every fp32 operation charged 2 u of its running magnitude, as in gemm_route_cases.py
and rowop_cases.py; U and EXP_ULPS are theirs).  a = s c is the exact exponent argument in octaves (c = scale log2 e,
or 1 for pre-scaled q), R_i = max(|tile-0 maximum|, |max a| + log2 nk + 1) bounds every reference a row can hold:
  score          128 products in 8 MFMA updates of 16, then the subtraction of the reference (ca_attn4: the chain
                 starts from -reference; ca_attn_kernel: fma with scale_log2): delta = 2 u SCORE_C (|q| |k| c + R) +
                 2 u (|a| + R) + |s| |c - scale_log2| (the fp32 rounding of scale_log2 itself).
  exp            p relative eps = ln2 delta + EXP_ULPS u.
  P              rounded to bf16 (RNE, relative 2^-8) on the P.V side only; l sums the unrounded fp32 p.
  O^T            the fp32 MFMA chain: 2 u (nk / 16 + nt + 8) sum p |v| (one update per 16 keys, log2 16 inside,
                 a rescale per tile on the recomputation path).
  l              per-lane tile sums, then the running sum, the half-wave exchange: 2 u (nt + 40) l.
  re-reference   exact powers of two: nothing.
  finish         1 / l and the product: 2 u FIN_ULPS |o|; then the store (bf16: 1 ulp as in gemm_route_cases.bound,
                 fp32: F32_ULPS ulps).
  out error      (sum p eps (|v| + |o|) + P + O^T terms) / l + |o| (l term) + finish, first order; second-order terms
                 (products of relative errors <= 2^-8) are covered by the factor 1 + 2^-6.
  probe          eps = ln2 |s| |c - scale_log2| on both sides; EXP_ULPS u on l only; no P or O^T term.
  hm_part        sum_d E_o[d] |con[d]| + 2 u (64 + 2) sum_d |o| |con| (an fp32 fma chain of 64, one exchange).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

import gemm_route_cases as G
import rowop_cases as R

U = R.U
EXP_ULPS = R.EXP_ULPS
F32_ULPS = G.F32_ULPS
Q_SCALE = G.Q_SCALE
LN2 = math.log(2.0)
SCORE_C = 128 / 16 + math.log2(16) + 2
FIN_ULPS = 3
BF16_U = 2.0 ** -8
LOG2E_F32 = np.float32(1.4426950408889634)
PROBE_SCALE = float(np.float32(1 / 1.4426950408889634))   # its fp32 scale_log2 is exactly 1.0f (test_attn_cases_cpu)
MODEL_SCALE = float(np.float32(1 / math.sqrt(128.0)))
N_CU = 256                   # MI355X; the GPU test reads the device's count
REDO_LIMIT = 2.0 ** 30       # ca_attn_common.h
REREF_ABOVE = 2.0 ** 64      # ca_attn4.hip
L_LIMIT = 2.0 ** 100
SPIKE_DIM = 126              # probe dimensions 126, 127 carry spikes only

# Measured on MI355X, tests/test_attn_routes_gpu.py (largest printed max err / bound per kernel and family):
#   exact probes: bf16 out 0.500 (the half-ulp store) on all three kernels; out_f32 0.019 (ca_attn4, both operand
#     types), 0.167 (ca_attn_kernel: PROBE_SCALE's distance from 1 / log2 e); hm_part 0.007.  Every ca_attn4 and
#     ca_attn4_qk16 probe with an fp32 copy came back bit-exact (the fp64 reference rounded to fp32).
#   rnd: out 0.371 / 0.441 / 0.431 (ca_attn4 / qk16 / ca_attn_kernel), out_f32 0.449 / 0.497 / 0.593, hm_part 0.045.
#   std8: out_f32 0.798 (ca_attn4), 0.801 (ca_attn_kernel); structured_far 0.740.  Spiked probes: out 0.319.
#   No constant needed widening: every bound above is as derived.

FORMS = {   # form: (entry point, kernel)
    "scale": ("ca_attn_fwd_bf16", "ca_attn_kernel<8>"),
    "pre": ("ca_attn_fwd_bf16", "ca_attn4_kernel"),
    "qk16": ("ca_attn_fwd_qk16", "ca_attn4_qk16_kernel"),
}


@dataclass(frozen=True)
class Prob:
    nq: int
    n0: int
    n1: int = 0
    nq0: int = 0                 # 0: one query segment
    f32: bool = False            # out_f32 copy
    hm_C: int = 0                # heat-map partials (pre-scaled kernels; needs two query segments)
    spikes: tuple = ()           # (head, query row, key, octaves): probe spikes in dimension SPIKE_DIM
    seed: int = 0

    @property
    def nk(self):
        return self.n0 + self.n1

    @property
    def two_q(self):
        return 0 < self.nq0 < self.nq


@dataclass(frozen=True)
class Case:
    name: str
    form: str                    # scale | pre | qk16
    heads: int
    probs: tuple
    family: str = "probe"
    stats: Optional[tuple] = None   # ca_attn4 counters (recomputed workgroups, re-reference events); None entries free

    @property
    def id(self):
        return self.name

    @property
    def entry(self):
        return FORMS[self.form][0] if self.form != "pre" else "ca_attn_fwd_bf16(CA_ATTN_Q_PRESCALED)"

    @property
    def kernel(self):
        return FORMS[self.form][1]

    @property
    def exact(self):
        return self.family == "probe" and not any(p.spikes for p in self.probs)

    @property
    def scale(self):
        if self.form != "scale":
            return None
        return PROBE_SCALE if self.family == "probe" else MODEL_SCALE


# --------------------------------------------------------------------------------------------------- geometry
def tiles(nk):
    """(nt, nt_full, ragged) as both kernels compute them."""
    nt = (nk + 63) // 64
    ragged = nk % 64 != 0
    return nt, nt - 1 if ragged else nt, ragged


def t_straddle(n0, nk):
    return n0 // 64 if (n0 % 64 and n0 < nk) else -1


def loop_T(nk):
    """ca_attn4's pipelined iterations (its loop body is three in a row: T % 3 are left over)."""
    _, nt_full, _ = tiles(nk)
    return nt_full - 1 if nt_full > 0 else 0


def reref_checks(nk):
    """The iterations at whose top ca_attn4 looks at its running sums (t % 3 == 0 inside the three-iteration loop)."""
    T = loop_T(nk)
    return [t for t in range(0, T, 3) if t + 3 <= T]


def units(case: Case, qrows=256):
    """(total, [(problem, head, query block) of every unit or None where the head does not exist]) as ca_attn_fwd_impl
    lays the workgroups out."""
    hx = (case.heads + 7) // 8
    out = []
    for i, p in enumerate(case.probs):
        nqb = (p.nq + qrows - 1) // qrows
        for bid in range(8 * hx * nqb):
            xg, idx = bid & 7, bid >> 3
            head, qb = xg + 8 * (idx // nqb), idx % nqb
            out.append((i, head, qb) if head < case.heads else None)
    return len(out), out


def walks(case: Case, n_cu=N_CU):
    total, _ = units(case)
    return case.form != "scale" and n_cu % 8 == 0 and total > n_cu


def expected_stats(case: Case):
    """Counters the design fixes for the case: spikes of a row into tiles the re-reference checks see (one event per
    wave of 64 query rows), and spikes no check sees that push a row sum past 2^100 (one recomputed workgroup per
    256-row block)."""
    if case.stats is not None:
        return case.stats
    waves, blocks = set(), set()
    for i, p in enumerate(case.probs):
        checks = reref_checks(p.nk)
        for (h, row, key, octv) in p.spikes:
            # a probe score is the spike plus [-2, 2], the tile-0 reference in [-2, 2]: p = 2^(octv +- 4)
            seen = any(t >= key // 64 + 1 for t in checks)
            if seen and 64 + 4 < octv < 124:
                waves.add((i, h, row // 64))
            elif not seen and octv - 4 > 100:
                blocks.add((i, h, row // 256))
            elif octv + 4 + math.log2(p.nk) >= (64 if seen else 100):
                return (None, None)
    return (len(blocks), len(waves))


# --------------------------------------------------------------------------------------------------- cases
def P(*a, **k):
    return Prob(*a, **k)


def _per_form(form, heads_small, seed):
    """The key, segment and query edges for one kernel form."""
    s = seed
    f = form
    c = [
        Case(f"{f}_nk40_nq20_h1", f, 1, (P(20, 40, f32=True, seed=s),)),
        Case(f"{f}_nk64_straddle0_nq50_h3", f, 3, (P(50, 30, 34, nq0=17, f32=True, seed=s + 1),)),
        Case(f"{f}_nk65_n1is1_h8", f, 8, (P(300, 64, 1, nq0=1, f32=True, seed=s + 2),), "rnd"),
        Case(f"{f}_nk65_probe", f, heads_small, (P(33, 64, 1, f32=True, seed=s + 3),)),
        Case(f"{f}_nk128_h9", f, 9, (P(70, 128, seed=s + 4),)),
        Case(f"{f}_nk145_ragged_straddle_tail", f, 3, (P(257, 130, 15, nq0=256, f32=True, seed=s + 5),)),
        Case(f"{f}_nk192_seg_on_tile", f, 1, (P(96, 128, 64, nq0=95, f32=True, seed=s + 6),)),
        Case(f"{f}_nk225_n0_is_nk_minus_1", f, 3, (P(200, 224, 1, nq0=77, f32=True, seed=s + 7),)),
        Case(f"{f}_nk256_n1_0", f, heads_small, (P(130, 256, seed=s + 8),)),
        Case(f"{f}_nk261_n0_lt_64", f, 1, (P(64, 40, 221, f32=True, seed=s + 9),)),
        Case(f"{f}_nk320_rnd", f, 3, (P(300, 100, 220, nq0=33, f32=True, seed=s + 10),), "rnd"),
        Case(f"{f}_nk4339_rnd", f, 1, (P(300, 300, 4039, nq0=44, f32=True, seed=s + 11),), "rnd"),
        Case(f"{f}_nq512_nk4352", f, 3, (P(512, 300, 4052, nq0=200, f32=True, seed=s + 12),)),
        Case(f"{f}_nq512_nk4339_h1", f, 1, (P(512, 300, 4039, f32=True, seed=s + 13),)),
        Case(f"{f}_two_problems", f, 3, (P(5, 5, 333, f32=True, seed=s + 14),
                                          P(373, 40, 333, nq0=40, f32=True, seed=s + 15)), "rnd"),
        Case(f"{f}_two_problems_probe", f, 8, (P(8, 8, 1024, f32=True, seed=s + 16),
                                                P(1032, 512, 1024, nq0=512, f32=True, seed=s + 17))),
    ]
    return c


def _mixed16(seed, heads_cycle=None):
    """16 problems of different shapes and segment layouts: ragged or not, straddling or not, one or two key and query
    segments (the blk_end walk; with 24 heads, more units than CUs)."""
    shapes = [(33, 64, 1, 0), (70, 40, 0, 0), (300, 128, 97, 150), (257, 300, 300, 1), (20, 100, 29, 19),
              (64, 192, 0, 0), (129, 5, 700, 64), (513, 256, 64, 300), (96, 63, 2, 95), (40, 1000, 0, 0),
              (300, 65, 65, 257), (1, 200, 13, 0), (200, 64, 64, 100), (31, 777, 1, 0), (256, 11, 300, 128),
              (90, 130, 130, 45)]
    return tuple(P(nq, n0, n1, nq0=nq0, f32=(i % 3 != 1), seed=seed + i) for i, (nq, n0, n1, nq0) in enumerate(shapes))


def _hm(form, seed):
    return [
        Case(f"{form}_hm_C1", form, 3, (P(300, 77, 300, nq0=77, hm_C=1, f32=True, seed=seed),)),
        Case(f"{form}_hm_C5", form, 9, (P(5, 5, 600, f32=True, seed=seed + 1),
                                         P(605, 40, 600, nq0=45, hm_C=5, seed=seed + 2)), "rnd"),
        Case(f"{form}_hm_C8_nk4352", form, 1, (P(600, 256, 4096, nq0=263, hm_C=8, f32=True, seed=seed + 3),)),
        Case(f"{form}_hm_C8_rnd", form, 24, (P(290, 30, 270, nq0=31, hm_C=8, f32=True, seed=seed + 4),), "rnd"),
    ]


CASES = (
    _per_form("scale", 24, 100)
    + _per_form("pre", 24, 200)
    + _per_form("qk16", 24, 300)
    + [
        Case("scale_16_problems", "scale", 3, _mixed16(400)),
        Case("pre_16_problems", "pre", 1, _mixed16(420)),
        Case("pre_16_problems_walk", "pre", 24, _mixed16(440)),
        Case("qk16_16_problems_walk", "qk16", 24, _mixed16(460)),
        Case("qk16_16_problems_rnd", "qk16", 8, _mixed16(480), "rnd"),
    ]
    + _hm("pre", 500) + _hm("qk16", 520)
    + [
        # rare paths.  scaling kernel: a later tile whose row sum passes 2^30 is redone with its maximum
        Case("scale_redo_late_tile", "scale", 1, (P(300, 700, 0, spikes=((0, 17, 500, 40), (0, 290, 70, 45)), seed=600),)),
        Case("scale_redo_masked_tail", "scale", 3, (P(96, 650, 0, f32=True, spikes=((2, 5, 645, 40),), seed=601),)),
        Case("scale_redo_straddle", "scale", 1, (P(96, 100, 533, spikes=((0, 70, 101, 40), (0, 71, 127, 60)),
                                                   seed=602),)),
        # ca_attn4: a spike a check sees re-references its wave in place; one no check sees and beyond 2^100 sends the
        # workgroup through the classical recomputation; a spike in the masked tail stays on the kept reference
        Case("pre_reref_spikes", "pre", 3, (P(300, 64 * 11 + 5, spikes=((0, 17, 130, 70), (0, 20, 64 * 4 + 3, 80),
                                                                        (2, 290, 64 * 5 + 63, 70)), f32=True,
                                              seed=610),)),
        Case("pre_reref_straddle", "pre", 1, (P(200, 100, 640, nq0=100, spikes=((0, 150, 120, 72),), f32=True,
                                                seed=611),)),
        Case("pre_recompute_late", "pre", 1, (P(386, 64 * 11 + 5, spikes=((0, 326, 64 * 10 + 3, 110),), f32=True,
                                                seed=612),)),
        Case("pre_spike_masked_tail", "pre", 1, (P(96, 650, spikes=((0, 5, 645, 70),), f32=True, seed=613),)),
        Case("qk16_recompute_overflow", "qk16", 1, (P(300, 300, 333, nq0=3, spikes=((0, 7, 630, 130),), f32=True,
                                                      seed=614),), stats=(1, None)),
        Case("qk16_reref_spikes", "qk16", 9, (P(260, 64 * 9, spikes=((8, 200, 64 + 7, 70), (8, 259, 64 * 2, 99)),
                                                seed=615),)),
        # model statistics with peaky logits (test_kernels_gpu._peaky_case)
        Case("pre_std8", "pre", 1, (P(300, 4339, f32=True, seed=620),), "std8", stats=(0, 0)),
        Case("pre_structured_far", "pre", 1, (P(300, 4339, f32=True, seed=621),), "structured_far",
             stats=(0, None)),
        Case("scale_std8", "scale", 1, (P(300, 4339, f32=True, seed=622),), "std8"),
    ]
)
BY_ID = {c.id: c for c in CASES}


# --------------------------------------------------------------------------------------------------- inputs
@dataclass
class ProbInputs:
    D: int
    ldq: int
    ldkv: int
    ldo: int
    ldo32: int
    ldhc: int
    qbuf: torch.Tensor           # bf16-typed [rows, ldq] (half bits for qk16)
    kvbuf: torch.Tensor          # bf16-typed [rows, ldkv]
    hmbuf: Optional[torch.Tensor]
    gq0: int = 0                 # row of q segment 0 in qbuf (segment 1 at gq1)
    gq1: int = 0
    gk0: int = 0
    gk1: int = 0
    out_rows: int = 0
    extra: dict = field(default_factory=dict)


def strides(heads):
    D = heads * 128
    return dict(ldq=3 * D + 8, ldkv=3 * D + 24, ldo=D + 16, ldo32=D + 12, ldhc=D + 20)


def _store_qk(x: torch.Tensor, form: str) -> torch.Tensor:
    return x.half().view(torch.bfloat16) if form == "qk16" else x.bfloat16()


def decode_qk(t: torch.Tensor, form: str) -> torch.Tensor:
    return (t.view(torch.float16) if form == "qk16" else t).double()


def _peaky(kind, g, nq, nk):
    if kind.startswith("std"):
        a = math.sqrt(float(kind[3:]))
        return torch.randn(nq, 128, generator=g) * a, torch.randn(nk, 128, generator=g) * a, torch.randn(nk, 128, generator=g)
    u = torch.randn(128, generator=g)
    u = u / u.norm()
    q = u[None, :] * (math.sqrt(128.0) ** 0.5 * 3.0) + torch.randn(nq, 128, generator=g) * 0.05
    k = torch.randn(nk, 128, generator=g) * 0.05
    qs = float(q[0] @ u)
    k[:64] += u[None, :] * (-40.0 * math.sqrt(128.0) / qs)
    hot = torch.randperm(nk - 64, generator=g)[:5] + 64
    k[hot] += u[None, :] * (45.0 * math.sqrt(128.0) / qs)
    return q, k, torch.randn(nk, 128, generator=g)


def make_inputs(case: Case) -> list:
    st = strides(case.heads)
    D = case.heads * 128
    res = []
    for p in case.probs:
        g = torch.Generator().manual_seed(1000 + p.seed)
        nq1 = p.nq - p.nq0 if p.two_q else 0
        nq0 = p.nq - nq1
        gq1, gq0 = 2, 2 + nq1 + 3
        QR = gq0 + nq0 + 2
        gk1, gk0 = 1, 1 + p.n1 + 5
        KR = gk0 + p.n0 + 1
        qb = torch.empty(QR, st["ldq"], dtype=torch.float64)
        kb = torch.empty(KR, st["ldkv"], dtype=torch.float64)
        if case.family == "probe":
            qb.copy_(torch.randint(-3, 4, qb.shape, generator=g).double())
            kb.copy_(torch.randint(-3, 4, kb.shape, generator=g).double())
            qh = torch.zeros(QR, case.heads, 128, dtype=torch.float64)
            for j in range(2):
                dims = torch.randint(0, SPIKE_DIM, (QR, case.heads, 1), generator=g)
                sgn = torch.randint(0, 2, (QR, case.heads, 1), generator=g).double() * 2 - 1
                qh.scatter_(2, dims, sgn)
            qb[:, :D] = qh.reshape(QR, D)
            kh = torch.randint(-1, 2, (KR, case.heads, 128), generator=g).double()
            kh[:, :, SPIKE_DIM:] = 0
            kb[:, D:2 * D] = kh.reshape(KR, D)
            kb[:, 2 * D:3 * D] = torch.randint(-8, 9, (KR, D), generator=g).double()
            for (h, row, key, octv) in p.spikes:
                qrow = gq0 + row if row < nq0 else gq1 + row - nq0
                krow = gk0 + key if key < p.n0 else gk1 + key - p.n0
                qb[qrow, h * 128 + SPIKE_DIM] = 1.0
                kb[krow, D + h * 128 + SPIKE_DIM] = float(octv)
        elif case.family == "rnd":
            qb.normal_(generator=g)
            kb.normal_(generator=g)
            if case.form != "scale":
                qb[:, :D] *= Q_SCALE
        else:
            assert case.heads == 1 and len(case.probs) == 1 and not p.two_q and p.n1 == 0
            qb.normal_(generator=g)
            kb.normal_(generator=g)
            q, k, v = _peaky(case.family, g, p.nq, p.n0)
            if case.form != "scale":
                q = q * (MODEL_SCALE * math.log2(math.e))
            qb[gq0:gq0 + p.nq, :128] = q.double()
            kb[gk0:gk0 + p.n0, 128:256] = k.double()
            kb[gk0:gk0 + p.n0, 256:384] = v.double()
        qbuf = qb.bfloat16()
        kvbuf = kb.bfloat16()
        if case.form == "qk16":
            qbuf[:, :D] = _store_qk(qb[:, :D].float(), "qk16")
            kvbuf[:, D:2 * D] = _store_qk(kb[:, D:2 * D].float(), "qk16")
        hmbuf = None
        if p.hm_C:
            if case.family == "probe":
                hmbuf = torch.randint(-4, 5, (p.hm_C, st["ldhc"]), generator=g).float()
            else:
                hmbuf = torch.randn(p.hm_C, st["ldhc"], generator=g) * 0.1
        res.append(ProbInputs(D=D, qbuf=qbuf, kvbuf=kvbuf, hmbuf=hmbuf, gq0=gq0, gq1=gq1, gk0=gk0, gk1=gk1,
                              out_rows=QR, **st))
    return res


def views(case: Case, p: Prob, x: ProbInputs):
    """q rows (segment 0, segment 1), k / v rows of both key segments as the views the kernel gets."""
    D = x.D
    nq1 = p.nq - p.nq0 if p.two_q else 0
    nq0 = p.nq - nq1
    q0 = x.qbuf[x.gq0:x.gq0 + nq0, :D]
    q1 = x.qbuf[x.gq1:x.gq1 + nq1, :D] if nq1 else None
    k0 = x.kvbuf[x.gk0:x.gk0 + p.n0, D:2 * D]
    v0 = x.kvbuf[x.gk0:x.gk0 + p.n0, 2 * D:3 * D]
    k1 = x.kvbuf[x.gk1:x.gk1 + p.n1, D:2 * D] if p.n1 else None
    v1 = x.kvbuf[x.gk1:x.gk1 + p.n1, 2 * D:3 * D] if p.n1 else None
    return q0, q1, k0, v0, k1, v1


def problem_values(case: Case, p: Prob, x: ProbInputs, dev="cpu"):
    """fp64 q [nq, D] (problem row order), k / v [nk, D] (key order), con [C, D] or None."""
    q0, q1, k0, v0, k1, v1 = views(case, p, x)
    q = torch.cat([q0] + ([q1] if q1 is not None else [])).to(dev)
    k = torch.cat([k0] + ([k1] if k1 is not None else [])).to(dev)
    v = torch.cat([v0] + ([v1] if v1 is not None else [])).to(dev)
    con = x.hmbuf[:, :x.D].to(dev).double() if x.hmbuf is not None else None
    return decode_qk(q, case.form), decode_qk(k, case.form), v.double(), con


def scale_terms(case: Case):
    """(c, scale_log2): the exact exponent factor and the kernel's fp32 one."""
    if case.form != "scale":
        return 1.0, 1.0
    s = np.float32(case.scale)
    return float(s) * 1.4426950408889634, float(np.float32(s * LOG2E_F32))


# --------------------------------------------------------------------------------------------------- reference
def reference_head(q, k, v, c, sl2, exact, con=None):
    """fp64 softmax(q k^T c, base 2) v for one head's rows, the bound before the output's rounding (pre), and with
    con the heat-map partials <o, con_c> and their bound.  q [r, 128], k / v [nk, 128], con [C, 128]."""
    nk = k.shape[0]
    nt = (nk + 63) // 64
    s = q @ k.T
    a = s * c
    amax = a.max(1, keepdim=True).values
    w = torch.exp2(a - amax)
    D = w.sum(1, keepdim=True)
    av = v.abs()
    o = (w @ v) / D
    m_t0 = a[:, :min(64, nk)].max(1, keepdim=True).values
    Rr = torch.maximum(m_t0.abs(), amax.abs() + math.log2(nk) + 1)
    dc = s.abs() * abs(c - sl2)
    if exact:
        eps = LN2 * (dc + s.abs().max(1, keepdim=True).values * abs(c - sl2))
        we = w * eps
        num = we @ av + we.sum(1, keepdim=True) * o.abs()
        rho_l = (EXP_ULPS + 2 * (nt + 40)) * U
    else:
        A = q.abs() @ k.abs().T
        delta = 2 * U * SCORE_C * (A * abs(sl2) + Rr) + 2 * U * (a.abs() + Rr) + dc
        eps = LN2 * delta + EXP_ULPS * U
        we = w * eps
        Wv = w @ av
        num = we @ av + we.sum(1, keepdim=True) * o.abs() + (BF16_U + 2 * U * (nk / 16 + nt + 8)) * Wv
        rho_l = 2 * (nt + 40) * U
    underflow = nk * 2.0 ** -110 * (av.max() + o.abs())
    pre = (num / D + o.abs() * rho_l + 2 * U * FIN_ULPS * o.abs() + underflow) * (1 + 2.0 ** -6)
    if con is None:
        return o, pre, None, None
    hm = o @ con.T
    hm_pre = pre @ con.abs().T + 2 * U * 66 * (o.abs() @ con.abs().T)
    return o, pre, hm, hm_pre


def probe_bits(case: Case, inp: list) -> float:
    """Bits an exact probe's O^T sums need above their smallest term (must be <= 24): per row, with p = 2^(s - tile-0
    maximum), log2(sum p max|v| / min p)."""
    worst = 0.0
    for p, x in zip(case.probs, inp):
        q, k, v, _ = problem_values(case, p, x)
        for h in range(case.heads):
            sl = slice(h * 128, h * 128 + 128)
            s = q[:, sl] @ k[:, sl].T
            assert bool((s == s.round()).all())
            e = s - s[:, :min(64, p.nk)].max(1, keepdim=True).values
            vm = max(float(v[:, sl].abs().max()), 1.0)
            bits = torch.log2(torch.exp2(e).sum(1) * vm) - e.min(1).values
            worst = max(worst, float(bits.max()))
    return worst


# --------------------------------------------------------------------------------------------------- emulation (CPU)
def emulate_head(form, q, k, v, sl2=1.0, slip=None):
    """The kernels' fp32 numerics for one head: fp32 scores, the tile-0 maximum as reference, fp32 exp2, P rounded to
    bf16 for P.V, fp32 sums in tile order.  Returns (fp32 output rows, bf16 output rows) as fp64.  `slip` names a
    kernel slip to emulate (see SLIPS)."""
    slip = slip or {}
    nk = k.shape[0]
    S = q.float() @ k.float().T
    m = S[:, :min(64, nk)].max(1, keepdim=True).values
    if form == "scale":
        sl2_f = slip.get("scale_log2", sl2)
        m = (m.double() * sl2_f).float()
        arg = (S.double() * sl2_f - m.double()).float()
    else:
        arg = S - m
    p = torch.exp2(arg)
    Pb = p.bfloat16().float()
    vf = v.float()
    nt = (nk + 63) // 64
    l = [torch.zeros(q.shape[0], 1), torch.zeros(q.shape[0], 1)]
    O = torch.zeros(q.shape[0], 128)
    half = (torch.arange(nk) % 8) // 4     # the lane half that holds a key's score
    for t in range(nt):
        sl = slice(64 * t, min(64 * t + 64, nk))
        for hh in range(2):
            l[hh] = l[hh] + (p[:, sl] * (half[sl] == hh)).sum(1, keepdim=True)
        O = O + Pb[:, sl] @ vf[sl]
    if slip.get("l_half"):
        col_half = (torch.arange(128) % 8) // 4
        inv = torch.where(col_half[None, :] == 0, 1.0 / l[0], 1.0 / l[1])
    else:
        inv = 1.0 / (l[0] + l[1])
    o32 = O * inv
    return o32.double(), o32.bfloat16().double()


def emulate(case: Case, p: Prob, x: ProbInputs, slip=None):
    """Per head, the emulated fp32 and bf16 outputs [nq, D] and heat-map partials [heads, nq - nq0, 8] (NaN where
    never written), with the problem-level slips applied."""
    slip = slip or {}
    q, k, v, con = problem_values(case, p, x)
    c, sl2 = scale_terms(case)
    nq, D = p.nq, x.D
    nq0 = p.nq0 if p.two_q else nq
    o32 = torch.full((nq, D), float("nan"), dtype=torch.float64)
    o16 = o32.clone()
    if "kv" in slip:
        k, v = slip["kv"](k, v)
    qr = q
    if slip.get("q1_row_off") and p.two_q:
        qr = q.clone()
        qr[nq0:nq - 1] = q[nq0 + 1:nq]
    for h in range(case.heads):
        sl = slice(h * 128, h * 128 + 128)
        vh = v[:, sl]
        if slip.get("v_neighbour_head"):
            hn = h + 1 if h + 1 < case.heads else h - 1
            vh = v[:, hn * 128:hn * 128 + 128]
        f, b = emulate_head(case.form, qr[:, sl], k[:, sl], vh, sl2, slip)
        o32[:, sl], o16[:, sl] = f, b
    got32 = o32
    if slip.get("f32_segment_row") and p.two_q:
        got32 = torch.full_like(o32, float("nan"))
        got32[:nq0] = o32[:nq0]
        got32[:nq - nq0] = o32[nq0:]
    hm = None
    if con is not None:
        nseg = nq - nq0
        flat = torch.full((case.heads * nseg * 8,), float("nan"), dtype=torch.float64)
        stride = nq if slip.get("hm_head_nq") else nseg
        for h in range(case.heads):
            sl = slice(h * 128, h * 128 + 128)
            part = (o32[nq0:, sl].float() @ con[:, sl].float().T).double()
            if slip.get("hm_swap_cols"):
                part = part[:, [1, 0] + list(range(2, part.shape[1]))]
            for r in range(nseg):
                base = (h * stride + r) * 8
                if base + 8 <= flat.numel():
                    flat[base:base + part.shape[1]] = part[r]
        hm = flat.view(case.heads, nseg, 8)
    return got32, o16, hm


def reference(case: Case, p: Prob, x: ProbInputs, dev="cpu", rows=None):
    """fp64 reference of one problem on `dev`: out [nq, D], pre [nq, D], hm [heads, nq - nq0, C], hm_pre."""
    q, k, v, con = problem_values(case, p, x, dev)
    c, sl2 = scale_terms(case)
    exact = case.exact
    nq0 = p.nq0 if p.two_q else p.nq
    o = torch.empty(p.nq, x.D, dtype=torch.float64, device=dev)
    pre = torch.empty_like(o)
    hm = hm_pre = None
    if con is not None:
        hm = torch.empty(case.heads, p.nq - nq0, con.shape[0], dtype=torch.float64, device=dev)
        hm_pre = torch.empty_like(hm)
    step = rows or p.nq
    for h in range(case.heads):
        sl = slice(h * 128, h * 128 + 128)
        for r0 in range(0, p.nq, step):
            r1 = min(p.nq, r0 + step)
            oo, pp, hh, hp = reference_head(q[r0:r1, sl], k[:, sl], v[:, sl], c, sl2, exact,
                                            None if con is None else con[:, sl])
            o[r0:r1, sl], pre[r0:r1, sl] = oo, pp
            if con is not None and r1 > nq0:
                a = max(r0, nq0)
                hm[h, a - nq0:r1 - nq0] = hh[a - r0:]
                hm_pre[h, a - nq0:r1 - nq0] = hp[a - r0:]
    return o, pre, hm, hm_pre


excess = G.excess
bound = G.bound


def old_tolerance_ratio(got, ref):
    """max err / (1e-2 + 8e-3 |ref|): the tolerance of the attention tests in test_kernels_gpu.py."""
    return float(((got - ref).abs() / (1e-2 + 8e-3 * ref.abs())).max())


# --------------------------------------------------------------------------------------------------- slips (CPU)
def _drop(idx):
    def f(k, v):
        keep = [i for i in range(k.shape[0]) if i not in set(idx)]
        return k[keep], v[keep]
    return f


def _replace(dst, src):
    def f(k, v):
        k, v = k.clone(), v.clone()
        k[dst], v[dst] = k[src], v[src]
        return k, v
    return f


def _swap_v(a, b):
    def f(k, v):
        v = v.clone()
        v[[a, b]] = v[[b, a]]
        return k, v
    return f


SLIP_PROB = P(64, 300, 4039, nq0=40, f32=True, hm_C=3, seed=700)     # nk = 4339: ragged; tile 4 straddles
SLIP_SMALL = P(96, 100, 233, nq0=45, f32=True, hm_C=3, seed=701)     # nk = 333: ragged; tile 1 straddles


def _straddle_slip(case, p, x):
    """The straddling tile reads segment 0's row n0 (the row after k0 in memory) instead of k1[0]."""
    D = x.D
    row = x.kvbuf[x.gk0 + p.n0]
    kk = decode_qk(row[D:2 * D], case.form)
    vv = row[2 * D:3 * D].double()

    def f(k, v):
        k, v = k.clone(), v.clone()
        k[p.n0], v[p.n0] = kk, vv
        return k, v
    return f


SLIPS = {
    # name: (problem, slip builder (case, prob, inputs) -> emulate() slip dict, output, single key)
    "last key of the ragged tile dropped": (lambda c, p, x: {"kv": _drop([p.nk - 1])}, "out_f32", True),
    "a whole tile dropped": (lambda c, p, x: {"kv": _drop(list(range(128, 192)))}, "out_f32", False),
    "straddling tile reads segment 0 row n0 instead of k1[0]": (lambda c, p, x: {"kv": _straddle_slip(c, p, x)},
                                                                "out_f32", True),
    "key n0 - 1 duplicated": (lambda c, p, x: {"kv": _replace(p.n0, p.n0 - 1)}, "out_f32", True),
    "two V rows of one tile exchanged": (lambda c, p, x: {"kv": _swap_v(64 * (p.nk // 128) + 3, 64 * (p.nk // 128) + 45)},
                                         "out_f32", True),
    "V of the neighbouring head": (lambda c, p, x: {"v_neighbour_head": True}, "out_f32", False),
    "l missing the lane ^ 32 half": (lambda c, p, x: {"l_half": True}, "out_f32", False),
    "second query segment read one row off": (lambda c, p, x: {"q1_row_off": True}, "out", False),
    "out_f32 indexed by segment row": (lambda c, p, x: {"f32_segment_row": True}, "out_f32", False),
    "hm_part indexed with head * nq": (lambda c, p, x: {"hm_head_nq": True}, "hm", False),
    "hm_part concept columns exchanged": (lambda c, p, x: {"hm_swap_cols": True}, "hm", False),
    "scaling kernel without log2(e)": (lambda c, p, x: {"scale_log2": float(np.float32(c.scale))}, "out_f32", False),
}


def slip_case(name, big, family="probe"):
    form = "scale" if "scaling kernel" in name else "pre"
    p = SLIP_PROB if big else SLIP_SMALL
    if form == "scale":
        p = Prob(p.nq, p.n0, p.n1, nq0=p.nq0, f32=True, seed=p.seed)
    heads = 1 if big else 2
    return Case(f"slip_{'big' if big else 'small'}", form, heads, (p,), family)


def discrimination(name, big=False, family="probe"):
    """(faithful emulation within every bound, max err / bound of the slipped output (inf where it leaves an element
    unwritten), its max err / the old test tolerance (1e-2 + 8e-3 |ref|) on the bf16 output)."""
    build, which, _ = SLIPS[name]
    case = slip_case(name, big, family)
    p = case.probs[0]
    x = make_inputs(case)[0]
    ref, pre, hm, hm_pre = reference(case, p, x)
    f32, b16, hmg = emulate(case, p, x)
    ok = excess(f32, ref, pre, "f32")[1] == 0 and excess(b16, ref, pre, "bf16")[1] == 0
    if hm is not None:
        ok &= excess(hmg[..., :hm.shape[2]], hm, hm_pre, "f32")[1] == 0
    s32, s16, shm = emulate(case, p, x, build(case, p, x))
    if which == "out_f32":
        r, n = excess(s32, ref, pre, "f32")
    elif which == "out":
        r, n = excess(s16, ref, pre, "bf16")
    else:
        r, n = excess(shm[..., :hm.shape[2]], hm, hm_pre, "f32")
    if math.isnan(r):                 # an element never written keeps its NaN: over any bound
        r = math.inf
    return ok, (r if n else min(r, 1.0)), old_tolerance_ratio(s16, ref)
