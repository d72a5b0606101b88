"""Launch cases of ca_propagate_maps (conceptattention_amd/csrc/ca_propmap.hip): seeded inputs, the fp64 reference with a
derived error bound, and an fp32 emulation of the kernel's order with named slips.

Imported by tests/test_propmap_kernels_gpu.py (the device) and tests/test_propmap_cases_cpu.py (the emulation lies inside
every bound, every slip leaves it).  Nothing here touches torch.cuda.  The q / k values and their logit families are
tests/querymap_cases.py's (they differ from head to head); bit conversion, seeding and the comparison come from
tests/tokmap_cases.py.

The quantity (csrc/ca_propmap.h), per head h and query row i, over the keys j of [k0 | k1], n = n0 + n1:
    s_ij = scale_log2 <q_i, k_j>,  m_i = max_j s_ij,  l_i = sum_j exp2(s_ij - m_i),  w_ij = exp2(s_ij - m_i) / l_i
    o_h[c, i] = sum_{j < n1} w_i(n0 + j) v[c, j],      out[c, i] = (1 / H) sum_h o_h[c, i].

The kernel's summation order (ca_propmap.hip's header): per head and row, wave w of four takes keys 64 t + 16 w + 0..15 of
every key tile t; within a wave the lane group g holds keys 4 g + 0..3 of the 16.  Per tile the wave's running maximum m
moves to m' = max(m, the 16 scores), p = exp2(s - m'), a = exp2(m - m'); a lane group's running sum is
l_g = l_g a + (((p0 + p1) + p2) + p3); the wave's numerator of map row c is O = O a followed by 16 fused multiply-adds
O = fma(v, p, O), key 4 g + e in the order e = 0..3 outside, g = 0..3 inside (four fp32-input MFMAs, each a k-ordered fma
chain).  Then l_w = (l_0 + l_1) + (l_2 + l_3); the four waves are brought to the common maximum M (one product with
exp2(m - M) each for l_w and O) and added pairwise; o_h = O / L; the heads are added in head order from zero; one product
with the rounded 1 / H; one fused multiply-add into each accumulator.

Bound, elementwise and first order, u = 2^-24, derived from that order as tests/querymap_cases.py derives ca_query_maps':
  products   bf16 x bf16 and half x half are exact in fp32's 24 bits: no term.
  score      fp32 accumulation of 128 products on the matrix unit, every addition charged a whole ulp (2 u) of the running
             magnitude, at most A_ij = |scale_log2| sum_d |q_id| |k_jd|; the product with scale_log2 rounds once:
                 eps_ij = 2 * 128 u A_ij + u |s_ij|                       (in log2 units)
  exponent   s - m' is one subtraction, and |s - m'| <= |s - m_i| for every running maximum m': u |s_ij - m_i|.
  exp2       one hardware v_exp_f32 per term, 1 ulp: EXP_REL = 2 u, relative.
  term       E_num(j) = ln 2 (eps_ij + u |s_ij - m_i|) + EXP_REL
  rescaling  a running sum (l or O) is rescaled once per key tile and once more to the common maximum, each time by one
             exp2 (EXP_REL) and one product (u; charged 2 u as in the sibling): (ceil(n / 64) + 1) (EXP_REL + 2 u); the
             exponents of those factors are differences of maxima that round once each, u ln 2 times their total, which is
             at most the row's spread R_i = max_j s_ij - min_j s_ij along the tiles and again R_i for the last step:
                 E_resc = (ceil(n / 64) + 1) (EXP_REL + 2 u) + 2 u ln 2 R_i
  row sum    every term carries its own E_num(j): their average under the softmax weights; n - 1 fp32 additions of positive
             terms in any order ((n - 1) u; the zeros of masked keys and empty waves add exactly):
                 E_den = sum_j w_ij E_num(j) + (n - 1) u + E_resc
  numerator  the terms e_ij v_cj are signed, so everything is charged against S_ci = sum_j w_i(n0 + j) |v_cj|: each term's
             own E_num(j) and E_resc; a wave's chain is 16 ceil(n / 64) fused multiply-adds on the fp32 matrix unit, each
             charged a whole ulp (2 u) of the running magnitude (at most the chain's absolute sum), and two more additions
             across the waves (2 u):
                 E_add = (32 ceil(n / 64) + 2) u
  division   one per cell; charged DIV_REL = 3 u (a correctly rounded one is u).
  cell       |do_h[c, i]| <= sum_j w_ij |v_cj| E_num(j) + S_ci (E_resc + E_add) + |o_h[c, i]| (E_den + DIV_REL)
  heads      H - 1 fp32 additions of signed terms (the first one, to zero, is exact) and the product with the rounded
             1 / H: (H + 1) u (1 / H) sum_h |o_h[c, i]|.
  floor      a term whose exp2 lies below fp32's normal range may be flushed to zero: 2^-126 (1 + sum_j |v_cj|), absolute.
  accumulate acc + weight out is one fused multiply-add: u |acc + weight out| (tokmap_cases.acc_bound()).
  everything times SECOND_ORDER = 1 + 2^-6.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

import querymap_cases as Q
import tokmap_cases as T
from tokmap_cases import (DIV_REL, EXP_REL, FLOOR, LN2, LOG2E, NAN_BITS, SCALE_LOG2, SECOND_ORDER, U, W1, W2,  # noqa: F401
                          acc_bound, emulate_acc, from_bits, over_the_bound, to_bits)

FAMILIES = Q.FAMILIES
TILE = 64                        # keys of a tile (16 per wave)
ROWS = 64                        # query rows of a workgroup
M_INIT = -3.0e38
PADS = (0, 8, 16, 264)           # NaN columns behind every row of q (PADS[i]) and of k0 / k1 (PADS[(i + 1) % 4])
VPADS = (1, 3, 8)                # NaN columns behind every row of v: ldv > n1
VKINDS = ("softmax", "normal", "onehot", "const")
CONST = 0.3125                   # the constant map's value (exact in fp32)


@dataclass(frozen=True)
class Case:
    heads: int
    nq: int
    n0: int
    n1: int
    C: int
    f16: bool
    family: str = "unit"
    vkind: str = "softmax"
    pad: int = 0             # index into PADS
    vpad: int = 0            # index into VPADS
    prescaled: bool = False  # the q rows carry softmax_scale * log2(e), scale_log2 = 1.0 (the model's form)

    @property
    def id(self):
        return (f"h{self.heads}_nq{self.nq}_k{self.n0}_v{self.n1}_C{self.C}_{'f16' if self.f16 else 'bf16'}_{self.family}"
                f"_{self.vkind}_p{self.pad}{self.vpad}{'_pre' if self.prescaled else ''}")

    @property
    def scale_log2(self):
        return 1.0 if self.prescaled else SCALE_LOG2

    @property
    def qcase(self):
        """tests/querymap_cases.py's case of the same q / k values."""
        return Q.Case(self.heads, self.nq, self.n0, self.n1, self.f16, self.family, "qkv", self.prescaled)


HEADS = (1, 2, 3, 5, 24)
NQ = (1, 15, 16, 17, 63, 64, 65, 200, 513)
N0 = (0, 1, 77, 512)
N1 = (1, 31, 127, 128, 129, 1100)
CS = (1, 5, 16, 17, 32)


def _cases():
    out = []
    k = 0

    def add(**kw):
        nonlocal k
        kw.setdefault("heads", (2, 3, 1, 5)[k % 4])
        kw.setdefault("nq", NQ[(k * 2 + k // 9) % len(NQ)])
        kw.setdefault("n0", N0[(k + k // 4) % len(N0)])
        kw.setdefault("family", FAMILIES[k % len(FAMILIES)])
        kw.setdefault("vkind", VKINDS[(k + k // 7) % len(VKINDS)])
        kw.setdefault("f16", bool((k + k // 5) & 1))
        kw.setdefault("pad", k % len(PADS))
        kw.setdefault("vpad", k % len(VPADS))
        kw.setdefault("prescaled", bool((k >> 2) & 1))
        if kw["family"] == "cold_text" and kw["n0"] == 0:     # (the cold family needs leading keys to be cold against)
            kw["n0"] = 77
        out.append(Case(**kw))
        k += 1
    for C in CS:                                    # every pair (C, n1); the other axes rotate through their values
        for n1 in N1:
            add(C=C, n1=n1)
    for fam in FAMILIES:                            # every family in the other storage type as well, several blocks of rows
        have = {c.f16 for c in out if c.family == fam}
        for f16 in {False, True} - have or {False}:
            add(C=5, n1=129, nq=65, heads=3, family=fam, f16=f16)
    for vkind in VKINDS:                            # every kind of map without leading keys (the weights sum to 1)
        add(C=17, n1=127, nq=17, n0=0, heads=2, family="unit", vkind=vkind)
    for f16 in (False, True):                       # the model's head count, ragged rows
        add(C=5, n1=127, nq=65, n0=77, heads=24, family="peaky8", f16=f16)
    add(C=32, n1=1100, nq=513, n0=512, heads=2, family="unit", vkind="normal")      # everything large at once
    add(C=1, n1=1, nq=1, n0=0, heads=1, family="unit", vkind="normal")              # one key: out is v[c, 0]
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def map_values(c: Case) -> torch.Tensor:
    """v [C, n1] fp32: softmax maps over the concepts, signed N(0, 1), one key per row, or a constant."""
    g = T._gen("propmap.v." + c.id)
    if c.vkind == "softmax":
        return torch.softmax(torch.randn(c.C, c.n1, generator=g) * 2.0, 0).to(torch.float32)
    if c.vkind == "normal":
        return torch.randn(c.C, c.n1, generator=g)
    if c.vkind == "onehot":
        v = torch.zeros(c.C, c.n1)
        for r in range(c.C):
            v[r, onehot_key(c, r)] = 1.0
        return v
    assert c.vkind == "const", c.vkind
    return torch.full((c.C, c.n1), CONST)


def onehot_key(c: Case, r: int) -> int:
    return (7 * r + 3) % c.n1


def _padded(x: torch.Tensor, pad: int, fill):
    out = torch.full((x.shape[0] + 1, x.shape[1] + pad), fill, dtype=x.dtype)
    out[:-1, :x.shape[1]] = x
    return out


@functools.lru_cache(maxsize=None)
def make_inputs(c: Case):
    """dict(buffers = {q | k0 | k1: int16 [rows + 1, W + pad], v: fp32 [C + 1, n1 + vpad]}, acc0, acc20): acc0 the first
    accumulator's non-zero start, acc20 the second one's zeros.  Everything a launch may not read is NaN: the padding
    columns and a guard row behind every operand (k0 and k1 share a row stride, as the entry wants it)."""
    W = c.heads * 128
    q, k = Q._values(c.qcase)
    qb, kb = to_bits(q.reshape(c.nq, W), c.f16), to_bits(k.reshape(-1, W), c.f16)
    kp = PADS[(c.pad + 1) % len(PADS)]
    buffers = {"q": _padded(qb, PADS[c.pad], NAN_BITS), "k0": _padded(kb[:c.n0], kp, NAN_BITS),
               "k1": _padded(kb[c.n0:], kp, NAN_BITS), "v": _padded(map_values(c), VPADS[c.vpad], float("nan"))}
    g = T._gen("propmap.acc." + c.id)
    acc0 = (torch.randn(c.C, c.nq, generator=g) * 0.1).to(torch.float32)
    return dict(buffers=buffers, acc0=acc0, acc20=torch.zeros(c.C, c.nq, dtype=torch.float32))


def view(c: Case, buffers, name: str):
    """The operand as a slice of its buffer (host or device): q / k0 / k1 [rows, heads 128], v [C, n1]."""
    rows, cols = {"q": (c.nq, c.heads * 128), "k0": (c.n0, c.heads * 128), "k1": (c.n1, c.heads * 128), "v": (c.C, c.n1)}[name]
    return buffers[name][:rows, :cols]


def operands(c: Case, dtype=torch.float64):
    """(q [nq, H, 128], k [n, H, 128], v [C, n1]) decoded from the stored bits."""
    b = make_inputs(c)["buffers"]
    q = from_bits(view(c, b, "q"), c.f16, dtype).reshape(c.nq, c.heads, 128)
    k = torch.cat([from_bits(view(c, b, n), c.f16, dtype) for n in ("k0", "k1")]).reshape(-1, c.heads, 128)
    return q, k, view(c, b, "v").to(dtype)


def reference_qkv(q, k, v, n0: int, scale_log2: float):
    """fp64 (out [C, nq], its bound [C, nq]) from q [nq, H, 128], k [n0 + n1, H, 128] and v [C, n1]; the bound is the
    module docstring's."""
    q, k, v = q.double(), k.double(), v.double()
    nq, H, _ = q.shape
    n = k.shape[0]
    tiles = (n + TILE - 1) // TILE
    C = v.shape[0]
    out = torch.zeros(C, nq, dtype=torch.float64)
    err = torch.zeros(C, nq, dtype=torch.float64)
    absum = torch.zeros(C, nq, dtype=torch.float64)
    va = v.abs()
    e_add = (32 * tiles + 2) * U
    for h in range(H):
        s = (q[:, h] @ k[:, h].T) * scale_log2
        A = (q[:, h].abs() @ k[:, h].abs().T) * abs(scale_log2)
        m = s.amax(1, keepdim=True)
        e = torch.exp2(s - m)
        w = e / e.sum(1, keepdim=True)
        e_num = LN2 * (2 * 128 * U * A + U * s.abs() + U * (s - m).abs()) + EXP_REL
        spread = m - s.amin(1, keepdim=True)
        e_resc = (tiles + 1) * (EXP_REL + 2 * U) + 2 * U * LN2 * spread              # [nq, 1]
        e_den = (w * e_num).sum(1, keepdim=True) + (n - 1) * U + e_resc              # [nq, 1]
        wv = w[:, n0:]
        o = (wv @ v.T).T                                                             # [C, nq]
        S = (wv @ va.T).T
        own = ((wv * e_num[:, n0:]) @ va.T).T
        err += own + S * (e_resc + e_add).T + o.abs() * (e_den + DIV_REL).T
        out += o
        absum += o.abs()
    out = out / H
    bound = (err / H + (H + 1) * U * absum / H) * SECOND_ORDER + FLOOR * (1 + va.sum(1, keepdim=True))
    return out, bound


@functools.lru_cache(maxsize=None)
def reference(c: Case):
    """fp64 (out, bound) of a case; computed once and shared (read-only)."""
    q, k, v = operands(c)
    return reference_qkv(q, k, v, c.n0, c.scale_log2)


def _fma(a, b, acc):
    """One fused multiply-add of fp32 values (fp64 holds the product exactly and the sum to well below u)."""
    return (a.double() * b.double() + acc.double()).to(torch.float32)


SLIPS = ("denominator_over_valued_keys_only", "heads_averaged_before_division", "mean_over_heads_minus_one",
         "last_ragged_tile_dropped", "query_block_reads_its_neighbour", "v_read_transposed", "v_read_at_offset_one",
         "row_c_gets_row_c_plus_one_at_the_padding_edge", "acc2_given_weight")


def emulate(c: Case, slip=None):
    """The kernel's order in fp32 -> out [C, nq]; the order is the module docstring's.  ``slip``, one of SLIPS
    (acc2_given_weight acts in emulate_outputs):
      denominator_over_valued_keys_only  the leading keys never reach the row sum;
      heads_averaged_before_division     mean_h O / mean_h L;
      mean_over_heads_minus_one          the head sum times 1 / (H - 1);
      last_ragged_tile_dropped           the keys of a last tile of fewer than 64 never reach the row sum or the numerator;
      query_block_reads_its_neighbour    the rows of query block b are computed from the q rows of block b ^ 1 (where it exists);
      v_read_transposed                  v's [C, n1] cells read as an [n1, C] array;
      v_read_at_offset_one               key j takes v[c, j + 1] (the last one repeats);
      row_c_gets_row_c_plus_one_at_the_padding_edge   the last row of a group of 16 map rows takes the next row's values:
                                         row 15 row 16's, row C - 1 the zeros of the padding."""
    assert slip is None or slip in SLIPS, slip
    f = torch.float32
    q, k, v = operands(c, dtype=f)
    if slip == "query_block_reads_its_neighbour":
        src = torch.arange(c.nq)
        nb = ((src // ROWS) ^ 1) * ROWS + src % ROWS
        q = q[torch.where(nb < c.nq, nb, src)]
    if slip == "v_read_transposed":
        v = v.T.contiguous().reshape(c.C, c.n1)
    if slip == "v_read_at_offset_one":
        v = torch.cat([v[:, 1:], v[:, -1:]], 1)
    if slip == "row_c_gets_row_c_plus_one_at_the_padding_edge":
        v = v.clone()
        if c.C > 16:
            v[15] = v[16]
        v[c.C - 1] = 0.0
    n = c.n0 + c.n1
    scale = torch.tensor(c.scale_log2, dtype=f)
    tiles = (n + TILE - 1) // TILE
    walk = tiles - 1 if slip == "last_ragged_tile_dropped" and n % TILE and tiles > 1 else tiles
    heads_div = c.heads - 1 if slip == "mean_over_heads_minus_one" and c.heads > 1 else c.heads
    inv_h = torch.tensor(1.0, dtype=f) / torch.tensor(float(heads_div), dtype=f)
    vp = torch.zeros(c.C, tiles * TILE, dtype=f)                   # (a leading key and a key past the end carry a zero)
    vp[:, c.n0:n] = v
    vp = vp.reshape(c.C, tiles, 4, 4, 4)                           # [row, tile, wave, lane group, key of the lane]
    total = torch.zeros(c.nq, c.C, dtype=f)
    num_sum, den_sum = torch.zeros(c.nq, c.C, dtype=f), torch.zeros(c.nq, 1, dtype=f)
    for h in range(c.heads):
        s = (q[:, h] @ k[:, h].T) * scale
        sp = torch.full((c.nq, tiles * TILE), -math.inf, dtype=f)
        sp[:, :n] = s
        sp = sp.reshape(c.nq, tiles, 4, 4, 4)
        m = torch.full((c.nq, 4), M_INIT, dtype=f)
        l = torch.zeros(c.nq, 4, 4, dtype=f)
        O = torch.zeros(c.nq, 4, c.C, dtype=f)
        for t in range(walk):
            st = sp[:, t]
            m_new = torch.maximum(m, st.amax((-1, -2)))
            a = torch.exp2(m - m_new)
            p = torch.exp2(st - m_new[:, :, None, None])
            pl = p
            if slip == "denominator_over_valued_keys_only":
                lead = (torch.arange(t * TILE, (t + 1) * TILE) < c.n0).reshape(4, 4, 4)
                pl = torch.where(lead, torch.zeros((), dtype=f), p)
            l = l * a[:, :, None] + (((pl[..., 0] + pl[..., 1]) + pl[..., 2]) + pl[..., 3])
            O = O * a[:, :, None]
            for e in range(4):
                for g in range(4):
                    O = _fma(vp[:, t, :, g, e].T[None], p[:, :, g, e, None], O)
            m = m_new
        lw = (l[:, :, 0] + l[:, :, 1]) + (l[:, :, 2] + l[:, :, 3])
        M = m.amax(1, keepdim=True)
        sc = torch.exp2(m - M)
        lw, O = lw * sc, O * sc[:, :, None]
        Ls = ((lw[:, 0] + lw[:, 1]) + (lw[:, 2] + lw[:, 3]))[:, None]
        Os = (O[:, 0] + O[:, 1]) + (O[:, 2] + O[:, 3])
        total = total + Os / Ls
        num_sum, den_sum = num_sum + Os, den_sum + Ls
    out = (num_sum * inv_h) / (den_sum * inv_h) if slip == "heads_averaged_before_division" else total * inv_h
    return out.T.contiguous()


def emulate_outputs(c: Case, slip=None):
    """(acc, acc2) as the kernel leaves them from make_inputs' starts: acc = fma(W1, out, acc0), acc2 = fma(W2, out, 0)."""
    inp = make_inputs(c)
    out = emulate(c, slip)
    return emulate_acc(inp["acc0"], W1, out), emulate_acc(inp["acc20"], W1 if slip == "acc2_given_weight" else W2, out)


def check_outputs(c: Case, got: dict):
    """{name: (largest error / bound, elements over the bound)} of whichever of acc / acc2 ``got`` holds, against the fp64
    reference: acc2 (zero start, weight 1) holds the propagated map itself and is held to the map's own bound."""
    inp = make_inputs(c)
    out, bound = reference(c)
    res = {}
    if "acc2" in got:
        assert W2 == 1.0 and not bool(inp["acc20"].any())
        res["maps"] = over_the_bound(got["acc2"], out, bound)
    if "acc" in got:
        a0 = inp["acc0"]
        res["acc"] = over_the_bound(got["acc"], a0.double() + W1 * out, acc_bound(W1, a0, out, bound))
    return res
