"""Launch cases of ca_query_maps (conceptattention_amd/csrc/ca_querymap.hip): seeded inputs, the fp64 reference with a
derived error bound, and an fp32 emulation of the kernel's order with named slips.

Imported by tests/test_querymap_kernels_gpu.py (the device) and tests/test_querymap_cases_cpu.py (the emulation lies
inside every bound, every slip leaves it).  Nothing here touches torch.cuda.  Helpers shared with ca_token_maps' cases
(bit conversion, seeding, the comparison) come from tests/tokmap_cases.py.

The quantity (csrc/ca_querymap.h), per head h and query row i, over the keys j of [k0 | k1], n = n0 + n1:
    s_ij = scale_log2 <q_i, k_j>,  m_i = max_j s_ij,  l_i = sum_j exp2(s_ij - m_i),  p_ij = exp2(s_ij - m_i) / l_i
    map[i, j] = (1 / H) sum_h p_i(n0 + j)  (j < n1),     lse[h, i] = (m_i + log2 l_i) ln 2.

The kernel's summation order (ca_querymap.hip's header): per head and row the keys fall into 16 chains by (j mod 64) / 4;
a chain walks its keys four at a time (one group per key tile of 64), keeps a running maximum m and a running sum
l = l exp2(m - m') + (((e0 + e1) + e2) + e3); the 16 chains are brought to the common maximum M (l exp2(m - M)) and added
pairwise; a cell is exp2(s - M) / L; the heads are added in head order from zero; one product with the rounded 1 / H; one
fused multiply-add into the accumulator.

Bound, elementwise and first order, u = 2^-24, derived from that order as tests/tokmap_cases.py derives ca_token_maps':
  products   bf16 x bf16 and half x half are exact in fp32's 24 bits: no term.
  score      fp32 accumulation of 128 products on the matrix unit, every addition charged a whole ulp (2 u) of the running
             magnitude, at most A_ij = |scale_log2| sum_d |q_id| |k_jd|; the product with scale_log2 rounds once:
                 eps_ij = 2 * 128 u A_ij + u |s_ij|                       (in log2 units)
  exponent   s - M is one subtraction (u |s_ij - m_i|); M is the same fp32 number in a cell and in its row sum.
  exp2       one hardware v_exp_f32 per cell, 1 ulp: EXP_REL = 2 u, relative.
  numerator  E_num(j) = ln 2 (eps_ij + u |s_ij - m_i|) + EXP_REL
  row sum    every term carries its own E_num(j): their average under the softmax weights w_ij; n - 1 fp32 additions of
             positive terms in any order ((n - 1) u; additions of the zeros of masked keys and empty chains are exact);
             a chain is rescaled once per key tile and once more to the common maximum, each time by one exp2 (EXP_REL),
             one product and, in the tile step, one addition (2 u): (ceil(n / 64) + 1) (EXP_REL + 2 u); the exponents of
             those factors are differences of maxima that round once each, u ln 2 times their total, which is at most the
             row's spread R_i = max_j s_ij - min_j s_ij along the chain and again R_i for the last step:
                 E_den = sum_j w_ij E_num(j) + (n - 1) u + (ceil(n / 64) + 1) (EXP_REL + 2 u) + 2 u ln 2 R_i
  division   one per cell; charged DIV_REL = 3 u (a correctly rounded one is u).
  cell       |dp_ij| <= p_ij rel (1 + rel),  rel = E_num(j) + E_den + DIV_REL.
  heads      H - 1 fp32 additions of non-negative terms (the first one, to zero, is exact) and the product with the
             rounded 1 / H: (H + 1) u map.
  floor      a cell whose exp2 lies below fp32's normal range may be flushed to zero: 2^-126, absolute.
  accumulate acc + weight map is one fused multiply-add: u |acc + weight map| (tokmap_cases.acc_bound()).
  everything times SECOND_ORDER = 1 + 2^-6.
lse: as in tokmap_cases with this E_den:
      |dlse| <= E_den + eps at the maximum + ln 2 (2 u log2 l + 2^-21 + u |m + log2 l|) + u |lse|.

The cold family is why the bound is relative: its emitted cells are about e^-20 / n, and an absolute bound at the scale
of the large cells would pass a kernel that returns zeros there.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

import tokmap_cases as T
from tokmap_cases import (DIV_REL, EXP_REL, FAMILIES, FLOOR, LN2, LOG2E, NAN_BITS, SCALE_LOG2, SECOND_ORDER, U, W1, W2,  # noqa: F401
                          acc_bound, emulate_acc, from_bits, over_the_bound, to_bits)

TILE = 64                        # the statistics pass's key tile
EMIT = 128                       # the emit pass's key block
ROWS = 16                        # query rows of a workgroup
M_INIT = -3.0e38
PADS = (8, 16, 264)              # NaN columns behind every row of an "apart" operand: three row strides per width
OUTPUTS = ("acc+acc2+lse", "acc", "acc2", "acc+acc2", "acc+lse", "acc2+lse")


@dataclass(frozen=True)
class Case:
    heads: int
    nq: int
    n0: int
    n1: int
    f16: bool
    family: str = "unit"
    layout: str = "qkv"      # qkv: q and k column slices of one [rows, 3 heads 128] buffer; apartN: three padded buffers,
                             # q with PADS[N] pad columns, k0 and k1 with PADS[(N + 1) % 3]
    prescaled: bool = False  # the q rows carry softmax_scale * log2(e), scale_log2 = 1.0 (the model's form)
    outputs: str = "acc+acc2+lse"

    @property
    def id(self):
        return (f"h{self.heads}_nq{self.nq}_k{self.n0}_e{self.n1}_{'f16' if self.f16 else 'bf16'}_{self.family}"
                f"_{self.layout}{'_pre' if self.prescaled else ''}_{self.outputs}")

    @property
    def scale_log2(self):
        return 1.0 if self.prescaled else SCALE_LOG2

    @property
    def outs(self):
        return tuple(self.outputs.split("+"))


HEADS = (1, 2, 3, 24)
NQ = (1, 4, 15, 16, 17, 32, 33, 77, 512)
N0 = (0, 1, 4, 77, 512)
N1 = (1, 15, 63, 64, 65, 200, 1100)


def _cases():
    out = []
    k = 0

    def add(**kw):
        nonlocal k
        kw.setdefault("f16", bool(k & 1))
        kw.setdefault("layout", ("qkv", "apart0", "apart1", "apart2")[(k >> 1) & 3])
        kw.setdefault("prescaled", bool((k >> 2) & 1))
        kw.setdefault("outputs", OUTPUTS[0])
        out.append(Case(**kw))
        k += 1
    for nq in NQ:                                   # around the workgroup's 16 rows; 32 row blocks at the limit
        add(heads=2, nq=nq, n0=4, n1=65)
    for n0 in N0:                                   # no leading keys .. 8 key tiles of them
        add(heads=2, nq=17, n0=n0, n1=63)
    for n1 in N1:                                   # around the key tile and the emit block; 9 emit blocks, the last ragged
        add(heads=2, nq=17, n0=77, n1=n1)
    for heads in HEADS:
        add(heads=heads, nq=17, n0=4, n1=65)
    for fam in FAMILIES:                            # every family in both storage types, with and without leading keys
        for f16 in (False, True):
            add(heads=3, nq=33, n0=77, n1=200, family=fam, f16=f16)
        if fam != "cold_text":                      # (the cold family needs leading keys to be cold against)
            add(heads=3, nq=33, n0=0, n1=200, family=fam)
    for f16 in (False, True):                       # everything large at once
        add(heads=3, nq=77, n0=512, n1=1100, family="peaky8", f16=f16, layout="qkv")
    add(heads=2, nq=512, n0=512, n1=200, family="unit", layout="apart1")
    add(heads=2, nq=17, n0=0, n1=1, family="unit")                                  # one key: every cell is 1
    add(heads=2, nq=4, n0=0, n1=1100, family="last_tile_max", f16=True)             # the concept rows' shape, no leading keys
    add(heads=2, nq=17, n0=77, n1=51, family="last_tile_max", f16=False)            # 128 keys: no ragged tile
    for o in OUTPUTS[1:]:                           # each accumulator alone, with and without lse
        add(heads=3, nq=33, n0=77, n1=200, outputs=o, f16=False, layout="qkv", prescaled=False)
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def _values(c: Case):
    """(q [nq, H, 128], k [n0 + n1, H, 128]) fp32 before the storage rounding.  scale <q, k> has a standard deviation of
    1 nat in the unit family; u is a unit vector per head along which the other families push rows apart.  Every family
    differs from head to head: the push, the row it lands on, or the sharpness depends on h."""
    g = T._gen("querymap." + c.id)
    n = c.n0 + c.n1
    q = torch.randn(c.nq, c.heads, 128, generator=g)
    k = torch.randn(n, c.heads, 128, generator=g)
    u = torch.randn(c.heads, 128, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    a = math.sqrt(20.0 * math.sqrt(128.0))          # scale * a * a = 20 nats
    fam = c.family
    for h in range(c.heads):
        if fam in ("peaky8", "peaky16"):
            q[:, h] *= float(fam[5:]) * (1.0 - 0.125 * (h % 3))
        elif fam == "cold_text":                    # the emitted (image) keys 20, 22, 24 nats BELOW the leading keys
            assert c.n0 > 0
            q[:, h] += a * u[h]
            k[:c.n0, h] += (1.0 + 0.1 * (h % 3)) * a * u[h]
        elif fam == "dominant":                     # one emitted key 30 nats up, another one per head
            q[:, h] += a * u[h]
            k[c.n0 + (c.n1 // 2 + 7 * h) % c.n1, h] += 1.5 * a * u[h]
        elif fam == "ties":                         # the same row four times, 20 nats up: exact ties at the maximum
            q[:, h] += a * u[h]
            row = k[c.n0, h] + a * u[h]
            for j in {c.n0, n - 1, (n // 2 + h) % n, h % n}:
                k[j, h] = row
        elif fam == "last_tile_max":                # the row maximum is one of the last keys: the last, ragged emit block
            q[:, h] += a * u[h]
            k[n - 1 - h % min(3, c.n1), h] += 0.6 * a * u[h]
        else:
            assert fam == "unit", fam
    if c.prescaled:
        q = q * SCALE_LOG2
    return q, k


@functools.lru_cache(maxsize=None)
def make_inputs(c: Case):
    """dict(buffers = {name: int16 [rows, ld]}, views = {q | k0 | k1: (buffer, first row, rows, first column)}, acc0, acc20):
    acc0 the first accumulator's non-zero start, acc20 the second one's zeros.
    Everything a launch may not read is NaN: the other columns and rows of the shared buffer, the padding columns and a
    guard row behind every operand."""
    W = c.heads * 128
    q, k = _values(c)
    qb, kb = to_bits(q.reshape(c.nq, W), c.f16), to_bits(k.reshape(-1, W), c.f16)
    n = c.n0 + c.n1
    if c.layout == "qkv":                           # rows [leading | emitted], columns [q | k | v]; the q rows come first
        buf = torch.full((max(c.nq, n) + 1, 3 * W), NAN_BITS, dtype=torch.int16)
        buf[:c.nq, :W] = qb
        buf[:n, W:2 * W] = kb
        buffers = {"qkv": buf}
        views = {"q": ("qkv", 0, c.nq, 0), "k0": ("qkv", 0, c.n0, W), "k1": ("qkv", c.n0, c.n1, W)}
    else:
        i = int(c.layout[5:])

        def padded(b, pad):
            out = torch.full((b.shape[0] + 1, W + pad), NAN_BITS, dtype=torch.int16)
            out[:-1, :W] = b
            return out
        # (k0 and k1 share a row stride, as ca_query_maps wants it; they are two allocations all the same)
        buffers = {"q": padded(qb, PADS[i]), "k0": padded(kb[:c.n0], PADS[(i + 1) % 3]), "k1": padded(kb[c.n0:], PADS[(i + 1) % 3])}
        views = {"q": ("q", 0, c.nq, 0), "k0": ("k0", 0, c.n0, 0), "k1": ("k1", 0, c.n1, 0)}
    g = T._gen("querymap.acc." + c.id)
    acc0 = (torch.randn(c.nq, c.n1, generator=g) * 0.1).to(torch.float32)
    acc20 = torch.zeros(c.nq, c.n1, dtype=torch.float32)
    return dict(buffers=buffers, views=views, acc0=acc0, acc20=acc20)


def view(c: Case, buffers, name: str):
    """The operand as a [rows, heads 128] slice of its buffer (host or device)."""
    b, r0, n, c0 = make_inputs(c)["views"][name]
    return buffers[b][r0:r0 + n, c0:c0 + c.heads * 128]


def operands(c: Case, inp=None, dtype=torch.float64):
    """(q [nq, H, 128], k [n, H, 128]) decoded from the stored bits."""
    inp = inp or make_inputs(c)
    q = from_bits(view(c, inp["buffers"], "q"), c.f16, dtype).reshape(c.nq, c.heads, 128)
    k = torch.cat([from_bits(view(c, inp["buffers"], n), c.f16, dtype) for n in ("k0", "k1")]).reshape(-1, c.heads, 128)
    return q, k


@dataclass
class Bound:
    maps: torch.Tensor    # [nq, n1]
    lse: torch.Tensor     # [heads, nq]


def reference_qk(q, k, n0: int, scale_log2: float):
    """fp64 (maps [nq, n1], lse [H, nq], Bound) from q [nq, H, 128] and k [n0 + n1, H, 128]."""
    q, k = q.double(), k.double()
    nq, H, _ = q.shape
    n = k.shape[0]
    n1 = n - n0
    maps = torch.zeros(nq, n1, dtype=torch.float64)
    err = torch.zeros(nq, n1, dtype=torch.float64)
    lse = torch.zeros(H, nq, dtype=torch.float64)
    blse = torch.zeros(H, nq, dtype=torch.float64)
    tiles = (n + TILE - 1) // TILE
    for h in range(H):
        s = (q[:, h] @ k[:, h].T) * scale_log2
        A = (q[:, h].abs() @ k[:, h].abs().T) * abs(scale_log2)
        m = s.amax(1, keepdim=True)
        e = torch.exp2(s - m)
        l = e.sum(1, keepdim=True)
        w = e / l
        e_num = LN2 * (2 * 128 * U * A + U * s.abs() + U * (s - m).abs()) + EXP_REL
        spread = m - s.amin(1, keepdim=True)
        e_den = (w * e_num).sum(1, keepdim=True) + (n - 1) * U + (tiles + 1) * (EXP_REL + 2 * U) + 2 * U * LN2 * spread
        rel = e_num[:, n0:] + e_den + DIV_REL
        maps += w[:, n0:]
        err += w[:, n0:] * rel * (1 + rel)
        log2l = torch.log2(l)
        lse[h] = ((m + log2l) * LN2)[:, 0]
        at_max = (LN2 * (2 * 128 * U * A + U * s.abs())).amax(1, keepdim=True)     # (of all keys: at least the maximum's)
        blse[h] = (e_den + at_max + LN2 * (2 * U * log2l + 2.0 ** -21 + U * (m + log2l).abs()) + U * lse[h][:, None].abs())[:, 0]
    maps = maps / H
    bound = (err / H + (H + 1) * U * maps) * SECOND_ORDER + FLOOR
    return maps, lse, Bound(bound, blse * SECOND_ORDER)


@functools.lru_cache(maxsize=None)
def reference(c: Case):
    """fp64 (maps, lse, bound) of a case; computed once and shared (read-only)."""
    q, k = operands(c)
    return reference_qk(q, k, c.n0, c.scale_log2)


SLIPS = ("max_over_emitted_only", "k0_left_out_of_l", "heads_averaged_before_division", "last_ragged_block_not_emitted",
         "query_block_reads_its_neighbour", "mean_over_heads_minus_one", "acc2_given_weight", "emit_offset_one_when_n0_is_0")


def emulate(c: Case, slip=None):
    """The kernel's order in fp32 -> (maps [nq, n1], lse [H, nq]); the order is the module docstring's.  ``slip``, one of
    SLIPS (acc2_given_weight acts in emulate_outputs):
      max_over_emitted_only           the cells and lse use the maximum over the n1 emitted keys, the row sum the true one;
      k0_left_out_of_l                the leading keys never reach the row sum;
      heads_averaged_before_division  mean_h exp2(s - m) / mean_h l;
      last_ragged_block_not_emitted   the cells of a last emit block of fewer than 128 keys stay what they were;
      query_block_reads_its_neighbour the rows of query block b are computed from the q rows of block b ^ 1 (where it exists);
      mean_over_heads_minus_one       the head sum times 1 / (H - 1);
      emit_offset_one_when_n0_is_0    with n0 = 0 the emitted cells start at key 1 (the last one repeats)."""
    assert slip is None or slip in SLIPS, slip
    f = torch.float32
    q, k = operands(c, dtype=f)
    if slip == "query_block_reads_its_neighbour":
        src = torch.arange(c.nq)
        nb = ((src // ROWS) ^ 1) * ROWS + src % ROWS
        q = q[torch.where(nb < c.nq, nb, src)]
    n = c.n0 + c.n1
    scale = torch.tensor(c.scale_log2, dtype=f)
    tiles = (n + TILE - 1) // TILE
    heads_div = c.heads - 1 if slip == "mean_over_heads_minus_one" and c.heads > 1 else c.heads
    inv_h = torch.tensor(1.0, dtype=f) / torch.tensor(float(heads_div), dtype=f)
    total = torch.zeros(c.nq, c.n1, dtype=f)
    num_sum, den_sum = torch.zeros(c.nq, c.n1, dtype=f), torch.zeros(c.nq, 1, dtype=f)
    lse = torch.zeros(c.heads, c.nq, dtype=f)
    emit = slice(c.n0, n)
    for h in range(c.heads):
        s = (q[:, h] @ k[:, h].T) * scale
        sp = torch.full((c.nq, tiles * TILE), -math.inf, dtype=f)
        sp[:, :n] = s
        if slip == "k0_left_out_of_l":
            sp[:, :c.n0] = -math.inf
        sp = sp.reshape(c.nq, tiles, 4, 4, 4)                     # [row, tile, wave, lane group, key of the lane]
        m = torch.full((c.nq, 4, 4), M_INIT, dtype=f)
        l = torch.zeros(c.nq, 4, 4, dtype=f)
        for t in range(tiles):
            st = sp[:, t]
            m_new = torch.maximum(m, st.amax(-1))
            e = torch.exp2(st - m_new[..., None])
            l = l * torch.exp2(m - m_new) + (((e[..., 0] + e[..., 1]) + e[..., 2]) + e[..., 3])
            m = m_new
        M = m.amax((1, 2))
        l = l * torch.exp2(m - M[:, None, None])
        lw = (l[:, :, 0] + l[:, :, 1]) + (l[:, :, 2] + l[:, :, 3])
        Ls = ((lw[:, 0] + lw[:, 1]) + (lw[:, 2] + lw[:, 3]))[:, None]
        M = M[:, None]
        m_num = s[:, emit].amax(1, keepdim=True) if slip == "max_over_emitted_only" else M
        se = s[:, emit]
        if slip == "emit_offset_one_when_n0_is_0" and c.n0 == 0:
            se = torch.cat([se[:, 1:], se[:, -1:]], 1)
        e = torch.exp2(se - m_num)
        total = total + e / Ls
        num_sum, den_sum = num_sum + e, den_sum + Ls
        lse[h] = ((m_num + torch.log2(Ls)) * torch.tensor(LN2, dtype=f))[:, 0]
    maps = (num_sum * inv_h) / (den_sum * inv_h) if slip == "heads_averaged_before_division" else total * inv_h
    return maps, lse


def emulate_outputs(c: Case, slip=None):
    """(acc, acc2, lse) as the kernel leaves them from make_inputs' starts: acc = fma(W1, map, acc0), acc2 = fma(W2, map, 0)."""
    inp = make_inputs(c)
    maps, lse = emulate(c, slip)
    acc = emulate_acc(inp["acc0"], W1, maps)
    acc2 = emulate_acc(inp["acc20"], W1 if slip == "acc2_given_weight" else W2, maps)
    if slip == "last_ragged_block_not_emitted" and c.n1 % EMIT:
        j0 = c.n1 - c.n1 % EMIT
        acc[:, j0:], acc2[:, j0:] = inp["acc0"][:, j0:], inp["acc20"][:, j0:]
    return acc, acc2, lse


def check_outputs(c: Case, got: dict):
    """{name: (largest error / bound, elements over the bound)} of whichever of acc / acc2 / lse ``got`` holds, against the
    fp64 reference: acc2 (zero start, weight 1) holds the map itself and is held to the map's own bound."""
    inp = make_inputs(c)
    maps, lse, bound = reference(c)
    out = {}
    if "acc2" in got:
        assert W2 == 1.0 and not bool(inp["acc20"].any())
        out["maps"] = over_the_bound(got["acc2"], maps, bound.maps)
    if "acc" in got:
        a0 = inp["acc0"]
        out["acc"] = over_the_bound(got["acc"], a0.double() + W1 * maps, acc_bound(W1, a0, maps, bound.maps))
    if "lse" in got:
        out["lse"] = over_the_bound(got["lse"], lse, bound.lse)
    return out
