"""Launch cases of ca_token_maps (conceptattention_amd/csrc/ca_tokmap.hip): seeded inputs, the fp64 reference with a
derived error bound, and an fp32 emulation of the kernel's order with named slips.

Imported by tests/test_tokmap_kernels_gpu.py (the device) and tests/test_tokmap_cases_cpu.py (the emulation lies inside
every bound, every slip leaves it).  Nothing here touches torch.cuda.

The quantity (csrc/ca_tokmap.h), per head h and query row i, over the keys j of [k0 | k1]:
    s_ij = scale_log2 <q_i, k_j>,  m_i = max_j s_ij,  l_i = sum_j exp2(s_ij - m_i),  p_it = exp2(s_it - m_i) / l_i
    map[t, i] = (1 / H) sum_h p_it (t < n_tok),     lse[h, i] = (m_i + log2 l_i) ln 2.

Bound, elementwise and first order, u = 2^-24; what the kernel is allowed to do, term by term:
  products   bf16 x bf16 and half x half are exact in fp32's 24 bits: no term.
  score      fp32 accumulation of 128 products on the matrix unit, in an order and with an internal rounding that the
             instruction does not publish: every one of the 128 additions is charged a whole ulp (2 u) of the running
             magnitude, which is at most A_ij = |scale_log2| sum_d |q_id| |k_jd|; the product with scale_log2 rounds once:
                 eps_ij = 2 * 128 u A_ij + u |s_ij|                       (in log2 units)
  exponent   s - m is one subtraction (u |s_ij - m_i|); the error of m itself cancels between a cell and its row sum
             (p is invariant under a common shift) up to the second-order factor below.
  exp2       one hardware v_exp_f32 per cell, 1 ulp: EXP_REL = 2 u, relative.
  numerator  E_num(t) = ln 2 (eps_it + u |s_it - m_i|) + EXP_REL
  row sum    every term carries its own E_num(j), so the sum carries their average under the softmax weights w_ij; then
             n0 + n1 - 1 fp32 additions of positive terms in any order ((n - 1) u), and the online form: once per key tile
             of 64 the running sum is multiplied by exp2(m_old - m_new) and added to (EXP_REL + 2 u per tile), and the
             exponents of those factors round like any other (u ln 2 times their total, which is at most the row's spread
             R_i = max_j s_ij - min_j s_ij):
                 E_den = sum_j w_ij E_num(j) + (n - 1) u + ceil(n / 64) (EXP_REL + 2 u) + u ln 2 R_i
  division   one per cell; charged DIV_REL = 3 u (a correctly rounded one is u).
  cell       |dp_it| <= p_it rel (1 + rel),  rel = E_num(t) + E_den + DIV_REL   (the second-order factor of the product).
  heads      H - 1 fp32 additions of non-negative terms and the product with the rounded 1 / H: (H + 1) u map.
  floor      a cell whose exp2 lies below fp32's normal range may be flushed to zero: 2^-126, absolute.
  accumulate acc + weight map is one fused multiply-add: u |acc + weight map| (acc_bound()).
  everything times SECOND_ORDER = 1 + 2^-6.
lse: the relative error of l is E_den, which is an absolute error in nats; log2 l is one v_log_f32 (1 ulp of its result,
  and 2^-21 absolute where l is next to 1), the addition and the product with ln 2 round once each:
      |dlse| <= E_den + ln 2 (2 u log2 l + 2^-21 + u |m + log2 l|) + u |lse|,   the score error of m being part of E_den
      through the weights (the maximum's own weight is at least 1 / n) plus eps at the maximum itself.

The cold-text family is why the bound is relative: its text cells are about e^-20 / n, and an absolute bound at the scale
of the large cells would pass a kernel that returns zeros there.
"""
from __future__ import annotations

import functools
import math
import zlib
from dataclasses import dataclass

import torch

U = 2.0 ** -24
EXP_REL = 2 * U
DIV_REL = 3 * U
SECOND_ORDER = 1 + 2.0 ** -6
FLOOR = 2.0 ** -126
LN2 = math.log(2.0)
LOG2E = 1.4426950408889634
SCALE_LOG2 = float(torch.tensor(LOG2E / math.sqrt(128.0), dtype=torch.float32))   # softmax_scale * log2(e), as fp32
TILE = 64
W1, W2 = 0.625, 1.0              # the accumulators' weights (exact in fp32): acc starts at N(0, 0.1) (the accumulate
                                 # semantics), acc2 at zero with weight 1, so that it holds the map itself, bit for bit,
                                 # and is compared with the map's own bound
NAN_BITS = 0x7FFF                # NaN as bf16 and as IEEE half
PAD_COLS = 8                     # NaN columns behind every row of an "apart" operand

FAMILIES = ("unit", "peaky8", "peaky16", "cold_text", "dominant", "ties", "last_tile_max")


@dataclass(frozen=True)
class Case:
    heads: int
    nq: int
    n0: int
    n_tok: int
    n1: int
    f16: bool
    family: str = "unit"
    layout: str = "qkv"      # qkv: q and k column slices of one [rows, 3 heads 128] buffer; apart: three padded buffers
    prescaled: bool = False  # the q rows carry softmax_scale * log2(e), scale_log2 = 1.0 (the model's form)

    @property
    def id(self):
        return (f"h{self.heads}_nq{self.nq}_t{self.n0}.{self.n_tok}_i{self.n1}_{'f16' if self.f16 else 'bf16'}_{self.family}"
                f"_{self.layout}{'_pre' if self.prescaled else ''}")

    @property
    def scale_log2(self):
        return 1.0 if self.prescaled else SCALE_LOG2


HEADS = (1, 2, 3, 24)
NQ = (1, 15, 16, 17, 63, 64, 65, 200)
N0_TOK = ((1, 1), (8, 1), (8, 4), (8, 8), (64, 1), (64, 32), (64, 64), (77, 1), (77, 40), (77, 77),
          (256, 1), (256, 100), (256, 256), (512, 1), (512, 300), (512, 512))
N1 = (0, 1, 63, 64, 65, 1100)


def _cases():
    out = []
    k = 0

    def add(**kw):
        nonlocal k
        kw.setdefault("f16", bool(k & 1))
        kw.setdefault("layout", ("qkv", "apart")[(k >> 1) & 1])
        kw.setdefault("prescaled", bool((k >> 2) & 1))
        out.append(Case(**kw))
        k += 1
    for nq in NQ:                                   # around the wave's 16 rows and the workgroup's 64; several workgroups
        add(heads=2, nq=nq, n0=8, n_tok=4, n1=65)
    for n0, n_tok in N0_TOK:                        # one text key .. the limit; n_tok 1, a middle value, n0
        add(heads=2, nq=65, n0=n0, n_tok=n_tok, n1=63)
    for n1 in N1:                                   # no image keys; around the key tile; many tiles
        add(heads=2, nq=17, n0=77, n_tok=40, n1=n1)
    for heads in HEADS:
        add(heads=heads, nq=17, n0=8, n_tok=8, n1=65)
    for fam in FAMILIES:                            # every family in both storage types
        for f16 in (False, True):
            add(heads=3, nq=65, n0=77, n_tok=40, n1=200, family=fam, f16=f16)
    for f16 in (False, True):                       # everything large at once: 4 workgroups, 26 key tiles, 32 token groups
        add(heads=3, nq=200, n0=512, n_tok=512, n1=1100, family="peaky8", f16=f16, layout="qkv")
    add(heads=2, nq=65, n0=8, n_tok=8, n1=0, family="ties")                      # the text keys alone, one ragged tile
    add(heads=2, nq=17, n0=77, n_tok=77, n1=51, family="last_tile_max", f16=True)  # 128 keys: no ragged tile
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def _gen(tag: str) -> torch.Generator:
    g = torch.Generator(device="cpu")
    g.manual_seed(zlib.crc32(tag.encode()))
    return g


def to_bits(x: torch.Tensor, f16: bool) -> torch.Tensor:
    """fp32 values -> the int16 bit patterns of their bf16 / IEEE half roundings."""
    return x.to(torch.float16 if f16 else torch.bfloat16).view(torch.int16)


def from_bits(bits: torch.Tensor, f16: bool, dtype=torch.float64) -> torch.Tensor:
    return bits.contiguous().view(torch.float16 if f16 else torch.bfloat16).to(dtype)


def _values(c: Case):
    """(q [nq, H, 128], k [n0 + n1, H, 128]) fp32 before the storage rounding.  scale <q, k> has a standard deviation of
    1 nat in the unit family; u is a unit vector per head along which the other families push rows apart."""
    g = _gen("tokmap." + c.id)
    n = c.n0 + c.n1
    q = torch.randn(c.nq, c.heads, 128, generator=g)
    k = torch.randn(n, c.heads, 128, generator=g)
    u = torch.randn(c.heads, 128, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    a = math.sqrt(20.0 * math.sqrt(128.0))          # scale * a * a = 20 nats
    fam = c.family
    if fam in ("peaky8", "peaky16"):
        q = q * float(fam[5:])
    elif fam == "cold_text":                        # every image key 20 nats above the text keys
        assert c.n1 > 0
        q = q + a * u
        k[c.n0:] += a * u
    elif fam == "dominant":                         # one text key 30 nats up: its cell is 1 to a few e^-30
        q = q + a * u
        k[c.n_tok // 2] += 1.5 * a * u
    elif fam == "ties":                             # the same row four times, 20 nats up: exact ties at the maximum
        q = q + a * u
        row = k[0] + a * u
        for j in {0, c.n_tok - 1, n // 2, n - 1}:
            k[j] = row
    elif fam == "last_tile_max":                    # the row maximum is the last key
        q = q + a * u
        k[n - 1] += 0.6 * a * u
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
    if c.layout == "qkv":                           # rows [text | image], columns [q | k | v]; the q rows are the image rows
        rows = c.n0 + max(c.nq, c.n1) + 1
        buf = torch.full((rows, 3 * W), NAN_BITS, dtype=torch.int16)
        buf[c.n0:c.n0 + c.nq, :W] = qb
        buf[:c.n0 + c.n1, W:2 * W] = kb
        buffers = {"qkv": buf}
        views = {"q": ("qkv", c.n0, c.nq, 0), "k0": ("qkv", 0, c.n0, W), "k1": ("qkv", c.n0, c.n1, W)}
    else:
        def padded(b):
            out = torch.full((b.shape[0] + 1, W + PAD_COLS), NAN_BITS, dtype=torch.int16)
            out[:-1, :W] = b
            return out
        # (k0 and k1 share a row stride, as ca_token_maps wants it; they are two allocations all the same)
        buffers = {"q": padded(qb), "k0": padded(kb[:c.n0]), "k1": padded(kb[c.n0:])}
        views = {"q": ("q", 0, c.nq, 0), "k0": ("k0", 0, c.n0, 0), "k1": ("k1", 0, c.n1, 0)}
    g = _gen("tokmap.acc." + c.id)
    acc0 = (torch.randn(c.n_tok, c.nq, generator=g) * 0.1).to(torch.float32)
    acc20 = torch.zeros(c.n_tok, c.nq, dtype=torch.float32)
    return dict(buffers=buffers, views=views, acc0=acc0, acc20=acc20)


def view(c: Case, buffers, name: str):
    """The operand as a [rows, heads 128] slice of its buffer (host or device)."""
    b, r0, n, c0 = make_inputs(c)["views"][name]
    return buffers[b][r0:r0 + n, c0:c0 + c.heads * 128]


def operands(c: Case, inp=None, f16=None, dtype=torch.float64):
    """(q [nq, H, 128], k [n, H, 128]) decoded from the stored bits."""
    inp = inp or make_inputs(c)
    f16 = c.f16 if f16 is None else f16
    q = from_bits(view(c, inp["buffers"], "q"), f16, dtype).reshape(c.nq, c.heads, 128)
    k = torch.cat([from_bits(view(c, inp["buffers"], n), f16, dtype) for n in ("k0", "k1")]).reshape(-1, c.heads, 128)
    return q, k


@dataclass
class Bound:
    maps: torch.Tensor    # [n_tok, nq]
    lse: torch.Tensor     # [heads, nq]


def reference_qk(q, k, n_tok: int, scale_log2: float):
    """fp64 (maps [n_tok, nq], lse [H, nq], Bound) from q [nq, H, 128] and k [n, H, 128]."""
    q, k = q.double(), k.double()
    nq, H, _ = q.shape
    n = k.shape[0]
    maps = torch.zeros(nq, n_tok, dtype=torch.float64)
    err = torch.zeros(nq, n_tok, dtype=torch.float64)
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
        e_den = (w * e_num).sum(1, keepdim=True) + (n - 1) * U + tiles * (EXP_REL + 2 * U) + U * LN2 * spread
        rel = e_num[:, :n_tok] + e_den + DIV_REL
        maps += w[:, :n_tok]
        err += w[:, :n_tok] * rel * (1 + rel)
        log2l = torch.log2(l)
        lse[h] = ((m + log2l) * LN2)[:, 0]
        at_max = (LN2 * (2 * 128 * U * A + U * s.abs())).amax(1, keepdim=True)     # (of all keys: at least the maximum's)
        blse[h] = (e_den + at_max + LN2 * (2 * U * log2l + 2.0 ** -21 + U * (m + log2l).abs()) + U * lse[h][:, None].abs())[:, 0]
    maps = maps / H
    bound = (err / H + (H + 1) * U * maps) * SECOND_ORDER + FLOOR
    return maps.T.contiguous(), lse, Bound(bound.T.contiguous(), blse * SECOND_ORDER)


@functools.lru_cache(maxsize=None)
def reference(c: Case):
    """fp64 (maps, lse, bound) of a case; computed once and shared (read-only)."""
    q, k = operands(c)
    return reference_qk(q, k, c.n_tok, c.scale_log2)


def acc_bound(weight: float, acc0: torch.Tensor, maps: torch.Tensor, bound_maps: torch.Tensor) -> torch.Tensor:
    """The bound of acc0 + weight * map, one fused multiply-add on top of the map's own error."""
    return abs(weight) * bound_maps + U * (acc0.double() + weight * maps).abs() * SECOND_ORDER


def over_the_bound(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor):
    """(largest error / bound, elements over the bound); a NaN or an element never written counts as over."""
    ratio = (got.double().cpu() - want).abs() / bound
    bad = ~(ratio <= 1.0)
    return float(torch.nan_to_num(ratio, nan=float("inf")).max()), int(bad.sum())


SLIPS = ("wrong_scale", "max_over_text_only", "last_ragged_tile_not_summed", "heads_averaged_before_division",
         "tokens_from_the_wrong_end", "half_bits_read_as_bf16")


def emulate(c: Case, slip=None):
    """The kernel's order in fp32 (maps [n_tok, nq], lse [H, nq]): fp32 scores times scale_log2; per key tile of 64 the
    running maximum, common to a row, and the running sum kept apart for the four key groups (j mod 16) / 4 that a lane
    group owns, rescaled by exp2(m_old - m_new); the four sums added pairwise; exp2(s - m) / l per cell; the heads added
    in order; the product with the rounded 1 / H.  ``slip``, one of SLIPS:
      wrong_scale                     the natural-log scale where the log2 one is wanted (scale_log2 / log2 e);
      max_over_text_only              the cells and lse use the maximum over the n0 text keys, the row sum the true one;
      last_ragged_tile_not_summed     the keys of a last tile that is not full never reach the row sum;
      heads_averaged_before_division  mean_h exp2(s - m) / mean_h l;
      tokens_from_the_wrong_end       the last n_tok text rows instead of the first;
      half_bits_read_as_bf16          (half-precision cases) the bits decoded as bf16."""
    assert slip is None or slip in SLIPS, slip
    f = torch.float32
    q, k = operands(c, f16=False if slip == "half_bits_read_as_bf16" else None, dtype=f)
    n = c.n0 + c.n1
    scale = torch.tensor(c.scale_log2 / LOG2E if slip == "wrong_scale" else c.scale_log2, dtype=f)
    tiles = (n + TILE - 1) // TILE
    tok = slice(c.n0 - c.n_tok, c.n0) if slip == "tokens_from_the_wrong_end" else slice(0, c.n_tok)
    inv_h = torch.tensor(1.0, dtype=f) / torch.tensor(float(c.heads), dtype=f)
    total = torch.zeros(c.nq, c.n_tok, dtype=f)
    num_sum, den_sum = torch.zeros(c.nq, c.n_tok, dtype=f), torch.zeros(c.nq, 1, dtype=f)
    lse = torch.zeros(c.heads, c.nq, dtype=f)
    for h in range(c.heads):
        s = (q[:, h] @ k[:, h].T) * scale
        sp = torch.full((c.nq, tiles * TILE), -math.inf, dtype=f)
        sp[:, :n] = s
        sp = sp.reshape(c.nq, tiles, 4, 4, 4)                     # [row, tile, 16-key group, lane group, key of the lane]
        m = torch.full((c.nq,), -math.inf, dtype=f)
        l = torch.zeros(c.nq, 4, dtype=f)
        for t in range(tiles):
            st = sp[:, t]
            m_new = torch.maximum(m, st.amax((1, 2, 3)))
            part = torch.exp2(st - m_new[:, None, None, None]).permute(0, 2, 1, 3).reshape(c.nq, 4, 16).sum(-1)
            if slip == "last_ragged_tile_not_summed" and t == tiles - 1 and n % TILE:
                part = torch.zeros_like(part)
            l = l * torch.exp2(m - m_new)[:, None] + part
            m = m_new
        l = ((l[:, 0] + l[:, 1]) + (l[:, 2] + l[:, 3]))[:, None]
        m = m[:, None]
        m_num = s[:, :c.n0].amax(1, keepdim=True) if slip == "max_over_text_only" else m
        e = torch.exp2(s[:, tok] - m_num)
        total = total + e / l
        num_sum, den_sum = num_sum + e, den_sum + l
        lse[h] = ((m_num + torch.log2(l)) * torch.tensor(LN2, dtype=f))[:, 0]
    maps = (num_sum * inv_h) / (den_sum * inv_h) if slip == "heads_averaged_before_division" else total * inv_h
    return maps.T.contiguous(), lse


def emulate_acc(acc0: torch.Tensor, weight: float, maps: torch.Tensor) -> torch.Tensor:
    """acc0 + weight * map as one fused multiply-add (fp64 holds the product and the sum of fp32 values to well below u)."""
    return (acc0.double() + float(weight) * maps.double()).to(torch.float32)
