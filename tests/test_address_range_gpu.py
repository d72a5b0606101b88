"""Where the kernels read and write once addresses get large ("Address arithmetic").

a. Placement.  One small case of tests/attn_cases.py per attention kernel and, per GEMM launch route of
   tests/gemm_route_cases.py, the epilogues that between them use every operand, run with all buffers at `bit31`
   (tests/placement.py: bit 31 of every address set) and then once per operand role with that role's buffer across a
   2^32 line (`straddle`) and the others at bit31.  Every run must give the bits of the `plain` run (ordinary torch
   allocations) and stay inside the case table's own fp64 bound; padding comes back NaN, guard bands and inputs
   unchanged.
b. Far rows.  The three attention kernels on key / value rows with a huge row stride: (n0 + n1) * ldkv * 2 at 3 GiB and
   at the largest extent the validator accepts, once with every key in segment 0 and once with segment 1 carrying the
   far rows behind a straddling tile, with a ragged tail (the fast path and stage() use different arithmetic).
c. Rejection.  Both limits of ca_attn_fwd_bf16 / ca_attn_fwd_qk16 exactly: the value just under runs and is right,
   the value at the limit is refused with its message and no byte of the declared extent, which is real memory the
   test owns, changes.

The row-op cases of tests/rowop_cases.py are placed the same way (every case, every input and output plane).  GEMM far
rows: A alone and W alone per launch route at 3 GiB and at the largest accepted extent, and one real modulation_gemm
chunk (W contiguous over just under 4 GiB).  The operands DESIGN.md calls 64-bit clean get one case each with their
last row more than 4 GiB from the base.

At most the 8 GiB arena plus the small plain buffers of one case are live (the condition is 10 GiB); the peak is
printed by the last test."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_cases as A  # noqa: E402
import gemm_route_cases as G  # noqa: E402
import placement as PL  # noqa: E402
import test_attn_routes_gpu as TA  # noqa: E402
import test_gemm_routes_gpu as TG  # noqa: E402
import address_range_cases as C  # noqa: E402
import rowop_cases as R  # noqa: E402
import test_rowop_routes_gpu as TR  # noqa: E402
import test_vae_routes_gpu as TV  # noqa: E402
import vae_cases as V  # noqa: E402
import clip_cases as CL  # noqa: E402
import pixel_cases as PX  # noqa: E402
import seg_cases as SG  # noqa: E402
import t5_fp8_cases as F8  # noqa: E402
import test_clip_kernels_gpu as TC  # noqa: E402
import test_pixel_kernels_gpu as TP  # noqa: E402
import test_seg_kernels_gpu as TS  # noqa: E402
import test_t5_fp8_kernels_gpu as TF  # noqa: E402
import test_t5_kernels_gpu as TT  # noqa: E402
from address_range_cases import (ATTN_FAR, ATTN_LIMITS, ATTN_PLACEMENT, ATTN_ROLES, GEMM_INPUT_FIELD,  # noqa: E402
                                 far_ldkv, gemm_epis_for)
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
NAN = float("nan")
COUNTS = {"attention placement": 0, "gemm placement": 0, "rowop placement": 0, "vae placement": 0, "text placement": 0,
          "attention far": 0, "gemm far": 0, "past 4 GiB": 0}


def _bytes(t):
    return t.contiguous().view(torch.uint8)


@pytest.fixture(scope="module")
def arena():
    torch.cuda.reset_peak_memory_stats()
    a = PL.Arena(DEV)
    yield a
    a.buf = None
    torch.cuda.empty_cache()


def _assert_placed(pl, role):
    B = pl.arena.B
    for r, (start, n) in pl.placed.items():
        if r == role or (role is not None and pl.placed[r] == pl.placed.get(role)):
            assert start < B < start + n or n <= 16, (r, hex(start), n)
        else:
            assert start + n <= B and start >> 31 & 1, (r, hex(start), n)
    if role is not None:
        assert role in pl.placed, f"role {role} was never allocated"


# ---------------------------------------------------------------------------------------------- a. placement
@pytest.mark.parametrize("kernel", list(ATTN_PLACEMENT), ids=str)
def test_attention_placement(arena, kernel):
    case = A.BY_ID[ATTN_PLACEMENT[kernel]]
    assert case.kernel == kernel
    inp = A.make_inputs(case)
    plain = TA.launch(case, inp)
    TA.check_untouched(case, plain)
    TA.check_bounds(case, inp, plain)
    for role in [None] + ATTN_ROLES[kernel]:
        pl = arena.placer(role)
        res = TA.launch(case, inp, alloc=pl)
        _assert_placed(pl, role)
        TA.check_untouched(case, res)          # padding NaN, inputs unchanged
        pl.check_guards()
        TA.check_bounds(case, inp, res)
        for i, (a, b) in enumerate(zip(plain, res)):
            for k in ("out", "f32", "hm"):
                if a[k] is not None:
                    assert torch.equal(_bytes(a[k]), _bytes(b[k])), f"{case.id}[{i}] {k}: {role or 'bit31'} != plain"
        COUNTS["attention placement"] += 1


GEMM_RUNS = [(r, e) for r in G.ROUTES for e in gemm_epis_for(r)]


@pytest.mark.parametrize("route,epi", GEMM_RUNS, ids=lambda v: str(v))
def test_gemm_placement(arena, route, epi):
    r = G.ROUTES[route]
    M, N, ns = TG.shape_or_skip(route, epi, 128)
    x = G.make_inputs(epi, M, N, 128, ns, r.fp8, r.rem)
    (plain,), info = TG.launch([x], r.tile, route=route)
    TG.check_against_fp64(x, plain, f"{route}-{epi} plain")
    roles = C.gemm_roles(epi, r.fp8)
    for role in [None] + roles:
        pl, keep = arena.placer(role), {}
        (got,), _ = TG.launch([x], r.tile, route=route, alloc=pl, keep=keep)
        _assert_placed(pl, role)
        assert set(pl.placed) == set(roles), set(pl.placed) ^ set(roles)
        pl.check_guards()
        if role is None:       # (the other runs are held to the same bound by their bit identity with `plain`)
            TG.check_against_fp64(x, got, f"{route}-{epi} bit31")
        for k in plain:
            assert torch.equal(_bytes(plain[k]), _bytes(got[k])), f"{route}-{epi} {k}: {role or 'bit31'} != plain"
        for name, field in GEMM_INPUT_FIELD.items():
            if name in keep:
                assert torch.equal(_bytes(keep[name]), _bytes(getattr(x, field).to(DEV))), f"{name} changed"
        if "out2" in keep:
            c0, c1 = keep["out2_cols"]
            assert bool(keep["out2"][:, :c0].isnan().all()) and bool(keep["out2"][:, c1:].isnan().all()), \
                "out2 padding written"
        COUNTS["gemm placement"] += 1


# ---------------------------------------------------------------------------------------------- b. far rows
def far_launch(arena, case, inp, ldkv, expect_error=None):
    """TA.launch with the key / value rows at row stride ldkv inside the arena: segment 1's rows first in memory, then
    segment 0's.  Only the touched rows (one head-width of k and of v per row) are written."""
    (p,), (x,) = case.probs, inp
    D = case.heads * 128
    nk = p.nk
    q0c, q1c, k0, v0, k1, v1 = A.views(case, p, x)
    ext = ((nk - 1) * ldkv + 2 * D) * 2
    declared = nk * ldkv * 2                       # what the validator measures
    start = (arena.base + PL.GUARD + 255) // 256 * 256
    span = (max(ext, declared) + 255) // 256 * 256
    for g in (start - PL.GUARD, start + span):
        arena.window(g, PL.GUARD).fill_(PL.PATTERN)
    far = arena.window(start, span).view(torch.bfloat16)
    rows = far.as_strided((nk, 2 * D), (ldkv, 1))
    rows.fill_(NAN)
    if p.n1:
        rows[:p.n1, :D], rows[:p.n1, D:] = k1.to(DEV), v1.to(DEV)
    rows[p.n1:, :D], rows[p.n1:, D:] = k0.to(DEV), v0.to(DEV)
    rows0 = rows.clone()
    K1, V1 = (rows[:p.n1, :D], rows[:p.n1, D:]) if p.n1 else (None, None)
    K0, V0 = rows[p.n1:, :D], rows[p.n1:, D:]
    qbuf = x.qbuf.to(DEV)
    gx = dataclasses.replace(x, qbuf=qbuf)
    nq1 = p.nq - p.nq0 if p.two_q else 0
    nq0 = p.nq - nq1
    q0 = qbuf[x.gq0:x.gq0 + nq0, :D]
    q1 = qbuf[x.gq1:x.gq1 + nq1, :D] if nq1 else None
    out = torch.full((x.out_rows, x.ldo), NAN, device=DEV, dtype=torch.bfloat16)
    own = torch.zeros(out.shape, dtype=torch.bool, device=DEV)
    own[x.gq0:x.gq0 + nq0, :D] = True
    own[x.gq1:x.gq1 + nq1, :D] = True
    f32 = torch.full((p.nq + 1, x.ldo32), NAN, device=DEV)
    attn = ops.Attn(q0, out[x.gq0:x.gq0 + nq0, :D], K0, V0, K1, V1, out_f32=f32[:p.nq, :D], q1=q1,
                    out1=out[x.gq1:x.gq1 + nq1, :D] if nq1 else None)
    kw = dict(scale=case.scale) if case.form == "scale" else dict(q_prescaled=True, qk_f16=case.form == "qk16")
    if expect_error is not None:
        sum0 = arena.window(start, span).view(torch.int64).sum().item()
        with pytest.raises(ValueError, match=expect_error):
            ops.attention([attn], case.heads, **kw)
        torch.cuda.synchronize()
        sum1 = arena.window(start, span).view(torch.int64).sum().item()
        assert sum0 == sum1, "a refused call changed the key / value extent"
        assert bool(out.isnan().all()) and bool(f32.isnan().all()), "a refused call wrote an output"
    else:
        ops.attention([attn], case.heads, **kw)
        torch.cuda.synchronize()
    assert torch.equal(_bytes(rows), _bytes(rows0)), "k / v rows changed"
    assert torch.equal(_bytes(qbuf), _bytes(x.qbuf.to(DEV))), "q buffer changed"
    for g in (start - PL.GUARD, start + span):
        assert bool((arena.window(g, PL.GUARD) == PL.PATTERN).all()), "guard band written"
    res = [dict(x=gx, out=out, own=own, f32=f32, hm=None, hmcon=None, nq0=nq0, nq1=nq1)]
    if expect_error is None:
        assert bool(out[~own].isnan().all()) and bool(f32[-1].isnan().all()) and bool(f32[:, D:].isnan().all())
    return res


def _far_case(form, layout):
    nq, n0, n1, nq0 = layout
    return A.Case(f"far_{form}_{n0}_{n1}", form, 1, (A.Prob(nq, n0, n1, nq0=nq0, f32=True, seed=900 + n1),))


@pytest.mark.parametrize("form", list(A.FORMS))
@pytest.mark.parametrize("name", list(ATTN_FAR))
def test_attention_far_rows(arena, form, name):
    layout, extent = ATTN_FAR[name]
    case = _far_case(form, layout)
    ldkv = far_ldkv(case.probs[0].nk, extent)
    assert case.probs[0].nk * ldkv * 2 < 1 << 32
    print(f"\n  {case.id}: ldkv={ldkv}, (n0 + n1) * ldkv * 2 = {case.probs[0].nk * ldkv * 2}")
    inp = A.make_inputs(case)
    res = far_launch(arena, case, inp, ldkv)
    TA.check_bounds(case, inp, res)
    plain = TA.launch(case, inp)                       # the same problem at the case table's small stride
    for k in ("out", "f32"):
        assert torch.equal(_bytes(plain[0][k]), _bytes(res[0][k])), f"{case.id} {k}: far rows != small stride"
    COUNTS["attention far"] += 1


class FarAlloc(PL.Plain):
    """Ordinary allocations, except the 2-D buffer that carries `role`: that one gets a huge row stride inside the
    arena, the largest multiple of 64 elements with rows * ld * itemsize <= extent (so with extent > 4 GiB its last row
    starts more than 4 GiB from its base).  Only its rows are written; guard bands at both ends."""

    def __init__(self, arena, role, extent):
        super().__init__(DEV)
        self.arena, self.role, self.extent = arena, role, extent
        self.view = None

    def _far(self, shape, dtype):
        assert self.view is None and len(shape) == 2, (self.role, shape)
        rows, cols = shape
        item = torch.empty((), dtype=dtype).element_size()
        self.ld = C.far_ld(rows, item, self.extent)
        assert self.ld >= cols, (shape, self.ld)
        span = (((rows - 1) * self.ld + cols) * item + 255) // 256 * 256
        self.last_row_offset = (rows - 1) * self.ld * item
        self.start = (self.arena.base + PL.GUARD + 255) // 256 * 256
        self.span = span
        for g in (self.start - PL.GUARD, self.start + span):
            self.arena.window(g, PL.GUARD).fill_(PL.PATTERN)
        self.view = self.arena.window(self.start, span).view(dtype).as_strided((rows, cols), (self.ld, 1))
        return self.view

    def to(self, t, roles=None):
        if roles and self.role in roles:
            v = self._far(tuple(t.shape), t.dtype)
            v.copy_(t.to(DEV))
            return v
        return super().to(t, roles)

    def full(self, shape, fill, dtype, roles=None):
        if roles and self.role in roles:
            v = self._far(tuple(shape), dtype)
            v.fill_(fill)
            return v
        return super().full(shape, fill, dtype, roles)

    def check_guards(self):
        assert self.view is not None, f"role {self.role} was never allocated"
        for g in (self.start - PL.GUARD, self.start + self.span):
            assert bool((self.arena.window(g, PL.GUARD) == PL.PATTERN).all()), "guard band written"


def run_rowop(case, inp, alloc=None):
    """A row-op case as test_rowop_against_fp64 runs and checks it; returns the outputs."""
    got, pads = TR.RUN[case.op](case, inp, alloc)
    scale = got.get("scale") if case.op in ("ln", "quant") else None
    ref = R.reference(case, inp, dev=DEV, scale_got=scale)
    assert set(ref) == set(got), (set(ref), set(got))
    for name, (r, pre, kind) in ref.items():
        ratio, n_over = R.excess(got[name], r, pre, kind)
        assert n_over == 0, f"{case.id}: {name} ({kind}) {n_over} elements over the bound, max err / bound {ratio:.3g}"
    for buf, before, w in pads:
        TR.assert_same_bytes(buf[:, w:], before[:, w:], f"{case.id}: padding beyond column {w}")
    return {k: v.clone() for k, v in got.items()}


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_rowop_placement(arena, case):
    inp = R.make_inputs(case)
    plain = run_rowop(case, inp)
    roles = C.rowop_roles(case)
    for role in [None] + roles:
        pl = arena.placer(role)
        got = run_rowop(case, inp, pl)
        _assert_placed(pl, role)
        assert {r for r in pl.placed if "[" not in r} == set(roles), (set(pl.placed), roles)
        pl.check_guards()
        for k in plain:
            assert torch.equal(_bytes(plain[k]), _bytes(got[k])), f"{case.id} {k}: {role or 'bit31'} != plain"
        COUNTS["rowop placement"] += 1


# ------------------------------------------------------------------------------- b. GEMM far rows, operands past 4 GiB
def _gemm_far(arena, route, epi, role, extent, past=False):
    r = G.ROUTES[route]
    M, N, ns = TG.shape_or_skip(route, epi, 128)
    x = G.make_inputs(epi, M, N, 128, ns, r.fp8, r.rem)
    (plain,), _ = TG.launch([x], r.tile, route=route)
    fa, keep = FarAlloc(arena, role, extent), {}
    (got,), info = TG.launch([x], r.tile, route=route, alloc=fa, keep=keep)
    fa.check_guards()
    assert (fa.last_row_offset >= 1 << 32) == past, (fa.last_row_offset, past)
    print(f"\n  {route}-{epi} {role}: ld={fa.ld}, last row {fa.last_row_offset} bytes from the base")
    TG.check_against_fp64(x, got, f"{route}-{epi} {role} far")
    for k in plain:
        assert torch.equal(_bytes(plain[k]), _bytes(got[k])), f"{route}-{epi} {k}: far {role} != plain"
    for name, field in GEMM_INPUT_FIELD.items():
        if name in keep:
            assert torch.equal(_bytes(keep[name]), _bytes(getattr(x, field).to(DEV))), f"{name} changed"


@pytest.mark.parametrize("role,name,extent", C.GEMM_FAR, ids=lambda v: str(v))
@pytest.mark.parametrize("route", list(G.ROUTES))
def test_gemm_far_rows(arena, route, role, name, extent):
    _gemm_far(arena, route, C.GEMM_FAR_EPI, role, extent)
    COUNTS["gemm far"] += 1


def test_modulation_gemm_chunk_w_just_under_4_gib(arena):
    """One chunk of ops.modulation_gemm as the full-depth model launches it: the stacked bf16 planes of 8 vectors
    through the thin-row kernel, K = 3072, W rows contiguous over just under 4 GiB (row offsets with bit 31 set from
    row 349 526 on), fp32 output, no bias.  The first, the middle and the last 256 columns against fp64."""
    M, K, N = C.MOD_CHUNK["M"], C.MOD_CHUNK["K"], C.MOD_CHUNK["N"]
    assert (1 << 32) - (1 << 21) < N * K * 2 < 1 << 32
    start = (arena.base + PL.GUARD + 255) // 256 * 256
    for g in (start - PL.GUARD, start + N * K * 2):
        arena.window(g, PL.GUARD).fill_(PL.PATTERN)
    w = arena.window(start, N * K * 2).view(torch.bfloat16).view(N, K)
    w.normal_(0.0, K ** -0.5)
    sum0 = w.view(torch.int64).sum().item()
    g = torch.Generator().manual_seed(5)
    a = torch.randn(M, K, generator=g).bfloat16()
    ad = a.to(DEV)
    out = torch.full((M, N), NAN, device=DEV)
    gm = ops.Gemm(ad, w, None, out, TG.L.EPI_BIAS)
    info = ops.gemm_plan([gm], tile=TG.L.TILE_PP_256x256)
    assert info["thin_mf"] > 0, info
    ops.gemm([gm], TG.L.TILE_PP_256x256)
    torch.cuda.synchronize()
    assert sum0 == w.view(torch.int64).sum().item() and torch.equal(ad.cpu(), a), "an operand changed"
    for gd in (start - PL.GUARD, start + N * K * 2):
        assert bool((arena.window(gd, PL.GUARD) == PL.PATTERN).all()), "guard band written"
    assert bool(torch.isfinite(out).all()), "columns never written"
    for c0 in (0, (N // 2) // 256 * 256, N - 256):
        x = G.Inputs(M, 256, K, 0, "bias_f32", False, a=a, w=w[c0:c0 + 256].cpu(), bias=torch.zeros(256).bfloat16())
        TG.check_against_fp64(x, {"out": out[:, c0:c0 + 256]}, f"modulation chunk columns {c0}..")
    COUNTS["gemm far"] += 1


@pytest.mark.parametrize("route,epi,role", C.GEMM_PAST, ids=lambda v: str(v))
def test_gemm_operand_past_4_gib(arena, route, epi, role):
    _gemm_far(arena, route, epi, role, C.PAST_4GIB, past=True)
    COUNTS["past 4 GiB"] += 1


@pytest.mark.parametrize("role", C.ATTN_PAST)
@pytest.mark.parametrize("kernel", list(ATTN_PLACEMENT), ids=str)
def test_attention_operand_past_4_gib(arena, kernel, role):
    case = A.BY_ID[ATTN_PLACEMENT[kernel]]
    inp = A.make_inputs(case)
    plain = TA.launch(case, inp)
    fa = FarAlloc(arena, role, C.PAST_4GIB)
    res = TA.launch(case, inp, alloc=fa)
    fa.check_guards()
    assert fa.last_row_offset >= 1 << 32
    TA.check_untouched(case, res)
    TA.check_bounds(case, inp, res)
    for a, b in zip(plain, res):
        for k in ("out", "f32", "hm"):
            if a[k] is not None:
                assert torch.equal(_bytes(a[k]), _bytes(b[k])), f"{case.id} {k}: far {role} != plain"
    COUNTS["past 4 GiB"] += 1


@pytest.mark.parametrize("cid,role", C.ROWOP_PAST, ids=lambda v: str(v))
def test_rowop_operand_past_4_gib(arena, cid, role):
    case = R.BY_ID[cid]
    inp = R.make_inputs(case)
    plain = run_rowop(case, inp)
    fa = FarAlloc(arena, role, C.PAST_4GIB)
    got = run_rowop(case, inp, fa)
    fa.check_guards()
    assert fa.last_row_offset >= 1 << 32, fa.last_row_offset
    for k in plain:
        assert torch.equal(_bytes(plain[k]), _bytes(got[k])), f"{case.id} {k}: far {role} != plain"
    COUNTS["past 4 GiB"] += 1


# ------------------------------------------------------------------------------------ the autoencoder kernels
@pytest.mark.parametrize("entry", list(C.VAE_PLACEMENT))
def test_vae_placement(arena, entry):
    """One case per entry point of ca_vae.hip with every operand role: all at bit31, then role by role across the
    2^32 line mid-row of a middle row.  Bit-identical to ordinary allocations, inside the case's own bounds, canary
    columns and guard bands intact."""
    case = V.BY_ID[C.VAE_PLACEMENT[entry]]
    inp = V.make_inputs(case)
    plain = TV.run_checked(case, inp)
    roles = C.VAE_ROLES[entry]
    for role in [None] + roles:
        pl = arena.placer(role)
        got = TV.run_checked(case, inp, pl)
        _assert_placed(pl, role)
        assert set(pl.placed) == set(roles), set(pl.placed) ^ set(roles)
        pl.check_guards()
        for k in plain:
            assert torch.equal(_bytes(plain[k]), _bytes(got[k])), f"{case.id} {k}: {role or 'bit31'} != plain"
        COUNTS["vae placement"] += 1


@pytest.mark.parametrize("cid,role", [v for v in C.VAE_PAST if v != C.VAE_PAST_OWN_TEST], ids=lambda v: str(v))
def test_vae_operand_past_4_gib(arena, cid, role):
    """One operand with its row stride from far_ld (its last row starts more than 4 GiB from its base), the others
    small; only the touched columns are written.  Equal to the same case at its ordinary stride."""
    case = V.BY_ID[cid]
    inp = V.make_inputs(case)
    plain = TV.run_checked(case, inp)
    fa = FarAlloc(arena, role, C.PAST_4GIB)
    got = TV.run_checked(case, inp, fa)
    fa.check_guards()
    assert fa.last_row_offset >= 1 << 32 and fa.ld < 1 << 31, (fa.last_row_offset, fa.ld)
    print(f"\n  {cid} {role}: ld={fa.ld}, last row {fa.last_row_offset} bytes from the base")
    for k in plain:
        assert torch.equal(_bytes(plain[k]), _bytes(got[k])), f"{cid} {k}: far {role} != plain"
    COUNTS["past 4 GiB"] += 1


def test_softmax_p_past_4_gib(arena):
    """ca_softmax_rows_f32 zeroes p[r, n:ldp]: with ldp from far_ld it owns, and writes, 5 rows of 1 GiB.  The test
    fills only the first n + 1024 and the last 1024 columns of every row with NaN; afterwards the probabilities equal
    the ordinary-stride run's, every other element of the extent is zero, and the guard bands are intact."""
    cid, role = C.VAE_PAST_OWN_TEST
    case = V.BY_ID[cid]
    s, inp = case.shape, V.make_inputs(case)
    rows, n = s["rows"], s["n"]
    plain = TV.run_checked(case, inp)
    ld = C.far_ld(rows, 2, C.PAST_4GIB)
    assert ld < 1 << 31 and (rows - 1) * ld * 2 >= 1 << 32     # the last row starts 2^32 bytes or more from the base
    start = (arena.base + PL.GUARD + 255) // 256 * 256
    span = rows * ld * 2
    for g in (start - PL.GUARD, start + span):
        arena.window(g, PL.GUARD).fill_(PL.PATTERN)
    full = arena.window(start, span).view(torch.bfloat16).view(rows, ld)
    full[:, :n + 1024] = NAN
    full[:, -1024:] = NAN
    sc = inp["s"].to(DEV)
    TV._call("ca_softmax_rows_f32", sc.data_ptr(), sc.stride(0), full.data_ptr(), ld, rows, n, s["scale"])
    for g in (start - PL.GUARD, start + span):
        assert bool((arena.window(g, PL.GUARD) == PL.PATTERN).all()), "guard band written"
    assert torch.equal(_bytes(plain["p"]), _bytes(full[:, :n])), "far p != plain"
    a = (n + 63) // 64 * 64                  # rows start 128-byte aligned: from column a on a row reads as int64
    for r in range(rows):                    # (min / max reductions: no temporary of the extent's size)
        body = full[r, a:].view(torch.int64)
        assert bool((full[r, n:a].view(torch.int16) == 0).all()) and body.max().item() == 0 == body.min().item(), \
            f"row {r}: padding not zero"
    COUNTS["past 4 GiB"] += 1


# ------------------------------------------------------------ the text, pixel and scoring kernels
LN_IDX = torch.tensor(CL.LN_GATHER, dtype=torch.int32)
# entry point -> the run helper of its kernel test file: (case, allocator, **kw) -> {name: a clone of the output}.  Every
# helper checks its case against the case table's own reference and bound, padding and guard rows included.
TEXT_RUN = {
    "ca_t5_attn_bf16": TT.run_attention,
    "ca_t5_rmsnorm_f32in": TT.run_rmsnorm,
    "ca_t5_rmsnorm_f32in_fp8": TF.run_rmsnorm_fp8,
    "ca_gated_mul_bf16": TT.run_gated_mul,
    "ca_gated_mul_fp8": TF.run_gated_mul_fp8,
    "ca_embed_rows_f32": lambda case, alloc=None, **kw: TT.run_embed_rows(case, alloc, **kw)[0],
    "ca_clip_attn_bf16": TC.run_attention,
    # (strided cases with the row_idx gather, the others row by row)
    "ca_layernorm_f32in": lambda case, alloc=None: TC.run_layernorm(case, alloc, gather=LN_IDX if case[2] else None)[0],
    "ca_quick_gelu_bf16": TC.run_quick_gelu,
    "ca_clip_embed_f32": lambda case, alloc=None, **kw: TC.run_clip_embed(case, alloc, **kw)[0],
    "ca_pixels_u8_to_nhwc32_bf16": TP.run_to_nhwc32,
    "ca_nhwc_f32_to_pixels_u8": TP.run_to_pixels,
    "ca_seg_score": lambda name, alloc=None: TS.run_case(next(c for c in SG.CASES if c.name == name), alloc or PL.Plain(DEV)),
}


@pytest.mark.parametrize("entry", list(C.TEXT_PLACEMENT))
def test_text_placement(arena, entry):
    """One case per entry point of ca_t5.hip, ca_clip.hip, ca_pixels.hip and ca_seg.hip with every operand role: plain,
    all at bit31, then role by role across the 2^32 line mid-row of a middle row.  Bit-identical to ordinary
    allocations, inside the case's own bound, padding columns, guard rows and guard bands intact."""
    case, roles, run = C.TEXT_PLACEMENT[entry], C.TEXT_ROLES[entry], TEXT_RUN[entry]
    plain = run(case)
    for role in [None] + roles:
        pl = arena.placer(role)
        got = run(case, pl)
        _assert_placed(pl, role)
        assert set(pl.placed) == set(roles), set(pl.placed) ^ set(roles)
        pl.check_guards()
        for k in plain:
            assert torch.equal(_bytes(plain[k]), _bytes(got[k])), f"{entry} {k}: {role or 'bit31'} != plain"
        COUNTS["text placement"] += 1


@pytest.mark.parametrize("entry,case,role,rows,item", C.TEXT_PAST, ids=lambda v: str(v))
def test_text_operand_past_4_gib(arena, entry, case, role, rows, item):
    """One operand with its row stride from far_ld (its last row starts more than 4 GiB from its base, the stride below
    2^31), the others small; only the touched columns are written.  Equal to the same case at its ordinary stride."""
    run = TEXT_RUN[entry]
    kw = dict(guard=0) if "attn" in entry else dict(vocab=8) if role in ("table", "tok") else {}
    plain = run(case, **kw)
    fa = FarAlloc(arena, role, C.PAST_4GIB)
    got = run(case, fa, **kw)
    fa.check_guards()
    assert tuple(fa.view.shape)[0] == rows and fa.view.element_size() == item, (fa.view.shape, rows, item)
    assert fa.last_row_offset >= 1 << 32 and fa.ld < 1 << 31, (fa.last_row_offset, fa.ld)
    print(f"\n  {entry} {role}: ld={fa.ld}, last row {fa.last_row_offset} bytes from the base")
    for k in plain:
        assert torch.equal(_bytes(plain[k]), _bytes(got[k])), f"{entry} {k}: far {role} != plain"
    COUNTS["past 4 GiB"] += 1


def test_pixel_source_past_4_gib(arena):
    """ca_pixels_u8_to_nhwc32_bf16 takes the source's row stride in bytes as an int64_t: five rows 2^30 bytes apart, the
    last one 2^32 bytes from the first.  The plane equals the contiguous source's."""
    h0, w0, h, w = C.PIXEL_FAR
    plain = TP.run_to_nhwc32(C.PIXEL_FAR)
    ld = C.far_ld(h0, 1, C.PAST_4GIB)
    assert (h0 - 1) * ld >= 1 << 32
    start = (arena.base + PL.GUARD + 255) // 256 * 256
    span = ((h0 - 1) * ld + w0 * 3 + 255) // 256 * 256
    for g in (start - PL.GUARD, start + span):
        arena.window(g, PL.GUARD).fill_(PL.PATTERN)
    src = arena.window(start, span).as_strided((h0, w0, 3), (ld, 3, 1))
    host = torch.from_numpy(PX.source_image(h0, w0))
    src.copy_(host)
    dst = torch.full((h, w, 32), TP.POISON, device=DEV, dtype=torch.bfloat16)
    ops.pixels_to_nhwc32(src, dst)
    torch.cuda.synchronize()
    assert torch.equal(_bytes(dst), _bytes(plain["dst"])), "far src != plain"
    assert torch.equal(src.cpu(), host), "the source changed"
    for g in (start - PL.GUARD, start + span):
        assert bool((arena.window(g, PL.GUARD) == PL.PATTERN).all()), "guard band written"
    COUNTS["past 4 GiB"] += 1


def test_a_row_stride_beyond_int32_is_refused_before_any_launch(arena):
    """A uint8 [2, 256] view whose rows are 2^32 + 256 bytes apart, as the out of t5_rmsnorm_fp8: ctypes would hand the
    library ldo = 256, which passes its ldo >= H check, and row 1 would land 256 bytes behind row 0.  ops._i32 raises,
    naming the argument; nothing is launched: both rows, the bytes a truncated stride would have hit and the scales
    still hold what they held."""
    H = 256
    x, w, _ = F8.rms_inputs(H, 2)
    start = (arena.base + PL.GUARD + 255) // 256 * 256
    plane = arena.window(start, C.BAD_STRIDE + H).as_strided((2, H), (C.BAD_STRIDE, 1))
    near = arena.window(start, 4 * H)                       # row 0 and where ldo = 256 would put the rows behind it
    near.fill_(TF.NAN_BYTE)
    plane.fill_(TF.NAN_BYTE)
    scale = torch.full((2,), NAN, device=DEV)
    assert plane.stride(0) == C.BAD_STRIDE and plane.stride(0) % (1 << 32) == H
    with pytest.raises(ValueError, match="ldo"):
        ops.t5_rmsnorm_fp8(x.to(DEV), w.to(DEV), plane, scale, F8.EPS)
    torch.cuda.synchronize()
    assert bool((plane == TF.NAN_BYTE).all()) and bool((near == TF.NAN_BYTE).all()) and bool(scale.isnan().all())


# ---------------------------------------------------------------------------------------------- c. rejection
@pytest.mark.parametrize("form", list(A.FORMS))
@pytest.mark.parametrize("limit", list(ATTN_LIMITS))
def test_attention_limits(arena, form, limit):
    nk, ld_at = ATTN_LIMITS[limit]
    case = _far_case(form, (70, nk, 0, 30))
    inp = A.make_inputs(case)
    res = far_launch(arena, case, inp, ld_at - 8)      # just under: runs and is right
    TA.check_bounds(case, inp, res)
    plain = TA.launch(case, inp)
    for k in ("out", "f32"):
        assert torch.equal(_bytes(plain[0][k]), _bytes(res[0][k])), f"{case.id} {k}: just under the limit != small stride"
    COUNTS["attention far"] += 1
    far_launch(arena, case, inp, ld_at, expect_error="keys larger than 4 GiB")


def test_zz_report(arena):
    """(runs last) the counts and the peak device memory next to the 10 GiB condition."""
    peak = torch.cuda.max_memory_allocated()
    print("\n  runs:", COUNTS, f" peak device memory {peak / 2 ** 30:.3f} GiB (condition: at most 10 GiB)")
    for key in sorted(TA.RATIOS):
        print("  max err / bound", *key, f"{TA.RATIOS[key]:.3f}")
    assert peak <= 10 * 2 ** 30
