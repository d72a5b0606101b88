"""The e4m3 value-range contract of include/conceptattn.h on the device: the five producers on every case of
tests/fp8_edge_cases.py (P2 .. P5 and ``rows``), ca_gemm_fp8 on NaN bytes, infinite row scales and results beyond the
bf16 range (G1 .. G4), and a NaN carried through the tiny T5 and the tiny DiT in fp8 mode.

Producers.  Every case is launched twice through ``ops``, on its inputs and on the replaced inputs (the special cells
made zero), into outputs pre-filled with 0xAB / NaN between guard rows and, for the strided layout, guard columns.  P2,
P3, P4 and ``rows`` are bit statements (fp8_edge_cases.violations); P5 is measured against the fp64 y with the derived
bound and printed per producer by the last test of the group.

Consumer.  M = 260 (a full row tile and four ragged rows), K = 128 and 384, every epilogue variant of
gemm_route_cases.EPIS that runs on e4m3 operands.  N = 512, except for the fused QK-norm + RoPE epilogue, whose column
count is a multiple of 768 (plus a 256-column GELU tail in the single-block form): 768 and 1024 there, the smallest that
exist.  The clean launch has byte 0 at every position a special launch sets, so every statement "bit-identical elsewhere"
is against that one launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp8_edge_cases as E  # noqa: E402
import gemm_route_cases as G  # noqa: E402
import model_route_cases as MR  # noqa: E402
import test_gemm_routes_gpu as TG  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
GUARD = 2                      # guard rows on either side (2 * ld bytes keeps the plane 16-byte aligned)
WORST = {}                     # producer -> [scale error / bound, value error / bound], the largest over its cases


# ------------------------------------------------------------------------------------------------------- producers
def _lay(t: torch.Tensor, strided: bool) -> torch.Tensor:
    """A [rows, width] host tensor on the device: as it is, or as the first columns of a wider NaN-filled buffer."""
    if not strided:
        return t.to(DEV)
    buf = torch.full((t.shape[0], t.shape[1] + 8), float("nan"), dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


def run_producer(case: E.Case, inp: dict):
    """(bytes uint8 [rows, width], scales fp32 [rows]) on the CPU, after the guards were checked."""
    R, W = E.N_ROWS, case.width
    ld = W + 16 if case.strided else W
    if case.producer.startswith("ln"):       # (these entries take an e4m3 row stride of a multiple of 16 only)
        ld = -(-W // 16) * 16 + (16 if case.strided else 0)
    plane = torch.full((R + 2 * GUARD, ld), 0xAB, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((R + 2 * GUARD,), float("nan"), device=DEV)
    out, scale = plane[GUARD:GUARD + R, :W], sbuf[GUARD:GUARD + R]
    p = case.producer
    if p == "quantize_rows":
        ops.quantize_rows_fp8(_lay(inp["x"], case.strided), out, scale)
    elif p == "gated_mul_fp8":
        ops.gated_mul_fp8(_lay(inp["g"], case.strided), _lay(inp["u"], case.strided), out, scale)
    elif p == "t5_rmsnorm_fp8":
        ops.t5_rmsnorm_fp8(_lay(inp["x"], case.strided), inp["w"].to(DEV), out, scale, E.F8.EPS)
    else:
        segs = [(end, sh.to(DEV), sc.to(DEV)) for end, sh, sc in zip(E.LN_SEGS, inp["shift"], inp["scale"])]
        ops.ln_modulate(_lay(inp["x"], case.strided), out, segs, eps=E.R.EPS, out_scale=scale)
    torch.cuda.synchronize()
    plane, sbuf = plane.cpu(), sbuf.cpu()
    assert (plane[:GUARD] == 0xAB).all() and (plane[GUARD + R:] == 0xAB).all() and (plane[:, W:] == 0xAB).all(), case.id
    assert torch.isnan(sbuf[:GUARD]).all() and torch.isnan(sbuf[GUARD + R:]).all(), case.id
    return plane[GUARD:GUARD + R, :W].contiguous(), sbuf[GUARD:GUARD + R].contiguous()


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c.id)
def test_producer_meets_the_contract(case):
    inp = E.make_inputs(case)
    got = run_producer(case, inp)
    twin = run_producer(case, E.replaced(case, inp))
    y = E.y32(case, inp)
    bad = E.violations(y, got, twin)
    rs, rv = E.p5_ratios(case, inp, *got)
    w = WORST.setdefault(case.producer, [0.0, 0.0])
    w[0], w[1] = max(w[0], rs), max(w[1], rv)
    print(f"\n  {case.id}: scale error / bound {rs:.3f}  value error / bound {rv:.3f}  NaN bytes "
          f"{int(E.is_nan_byte(got[0]).sum())} (0x7F {int((got[0] == 0x7F).sum())}, 0xFF {int((got[0] == 0xFF).sum())})")
    assert bad == set(), (case.id, sorted(bad))
    assert rs <= 1 and rv <= 1, (case.id, rs, rv)


def test_producer_error_over_bound_figures():
    """Prints the largest P5 figures per producer (recorded in the header of tests/fp8_edge_cases.py)."""
    assert set(WORST) == set(E.PRODUCERS), "run with the parametrised test above"
    for p in E.PRODUCERS:
        print(f"\n  {p}: largest scale error / bound {WORST[p][0]:.3f}, value error / bound {WORST[p][1]:.3f}")
        assert WORST[p][0] <= 1 and WORST[p][1] <= 1


@pytest.mark.parametrize("producer", ("t5_rmsnorm_fp8", "gated_mul_fp8"))
def test_grid_wrap_special_rows_stay_in_their_rows(producer):
    """65541 x 264: workgroups 2 and 3 quantise a NaN row and an inf row, then walk rows 65538 and 65539 through the same
    `red` array.  Every row but 2 and 3 has the bits of the clean run; rows 2 and 3 meet P2 .. P4."""
    a, special, b = E.wrap_inputs(producer)
    rows, W = a.shape

    def run(first):
        out = torch.full((rows, W), 0xAB, dtype=torch.uint8, device=DEV)
        scale = torch.full((rows,), float("nan"), device=DEV)
        if producer == "t5_rmsnorm_fp8":
            ops.t5_rmsnorm_fp8(first.to(DEV), b.to(DEV), out, scale, E.F8.EPS)
        else:
            ops.gated_mul_fp8(first.to(DEV), b.to(DEV), out, scale)
        return out, scale
    (q0, s0), (q1, s1) = run(a), run(special)
    other = torch.ones(rows, dtype=torch.bool, device=DEV)
    other[list(E.WRAP_SPECIAL_ROWS)] = False
    assert torch.equal(q0[other], q1[other]) and torch.equal(s0[other].view(torch.int32), s1[other].view(torch.int32))
    for r in E.WRAP_SAME_WORKGROUP:
        assert torch.equal(q0[r], q1[r]) and torch.equal(s0[r:r + 1].view(torch.int32), s1[r:r + 1].view(torch.int32)), r
    head = slice(0, 8)
    if producer == "t5_rmsnorm_fp8":
        y = E.F8.rmsnorm_y32(special[head], b)
    else:
        y = special[head].float() * b[head].float()
    bad = E.violations(y, (q1[head].cpu(), s1[head].cpu()), (q0[head].cpu(), s0[head].cpu()))
    assert bad <= {"P3"} and torch.isnan(y[2]).any() and not torch.isfinite(y[3]).all(), bad
    # (P3's twin here is the clean run, whose special cells are not zero: the clause is stated directly instead)
    q, s = q1[head].cpu(), s1[head].cpu()
    assert E.is_nan_byte(q)[torch.isnan(y)].all()
    if producer == "gated_mul_fp8":        # row 2: one NaN, the scale of the other elements; row 3: an infinite scale
        rest = torch.where(torch.isnan(y[2]), torch.zeros_like(y[2]), y[2])
        q2, s2 = E.pack_rows(rest[None])
        assert torch.equal(s[2:3].view(torch.int32), s2.view(torch.int32)) and (q[2] == q2[0])[~torch.isnan(y[2])].all()
        assert s[3] == E.INF
    else:                                  # a NaN or an inf in x: no finite non-zero element is left, scale 1
        assert s[2] == 1 and s[3] == 1 and E.is_nan_byte(q[2]).all()


# ------------------------------------------------------------------------------------------------------- consumer
GEMM_M = 260
G1_ROWS, G2_COLS, G3_ROWS = (0, 255, 256, 259), (0, 255, 511), (0, 259)
NAN_BYTES = (0x7F, 0xFF)
FP8_EPIS = [e for e in G.EPIS if G.compatible("fp8", e)]


def gemm_shape(epi: str):
    e = G.EPIS[epi]
    N = 512
    if e["epi"] == L.EPI_QKV_NORM_ROPE:
        N = 768 if e["form"] == "double" else 1024
    return N, G.n_split_of(epi, N, 256)


def zero_row_of_w(N: int) -> int:
    """The W row that is all zero (accumulator 0 in every output row): in the v third / the GELU tail / the second half."""
    return N - 2


def coupled(x: G.Inputs, n: int) -> dict:
    """output name -> the columns of that output that W row n reaches."""
    e = G.EPIS[x.epi]
    if e["epi"] == L.EPI_SPLIT_GELU:
        return {"out": [n]} if n < x.n_split else {"out2": [n - x.n_split]}
    if e["epi"] != L.EPI_QKV_NORM_ROPE:
        return {"out": [n]}
    hd = x.n_split // 3
    head = lambda c: list(range(c // 128 * 128, c // 128 * 128 + 128))  # noqa: E731  (the norm couples a head's columns)
    if n < hd:
        return {"q": head(n), "q_prerope": [n] if e["qpre"] == 2 else head(n)}     # (raw: stored before the norm)
    if n < 2 * hd:
        return {"k": head(n - hd)}
    if n < x.n_split:
        return {"v": [n - 2 * hd]}
    return {"out2": [n - x.n_split]}


def _launch(x: G.Inputs) -> dict:
    (got,), _ = TG.launch([x], L.TILE_PP_256x256)
    return {k: v.cpu() for k, v in got.items()}


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("K", (128, 384))
@pytest.mark.parametrize("epi", FP8_EPIS)
def test_gemm_fp8_nan_bytes_and_infinite_scales(epi, K):
    from dataclasses import replace
    N, ns = gemm_shape(epi)
    M = GEMM_M
    base = G.make_inputs(epi, M, N, K, ns, True, rem=M % 256, seed=5)
    ks = sorted({0, 127, K - 1})
    for m in G1_ROWS:
        base.a[m, ks] = 0
    for n in G2_COLS:
        base.w[n, 3] = 0
    n0 = zero_row_of_w(N)
    base.w[n0] = 0
    clean = _launch(base)
    assert all(torch.isfinite(v.float()).all() for v in clean.values()), epi
    rows = torch.arange(M)
    # G1: a NaN byte in A
    for i, (m, k) in enumerate((m, k) for m in G1_ROWS for k in ks):
        a = base.a.clone()
        a[m, k] = NAN_BYTES[i % 2]
        got = _launch(replace(base, a=a))
        assert got.keys() == clean.keys()
        for name, t in got.items():
            assert torch.isnan(t[m].float()).all(), (epi, "G1", m, k, name)
            assert _same(t[rows != m], clean[name][rows != m]), (epi, "G1", m, k, name)
    # G2: a NaN byte in W
    for i, n in enumerate(G2_COLS):
        w = base.w.clone()
        w[n, 3] = NAN_BYTES[i % 2]
        got = _launch(replace(base, w=w))
        hit = coupled(base, n)
        assert set(hit) <= set(got)
        for name, t in got.items():
            cols = torch.zeros(t.shape[1], dtype=torch.bool)
            cols[hit.get(name, [])] = True
            assert torch.isnan(t[:, cols].float()).all(), (epi, "G2", n, name)
            assert _same(t[:, ~cols], clean[name][:, ~cols]), (epi, "G2", n, name)
    # G3: an infinite row scale
    for m in G3_ROWS:
        s = base.a_scale.clone()
        s[m] = E.INF
        got = _launch(replace(base, a_scale=s))
        zero_acc = coupled(base, n0)
        for name, t in got.items():
            assert not torch.isfinite(t[m].float()).any(), (epi, "G3", m, name)
            assert _same(t[rows != m], clean[name][rows != m]), (epi, "G3", m, name)
            if name in zero_acc:
                assert torch.isnan(t[m, zero_acc[name]].float()).all(), (epi, "G3", m, name, "0 * inf")


def test_gemm_fp8_result_beyond_bf16_is_infinite():
    """G4.  Integer operands under power-of-two scales: row r's accumulator is +-(1016 + r % 8), the scales 2^59 each, so
    the fp32 result +-(1016 + r % 8) 2^118 is finite (below 2^128) and straddles the point (1020 2^118) from which bf16's
    round-to-nearest-even gives infinity; the largest finite bf16 is 1016 2^118.  The store is torch's fp32 -> bf16 cast."""
    M = N = 256
    K = 128
    a = torch.full((M, K), 8.0)
    a[:, K - 1] = (torch.arange(M) % 8).float()
    a[1::2] *= -1
    w = torch.ones(N, K)
    w[1::2] *= -1
    acc = a @ w.t()
    assert acc.abs().min() == 1016 and acc.abs().max() == 1023
    want = (acc * 2.0 ** 118).to(torch.bfloat16)
    assert torch.isinf(want).any() and torch.isfinite(want).any() and (want < 0).any() and not torch.isnan(want).any()
    qa = a.to(torch.float8_e4m3fn).view(torch.uint8).to(DEV)
    qw = w.to(torch.float8_e4m3fn).view(torch.uint8).to(DEV)
    out = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
    ops.gemm([ops.Gemm(qa, qw, None, out, a_scale=torch.full((M,), 2.0 ** 59, device=DEV),
                       w_scale=torch.full((N,), 2.0 ** 59, device=DEV))])
    assert _same(out.cpu(), want)
    # a result beyond fp32 itself (2^60 * 2^60): infinite as well, with the accumulator's sign
    ops.gemm([ops.Gemm(qa, qw, None, out, a_scale=torch.full((M,), 2.0 ** 60, device=DEV),
                       w_scale=torch.full((N,), 2.0 ** 60, device=DEV))])
    assert _same(out.cpu(), (acc * E.INF).to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("precision", ("bf16", "fp8"))
def test_tiny_t5_nan_embedding_row_stays_in_its_sequence(precision):
    """A NaN in the embedding row of a token that only sequence 1 uses: sequence 1 leaves all NaN, in fp8 mode as in bf16
    (where the e4m3 producers turned it into a finite -448, the fp8 output was finite); sequences 0 and 2 have the bits of
    the clean model."""
    from conceptattention_amd.params import tiny_t5_params
    from conceptattention_amd.t5 import load_t5, synthetic_t5_state_dict
    p = tiny_t5_params()
    sd = synthetic_t5_state_dict(p, 0)
    token = 7
    ids = torch.randint(8, p.vocab_size, (3, 64), generator=torch.Generator().manual_seed(64))
    ids[1, 40] = token
    clean = load_t5(p, DEV, weights=sd, precision=precision).encode_ids(ids)
    bad = dict(sd)
    bad["shared.weight"] = sd["shared.weight"].clone()
    bad["shared.weight"][token, 3] = float("nan")
    got = load_t5(p, DEV, weights=bad, precision=precision).encode_ids(ids)
    assert torch.isfinite(clean.float()).all()
    assert torch.isnan(got[1].float()).all(), f"{precision}: {int(torch.isnan(got[1].float()).sum())} of {got[1].numel()} NaN"
    assert _same(got[0].cpu(), clean[0].cpu()) and _same(got[2].cpu(), clean[2].cpu())


def _dit(case, weights=None):
    import test_model_routes_gpu as TM
    from conceptattention_amd.flux_dit import HipFluxDiT
    return TM.configure(HipFluxDiT(MR.params(case), TM.DEV, weights=weights or TM.weights(case)), case), TM


@pytest.mark.parametrize("name", ("default", "fp8"))
def test_tiny_dit_nan_latent_element_gives_a_nan_latent(name):
    case = MR.BY_NAME[name]
    m, TM = _dit(case)
    item = dict(TM.dev_item(case, 0))
    assert torch.isfinite(TM.forward(m, case, items=[item]).pred.float()).all()
    item["img"] = item["img"].clone()
    item["img"][0, 5, 3] = float("nan")
    pred = TM.forward(m, case, items=[item]).pred
    assert torch.isnan(pred.float()).all(), f"{name}: {int(torch.isnan(pred.float()).sum())} of {pred.numel()} NaN"


@pytest.mark.parametrize("name", ("default", "fp8"))
def test_tiny_dit_nan_weight_gives_a_nan_latent(name):
    """set_precision("fp8") quantises the weights with ca_quantize_rows_fp8: the NaN has to survive it."""
    from conceptattention_amd.flux_dit import FluxWeights
    import test_model_routes_gpu as TM
    case = MR.BY_NAME[name]
    sd = dict(MR.state_dict(case))
    key = "double_blocks.0.img_mlp.2.weight"
    sd[key] = sd[key].clone()
    sd[key][5, 7] = float("nan")
    w = FluxWeights(MR.params(case), TM.DEV)
    w.load_state_dict(sd)
    m, _ = _dit(case, w)
    pred = TM.forward(m, case, items=[dict(TM.dev_item(case, 0))]).pred
    assert torch.isnan(pred.float()).all(), f"{name}: {int(torch.isnan(pred.float()).sum())} of {pred.numel()} NaN"
