"""The grouped GEMM on every launch route x epilogue x precision (tests/gemm_route_cases.py), against an fp64
reference of the same operation on the same inputs with derived bounds, and bit for bit across routes.

Every case asserts, through ca_gemm_plan at the device's CU count, that its launch takes the route it names before it
launches.  The plan of each case is printed (pytest -s) so that a run shows which routes ran."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_route_cases as G  # noqa: E402
import placement  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def shape_or_skip(route, epi, K):
    s = G.find_shape(route, epi, K, n_cu())
    if s is None:
        pytest.skip(f"route {route} cannot be reached with {epi} on a {n_cu()}-CU device")
    return s


def build(x: G.Inputs, alloc=None, keep=None):
    """ops.Gemm of the problem on the device and a function that returns its outputs by name.  `alloc`
    (tests/placement.py) decides where every buffer lies (default: ordinary torch allocations); `keep`, a dict,
    receives the device buffers by operand role."""
    al = alloc or placement.Plain(DEV)
    e = G.EPIS[x.epi]
    M, N, ns = x.M, x.N, x.n_split
    nan = float("nan")
    a, w, bias = al.to(x.a, {"A": None}), al.to(x.w, {"W": None}), al.to(x.bias, {"bias": None})
    bufs = dict(A=a, W=w, bias=bias)
    kw = {}
    if x.fp8:
        kw.update(a_scale=al.to(x.a_scale, {"scales": None}), w_scale=al.to(x.w_scale, {"w_scale": None}))
        bufs.update(scales=kw["a_scale"], w_scale=kw["w_scale"])
    get = {}
    if e["epi"] in (L.EPI_BIAS, L.EPI_GELU_TANH):
        out = al.full((M, N), nan, torch.float32 if e["f32"] else torch.bfloat16, {"out": None})
        get["out"] = lambda: out
    elif e["epi"] == L.EPI_GATE_RESIDUAL:
        out = al.to(x.resid, {"resid": None, "out": None})   # in place: resid is out
        kw.update(resid=out, gate=al.to(x.gate, {"gates": None}), gate2=al.to(x.gate2, {"gate2": None}),
                  gate_rows=x.gate_rows, gate_stride=x.gate_stride, gate_item_rows=x.gate_item_rows,
                  gate2_item_rows=x.gate2_item_rows)
        bufs.update(gates=kw["gate"], gate2=kw["gate2"])
        get["out"] = lambda: out
    elif e["epi"] == L.EPI_SPLIT_GELU:
        out = al.full((M, ns), nan, torch.bfloat16, {"out": None})
        buf2 = al.full((M, N - ns + 24), nan, torch.bfloat16, {"out2": None})
        out2 = buf2[:, 8:8 + N - ns]                     # at a column offset of a wider buffer
        kw.update(out2=out2, n_split=ns)
        bufs.update(out2=buf2, out2_cols=(8, 8 + N - ns))
        get["out"], get["out2"] = (lambda: out), (lambda: out2)
    else:
        hd = ns // 3
        out = al.full((M, min(N, ns)), nan, torch.bfloat16, {"out": None})
        kw.update(n_split=ns, norm_q=al.to(x.norm_q, {"norm_q": None}), norm_k=al.to(x.norm_k, {"norm_k": None}),
                  rope=al.to(x.rope, {"rope": None}), q_out_scale=e["qos"], qk_f16=bool(e.get("f16")))
        bufs.update(norm_q=kw["norm_q"], norm_k=kw["norm_k"], rope=kw["rope"])
        qk = (lambda t: t.view(torch.float16)) if e.get("f16") else (lambda t: t)
        get["q"] = lambda: qk(out[:, :hd])
        if N > hd:
            get["k"] = lambda: qk(out[:, hd:2 * hd])
        if N >= ns:
            get["v"] = lambda: out[:, 2 * hd:3 * hd]
        if N > ns:
            buf2 = al.full((M, N - ns + 24), nan, torch.bfloat16, {"out2": None})
            out2 = buf2[:, 16:16 + N - ns]
            kw["out2"] = out2
            bufs.update(out2=buf2, out2_cols=(16, 16 + N - ns))
            get["out2"] = lambda: out2
        if e["qpre"] is not None:
            if e["qpre"] == 3:
                pre = al.to(x.qraw, {"q_prerope": None})
            else:
                pre = al.full((M, hd), nan, torch.bfloat16 if e["qpre"] == 0 else torch.float32, {"q_prerope": None})
            kw.update(q_prerope=pre, qpre_raw=e["qpre"] == 2, qpre_add=e["qpre"] == 3)
            bufs["q_prerope"] = pre
            get["q_prerope"] = lambda: pre
    bufs["out"] = out
    if keep is not None:
        keep.update(bufs)
    g = ops.Gemm(a, w, bias, out, e["epi"], **kw)
    return g, (lambda: {k: f().clone() for k, f in get.items()})


def launch(problems, tile, route=None, expect=None, alloc=None, keep=None):
    """Plan (asserting the route), launch, return the outputs of every problem.  `alloc` / `keep`: as in build (keep
    receives the buffers of the first problem)."""
    gs = [build(x, alloc, keep if i == 0 else None) for i, x in enumerate(problems)]
    info = ops.gemm_plan([g for g, _ in gs], tile=tile)
    if route is not None:
        assert G.route_matches(info, G.ROUTES[route]), (route, info)
    if expect is not None:
        assert expect(info), info
    ops.gemm([g for g, _ in gs], tile)
    torch.cuda.synchronize()
    return [f() for _, f in gs], info


def check_against_fp64(x: G.Inputs, got: dict, what: str):
    ref = G.reference(x, dev=DEV)
    assert set(ref) == set(got), (set(ref), set(got))
    for name, (r, pre, kind) in ref.items():
        out = got[name].to(DEV)
        n_bad = int((~torch.isfinite(out)).sum().item())
        assert n_bad == 0, f"{what}: {name} ({kind}) {n_bad} elements NaN / inf (never written?)"
        ratio, n_over = G.excess(out, r, pre, kind)
        acc_ratio = ((out.double() - r).abs() / pre).max().item()
        print(f"    {what} {name:9s} {kind}: max err / bound = {ratio:.3f}  max err / accumulation term = {acc_ratio:.3f}")
        assert n_over == 0, f"{what}: {name} ({kind}) {n_over} elements over the bound, max err/bound {ratio:.3g}"


def second_problem(fp8, K, tile):
    """A plain BIAS problem with more tiles than CUs: grouped with a problem it changes the launch's route."""
    bn = G.TILE_W[tile]
    M, N = 512, bn * (n_cu() // 2 + 1)
    return G.make_inputs("bias_bf16", M, N, K, 0, fp8, rem=0, seed=99)


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.id)
def test_route_against_fp64_and_bit_identical_across_routes(case):
    r = G.ROUTES[case.route]
    M, N, ns = shape_or_skip(case.route, case.epi, case.K)
    x = G.make_inputs(case.epi, M, N, case.K, ns, r.fp8, r.rem)
    (got,), info = launch([x], r.tile, route=case.route)
    print(f"\n  {case.id}: M={M} N={N} K={case.K} n_split={ns} plan={info}")
    check_against_fp64(x, got, case.id)

    # the same rows through another route of the same tile width (the k order per accumulator is the contract)
    if r.thin is not None:
        # a thin last row tile (in the walk, or in the thin-row kernel) == the same rows inside a FULL row tile
        Mf = 256 * (M // 256 + 1)
        xf = G.make_inputs(case.epi, Mf, N, case.K, ns, r.fp8, r.rem, layout_M=M)
        (gf,), infof = launch([xf], r.tile, expect=lambda i: i["thin_tiles"] == 0 and i["thin_mf"] == 0)
        for k in got:
            assert torch.equal(got[k], gf[k][:M]), f"{k}: thin part != the same rows in a full tile ({infof})"
    elif r.persistent:
        # persistent walk == one tile per workgroup (a row prefix of the launch)
        bn = G.TILE_W[r.tile]
        Ms = 256 * max(1, n_cu() // (N // bn))
        Ms = min(Ms, 256 * (M // 256))
        xs = G.make_inputs(case.epi, Ms, N, case.K, ns, r.fp8, r.rem, layout_M=M)
        (gs,), infos = launch([xs], r.tile, expect=lambda i: not i["persistent"])
        for k in got:
            assert torch.equal(gs[k], got[k][:Ms]), f"{k}: persistent walk != one tile per workgroup ({infos})"
    else:
        # alone == grouped with a second problem that makes the launch persistent (or, classic kernel, bigger)
        q = second_problem(r.fp8, case.K, r.tile)
        (g2, _), info2 = launch([x, q], r.tile, expect=lambda i: i["grid"] != info["grid"])
        for k in got:
            assert torch.equal(g2[k], got[k]), f"{k}: alone != grouped ({info2})"


THIN_PAIRS = [(r, e) for r, v in G.ROUTES.items() if isinstance(v.thin, tuple)
              for e in ("bias_bf16", "gelu", "split_gelu", "qkv_double_qpre_bf16", "qkv_single_qpre_f32_f16")
              if G.compatible(r, e)]


@pytest.mark.parametrize("route,epi", THIN_PAIRS, ids=lambda v: str(v))
def test_thin_rows_in_kernel_equal_thin_rows_in_walk(route, epi):
    """The thin part in ca_gemm_thin_kernel == the same rows (same N, K, weights) as thin tiles riding in the walk."""
    r = G.ROUTES[route]
    M, N, ns = shape_or_skip(route, epi, 128)
    x = G.make_inputs(epi, M, N, 128, ns, False, r.rem)
    (got,), info = launch([x], r.tile, route=route)
    # another number of full row tiles in front of the same thin rows, such that the thin tiles fit into the walk
    for m in range(0, 16):
        idx = torch.cat((torch.arange(256 * m) % (M - r.rem), torch.arange(M - r.rem, M)))
        xw = G.select_rows(x, idx)
        iw = ops.gemm_plan([build(xw)[0]], tile=r.tile)
        if iw["kernel"] == L.GEMM_KERNEL_PP and iw["thin_tiles"] > 0 and iw["thin_mf"] == 0:   # (persistent or not)
            break
    else:
        pytest.skip(f"no row count puts N={N}'s thin tiles into the walk on {n_cu()} CUs")
    (gw,), iw = launch([xw], r.tile, expect=lambda i: i["thin_tiles"] > 0 and i["thin_mf"] == 0)
    print(f"\n  {route} {epi}: thin kernel {info} vs in-walk (m={m}) {iw}")
    for k in got:
        assert torch.equal(gw[k][-r.rem:], got[k][-r.rem:]), f"{k}: thin kernel != in-walk"
