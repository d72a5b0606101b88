"""Every launch form of the row kernels (tests/rowop_cases.py) through conceptattention_amd.ops and the C ABI, against
an fp64 reference of the same operation on the same inputs with derived bounds, and bit for bit across the routes
whose kernels claim it.

Outputs and the padding columns between width and row stride are filled with NaN (0xFF for fp8) before the launch: an
element the kernel never writes fails its bound, and the padding, like the columns of in-place operands the op does
not own, must come back byte for byte.  max err / bound is printed per output (pytest -s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import placement  # noqa: E402
import rowop_cases as R  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
NAN = float("nan")


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def assert_same_bytes(after, before, what):
    assert torch.equal(_bytes(after), _bytes(before)), f"{what}: bytes changed"


def _fp8(t):
    return t.view(torch.float8_e4m3fn).double()


def _nan(shape, dtype):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def _al(alloc):
    """The allocator of a run helper (tests/placement.py): where every buffer the kernel sees lies; by default ordinary
    torch allocations.  Every buffer is named by its operand role."""
    return alloc or placement.Plain(DEV)


def _seg_vectors(al, vecs, role):
    """Per-segment vectors: the middle segment's carries the role (one buffer per role can straddle)."""
    return [al.to(v, {role: None} if i == len(vecs) // 2 else {f"{role}[{i}]": None}) for i, v in enumerate(vecs)]


def run_ln(c, inp, alloc=None):
    al = _al(alloc)
    s = c.shape
    M, H = s["M"], s["H"]
    x = al.to(inp["x"], {"x": None})
    x0 = x.clone()
    segs = list(zip(s["segs"], _seg_vectors(al, inp["shift"], "shift"), _seg_vectors(al, inp["scale"], "scale")))
    pads = []
    if s["out"] == "fp8":
        buf = al.full((M, s["ldo"]), 0xFF, torch.uint8, {"out": None})
        scale = al.full((M,), NAN, torch.float32, {"out_scale": None})
        pads.append((buf, buf.clone(), H))
        ops.ln_modulate(x[:, :H], buf[:, :H], segs, out_scale=scale)
        got = {"scale": scale, "q": _fp8(buf[:, :H])}
    else:
        buf = al.full((M, s["ldo"]), NAN, torch.bfloat16, {"out": None})
        pads.append((buf, buf.clone(), H))
        if s["out"] == "split":
            lo = al.full((M, s["ldlo"]), NAN, torch.bfloat16, {"out_lo": None})
            pads.append((lo, lo.clone(), H))
            ops.ln_modulate(x[:, :H], buf[:, :H], segs, out_lo=lo[:, :H])
            got = {"out": buf[:, :H], "hi+lo": buf[:, :H].double() + lo[:, :H].double()}
        else:
            ops.ln_modulate(x[:, :H], buf[:, :H], segs)
            got = {"out": buf[:, :H]}
    torch.cuda.synchronize()
    assert_same_bytes(x, x0, "x")
    return got, pads


def run_quant(c, inp, alloc=None):
    al = _al(alloc)
    s = c.shape
    M, K = s["M"], s["K"]
    x = al.to(inp["x"], {"x": None})
    x0 = x.clone()
    buf = al.full((M, s["ldo"]), 0xFF, torch.uint8, {"out": None})
    scale = al.full((M,), NAN, torch.float32, {"out_scale": None})
    pads = [(buf, buf.clone(), K)]
    ops.quantize_rows_fp8(x[:, :K], out=buf[:, :K], out_scale=scale)
    torch.cuda.synchronize()
    assert_same_bytes(x, x0, "x")
    zero = (inp["x"][:, :K].float() == 0).all(1)
    assert bool((buf[zero.to(DEV), :K] == 0).all()), "zero rows: bytes must be 0"
    assert bool((scale[zero.to(DEV)] == 1).all()), "zero rows: scale must be 1"
    return {"scale": scale, "q": _fp8(buf[:, :K])}, pads


def run_qk(c, inp, alloc=None):
    al = _al(alloc)
    s = c.shape
    M, nh = s["M"], s["heads"]
    W = nh * 128
    qkv = al.to(inp["qkv"], {"qkv": None})
    q0 = qkv.clone()
    segs = list(zip(s["segs"], _seg_vectors(al, inp["q_scale"], "q_scale"), _seg_vectors(al, inp["k_scale"], "k_scale")))
    pads, pre = [(qkv, q0, 3 * W)], None
    if s["pre"]:
        pbuf = al.full((M, s["ldp"]), NAN, torch.bfloat16, {"q_prerope": None})
        pads.append((pbuf, pbuf.clone(), W))
        pre = pbuf[:, :W]
    ops.qknorm_rope(qkv[:, :3 * W], nh, segs, al.to(inp["rope"], {"rope": None}), q_prerope=pre)
    torch.cuda.synchronize()
    got = {"q": qkv[:, :W], "k": qkv[:, W:2 * W], "v": qkv[:, 2 * W:3 * W]}
    if pre is not None:
        got["q_prerope"] = pre
    return got, pads


def run_qpre(c, inp, alloc=None):
    al = _al(alloc)
    s = c.shape
    M, W = s["M"], s["heads"] * 128
    x = al.to(inp["x"], {"x": None})
    pads = [(x, x.clone(), W)]
    d = None
    if s["d"]:
        dd = al.to(inp["d"], {"d": None})
        d0 = dd.clone()
        d = dd[:, :W]
    sc = al.to(inp["scale"], {"scale": None})
    got = {}
    if s["rope"]:
        qb = al.full((M, s["ldq"]), NAN, torch.bfloat16, {"q_out": None})
        pads.append((qb, qb.clone(), W))
        ops.qpre_finish(x[:, :W], d, sc, s["heads"], rope=al.to(inp["rope"], {"rope": None}), q_out=qb[:, :W],
                        q_out_scale=s["qos"], q_f16=s["f16"])
        got["q"] = qb[:, :W].view(torch.float16) if s["f16"] else qb[:, :W]
    else:
        ops.qpre_finish(x[:, :W], d, sc, s["heads"])
    torch.cuda.synchronize()
    if d is not None:
        assert_same_bytes(dd, d0, "d")
    got["x"] = x[:, :W]
    return got, pads


def run_gemv(c, inp, alloc=None):
    al = _al(alloc)
    s = c.shape
    nv, K, N = s["nv"], s["K"], s["N"]
    if s["acc"]:      # (uploaded with the buffer: nothing between the allocations and the launch waits for the device)
        out0 = torch.full((nv, s["ldo"]), NAN, dtype=torch.float32)
        out0[:, :N] = inp["out0"]
        out = al.to(out0, {"out": None})
    else:
        out = al.full((nv, s["ldo"]), NAN, torch.float32, {"out": None})
    pads = [(out, out.clone(), N)]
    x = al.to(inp["x"], {"x": None})
    bias = al.to(inp["bias"], {"bias": None}) if s["bias"] else None
    ops.gemv(x[:, :K], al.to(inp["w"], {"w": None}), bias, out[:, :N], silu_input=s["silu"], accumulate=s["acc"])
    torch.cuda.synchronize()
    return {"out": out[:, :N]}, pads


def run_split(c, inp, alloc=None):
    al = _al(alloc)
    s = c.shape
    rows, K = s["rows"], s["K"]
    x = al.to(inp["x"], {"x": None})
    x0 = x.clone()
    hi = al.full((rows, s["ldo"]), NAN, torch.bfloat16, {"hi": None})
    lo = al.full((rows, s["ldo"]), NAN, torch.bfloat16, {"lo": None})
    pads = [(hi, hi.clone(), K), (lo, lo.clone(), K)]
    (ops.silu_split if s["silu"] else ops.split_planes)(x[:, :K], hi[:, :K], lo[:, :K])
    torch.cuda.synchronize()
    assert_same_bytes(x, x0, "x")
    if s["silu"]:
        return {"hi": hi[:, :K], "hi+lo": hi[:, :K].double() + lo[:, :K].double()}, pads
    return {"hi": hi[:, :K], "lo": lo[:, :K]}, pads


def run_combine(c, inp, alloc=None):
    """ca_modulation_combine_f32 on its own (ops calls it only inside modulation_gemm), through the C ABI."""
    al = _al(alloc)
    s = c.shape
    nv, N = s["nv"], s["N"]
    pair = al.to(inp["pair"], {"pair": None})
    bias = al.to(inp["bias"], {"bias": None}) if s["bias"] else None
    out = al.full((nv, s["ldo"]), NAN, torch.float32, {"out": None})
    pads = [(out, out.clone(), N)]
    L.check(L.load().ca_modulation_combine_f32(pair.data_ptr(), pair.stride(0), None if bias is None else bias.data_ptr(),
                                               out.data_ptr(), out.stride(0), nv, N,
                                               torch.cuda.current_stream().cuda_stream), "ca_modulation_combine_f32")
    torch.cuda.synchronize()
    return {"out": out[:, :N]}, pads


def run_logits(c, inp, alloc=None):
    al = _al(alloc)
    s = c.shape
    img, con = al.to(inp["img"], {"img": None}), al.to(inp["con"], {"con": None})
    lg = al.full((s["C"], s["L"]), NAN, torch.float32, {"logits": None})
    ops.heatmap_logits(img[:, :s["dim"]], con[:, :s["dim"]], lg)
    torch.cuda.synchronize()
    return {"logits": lg}, []


def run_norm(c, inp, alloc=None):
    al = _al(alloc)
    s = c.shape
    lg = al.to(inp["logits"], {"logits": None})
    acc = al.to(inp["acc0"], {"acc": None})
    norm = L.NORMS[s["norm"]]
    if c.entry == "ca_heatmap_norm_accumulate":      # (ops sends softmax to ca_heatmap_softmax_accumulate directly)
        L.check(L.load().ca_heatmap_norm_accumulate(lg.data_ptr(), s["C"], s["L"], norm, s["w"], acc.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream),
                "ca_heatmap_norm_accumulate")
    else:
        ops.heatmap_softmax_accumulate(lg, acc, s["w"], norm=norm)
    torch.cuda.synchronize()
    return {"acc": acc}, []


def run_fused(c, inp, alloc=None):
    al = _al(alloc)
    s = c.shape
    acc = al.to(inp["acc0"], {"acc": None})
    lg = al.full((s["C"], s["L"]), NAN, torch.float32, {"logits": None})
    if s["form"] == "part":
        h = ops.Heatmap(None, None, acc=acc, weight=R.FUSED_W, logits=lg, part=al.to(inp["part"], {"part": None}))
    else:
        h = ops.Heatmap(al.to(inp["img"], {"img": None}), al.to(inp["con"], {"con": None}), acc=acc, weight=R.FUSED_W,
                        logits=lg)
    ops.heatmap_fused([h], norm=L.NORMS[s["norm"]])
    torch.cuda.synchronize()
    return {"logits": lg, "acc": acc}, []


def run_axpy(c, inp, alloc=None):
    al = _al(alloc)
    s = c.shape
    x, y = al.to(inp["x"], {"x": None}), al.to(inp["y"], {"y": None})
    (ops.axpy if x.dtype == torch.bfloat16 else ops.axpy_f32)(x, y, s["a"])
    torch.cuda.synchronize()
    return {"x": x}, []


def run_temb(c, inp, alloc=None):
    al = _al(alloc)
    s = c.shape
    out = al.full((s["nt"], s["dim"]), NAN, torch.float32, {"out": None})
    ops.timestep_embedding(al.to(inp["t"], {"t": None}), out, time_factor=s["tf"])
    torch.cuda.synchronize()
    return {"out": out}, []


RUN = {"ln": run_ln, "quant": run_quant, "qk": run_qk, "qpre": run_qpre, "gemv": run_gemv, "split": run_split,
       "combine": run_combine, "logits": run_logits, "norm": run_norm, "fused": run_fused, "axpy": run_axpy,
       "temb": run_temb}


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_rowop_against_fp64(case):
    inp = R.make_inputs(case)
    got, pads = RUN[case.op](case, inp)
    scale = got.get("scale") if case.op in ("ln", "quant") else None
    ref = R.reference(case, inp, dev=DEV, scale_got=scale)
    assert set(ref) == set(got), (set(ref), set(got))
    print(f"\n  {case.id}: {case.entry} -> {case.kernel}")
    for name, (r, pre, kind) in ref.items():
        out = got[name]
        ratio, n_over = R.excess(out, r, pre, kind)
        print(f"    {name:9s} {kind:8s} max err / bound = {ratio:.3f}")
        assert n_over == 0, f"{case.id}: {name} ({kind}) {n_over} of {out.numel()} elements over the bound " \
                            f"(NaN = never written), max err / bound {ratio:.3g}"
    for buf, before, w in pads:
        assert_same_bytes(buf[:, w:], before[:, w:], f"{case.id}: padding beyond column {w}")


def _representable_rows(M, H, seed):
    g = torch.Generator().manual_seed(seed)
    xb = (torch.randn(M, H, generator=g) * 2 + 0.3).bfloat16()
    xb[3::11] = (1000 + torch.randn(len(range(3, M, 11)), H, generator=g)).bfloat16()
    xb[5::13] = 0.75
    return xb.to(DEV)


def test_ln_rows_kernel_bit_identical_to_generic_kernel_on_15_segments():
    """ca_ln_modulate_rows_kernel<6, *> (fp32 rows, H = 3072) performs ca_ln_modulate_kernel's arithmetic operation for
    operation: on bf16-representable rows, 15 segments (empty ones, boundaries inside one wave's 8-row walk), its
    output equals the bf16-input generic kernel's bit for bit, with and without the low plane; the fp8 kernels of
    both input types agree as well.  At H = 4096 the generic kernel's low-plane form stores the plain form's bytes."""
    M, H = 777, 3072
    c = R.BY_ID["ln_rows6_split_seg15"]
    inp = R.make_inputs(c)
    segs = [(re, sh.to(DEV), sc.to(DEV)) for re, sh, sc in zip(R.SEG15, inp["shift"], inp["scale"])]
    xb = _representable_rows(M, H, 7)
    o16, o32, ohi = (_nan((M, H), torch.bfloat16) for _ in range(3))
    lo = _nan((M, H), torch.bfloat16)
    ops.ln_modulate(xb, o16, segs)                          # ca_ln_modulate_kernel<false, bf16>
    ops.ln_modulate(xb.float(), o32, segs)                  # ca_ln_modulate_rows_kernel<6, false>
    ops.ln_modulate(xb.float(), ohi, segs, out_lo=lo)       # ca_ln_modulate_rows_kernel<6, true>
    q16, q32 = (torch.full((M, H), 0xFF, device=DEV, dtype=torch.uint8) for _ in range(2))
    s16, s32 = _nan((M,), torch.float32), _nan((M,), torch.float32)
    ops.ln_modulate(xb, q16, segs, out_scale=s16)           # ca_ln_modulate_kernel<true, bf16>
    ops.ln_modulate(xb.float(), q32, segs, out_scale=s32)   # ca_ln_modulate_kernel<true, float>
    torch.cuda.synchronize()
    assert torch.equal(o16, o32), "rows kernel != generic kernel"
    assert torch.equal(ohi, o32), "rows kernel: the low-plane form changes the bf16 plane"
    assert torch.equal(q16, q32) and torch.equal(s16, s32), "fp8: fp32-input kernel != bf16-input kernel"
    # the low plane against fp64: hi + lo within the bound of the unrounded y
    xin = dict(inp, x=xb.float().cpu())
    ref, pre, kind = R.ln_reference(c, xin, dev=DEV)["hi+lo"]
    ratio, n_over = R.excess(ohi.double() + lo.double(), ref, pre, kind)
    print(f"\n  rows kernel low plane, representable rows: max err / bound = {ratio:.3f}")
    assert n_over == 0
    # generic low-plane kernel (H = 4096): its bf16 plane equals the plain generic kernel's
    c2 = R.BY_ID["ln_split_H4096_seg16"]
    inp2 = R.make_inputs(c2)
    segs2 = [(re, sh.to(DEV), sc.to(DEV)) for re, sh, sc in zip(c2.shape["segs"], inp2["shift"], inp2["scale"])]
    x2 = inp2["x"].to(DEV)
    a, b, lo2 = (_nan((M, 4096), torch.bfloat16) for _ in range(3))
    ops.ln_modulate(x2, a, segs2)                           # ca_ln_modulate_kernel<false, float>
    ops.ln_modulate(x2, b, segs2, out_lo=lo2)               # ca_ln_modulate_kernel<false, float, true>
    torch.cuda.synchronize()
    assert torch.equal(a, b), "generic kernel: the low-plane form changes the bf16 plane"
