"""Every launch form of the autoencoder kernels (tests/vae_cases.py) through the C entry points of ca_vae.hip -- the
strided and explicit-n_chunks forms cannot go through conceptattention_amd.ops -- against an fp64 reference of the
same operation on the same inputs with derived bounds, and bit for bit where two routes must agree.

Every output buffer holds NaN in the range the kernel must write and a finite canary in the columns between width and
row stride: an element never written fails its bound, and the canary columns are an output of kind "exact".  Inputs
carry junk in their padding columns and must come back byte for byte.  max err / bound is printed per output
(pytest -s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import placement  # noqa: E402
import vae_cases as V  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
RATIOS = {}        # (op, output kind) -> the largest max err / bound seen


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def assert_same_bytes(after, before, what):
    assert torch.equal(_bytes(after), _bytes(before)), f"{what}: bytes changed"


def _al(alloc):
    return alloc or placement.Plain(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _call(entry, *args):
    L.check(getattr(L.load(), entry)(*args, _stream()), entry)
    torch.cuda.synchronize()


def run_conv(c, inp, alloc=None, out_f32=None):
    """out_f32 True: the same case with an fp32 output buffer (NaN and canaries carried over)."""
    al, s = _al(alloc), c.shape
    k, stride, up, Ho, Wo, M = V.conv_geometry(s)
    cout = s["cout"]
    x, w = al.to(inp["x"], {"x": None}), al.to(inp["w"], {"w": None})
    bias = al.to(inp["bias"], {"bias": None}) if s["bias"] else None
    f32 = s["out"] == "f32" or bool(out_f32)
    out = al.to(inp["out0"].float() if f32 else inp["out0"], {"out": None})
    resid = out if s["resid"] == "in place" else al.to(inp["resid"], {"resid": None}) if s["resid"] == "separate" else None
    keep = [(t, t.clone(), n) for t, n in ((x, "x"), (w, "w"), (bias, "bias")) if t is not None]
    if s["resid"] == "separate":
        keep.append((resid, resid.clone(), "resid"))
    assert x.shape[0] == s["B"] * s["H"] * s["W"] and out.shape[0] == M
    _call("ca_conv3x3_nhwc", x.data_ptr(), w.data_ptr(), _ptr(bias), _ptr(resid), out.data_ptr(), s["B"], s["H"], s["W"],
          V.ceil_to(s["cin"], 32), cout, x.stride(0), resid.stride(0) if resid is not None else 0, out.stride(0), k, stride,
          int(up), int(f32))
    for t, t0, n in keep:
        assert_same_bytes(t, t0, f"{c.id}: {n}")
    return {"out": out[:, :cout], **({"pad": out[:, cout:]} if out.shape[1] > cout else {})}


def run_gn(c, inp, alloc=None):
    al, s = _al(alloc), c.shape
    B, HW, C = s["B"], s["HW"], s["C"]
    n_chunks = s["n_chunks"] or V.groupnorm_chunks(HW)
    x = al.to(inp["x"], {"x": None})
    gamma, beta = al.to(inp["gamma"], {"gamma": None}), al.to(inp["beta"], {"beta": None})
    y = al.to(inp["y0"], {"y": None})
    part = al.full((B * n_chunks * 96,), V.NAN, torch.float32, {"part": None})
    keep = [(t, t.clone(), n) for t, n in ((x, "x"), (gamma, "gamma"), (beta, "beta"))]
    _call("ca_groupnorm_nhwc", x.data_ptr(), int(s["xdt"] == "f32"), x.stride(0), gamma.data_ptr(), beta.data_ptr(),
          y.data_ptr(), y.stride(0), B, HW, C, V.GN_EPS, int(s["swish"]), part.data_ptr(), n_chunks)
    for t, t0, n in keep:
        assert_same_bytes(t, t0, f"{c.id}: {n}")
    cnt = part.reshape(B, n_chunks, 32, 3)[..., 0]
    assert bool((cnt.sum(1) == HW * (C // 32)).all()), f"{c.id}: the chunks' counts do not add up to a group's elements"
    return {"y": y[:, :C], **({"pad": y[:, C:]} if y.shape[1] > C else {})}


def run_softmax(c, inp, alloc=None):
    al, s = _al(alloc), c.shape
    n = s["n"]
    sc = al.to(inp["s"], {"s": None})
    sc0 = sc.clone()
    p = al.to(inp["p0"], {"p": None})
    _call("ca_softmax_rows_f32", sc.data_ptr(), sc.stride(0), p.data_ptr(), p.stride(0), s["rows"], n, s["scale"])
    assert_same_bytes(sc, sc0, f"{c.id}: s")
    return {"p": p[:, :n], **({"pad": p[:, n:]} if p.shape[1] > n else {})}


def run_affine(c, inp, alloc=None):
    al, s = _al(alloc), c.shape
    C = s["C"]
    dev = {}
    if s["lv"] and s["view"]:
        dev["moments"] = al.to(inp["moments"], {"x": None, "logvar": None})
    else:
        dev["x"] = al.to(inp["x"], {"x": None})
        if s["lv"]:
            dev["logvar"] = al.to(inp["logvar"], {"logvar": None})
    if s["lv"]:
        dev["noise"] = al.to(inp["noise"], {"noise": None})
    keep = [(t, t.clone(), n) for n, t in dev.items()] if not s["big"] else []
    x, lv, nz = V.affine_operands(c, dev)
    out = al.to(inp["out0"], {"out": None})
    _call("ca_affine_rows_f32", x.data_ptr(), x.stride(0), _ptr(lv), lv.stride(0) if s["lv"] else 0, _ptr(nz),
          nz.stride(0) if s["lv"] else 0, out.data_ptr(), out.stride(0), int(s["out"] == "f32"), s["rows"], C,
          s["a"], s["b"])
    for t, t0, n in keep:
        assert_same_bytes(t, t0, f"{c.id}: {n}")
    return {"out": out[:, :C], **({"pad": out[:, C:]} if out.shape[1] > C else {})}


RUN = {"conv": run_conv, "gn": run_gn, "softmax": run_softmax, "affine": run_affine}


def check(case, inp, got, verbose=True):
    """Every output of the case within its bound (the canary columns: bit for bit)."""
    ref = V.reference(case, inp, dev=DEV)
    assert set(ref) == set(got), (set(ref), set(got))
    for name, (r, pre, kind) in ref.items():
        ratio, n_over = V.excess(got[name], r, pre, kind)
        if verbose:
            print(f"    {name:4s} {kind:6s} max err / bound = {ratio:.3f}")
        if name != "pad":
            RATIOS[(case.op, kind)] = max(RATIOS.get((case.op, kind), 0.0), ratio)
        assert n_over == 0, f"{case.id}: {name} ({kind}) {n_over} of {r.numel()} elements over the bound " \
                            f"(NaN = never written), max err / bound {ratio:.3g}"


def run_checked(case, inp, alloc=None):
    """A case as test_vae_against_fp64 runs and checks it; returns clones of the outputs."""
    got = RUN[case.op](case, inp, alloc)
    check(case, inp, got, verbose=False)
    return {k: v.clone() for k, v in got.items()}


@pytest.mark.parametrize("case", V.CASES, ids=lambda c: c.id)
def test_vae_against_fp64(case):
    inp = V.make_inputs(case)
    print(f"\n  {case.id}: {case.entry} -> {case.kernel}")
    check(case, inp, RUN[case.op](case, inp))


BF16_CONV = [c for c in V.CASES if c.op == "conv" and c.shape["out"] == "bf16"]


@pytest.mark.parametrize("case", BF16_CONV, ids=lambda c: c.id)
def test_conv_bf16_store_is_the_rne_of_the_fp32_store(case):
    """The same launch with an fp32 output: the bf16 result is its round-to-nearest-even, bit for bit, through the
    vector store (ca_pack2) and the scalar one alike."""
    inp = V.make_inputs(case)
    lo, hi = run_conv(case, inp), run_conv(case, inp, out_f32=True)
    assert hi["out"].dtype == torch.float32 and lo["out"].dtype == torch.bfloat16
    assert_same_bytes(lo["out"], hi["out"].to(torch.bfloat16), f"{case.id}: bf16 store != RNE(fp32 store)")


@pytest.mark.parametrize("cid", list(V.SCALAR_TWINS))
def test_conv_vector_and_scalar_epilogue_agree(cid):
    """A case that enters the scalar epilogue only through ldo / ldr against its contiguous twin (vector epilogue)."""
    case, twin = V.BY_ID[cid], V.SCALAR_TWINS[cid]
    assert not V.conv_vector_epilogue(case.shape) and V.conv_vector_epilogue(twin.shape)
    a, b = run_conv(case, V.make_inputs(case)), run_conv(twin, V.make_inputs(twin))
    assert_same_bytes(a["out"], b["out"], f"{cid}: scalar epilogue != vector epilogue")


def _expressible(c):
    s = c.shape
    if s.get("big") or c.id == "gn_C1024_hw40000_apply_grid_cap":
        return False
    if c.op == "conv":
        return s["ldx"] == V.ceil_to(s["cin"], 32) and s["ldo"] == s["cout"] and s["ldr"] in (None, s["cout"])
    if c.op == "gn":
        return s["ldx"] == s["C"] == s["ldy"] and s["n_chunks"] is None
    return True


@pytest.mark.parametrize("case", [c for c in V.CASES if _expressible(c)], ids=lambda c: c.id)
def test_wrapper_and_entry_point_agree(case):
    """ops.conv2d_nhwc / groupnorm_nhwc / softmax_rows / affine_rows give the entry point's bits."""
    s, inp = case.shape, V.make_inputs(case)
    want = RUN[case.op](case, inp)
    if case.op == "conv":
        k, stride, up, Ho, Wo, M = V.conv_geometry(s)
        out = inp["out0"].to(DEV).reshape(s["B"], Ho, Wo, s["cout"])
        resid = out if s["resid"] == "in place" else \
            inp["resid"].to(DEV).reshape(out.shape) if s["resid"] == "separate" else None
        ops.conv2d_nhwc(inp["x"].to(DEV).reshape(s["B"], s["H"], s["W"], -1), inp["w"].to(DEV),
                        inp["bias"].to(DEV) if s["bias"] else None, out, s["cout"], ksize=k, stride=stride, upsample=up,
                        resid=resid)
        got = {"out": out.reshape(M, -1)}
    elif case.op == "gn":
        y = inp["y0"].to(DEV).reshape(s["B"], s["HW"], s["C"])
        ops.groupnorm_nhwc(inp["x"].to(DEV).reshape(y.shape), inp["gamma"].to(DEV), inp["beta"].to(DEV), y, s["swish"])
        got = {"y": y.reshape(-1, s["C"])}
    elif case.op == "softmax":
        p = inp["p0"].to(DEV)
        ops.softmax_rows(inp["s"].to(DEV), p, s["n"], s["scale"])
        got = {"p": p[:, :s["n"]], "pad": p[:, s["n"]:]}
    else:
        dev = {k: v.to(DEV) for k, v in inp.items()}
        x, lv, nz = V.affine_operands(case, dev)
        ops.affine_rows(x, dev["out0"], s["a"], s["b"], logvar=lv, noise=nz, cols=s["C"])
        got = {"out": dev["out0"][:, :s["C"]], "pad": dev["out0"][:, s["C"]:]}
    torch.cuda.synchronize()
    for k, v in want.items():
        assert_same_bytes(got[k], v, f"{case.id} {k}: ops wrapper != entry point")


def test_zz_report():
    """(runs last) the largest max err / bound per family and output kind."""
    for key in sorted(RATIOS):
        print("\n  max err / bound", *key, f"{RATIOS[key]:.3f}", end="")
    assert RATIOS
