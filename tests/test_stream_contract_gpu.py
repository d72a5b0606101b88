"""The stream contract of include/conceptattn.h and INTEGRATION.md, entry point by entry point: every call runs on the
stream it was given, returns without waiting for it, allocates nothing and keeps no state between calls (so it can be
captured into a graph and replayed), and may be made from two host threads at once.

a. Order and no host wait (tests/stream_gate.py).  Every probe of tests/stream_contract_cases.py -- one small case per
   launch form, run by the launch helper of its own kernel test file -- runs twice.  Warm-up: ordinary allocations
   on the default stream, checked against the case's own reference as its test file checks it; the allocator records what
   was uploaded.  Probe: on a fresh side stream, every buffer holds poison until a 50 ms delay kernel on another stream
   has finished (inputs get the recorded payload and outputs their fill only behind it).  Every entry point must return
   while the delay is still running, the recorded entry points must be the ones the case table names, and every output
   byte must equal the warm-up's.  A launch on another stream reads poison or is overwritten by the late fill.
   The three wrappers of WAITS_BY_DESIGN read ids on the host: their C entry points are probed directly with device ids
   and meet the contract; the wrappers give the right bytes and must be seen to wait (no stale entry).
b. Capture and replay.  The entries that are more than one launch or own device-side state, hand-written on static
   buffers: captured with inputs A, replayed twice with inputs B and outputs poisoned in between; both replays equal
   eager(B) byte for byte.  Accumulators are reset inside the capture.
c. Two host threads, each with its own stream, 20 calls each (a GEMM route, an attention case), released by a barrier:
   every output equals the serial result."""
import dataclasses
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import address_range_cases as C  # noqa: E402
import attn_cases as A  # noqa: E402
import clip_cases as CL  # noqa: E402
import gemm_route_cases as G  # noqa: E402
import mseg_cases as MS  # noqa: E402
import render_cases as RC  # noqa: E402
import rowop_cases as R  # noqa: E402
import seg_cases as SC  # noqa: E402
import segtab_cases as ST  # noqa: E402
import stream_contract_cases as P  # noqa: E402
import stream_gate as SG  # noqa: E402
import t5_cases as T5  # noqa: E402
import test_attn_routes_gpu as TA  # noqa: E402
import test_clip_kernels_gpu as TC  # noqa: E402
import test_gemm_routes_gpu as TG  # noqa: E402
import test_mseg_kernels_gpu as TM  # noqa: E402
import test_pixel_kernels_gpu as TP  # noqa: E402
import test_render_kernels_gpu as TRN  # noqa: E402
import test_rowop_routes_gpu as TR  # noqa: E402
import test_seg_kernels_gpu as TS  # noqa: E402
import test_segtab_kernels_gpu as TSG  # noqa: E402
import test_t5_fp8_kernels_gpu as TF  # noqa: E402
import test_t5_kernels_gpu as TT  # noqa: E402
import test_vae_routes_gpu as TV  # noqa: E402
import vae_cases as V  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
NAN = float("nan")
BF = torch.bfloat16
ENQUEUE_MS = {}          # probe id -> host time of the warm-up run, first allocator call .. last entry point returned
_INPUTS = {}


def _raw(v) -> bytes:
    if isinstance(v, torch.Tensor):
        return v.contiguous().view(torch.uint8).cpu().numpy().tobytes()
    return np.ascontiguousarray(v).tobytes()


def _memo(key, make):
    if key not in _INPUTS:
        _INPUTS[key] = make()
    return _INPUTS[key]


# ------------------------------------------------------------------------------------------------- a. the runners
# (probe, allocator, warm) -> {name: output}.  `warm`: also the case's own reference check.
def run_gemm(p, al, warm):
    route, epi = p.arg
    r = G.ROUTES[route]
    M, N, ns = _memo(("shape", route, epi), lambda: TG.shape_or_skip(route, epi, 128))
    x = _memo(p.id, lambda: G.make_inputs(epi, M, N, 128, ns, r.fp8, r.rem))
    keep = {}
    (got,), info = TG.launch([x], r.tile, route=route, alloc=al, keep=keep)
    if warm:
        TG.check_against_fp64(x, got, p.id)
    for name, field in C.GEMM_INPUT_FIELD.items():
        if name in keep:
            assert torch.equal(keep[name].cpu(), getattr(x, field)), f"{p.id}: {name} changed"
    if "out2" in keep:
        c0, c1 = keep["out2_cols"]
        assert bool(keep["out2"][:, :c0].isnan().all()) and bool(keep["out2"][:, c1:].isnan().all()), "out2 padding written"
    return got


def run_attn(p, al, warm):
    case = A.BY_ID[p.arg]
    inp = _memo(p.id, lambda: A.make_inputs(case))
    res = TA.launch(case, inp, alloc=al)
    TA.check_untouched(case, res)
    if warm:
        TA.check_bounds(case, inp, res)
    return {f"{i}.{k}": r[k].clone() for i, r in enumerate(res) for k in ("out", "f32", "hm") if r[k] is not None}


def run_rowop(p, al, warm):
    case = R.BY_ID[p.arg]
    inp = _memo(p.id, lambda: R.make_inputs(case))
    got, pads = TR.RUN[case.op](case, inp, al)
    if warm:
        scale = got.get("scale") if case.op in ("ln", "quant") else None
        ref = R.reference(case, inp, dev=DEV, scale_got=scale)
        assert set(ref) == set(got), (set(ref), set(got))
        for name, (r, pre, kind) in ref.items():
            ratio, n_over = R.excess(got[name], r, pre, kind)
            assert n_over == 0, f"{case.id}: {name} ({kind}) {n_over} elements over the bound, max err / bound {ratio:.3g}"
    for buf, before, w in pads:
        TR.assert_same_bytes(buf[:, w:], before[:, w:], f"{case.id}: padding beyond column {w}")
    return {k: v.clone() for k, v in got.items()}


def run_vae(p, al, warm):
    case = V.BY_ID[p.arg]
    inp = _memo(p.id, lambda: V.make_inputs(case))
    got = TV.RUN[case.op](case, inp, al)
    if warm:
        TV.check(case, inp, got, verbose=False)
    return {k: v.clone() for k, v in got.items()}


LN_IDX = torch.tensor(CL.LN_GATHER, dtype=torch.int32)
TEXT_RUN = {          # every helper checks its case against its own reference and bound on every run
    "ca_t5_attn_bf16": TT.run_attention,
    "ca_t5_rmsnorm_f32in": TT.run_rmsnorm,
    "ca_t5_rmsnorm_f32in_fp8": TF.run_rmsnorm_fp8,
    "ca_gated_mul_bf16": TT.run_gated_mul,
    "ca_gated_mul_fp8": TF.run_gated_mul_fp8,
    "ca_embed_rows_f32": lambda case, al: TT.run_embed_rows(case, al)[0],
    "ca_clip_attn_bf16": TC.run_attention,
    "ca_layernorm_f32in": lambda case, al: TC.run_layernorm(case, al, gather=LN_IDX if case[2] else None)[0],
    "ca_quick_gelu_bf16": TC.run_quick_gelu,
    "ca_clip_embed_f32": lambda case, al: TC.run_clip_embed(case, al)[0],
    "ca_pixels_u8_to_nhwc32_bf16": TP.run_to_nhwc32,
    "ca_nhwc_f32_to_pixels_u8": TP.run_to_pixels,
    "ca_seg_score": lambda name, al: TS.run_case(next(c for c in SC.CASES if c.name == name), al),
}


def _stream():
    return torch.cuda.current_stream().cuda_stream


# The three entry points behind the wrappers of WAITS_BY_DESIGN, straight through the binding with device ids.  The
# allocator calls are those of the wrapper's helper, in its order (the Gated allocator checks that).
def direct_embed_rows(case, al):
    H, rows, strided = case
    table, ids = T5.embed_inputs(H, rows, 512)
    pad = 64 if strided else 0
    ts = al.to(TT._widened(table, H + pad).to(BF), {"table": None})
    di = al.to(ids, {"ids": None})
    full = al.full((rows, H + 2 * pad), NAN, torch.float32, {"out": None})
    L.check(L.load().ca_embed_rows_f32(ts.data_ptr(), ts.stride(0), di.data_ptr(), full.data_ptr(), full.stride(0), rows, H,
                                       _stream()), "ca_embed_rows_f32")
    torch.cuda.synchronize()
    assert torch.isnan(full[:, H:]).all()
    return {"out": full[:, :H].clone()}


def direct_clip_embed(H, al):
    tok, pos, ids = CL.embed_inputs(H, 512)
    rows = ids.shape[0]
    ts = al.to(TC._widened(tok, H + 64).to(BF), {"tok": None})
    ps = al.to(TC._widened(pos, H + 8).to(BF), {"pos": None})
    di = al.to(ids, {"ids": None})
    full = al.full((rows, H + 128), NAN, torch.float32, {"out": None})
    L.check(L.load().ca_clip_embed_f32(ts.data_ptr(), ts.stride(0), ps.data_ptr(), ps.stride(0), di.data_ptr(),
                                       full.data_ptr(), full.stride(0), rows, CL.EMBED_L, H, _stream()), "ca_clip_embed_f32")
    torch.cuda.synchronize()
    assert torch.isnan(full[:, H:]).all()
    return {"out": full[:, :H].clone()}


def direct_layernorm(case, al):
    H, rows, strided = case
    x, w, b = CL.ln_inputs(H, rows)
    pad = 64 if strided else 0
    xs = al.to(TC._widened(x, H + pad), {"x": None})
    wd, bd = al.to(w, {"w": None}), al.to(b, {"b": None})
    idx = al.to(LN_IDX, {"row_idx": None})
    full = al.full((LN_IDX.shape[0], H + 2 * pad), NAN, BF, {"out": None})
    L.check(L.load().ca_layernorm_f32in(xs.data_ptr(), xs.stride(0), idx.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                        full.data_ptr(), full.stride(0), full.shape[0], H, CL.EPS, _stream()),
            "ca_layernorm_f32in")
    torch.cuda.synchronize()
    assert torch.isnan(full[:, H:]).all()
    return {"out": full[:, :H].clone()}


DIRECT = {"ca_embed_rows_f32": direct_embed_rows, "ca_clip_embed_f32": direct_clip_embed,
          "ca_layernorm_f32in": direct_layernorm}


def run_text(p, al, warm):
    entry, case = p.arg
    if p.direct and not warm:
        return DIRECT[entry](case, al)
    return TEXT_RUN[entry](case, al)


def run_segtab(p, al, warm):
    rec, ws, _, _ = TSG.run_case(next(c for c in ST.CASES if c.name == p.arg), al)
    return {"records": rec, "cells": ws}


def run_mseg(p, al, warm):
    counts, c_out, i_out = TM.run_case(next(c for c in MS.CASES if c.name == MS.PLACEMENT_CASE), al)
    return {k: v for k, v in (("counts", counts), ("class_out", c_out), ("index_out", i_out)) if v is not None}


def run_render(p, al, warm):
    out, ranges = TRN.run_case(RC.BY_NAME[p.arg], al)
    return {"out": out, "ranges": ranges}


RUN = {"gemm": run_gemm, "attn": run_attn, "rowop": run_rowop, "vae": run_vae, "text": run_text, "segtab": run_segtab,
       "mseg": run_mseg, "render": run_render}


@pytest.mark.parametrize("p", P.PROBES, ids=repr)
def test_runs_on_its_stream_and_returns_before_it_drains(p):
    rec = SG.Recording(DEV)
    with SG.watching() as warm_calls:
        want = RUN[p.family](p, rec, True)
    assert warm_calls and rec.t_first is not None
    ENQUEUE_MS[p.id] = (warm_calls[-1][2] - rec.t_first) * 1e3
    torch.cuda.synchronize()

    gate = SG.Gate()
    al = SG.Gated(rec, gate)
    s2 = torch.cuda.Stream()
    assert s2.cuda_stream != 0 and s2 != torch.cuda.current_stream()
    try:
        with torch.cuda.stream(s2), SG.watching(gate) as calls:
            got = RUN[p.family](p, al, False)
    finally:
        torch.cuda.synchronize()
    al.release()
    seen = [(n, running) for n, running, _ in calls if n not in P.NO_STREAM]
    print(f"\n  {p.id}: warm-up enqueue {ENQUEUE_MS[p.id]:.2f} ms; probe {seen}")
    assert seen, "no entry point went through check"
    assert tuple(n for n, _ in seen) == p.entries, (seen, p.entries)
    waited = [n for n, running in seen if not running]
    if p.wrapper is not None:
        assert p.wrapper in P.WAITS_BY_DESIGN
        assert waited, f"{p.wrapper} is listed in WAITS_BY_DESIGN but returned while the gate was running: a stale entry"
    else:
        assert not waited, f"{waited} returned only after the gate had finished: the call (or its helper) waits for the stream"
    assert set(got) == set(want), (set(got), set(want))
    for k in want:
        assert _raw(got[k]) == _raw(want[k]), f"{p.id}: {k} behind the gate != the warm-up run"


def test_every_wrapper_that_waits_is_probed_and_its_entry_point_directly():
    probed = {p.wrapper for p in P.PROBES if p.wrapper}
    assert probed == set(P.WAITS_BY_DESIGN), probed ^ set(P.WAITS_BY_DESIGN)
    for p in P.PROBES:
        if p.wrapper:
            assert any(q.direct and q.entries == p.entries for q in P.PROBES), p.id


# ------------------------------------------------------------------------------------------- b. capture and replay
def _poison(t):
    if t.dtype.is_floating_point:
        t.fill_(NAN)
    else:
        t.view(torch.uint8).fill_(SG.POISON_BYTE)


def _replay_check(name, sets, static, outs, call):
    """sets: (A, B), each {name: device tensor} for the static input buffers `static`; outs: {name: output tensor};
    call(): the ops calls (returns extra outputs or None).  Eager A and B, a warm-up on a side stream, a capture with A in
    the buffers, then two replays with B and poisoned outputs: both equal eager(B)."""
    a, b = sets
    assert set(a) == set(b) == set(static)

    def load(s):
        for k, v in s.items():
            static[k].copy_(v)

    def eager(s):
        load(s)
        for t in outs.values():
            _poison(t)
        extra = call() or {}
        torch.cuda.synchronize()
        return {k: _raw(v) for k, v in {**outs, **extra}.items()}
    ea, eb = eager(a), eager(b)
    assert any(ea[k] != eb[k] for k in ea), f"{name}: the two input sets give the same bytes"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    load(a)
    for t in outs.values():
        _poison(t)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        extra = call() or {}
    load(b)
    for i in (1, 2):
        for t in list(outs.values()) + list(extra.values()):
            _poison(t)
        g.replay()
        torch.cuda.synchronize()
        got = {k: _raw(v) for k, v in {**outs, **extra}.items()}
        for k in eb:
            assert got[k] != ea[k] or ea[k] == eb[k], f"{name}: replay {i}: {k} holds what capture-time inputs give"
            assert got[k] == eb[k], f"{name}: replay {i}: {k} != eager"


def _rand(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


def _labels(shape, seed, hi=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, hi, shape, generator=g, dtype=torch.uint8).to(DEV)


def _like(s):
    return {k: torch.empty_like(v) for k, v in s.items()}


def test_replay_segtab_score():
    M, h, w, Hl, Wl = 6, 16, 16, 64, 64
    sets = [dict(maps=_rand((M, h, w), s), label=_labels((Hl, Wl), s + 1)) for s in (1, 11)]
    st = _like(sets[0])
    outs = dict(records=torch.empty(M, 40, dtype=torch.uint8, device=DEV), cells=ops.segtab_cells(h, w, DEV))
    _replay_check("segtab_score", sets, st, outs, lambda: ops.segtab_score(
        st["maps"], None, st["label"], outs["records"], outs["cells"], downscale_for_eval=True,
        blur_weights=ops.seg_blur_weights()))


@pytest.mark.parametrize("given", [False, True], ids=["own-ranges", "given-ranges"])
def test_replay_heatmap_render(given):
    G_, n, h, w, H, W = 2, 3, 16, 12, 37, 53
    lut = torch.from_numpy(RC.synthetic_lut()).to(DEV)
    sets = []
    for s in (2, 12):
        d = dict(maps=_rand((G_, n, h, w), s), image=_labels((G_, H, W, 3), s + 1, 256))
        if given:
            d["ranges"] = torch.tensor([[-0.5, 0.5], [-1.0, 0.25]], device=DEV) * (1 + 0.1 * s)
        sets.append(d)
    st = _like(sets[0])
    outs = dict(out=torch.empty(G_, n, H, W, 3, dtype=torch.uint8, device=DEV))

    def call():
        _, used = ops.heatmap_render(list(st["maps"]), lut, size=(H, W), bilinear=not given, images=list(st["image"]),
                                     alpha=0.4, ranges=st["ranges"] if given else None, out=list(outs["out"]))
        return {"used": used}
    _replay_check("heatmap_render", sets, st, outs, call)


def test_replay_seg_score():
    n, h, w, Hl, Wl = 3, 16, 16, 64, 64
    sets = [dict(maps=_rand((n, h, w), s), labels=_labels((n, Hl, Wl), s + 1)) for s in (3, 13)]
    st = _like(sets[0])
    outs = dict(results=torch.empty(n, 40, dtype=torch.uint8, device=DEV),
                mask=torch.empty(n, h, w, dtype=torch.uint8, device=DEV), coeff=torch.empty(n, h, w, device=DEV))
    _replay_check("seg_score", sets, st, outs, lambda: ops.seg_score(
        st["maps"], list(st["labels"]), outs["results"], blur_weights=ops.seg_blur_weights(), mask_out=outs["mask"],
        coeff_out=outs["coeff"]))


def test_replay_mseg_score():
    n, K, h, w, Hl, Wl, nclass = 2, 5, 16, 16, 48, 48, 7
    sets = [dict(maps=_rand((n, K, h, w), s), labels=_labels((n, Hl, Wl), s + 1, nclass)) for s in (4, 14)]
    st = _like(sets[0])
    outs = dict(counts=torch.empty(n, 2 + 2 * nclass, dtype=torch.int32, device=DEV),
                cls=torch.empty(n, h, w, dtype=torch.uint8, device=DEV), idx=torch.empty(n, h, w, dtype=torch.uint8, device=DEV))
    class_of = [[1, 2, 3, 4, 6], [0, 2, 5, 1, 3]]
    _replay_check("mseg_score", sets, st, outs, lambda: ops.mseg_score(
        st["maps"], list(st["labels"]), outs["counts"], class_of, nclass, ignore_index=0, scale=[1.0, 0.5, 2.0, 1.5, 1.0],
        blur_weights=ops.seg_blur_weights(), class_out=outs["cls"], index_out=outs["idx"]))


def test_replay_groupnorm_nhwc():
    B, HW, Cc = 2, 1100, 64                      # two chunks per item: the partial-sum plane is used
    assert ops.groupnorm_chunks(HW) == 2
    sets = [dict(x=_rand((B, HW, Cc), s, 2.0), gamma=_rand((Cc,), s + 1), beta=_rand((Cc,), s + 2)) for s in (5, 15)]
    st = _like(sets[0])
    outs = dict(y=torch.empty(B, HW, Cc, dtype=BF, device=DEV), part=torch.empty(B * 2 * 96, device=DEV))
    _replay_check("groupnorm_nhwc", sets, st, outs, lambda: ops.groupnorm_nhwc(
        st["x"], st["gamma"], st["beta"], outs["y"], True, part=outs["part"]))


def test_replay_modulation_gemm_with_its_combine():
    nv, K, N = 3, 256, 512
    sets = [dict(vecs=_rand((nv, K), s), w=_rand((N, K), s + 1, K ** -0.5, BF), bias=_rand((N,), s + 2, 0.5, BF))
            for s in (6, 16)]
    st = _like(sets[0])
    ones = torch.ones(N, device=DEV)
    outs = dict(out=torch.empty(nv, N, device=DEV))
    seen = []

    def call():
        with SG.watching() as calls:
            assert ops.modulation_gemm(st["vecs"], st["w"], st["bias"], outs["out"], ones)
        seen[:] = [n for n, _, _ in calls]
    _replay_check("modulation_gemm", sets, st, outs, call)
    assert seen == ["ca_silu_split_bf16", "ca_gemm_bf16", "ca_modulation_combine_f32"], seen


def test_replay_heatmap_fused_with_the_accumulator_reset_inside_the_capture():
    Lp, Cc, dim = 300, 4, 256
    sets = [dict(img=_rand((Lp, dim), s, 1.0, BF), con=_rand((Cc, dim), s + 1, 0.2, BF), acc0=_rand((Cc, Lp), s + 2))
            for s in (7, 17)]
    st = _like(sets[0])
    outs = dict(acc=torch.empty(Cc, Lp, device=DEV), logits=torch.empty(Cc, Lp, device=DEV))

    def call():
        outs["acc"].copy_(st["acc0"])            # the accumulator's reset: inside the capture
        ops.heatmap_fused([ops.Heatmap(st["img"], st["con"], acc=outs["acc"], weight=0.5, logits=outs["logits"])])
    _replay_check("heatmap_fused", sets, st, outs, call)


def test_replay_ln_modulate_fp8():
    M, H = 37, 3072
    sets = [dict(x=_rand((M, H), s, 2.0, BF), shift=_rand((H,), s + 1, 0.3), scale=_rand((H,), s + 2, 0.3),
                 shift2=_rand((H,), s + 3, 0.3), scale2=_rand((H,), s + 4, 0.3)) for s in (8, 18)]
    st = _like(sets[0])
    outs = dict(q=torch.empty(M, H, dtype=torch.uint8, device=DEV), s=torch.empty(M, device=DEV))
    _replay_check("ln_modulate fp8", sets, st, outs, lambda: ops.ln_modulate(
        st["x"], outs["q"], [(20, st["shift"], st["scale"]), (M, st["shift2"], st["scale2"])], out_scale=outs["s"]))


def test_replay_attn4_on_the_re_reference_path():
    case = A.BY_ID["pre_reref_spikes"]
    (p,) = case.probs
    assert p.spikes and case.form == "pre" and not p.two_q and p.n1 == 0
    sets, xs = [], []
    for seed in (p.seed, p.seed + 1000):
        (x,) = A.make_inputs(dataclasses.replace(case, probs=(dataclasses.replace(p, seed=seed),)))
        xs.append(x)
        sets.append(dict(qbuf=x.qbuf.to(DEV), kvbuf=x.kvbuf.to(DEV)))
    st = _like(sets[0])
    x, D = xs[0], xs[0].D
    gx = dataclasses.replace(x, qbuf=st["qbuf"], kvbuf=st["kvbuf"])
    q0, _, k0, v0, _, _ = A.views(case, p, gx)
    outs = dict(out=torch.empty(x.out_rows, x.ldo, dtype=BF, device=DEV), f32=torch.empty(p.nq, x.ldo32, device=DEV))
    attn = ops.Attn(q0, outs["out"][x.gq0:x.gq0 + p.nq, :D], k0, v0, out_f32=outs["f32"][:, :D])
    st["qbuf"].copy_(sets[0]["qbuf"]), st["kvbuf"].copy_(sets[0]["kvbuf"])
    ops.attention_stats(reset=True)
    ops.attention([attn], case.heads, q_prescaled=True)
    torch.cuda.synchronize()
    assert ops.attention_stats()["rereference_events"] > 0, "the case does not take the re-reference path"
    _replay_check("attention (ca_attn4_kernel)", sets, st, outs, lambda: ops.attention([attn], case.heads, q_prescaled=True))
    # the rows and columns the kernel does not own still hold the poison of the last replay
    assert bool(outs["out"][:, D:].isnan().all()) and bool(outs["out"][:x.gq0].isnan().all()) and \
        bool(outs["f32"][:, D:].isnan().all())


@pytest.mark.parametrize("route", ["thin_4x4", "fp8"])
def test_replay_gemm(route):
    """thin_4x4: a bf16 plan with thin rows, the main launch and ca_gemm_thin_kernel's; fp8: ca_gemm_fp8."""
    r, epi = G.ROUTES[route], "bias_bf16"
    M, N, ns = TG.shape_or_skip(route, epi, 128)
    xa, xb = (G.make_inputs(epi, M, N, 128, ns, r.fp8, r.rem, seed=s) for s in (0, 50))
    keep = {}
    g, _ = TG.build(xa, keep=keep)
    info = ops.gemm_plan([g], tile=r.tile)
    assert G.route_matches(info, r), info
    assert r.fp8 or (info["thin_mf"] > 0 and info["main_tiles"] > 0), info        # two launches
    fields = {k: f for k, f in C.GEMM_INPUT_FIELD.items() if k in keep}
    sets = [{k: getattr(x, f).to(DEV) for k, f in fields.items()} for x in (xa, xb)]
    st = {k: keep[k] for k in fields}
    _replay_check(f"gemm {route}", sets, st, dict(out=keep["out"]), lambda: ops.gemm([g], r.tile))


# ------------------------------------------------------------------------------------------- c. two host threads
def test_two_host_threads_on_their_own_streams():
    """"its only process state is ... idempotent".  One thread repeats a GEMM route case, the other an
    attention case, 20 calls each at the same moment; every output equals the serial result."""
    N_CALLS = 20
    route, epi = "pp256", "bias_bf16"
    r = G.ROUTES[route]
    M, N, ns = TG.shape_or_skip(route, epi, 128)
    g, _ = TG.build(G.make_inputs(epi, M, N, 128, ns, False, r.rem))
    case = A.BY_ID["pre_nk320_rnd"]
    (p,), (x,) = case.probs, A.make_inputs(case)
    gx = dataclasses.replace(x, qbuf=x.qbuf.to(DEV), kvbuf=x.kvbuf.to(DEV))
    q0, q1, k0, v0, k1, v1 = A.views(case, p, gx)
    D, nq0 = x.D, q0.shape[0]
    out = torch.full((x.out_rows, x.ldo), NAN, dtype=BF, device=DEV)
    attn = ops.Attn(q0, out[x.gq0:x.gq0 + nq0, :D], k0, v0, k1, v1, q1=q1,
                    out1=out[x.gq1:x.gq1 + q1.shape[0], :D] if q1 is not None else None)
    work = {"gemm": (lambda: ops.gemm([g], r.tile), g.out), "attn": (lambda: ops.attention([attn], case.heads, q_prescaled=True), out)}
    serial = {}
    for k, (call, o) in work.items():            # warm-up and the serial result
        o.fill_(NAN)
        call()
        torch.cuda.synchronize()
        serial[k] = _raw(o)
    barrier, results, errors = threading.Barrier(2), {}, []

    def body(k):
        try:
            call, o = work[k]
            s = torch.cuda.Stream()
            got = []
            with torch.cuda.stream(s):
                barrier.wait(timeout=60)
                for _ in range(N_CALLS):
                    o.fill_(NAN)
                    call()
                    got.append(o.clone())
            s.synchronize()
            results[k] = [_raw(t) for t in got]
        except BaseException as e:   # noqa: BLE001
            errors.append((k, repr(e)))
    threads = [threading.Thread(target=body, args=(k,)) for k in work]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for k in work:
        assert len(results[k]) == N_CALLS
        for i, b in enumerate(results[k]):
            assert b == serial[k], f"{k}: call {i} of the concurrent run != the serial result"


def test_zz_report():
    """(runs last) the largest host enqueue time of a warm-up run next to the gate's length."""
    if ENQUEUE_MS:
        worst = max(ENQUEUE_MS, key=ENQUEUE_MS.get)
        print(f"\n  gate {SG.GATE_MS} ms ({SG.Gate.calibrate()}); largest warm-up enqueue {ENQUEUE_MS[worst]:.2f} ms ({worst}); "
              f"{len(ENQUEUE_MS)} probes")
