"""Concept re-query at the model level (GPU box): HipFluxDiT(..., trace=) and HipFluxDiT.requery on the tiny geometry of
tests/test_model_gpu.py::tiny_case (H = 256, 2 heads, 2 + 2 blocks, 256 image tokens, T = 8), layers [0, 1], one step.

Bounds.  Against the fp32 oracle the maps are held to what tests/test_model_gpu.py::
test_tiny_stop_after_multimodal_and_fused_heatmaps holds them to on this geometry (3e-3 output space, 5e-3 cross space);
the sparse norms to the same two figures, which is what tests/test_model_routes_gpu.py::test_case_against_the_oracle
(OUT_MAP_GATE / CROSS_MAP_GATE, cases noepi_entmax15_c8 and indep_sparsemax) holds them to, against oracle.sparse_norms on
the oracle's logits.  Against a fresh forward with the same concept set and the tracing routes a re-query is bit-identical.
"""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from conceptattention_amd import _lib as L, ops  # noqa: E402
from conceptattention_amd.flux_dit import HeatmapRequest, HipFluxDiT, StepTrace, step_trace_nbytes  # noqa: E402
from conceptattention_amd.params import tiny_params  # noqa: E402
from conceptattention_amd.weights import synthetic_inputs, synthetic_state_dict  # noqa: E402
from oracle import flux_oracle as O  # noqa: E402
from oracle import sparse_norms  # noqa: E402

DEV = "cuda:0"
LAYERS = (0, 1)
T_STEP = 0.5
OUT_GATE, CROSS_GATE = 3e-3, 5e-3
SPACES = (("out_space", "output_space", OUT_GATE), ("cross_space", "cross_attention", CROSS_GATE))
# concept sets: name -> (C', seed); A is the traced call's own set (tiny_case: C = 3, seed 2)
SETS = {"A": (3, 2), "B": (1, 11), "c5": (5, 12), "c9": (9, 13)}


def bf(x):
    return x.bfloat16().float()


def maxabs(a, b):
    return (torch.as_tensor(a).float().cpu() - torch.as_tensor(b).float().cpu()).abs().max().item()


def inputs(p, side=256, seed=2, C=3):
    return {k: (bf(v) if v.is_floating_point() else v)
            for k, v in synthetic_inputs(p, side, side, n_txt=8, n_concepts=C, seed=seed).items()}


@pytest.fixture(scope="module")
def ctx():
    p = tiny_params(guidance_embed=False, depth=2, depth_single_blocks=2)
    sd = {k: bf(v) for k, v in synthetic_state_dict(p, seed=1).items()}
    m = HipFluxDiT(p, DEV)
    m.load_state_dict(sd)
    return SimpleNamespace(p=p, sd=sd, m=m, inp=inputs(p), oracle={}, fresh={})


def concept_set(ctx, name):
    C, seed = SETS[name]
    inp = inputs(ctx.p, seed=seed, C=C)
    return inp["concepts"], inp["concept_ids"]


def request(C, norm=L.NORM_SOFTMAX, layers=LAYERS, n_img=256):
    return HeatmapRequest(tuple(layers), 1.0 / len(layers), torch.zeros(C, n_img, device=DEV),
                          torch.zeros(C, n_img, device=DEV), norm=norm)


def forward(ctx, con, con_ids, reqs, inp=None, trace=None, tracing_routes=False, model=None):
    """One full forward of ``inp`` (a list: one item each) with the concept rows ``con``; (pred, reqs)."""
    m = model or ctx.m
    items = inp if isinstance(inp, list) else [inp or ctx.inp]
    cat = lambda k: torch.cat([it[k] for it in items], 0).to(DEV)  # noqa: E731
    B = len(items)
    before = m.epilogue_logits
    if tracing_routes:
        m.epilogue_logits = False
    try:
        pred, _ = m(img=torch.cat([O.patchify(it["latent"]) for it in items], 0).to(DEV), img_ids=cat("img_ids"),
                    txt=cat("txt"), txt_ids=cat("txt_ids"), concepts=con.to(DEV), concept_ids=con_ids.to(DEV),
                    concept_vec=cat("concept_vec"), y=cat("vec"), timesteps=torch.full((B,), T_STEP, device=DEV),
                    return_vectors=False, heatmaps=reqs, **({} if trace is None else {"trace": trace}))
    finally:
        m.epilogue_logits = before
    return pred, reqs


def oracle_maps(ctx, name, norm):
    """The fp32 oracle's two maps [C', 256] for concept set ``name``: computed once per set, never modified."""
    if name not in ctx.oracle:
        con, con_ids = concept_set(ctx, name)
        inp = ctx.inp
        with torch.no_grad():
            ctx.oracle[name] = O.dit_forward(ctx.sd, ctx.p, O.patchify(inp["latent"]), inp["img_ids"], inp["txt"],
                                             inp["txt_ids"], con, con_ids, inp["concept_vec"], torch.tensor([T_STEP]),
                                             inp["vec"])
    pred, d = ctx.oracle[name]
    out = {}
    for attr, space, _ in SPACES:
        img, cv = d[f"{space}_image_vectors"][None], d[f"{space}_concept_vectors"][None]
        if norm == L.NORM_SOFTMAX:
            out[attr] = O.compute_heatmaps(img, cv, list(LAYERS), [0])[0].reshape(-1, 256)
        else:
            fn = {L.NORM_SPARSEMAX: sparse_norms.sparsemax, L.NORM_ENTMAX15: sparse_norms.entmax15}[norm]
            logits = O.heatmap_logits(img, cv)[0, list(LAYERS), 0]
            out[attr] = torch.from_numpy(fn(logits.double().numpy(), axis=1).mean(0)).float()
    return pred, out


@pytest.fixture(scope="module")
def traced(ctx):
    """The tracing forward with set A and the same forward without a trace: (trace, pred, reqs, pred_plain, reqs_plain)."""
    con, con_ids = concept_set(ctx, "A")
    pred0, req0 = forward(ctx, con, con_ids, [request(3)])
    trace = StepTrace()
    pred1, req1 = forward(ctx, con, con_ids, [request(3)], trace=trace)
    torch.cuda.synchronize()
    return SimpleNamespace(trace=trace, pred=pred1, reqs=req1, pred_plain=pred0, reqs_plain=req0)


def requery(ctx, traces, name_or_con, norm=L.NORM_SOFTMAX, layers=LAYERS):
    con, con_ids = concept_set(ctx, name_or_con) if isinstance(name_or_con, str) else name_or_con
    B = len(traces)
    reqs = [request(con.shape[1], norm, layers) for _ in range(B)]
    ctx.m.requery(traces, con.to(DEV).expand(B, -1, -1) if con.shape[0] == 1 else con.to(DEV),
                  con_ids.to(DEV).expand(B, -1, -1) if con_ids.shape[0] == 1 else con_ids.to(DEV), reqs)
    return reqs


# ------------------------------------------------------------------------------------ 1. the tracing forward
def test_tracing_forward_leaves_the_prediction_alone(ctx, traced):
    assert traced.trace.filled and traced.trace.model is ctx.m
    assert torch.equal(traced.pred, traced.pred_plain)
    _, want = oracle_maps(ctx, "A", L.NORM_SOFTMAX)
    for attr, _, gate in SPACES:
        got = getattr(traced.reqs[0], attr)
        print(f"\n[measured] tracing forward, {attr}: {maxabs(got, want[attr]):.3e} from the oracle (gate {gate:.0e}), "
              f"{maxabs(got, getattr(traced.reqs_plain[0], attr)):.3e} from the non-tracing call's maps")
        assert maxabs(got, want[attr]) < gate
    tr = traced.trace
    assert tr.layers == LAYERS and len(tr.qkv) == 2 and set(tr.att_img) == set(tr.qpre) == {0, 1}
    assert tr.nbytes == step_trace_nbytes(ctx.p, 3, 8, 256, 2, 2) == 1940480
    held = sum(t.numel() * t.element_size() for t in [*tr.qkv, *tr.att_img.values(), *tr.qpre.values(), tr.mod])
    assert held == tr.nbytes
    # storage of its own: none of it is the model's reusable workspace
    ws = {t.data_ptr() for t in ctx.m._ws_cache[ctx.m._ws_key].values() if isinstance(t, torch.Tensor)}
    assert not ws & {t.data_ptr() for t in [*tr.qkv, *tr.att_img.values(), *tr.qpre.values(), tr.mod]}
    assert ctx.m.QKV.data_ptr() in ws and ctx.m._traced == {} and ctx.m.epilogue_logits is True


# ------------------------------------------------------------------------------------ 2. re-query equals a fresh call
def test_prediction_does_not_depend_on_the_concept_set(ctx):
    """The precondition of an exact re-query: the image rows never see a concept row."""
    preds = []
    for name in ("A", "B"):
        con, con_ids = concept_set(ctx, name)
        preds.append(forward(ctx, con, con_ids, [request(con.shape[1])], tracing_routes=True)[0])
    assert torch.equal(preds[0], preds[1])


@pytest.mark.parametrize("name", list(SETS))
def test_requery_equals_a_fresh_call(ctx, traced, name):
    con, con_ids = concept_set(ctx, name)
    rq = requery(ctx, [traced.trace], name)[0]
    _, fresh = forward(ctx, con, con_ids, [request(con.shape[1])], tracing_routes=True)
    _, want = oracle_maps(ctx, name, L.NORM_SOFTMAX)
    for attr, _, gate in SPACES:
        got, fr = getattr(rq, attr), getattr(fresh[0], attr)
        print(f"\n[measured] requery {name} (C' = {con.shape[1]}), {attr}: {maxabs(got, want[attr]):.3e} from the oracle, "
              f"{maxabs(got, fr):.3e} from the fresh call (fresh call: {maxabs(fr, want[attr]):.3e} from the oracle)")
        assert abs(got.sum(0) - 1).max().item() < 1e-5
        assert maxabs(got, want[attr]) < gate                      # (i)
        assert torch.equal(got, fr), attr                          # (ii)


# ------------------------------------------------------------------------------------ 3. two items in one re-query
def test_two_items_in_one_requery(ctx):
    items = [ctx.inp, inputs(ctx.p, seed=5)]
    conA = torch.cat([it["concepts"] for it in items], 0)
    idsA = torch.cat([it["concept_ids"] for it in items], 0)
    trace = StepTrace()
    forward(ctx, conA, idsA, [request(3), request(3)], inp=items, trace=trace)
    views = trace.items()
    assert len(views) == 2 and trace.nbytes == 2 * views[0].nbytes
    new = torch.cat([concept_set(ctx, "c5")[0], inputs(ctx.p, seed=21, C=5)["concepts"]], 0)
    ids = torch.zeros(2, 5, 3)
    both = requery(ctx, views, (new, ids))
    for j in range(2):
        one = requery(ctx, [views[j]], (new[j:j + 1], ids[j:j + 1]))[0]
        for attr, _, _ in SPACES:
            assert torch.equal(getattr(both[j], attr), getattr(one, attr)), (j, attr)
    # and the item of a batched tracing forward is the item of its own one-item tracing forward
    t0 = StepTrace()
    forward(ctx, conA[:1], idsA[:1], [request(3)], inp=[items[0]], trace=t0)
    one = requery(ctx, [t0], (new[:1], ids[:1]))[0]
    for attr, _, _ in SPACES:
        assert torch.equal(getattr(both[0], attr), getattr(one, attr)), attr


# ------------------------------------------------------------------------------------ 4. the sparse norms
@pytest.mark.parametrize("norm", [L.NORM_SPARSEMAX, L.NORM_ENTMAX15], ids=["sparsemax", "entmax15"])
def test_requery_with_sparse_norms(ctx, traced, norm):
    con, con_ids = concept_set(ctx, "A")
    rq = requery(ctx, [traced.trace], "A", norm)[0]
    _, fresh = forward(ctx, con, con_ids, [request(3, norm)], tracing_routes=True)
    _, want = oracle_maps(ctx, "A", norm)
    for attr, _, gate in SPACES:
        got, fr = getattr(rq, attr), getattr(fresh[0], attr)
        print(f"\n[measured] requery, norm {norm}, {attr}: {maxabs(got, want[attr]):.3e} from the oracle, "
              f"{maxabs(got, fr):.3e} from the fresh call")
        assert maxabs(got, want[attr]) < gate
        assert torch.equal(got, fr), attr


# ------------------------------------------------------------------------------------ 5. nothing of the image pass runs
def test_requery_launches_concept_rows_only(ctx, traced):
    tr, W = traced.trace, ctx.m.weights
    gemms, attns = [], []

    def gemm_hook(arr, tile, launch):
        gemms.extend((arr[i].M, arr[i].W) for i in range(len(arr)))
        launch()

    def attn_hook(arr, num_heads, launch):
        attns.extend((arr[i].nq, arr[i].k1, arr[i].n1, arr[i].v1) for i in range(len(arr)))
        launch()
    B, C = 1, 5
    ops.set_gemm_hook(gemm_hook)
    ops.set_attn_hook(attn_hook)
    try:
        requery(ctx, [tr], "c5")
    finally:
        ops.set_gemm_hook(None)
        ops.set_attn_hook(None)
    allowed = {W[k].data_ptr() for k in W.tensors if k == "txt_in.weight" or (k.startswith("double_blocks.") and ".txt_" in k)}
    assert gemms and all(M <= B * C for M, _ in gemms), gemms
    assert all(w in allowed for _, w in gemms), "a GEMM outside txt_in and the double blocks' text weights"
    # block 0 in full (qkv, low plane, proj, mlp.0, mlp.2), block 1 up to its maps, and txt_in
    assert len(gemms) == 1 + 5 + 2, gemms
    assert len(attns) == 2
    for i, (nq, k1, n1, v1) in enumerate(attns):
        lo = tr.qkv[i].data_ptr()
        hi = lo + tr.qkv[i].numel() * 2
        assert nq <= C and n1 == 256
        assert lo <= k1 < hi and lo <= v1 < hi, "the second key / value segment is not the trace's storage"


# ------------------------------------------------------------------------------------ 6. the trace survives later work
def test_trace_survives_later_work_and_is_not_consumed(ctx, traced):
    first = requery(ctx, [traced.trace], "c5")[0]
    other = inputs(ctx.p, side=128, seed=7, C=2)
    forward(ctx, other["concepts"], other["concept_ids"], [request(2, n_img=64)], inp=[other])
    again = requery(ctx, [traced.trace], "c5")[0]
    third = requery(ctx, [traced.trace], "c5")[0]
    for attr, _, _ in SPACES:
        assert torch.equal(getattr(first, attr), getattr(again, attr)), attr
        assert torch.equal(getattr(first, attr), getattr(third, attr)), attr


def test_subset_of_the_traced_layers(ctx, traced):
    """A layer's maps do not depend on which other traced layers the re-query asks for: a re-query of one layer is that
    layer's row of the per-layer tables of a fresh forward that captures BOTH layers (a fresh forward capturing one layer
    alone has another route in the other layer, so other concept rows downstream)."""
    both = request(5)
    both.per_layer_out = torch.zeros(2, 5, 256, device=DEV)
    both.per_layer_cross = torch.zeros(2, 5, 256, device=DEV)
    con, con_ids = concept_set(ctx, "c5")
    forward(ctx, con, con_ids, [both], tracing_routes=True)
    for li in LAYERS:
        one = requery(ctx, [traced.trace], "c5", layers=(li,))[0]
        assert torch.equal(one.out_space, both.per_layer_out[li]) and torch.equal(one.cross_space, both.per_layer_cross[li])


# ------------------------------------------------------------------------------------ refusals, before any launch
def test_model_level_refusals_launch_nothing(ctx, traced):
    m, tr = ctx.m, traced.trace
    con, con_ids = (t.to(DEV) for t in concept_set(ctx, "B"))
    calls = []
    ops.set_gemm_hook(lambda arr, tile, launch: (calls.append("gemm"), launch()))
    ops.set_attn_hook(lambda arr, nh, launch: (calls.append("attn"), launch()))

    def refused(match, fn):
        with pytest.raises(ValueError, match=match):
            fn()
        assert calls == []
    try:
        other = HipFluxDiT(ctx.p, DEV, weights=m.weights)
        refused("another model", lambda: other.requery([tr], con, con_ids, [request(1)]))
        m.set_precision("fp8")
        refused("precision", lambda: m.requery([tr], con, con_ids, [request(1)]))
        refused("precision", lambda: forward(ctx, con, con_ids, [request(1)], trace=StepTrace()))
        m.set_precision("bf16")
        m.capture_independent_image = True
        refused("capture_independent_image", lambda: m.requery([tr], con, con_ids, [request(1)]))
        refused("capture_independent_image", lambda: forward(ctx, con, con_ids, [request(1)], trace=StepTrace()))
        m.capture_independent_image = False
        refused("layer_indices", lambda: m.requery([tr], con, con_ids, [request(1, layers=(0, 2))]))
        refused("already filled", lambda: forward(ctx, con, con_ids, [request(1)], trace=tr))
        big = torch.zeros(1, 33, ctx.p.context_in_dim, device=DEV, dtype=torch.bfloat16)
        refused("33", lambda: m.requery([tr], big, torch.zeros(1, 33, 3, device=DEV), [request(33, L.NORM_SPARSEMAX)]))
        gone = tr.items()[0]
        gone.release()
        assert gone.nbytes == 0 and tr.nbytes > 0
        refused("released", lambda: m.requery([gone], con, con_ids, [request(1)]))
        small = StepTrace()
    finally:
        m.set_precision("bf16")
        m.capture_independent_image = False
        ops.set_gemm_hook(None)
        ops.set_attn_hook(None)
    # another geometry in one call
    oth = inputs(ctx.p, side=128, seed=7, C=2)
    forward(ctx, oth["concepts"], oth["concept_ids"], [request(2, n_img=64)], inp=[oth], trace=small)
    with pytest.raises(ValueError, match="geometry"):
        m.requery([tr, small], con.expand(2, -1, -1), con_ids.expand(2, -1, -1), [request(1), request(1, n_img=64)])
