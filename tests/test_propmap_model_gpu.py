"""Propagated concept maps through HipFluxDiT on the tiny geometry of tests/model_route_cases.py (hidden 256 = 2 heads, 8
text tokens, 16 x 16 image tokens, 2 double blocks, 3 concepts):

  (a) plumbing, teacher-forced: after an encode-path forward that captures the last double block, model.QKV still holds
      that block's rows; both spaces must equal weight x A^n map in fp64 inside the kernel's bound, with A from those very
      q / k image rows and map the layer's own concept map, read through a per-layer table (weight 1 onto zeros) in a
      second, otherwise identical forward -- for prop_steps 1 and 2, on the default route and under
      capture_independent_image;
  (b) semantics, against an independent statement: layer 0's rotated image q and k restated from the model's inputs in
      fp32 with the oracle's primitives (tests/test_tokmap_model_gpu.restate_layer0), in the two-gate form of that file;
  (c) B = 3 gives every item the bits of its single forward;
  (d) asking for propagated maps leaves the latent and every other map bit for bit;
  (e) without a request the ops calls of a forward are what they are with one, less the ops.propagate_maps calls;
  (f) the refusals, each before anything is launched.
"""
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import model_route_cases as M  # noqa: E402
import propmap_cases as P  # noqa: E402
import test_model_routes_gpu as TM  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from conceptattention_amd.flux_dit import Q_OUT_SCALE, HeatmapRequest, _Geom  # noqa: E402
from test_tokmap_model_gpu import restate_layer0  # noqa: E402

DEV = TM.DEV
MARGIN = 1.5        # (b): the margin of tests/test_tokmap_model_gpu.py over what the route's rounding points cost


def case_of(B, layers, **settings):
    tag = "_".join(f"{k}{v}" for k, v in settings.items())
    return M.Case(f"propmap_b{B}_l{'.'.join(map(str, layers))}{tag}", B=B, return_vectors=False, layers=tuple(layers),
                  settings=settings)


def requests(case, weight, spaces=("output", "cross"), steps=1, tables=False, others=False, B=None):
    """One request per item: the concept maps of both spaces, the propagated maps of ``spaces``; ``tables``: per-layer
    tables (weight 1) in place of the propagated maps; ``others``: token and query maps as well."""
    reqs = []
    nl = len(case.layers)
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    for _ in range(case.B if B is None else B):
        kw = {}
        if tables:
            kw.update(per_layer_out=z(nl, case.C, case.L), per_layer_cross=z(nl, case.C, case.L), per_layer_weight=1.0)
        else:
            if "output" in spaces:
                kw["prop_out"] = z(case.C, case.L)
            if "cross" in spaces:
                kw["prop_cross"] = z(case.C, case.L)
            kw["prop_steps"] = steps
        if others:
            kw.update(token_space=z(5, case.L), token_query_space=z(5, case.L), concept_query_space=z(case.C, case.L))
        reqs.append(HeatmapRequest(tuple(case.layers), weight, z(case.C, case.L), z(case.C, case.L), **kw))
    return reqs


def run_model(m, case, reqs, stop, items=None, return_vectors=False, concepts=None):
    items = [TM.dev_item(case, j) for j in (range(case.B) if items is None else items)]
    cat = lambda k: torch.cat([it[k] for it in items], 0)  # noqa: E731
    con, con_ids = cat("concepts"), cat("concept_ids")
    if concepts is not None:
        con, con_ids = con[:, :concepts], con_ids[:, :concepts]
    pred, _ = m(img=cat("img"), img_ids=cat("img_ids"), txt=cat("txt"), txt_ids=cat("txt_ids"), concepts=con,
                concept_ids=con_ids, concept_vec=cat("concept_vec"), y=cat("vec"),
                timesteps=torch.tensor([it["t"] for it in items], device=DEV), guidance=None,
                stop_after_multimodal_attentions=stop, return_vectors=return_vectors, heatmaps=reqs)
    torch.cuda.synchronize()
    return pred


def propagate_fp64(q, k, v, steps):
    """(A^steps v, its bound) in fp64: every step's own bound, and the earlier steps' carried through A (row-stochastic)."""
    out, bound = v.double(), torch.zeros_like(v, dtype=torch.float64)
    for _ in range(steps):
        carried, _ = P.reference_qkv(q, k, bound, 0, 1.0)
        out, own = P.reference_qkv(q, k, out, 0, 1.0)
        bound = own + carried
    return out, bound


@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("indep", [False, True], ids=["default-route", "capture_independent_image"])
def test_a_both_spaces_are_the_reference_of_the_rows_the_layer_left_in_qkv(indep, steps):
    case = case_of(2, (1,), **({"capture_independent_image": True} if indep else {}))
    m = TM.build(case)
    assert m.capture_independent_image == indep
    w = 0.75
    tabs = requests(case, w, tables=True)
    run_model(m, case, tabs, stop=True)
    reqs = requests(case, w, steps=steps)
    assert run_model(m, case, reqs, stop=True) is None
    route = m._layer_route(1, case.C, False, reqs)
    f16 = bool(route.qk16)
    assert bool(route.indep) == indep
    g = _Geom(case.B, case.C, case.T, case.L)
    H, NH = m.hidden_size, m.params.num_heads
    bits = m.QKV.view(torch.int16).cpu()
    for j in range(case.B):
        ij = slice(g.oI + j * g.L, g.oI + (j + 1) * g.L)
        q = P.from_bits(bits[ij, :H], f16).reshape(g.L, NH, 128)
        k = P.from_bits(bits[ij, H:2 * H], f16).reshape(g.L, NH, 128)
        assert torch.equal(tabs[j].out_space, reqs[j].out_space) and torch.equal(tabs[j].cross_space, reqs[j].cross_space)
        for space, got, table in (("output", reqs[j].prop_out, tabs[j].per_layer_out), ("cross", reqs[j].prop_cross, tabs[j].per_layer_cross)):
            layer_map = table[0].cpu()                          # fma(1, map, 0): the layer's own map, bit for bit
            assert float(layer_map.min()) >= 0 and float(layer_map.max()) > 0
            out, bound = propagate_fp64(q, k, layer_map, steps)
            zero = torch.zeros_like(out)
            worst, n_over = P.over_the_bound(got, w * out, P.acc_bound(w, zero, out, bound))
            print(f"\n  item {j} {space} ({steps} steps, {'half' if f16 else 'bf16'} rows): max err / bound = {worst:.3f}")
            assert n_over == 0, (j, space, worst, n_over)
            # (the propagation moves the map: it is not the map itself)
            assert float((got.cpu().double() - w * layer_map.double()).abs().max()) > 1e2 * float(bound.max())


def test_b_layer_0_against_the_restatement_from_the_inputs():
    """A of layer 0 restated from the model's inputs; the map it is applied to is the model's own layer map (a per-layer
    table of a second forward).  Gate 1, the binding one: the model lies within 1.5 x the storage rounding's error of the
    restatement that rounds where the route rounds (q and k to the storage type, k projected from the bf16 GEMM operand).
    Gate 2: within 1.5 x that restatement's own distance from the plain fp32 restatement, around the plain one -- both
    figures come from the restatements, none from the code under test."""
    case = case_of(1, (0,))
    m = TM.build(case)
    tabs = requests(case, 1.0, tables=True)
    run_model(m, case, tabs, stop=True)
    reqs = requests(case, 1.0)
    run_model(m, case, reqs, stop=True)
    f16 = bool(m._layer_route(0, case.C, False, reqs).qk16)
    store = torch.float16 if f16 else torch.bfloat16
    scale = torch.tensor(Q_OUT_SCALE, dtype=torch.float32)
    with torch.no_grad():
        q, k = restate_layer0(case, 0)
        q2, k2 = restate_layer0(case, 0, bf16_operand=True)
    q, k, q2, k2 = (x.permute(1, 0, 2) for x in (q, k[:, case.T:], q2, k2[:, case.T:]))
    for space, got, table in (("output", reqs[0].prop_out, tabs[0].per_layer_out), ("cross", reqs[0].prop_cross, tabs[0].per_layer_cross)):
        v = table[0].cpu()
        plain, _ = P.reference_qkv(q, k, v, 0, P.LOG2E / math.sqrt(128.0))
        stored, _ = P.reference_qkv((q * scale).to(store), k.to(store), v, 0, 1.0)
        routed, _ = P.reference_qkv((q2 * scale).to(store), k2.to(store), v, 0, 1.0)
        err_round = float((stored - plain).abs().max())
        err_routed = float((routed - plain).abs().max())
        got64 = got.double().cpu()
        d_routed, d_plain = float((got64 - routed).abs().max()), float((got64 - plain).abs().max())
        print(f"\n  layer 0 {space}, {'half' if f16 else 'bf16'} rows: |model - routed restatement| {d_routed:.3e} "
              f"(storage rounding {err_round:.3e}, ratio {d_routed / err_round:.2f}, gate {MARGIN}); |model - plain "
              f"restatement| {d_plain:.3e} (routed restatement - plain {err_routed:.3e}, ratio {d_plain / err_routed:.2f}, "
              f"gate {MARGIN}); restatements' ratio {err_routed / err_round:.2f}; largest cell {float(plain.max()):.3e}")
        assert err_round > 0 and err_routed > 0
        assert d_routed <= MARGIN * err_round, "the model against the restatement that rounds where it rounds"
        assert d_plain <= MARGIN * err_routed, "the model against the plain fp32 restatement"


def test_c_three_items_have_the_bits_of_their_single_forwards():
    case = case_of(3, (0, 1))
    reqs = requests(case, 0.5, steps=2)
    run_model(TM.build(case), case, reqs, stop=True)
    solo_case = case_of(1, (0, 1))
    m1 = TM.build(solo_case)
    for j in range(3):
        solo = requests(solo_case, 0.5, steps=2)
        run_model(m1, solo_case, solo, stop=True, items=[j])
        for f in ("prop_out", "prop_cross", "out_space", "cross_space"):
            assert torch.equal(getattr(solo[0], f), getattr(reqs[j], f)), (j, f)
        assert float(reqs[j].prop_out.min()) > 0


def test_d_propagated_maps_leave_the_latent_and_every_other_map_bit_for_bit():
    case = case_of(2, (0, 1))
    m = TM.build(case)
    w = 1.0 / len(case.layers)
    without = requests(case, w, spaces=(), others=True)
    with_ = requests(case, w, others=True, steps=3)
    p0 = run_model(m, case, without, stop=False)
    p1 = run_model(m, case, with_, stop=False)
    assert torch.equal(p0, p1)
    for a, b in zip(without, with_):
        for f in ("out_space", "cross_space", "token_space", "token_query_space", "concept_query_space"):
            assert torch.equal(getattr(a, f), getattr(b, f)) and float(getattr(b, f).abs().max()) > 0, f
        assert a.prop_out is None and a.prop_cross is None
        assert float(b.prop_out.min()) > 0 and float(b.prop_cross.min()) > 0
        # the concept maps are a softmax over the concepts and A is row-stochastic: so are the propagated ones
        for prop, space in ((b.prop_out, b.out_space), (b.prop_cross, b.cross_space)):
            assert torch.allclose(prop.sum(0), space.sum(0), rtol=1e-5, atol=0)


def test_e_without_a_request_the_launch_sequence_is_unchanged(monkeypatch):
    case = case_of(2, (0, 1))
    m = TM.build(case)
    calls = []
    for name, fn in list(vars(ops).items()):
        if isinstance(fn, types.FunctionType) and not name.startswith("_") and fn.__module__ == ops.__name__:
            def hook(*a, __fn=fn, __name=name, **k):
                calls.append((__name, len(a[0]) if a and isinstance(a[0], (list, tuple)) else None))
                return __fn(*a, **k)
            monkeypatch.setattr(ops, name, hook)
    run_model(m, case, requests(case, 0.5, spaces=(), others=True), stop=False)
    plain, calls[:] = list(calls), []
    run_model(m, case, requests(case, 0.5, others=True, steps=2), stop=False)
    asked, calls[:] = list(calls), []
    names = [n for n, _ in plain]
    assert "propagate_maps" not in names and "propagate_maps_workspace_bytes" not in names
    assert "token_maps" in names and "gemm" in names and "attention" in names and "query_maps" in names
    mine = ("propagate_maps", "propagate_maps_workspace_bytes")
    assert [c for c in asked if c[0] not in mine] == plain
    # per captured layer one call per step: 2 items x 2 spaces = 4 problems each
    assert [c for c in asked if c[0] == "propagate_maps"] == [("propagate_maps", 4)] * (2 * len(case.layers))
    run_model(m, case, requests(case, 0.5, spaces=("cross",)), stop=False)
    assert [c for c in calls if c[0] == "propagate_maps"] == [("propagate_maps", 2)] * len(case.layers)


def test_f_the_refusals_fire_before_anything_is_launched():
    case = case_of(2, (0, 1))
    m = TM.build(case)
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731

    def refused(reqs, match, **kw):
        with pytest.raises(ValueError, match=match):
            run_model(m, case, reqs, stop=True, **kw)
        for r in reqs:
            for t in (r.out_space, r.cross_space, r.prop_out, r.prop_cross):
                assert t is None or not bool(t.any()), "something was launched"
    for steps in (0, 5, 1.0):
        refused(requests(case, 0.5, steps=steps), "prop_steps")
    table = requests(case, 0.5, spaces=("output",))
    table[1].per_layer_out = z(2, case.C, case.L)
    refused(table, "the output space also has a per-layer table")
    other = requests(case, 0.5, spaces=("output",))          # (the OTHER space's table is no obstacle)
    for r in other:
        r.per_layer_cross = z(2, case.C, case.L)
    run_model(m, case, other, stop=True)
    assert float(other[0].prop_out.min()) > 0 and float(other[0].per_layer_cross.min()) > 0
    missing = requests(case, 0.5, spaces=("cross",))
    missing[0].cross_space = None
    refused(missing, "the cross space's concept maps are not computed")
    shape = requests(case, 0.5, spaces=("output",))
    shape[0].prop_out = z(case.C + 1, case.L)
    refused(shape, "prop_out must be contiguous fp32")
    refused(requests(case, 0.5), "return_vectors=False", return_vectors=True)
    none = [HeatmapRequest(tuple(case.layers), 0.5, z(0, case.L), z(0, case.L), prop_out=z(0, case.L)) for _ in range(2)]
    refused(none, "0 concepts", concepts=0)
