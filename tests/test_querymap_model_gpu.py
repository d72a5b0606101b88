"""Query-row maps through HipFluxDiT on the tiny geometry of tests/model_route_cases.py (hidden 256 = 2 heads, 8 text
tokens, 16 x 16 image tokens, 2 double blocks, 3 concepts):

  (a) plumbing, teacher-forced: after an encode-path forward that captures the last double block, model.QKV still holds
      that block's rows; both kinds must equal the fp64 reference of those very rows inside the kernel's bound, per item,
      with different n_tok per item -- the text rows against [text | image], the concept rows against [concept | image] --
      on the default route and under capture_independent_image;
  (b) B = 3 gives every item the bits of its single forward;
  (c) asking for query maps leaves the latent, the concept maps and the token maps bit for bit;
  (d) without a request the ops calls of a forward are what they are with one, less the ops.query_maps calls: one per
      captured layer for all items and both kinds;
  (e) the per-layer rows sum, with their weights, to the accumulator; the refusals.
"""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import model_route_cases as M  # noqa: E402
import querymap_cases as Q  # noqa: E402
import test_model_routes_gpu as TM  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from conceptattention_amd.flux_dit import HeatmapRequest, _Geom  # noqa: E402

DEV = TM.DEV


def case_of(B, layers, **settings):
    tag = "_".join(f"{k}{v}" for k, v in settings.items())
    return M.Case(f"querymap_b{B}_l{'.'.join(map(str, layers))}{tag}", B=B, return_vectors=False, layers=tuple(layers),
                  settings=settings)


def requests(case, n_toks, weight, per_layer_weight=1.0, kinds=("tokens", "concepts"), token_maps=False, concept_maps=True):
    reqs = []
    nl = len(case.layers)
    for n_tok in n_toks:
        z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
        kw = {}
        if "tokens" in kinds:
            kw.update(token_query_space=z(n_tok, case.L), per_layer_token_query=z(nl, n_tok, case.L))
        if "concepts" in kinds:
            kw.update(concept_query_space=z(case.C, case.L), per_layer_concept_query=z(nl, case.C, case.L))
        if token_maps:
            kw.update(token_space=z(n_tok, case.L))
        reqs.append(HeatmapRequest(tuple(case.layers), weight, z(case.C, case.L) if concept_maps else None,
                                   z(case.C, case.L) if concept_maps else None, per_layer_weight=per_layer_weight, **kw))
    return reqs


def run_model(m, case, reqs, stop, items=None, jak=None):
    items = [TM.dev_item(case, j) for j in (range(case.B) if items is None else items)]
    cat = lambda k: torch.cat([it[k] for it in items], 0)  # noqa: E731
    pred, _ = m(img=cat("img"), img_ids=cat("img_ids"), txt=cat("txt"), txt_ids=cat("txt_ids"), concepts=cat("concepts"),
                concept_ids=cat("concept_ids"), concept_vec=cat("concept_vec"), y=cat("vec"),
                timesteps=torch.tensor([it["t"] for it in items], device=DEV), guidance=None,
                stop_after_multimodal_attentions=stop, joint_attention_kwargs=jak, return_vectors=False, heatmaps=reqs)
    torch.cuda.synchronize()
    return pred


@pytest.mark.parametrize("indep", [False, True], ids=["default-route", "capture_independent_image"])
def test_a_both_kinds_are_the_reference_of_the_rows_the_layer_left_in_qkv(indep):
    case = case_of(2, (1,), **({"capture_independent_image": True} if indep else {}))
    m = TM.build(case)
    assert m.capture_independent_image == indep
    n_toks, w, plw = (8, 5), 0.75, 0.5
    reqs = requests(case, n_toks, w, plw)
    assert run_model(m, case, reqs, stop=True) is None
    route = m._layer_route(1, case.C, False, reqs)
    f16 = bool(route.qk16)
    assert bool(route.indep) == indep
    g = _Geom(case.B, case.C, case.T, case.L)
    H, NH = m.hidden_size, m.params.num_heads
    bits = m.QKV.view(torch.int16).cpu()
    for j, n_tok in enumerate(n_toks):
        cj = slice(j * g.C, (j + 1) * g.C)
        tj, ij = slice(g.oT + j * g.T, g.oT + (j + 1) * g.T), slice(g.oI + j * g.L, g.oI + (j + 1) * g.L)
        img_k = bits[ij, H:2 * H]
        for kind, qrows, lead, acc, table in (
                ("tokens", bits[tj, :H][:n_tok], bits[tj, H:2 * H], reqs[j].token_query_space, reqs[j].per_layer_token_query),
                ("concepts", bits[cj, :H], bits[cj, H:2 * H], reqs[j].concept_query_space, reqs[j].per_layer_concept_query)):
            q = Q.from_bits(qrows, f16).reshape(-1, NH, 128)
            k = Q.from_bits(torch.cat([lead, img_k]), f16).reshape(-1, NH, 128)
            maps, _, bound = Q.reference_qk(q, k, lead.shape[0], 1.0)
            zero = torch.zeros_like(maps)
            for name, got, weight in (("space", acc, w), ("per_layer", table[0], plw)):
                worst, n_over = Q.over_the_bound(got, weight * maps, Q.acc_bound(weight, zero, maps, bound.maps))
                print(f"\n  item {j} {kind} ({q.shape[0]} rows, {'half' if f16 else 'bf16'}) {name}: max err / bound = {worst:.3f}")
                assert n_over == 0, (j, kind, name, worst, n_over)
            assert float(maps.min()) > 0 and bool((maps.sum(1) < 1).all())     # (the leading keys take their share)


def test_b_three_items_have_the_bits_of_their_single_forwards():
    case = case_of(3, (0, 1))
    n_toks = (8, 3, 5)
    reqs = requests(case, n_toks, 0.5)
    run_model(TM.build(case), case, reqs, stop=True)
    solo_case = case_of(1, (0, 1))
    m1 = TM.build(solo_case)
    for j, n_tok in enumerate(n_toks):
        solo = requests(solo_case, (n_tok,), 0.5)
        run_model(m1, solo_case, solo, stop=True, items=[j])
        for f in ("token_query_space", "per_layer_token_query", "concept_query_space", "per_layer_concept_query", "out_space"):
            assert torch.equal(getattr(solo[0], f), getattr(reqs[j], f)), (j, f)
        assert float(reqs[j].token_query_space.min()) > 0


def test_c_query_maps_leave_the_latent_the_concept_maps_and_the_token_maps_bit_for_bit():
    case = case_of(2, (0, 1))
    m = TM.build(case)
    w = 1.0 / len(case.layers)
    without = requests(case, (8, 3), w, kinds=(), token_maps=True)
    with_ = requests(case, (8, 3), w, token_maps=True)
    p0 = run_model(m, case, without, stop=False)
    p1 = run_model(m, case, with_, stop=False)
    assert torch.equal(p0, p1)
    for a, b in zip(without, with_):
        assert torch.equal(a.out_space, b.out_space) and torch.equal(a.cross_space, b.cross_space)
        assert torch.equal(a.token_space, b.token_space) and float(b.token_space.abs().max()) > 0
        assert a.token_query_space is None and a.concept_query_space is None
        assert float(b.token_query_space.min()) > 0 and float(b.concept_query_space.min()) > 0


def test_d_without_a_request_the_launch_sequence_is_unchanged(monkeypatch):
    case = case_of(2, (0, 1))
    m = TM.build(case)
    calls = []
    for name, fn in list(vars(ops).items()):
        if isinstance(fn, types.FunctionType) and not name.startswith("_") and fn.__module__ == ops.__name__:
            def hook(*a, __fn=fn, __name=name, **k):
                calls.append((__name, len(a[0]) if a and isinstance(a[0], (list, tuple)) else None))
                return __fn(*a, **k)
            monkeypatch.setattr(ops, name, hook)
    run_model(m, case, requests(case, (8, 3), 0.5, kinds=(), token_maps=True), stop=False)
    plain, calls[:] = list(calls), []
    run_model(m, case, requests(case, (8, 3), 0.5, token_maps=True), stop=False)
    asked, calls[:] = list(calls), []
    names = [n for n, _ in plain]
    assert "query_maps" not in names and "query_maps_workspace_bytes" not in names
    assert "token_maps" in names and "gemm" in names and "attention" in names
    mine = ("query_maps", "query_maps_workspace_bytes")
    assert [c for c in asked if c[0] not in mine] == plain
    # one launch per captured layer: 2 items x 2 kinds = 4 problems each
    assert [c for c in asked if c[0] == "query_maps"] == [("query_maps", 4)] * len(case.layers)
    run_model(m, case, requests(case, (8, 3), 0.5, kinds=("concepts",)), stop=False)
    assert [c for c in calls if c[0] == "query_maps"] == [("query_maps", 2)] * len(case.layers)


def test_e_the_per_layer_rows_sum_to_the_accumulator_and_the_refusals():
    case = case_of(2, (0, 1))
    m = TM.build(case)
    reqs = requests(case, (8, 3), 0.5, per_layer_weight=1.0, concept_maps=False)
    run_model(m, case, reqs, stop=True)
    for r in reqs:
        for acc, table in ((r.token_query_space, r.per_layer_token_query), (r.concept_query_space, r.per_layer_concept_query)):
            t = table.double()                              # rows: the maps themselves (weight 1 onto zeros)
            assert torch.equal((0.5 * t[0] + 0.5 * t[1]).float(), acc), "the accumulator != sum of weight x rows"
            assert float(t.min()) > 0
    # two requests that share an accumulator: a new launch, not a race -- item 1 adds to item 0's concept accumulator
    shared = requests(case, (8, 3), 0.5, kinds=("concepts",), concept_maps=False)
    shared[1].concept_query_space = shared[0].concept_query_space
    run_model(m, case, shared, stop=True)
    want = (reqs[0].concept_query_space.double() + reqs[1].concept_query_space.double()).float()
    assert torch.allclose(shared[0].concept_query_space, want, rtol=1e-6, atol=0)
    # the ablations change the concept rows' key set: refused before anything is launched; the text rows' maps are not
    for jak in ({"concept_cross_attention": False}, {"concept_self_attention": False}):
        fresh = requests(case, (8, 3), 0.5)
        with pytest.raises(ValueError, match="query maps: the ablation joint_attention_kwargs"):
            run_model(m, case, fresh, stop=True, jak=jak)
        assert not bool(fresh[0].token_query_space.any()) and not bool(fresh[0].out_space.any())
        tokens_only = requests(case, (8, 3), 0.5, kinds=("tokens",))
        run_model(m, case, tokens_only, stop=True, jak=jak)
        assert torch.equal(tokens_only[0].token_query_space, reqs[0].token_query_space)
