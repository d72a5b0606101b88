"""Per-head concept maps through HipFluxDiT on the tiny geometry of tests/model_route_cases.py (hidden 256 = 2 heads, 8
text tokens, 16 x 16 image tokens, 2 double blocks):

  (a) plumbing, teacher-forced: after an encode-path forward that captures the last double block, the model's QKV, ATT32,
      ATTI32 and QPRE still hold that block's rows; all three spaces' heads_* and raw_* must equal the fp64 reference of
      those very rows inside the kernel's bound (tests/headmap_cases.py), per item and norm;
  (b) semantics, against the fp32 oracle: the head-resolved "output" and "cross" maps of oracle/flux_oracle.py's dict
      vectors reshaped per head; the gate is 1.5 x the error that rounding the oracle's vectors to bf16 produces in the
      same maps (printed; the comment above test_b says why bf16 and what was measured on the device);
  (c) bit for bit: latent and image rows with head maps equal the call without; the cross-space concept maps are
      unchanged; the output-space concept maps are unchanged when only "cross" / "value" are asked; B = 3 items per
      forward equal their single-item calls, head maps included;
  (d) the shift of the output-space concept maps when "output" is asked is measured and printed, and held to the
      summation-order bound of the two routes;
  (e) the refusals are ValueErrors, and no request means no launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import headmap_cases as H  # noqa: E402
import model_route_cases as M  # noqa: E402
import test_model_routes_gpu as TM  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from conceptattention_amd.flux_dit import HeatmapRequest, StepTrace, _Geom  # noqa: E402

DEV = TM.DEV
SPACES = ("output", "cross", "value")
FIELDS = {"output": ("heads_out", "raw_out"), "cross": ("heads_cross", "raw_cross"), "value": ("heads_value", "raw_value")}
MARGIN = 1.5


def case_of(B, layers, **kw):
    return M.Case(f"headmap_b{B}_l{'.'.join(map(str, layers))}", B=B, return_vectors=False, layers=tuple(layers), **kw)


def requests(case, spaces, weight, head_norm=None, concept_maps=True, NH=2, normalize=False):
    reqs = []
    for _ in range(case.B):
        z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
        kw = {}
        for s in spaces:
            kw[FIELDS[s][0]], kw[FIELDS[s][1]] = z(NH, case.C, case.L), z(case.C, case.L)
        reqs.append(HeatmapRequest(tuple(case.layers), weight, z(case.C, case.L) if concept_maps else None,
                                   z(case.C, case.L) if concept_maps else None, head_norm=head_norm,
                                   head_normalize_concepts=normalize, **kw))
    return reqs


def run_model(m, case, reqs, stop, idx=None, **kw):
    items = [TM.dev_item(case, j) for j in (range(case.B) if idx is None else idx)]
    cat = lambda k: torch.cat([it[k] for it in items], 0)  # noqa: E731
    pred, _ = m(img=cat("img"), img_ids=cat("img_ids"), txt=cat("txt"), txt_ids=cat("txt_ids"), concepts=cat("concepts"),
                concept_ids=cat("concept_ids"), concept_vec=cat("concept_vec"), y=cat("vec"),
                timesteps=torch.tensor([it["t"] for it in items], device=DEV), guidance=None,
                stop_after_multimodal_attentions=stop, heatmaps=reqs, **{"return_vectors": False, **kw})
    torch.cuda.synchronize()
    return pred


def layer_rows(m, g, j, space):
    """(image rows, concept rows) of item j in the buffers the captured layer left behind, as the model hands them on."""
    H_ = m.hidden_size
    cj, ij = slice(j * g.C, (j + 1) * g.C), slice(g.oI + j * g.L, g.oI + (j + 1) * g.L)
    if space == "output":
        return m.ATTI32[j, g.T:], m.ATT32[cj]
    if space == "cross":
        return m.QPRE[ij], m.QPRE[cj]
    return m.QKV[ij, 2 * H_:], m.QKV[cj, 2 * H_:]


@pytest.mark.parametrize("norm", H.NORMS)
def test_a_the_maps_are_the_reference_of_the_rows_the_layer_left(norm):
    case = case_of(2, (1,))
    m = TM.build(case)
    w = 0.75
    NH = m.params.num_heads
    reqs = requests(case, SPACES, w, None if norm == "none" else L.NORMS[norm], NH=NH)
    assert run_model(m, case, reqs, stop=True) is None
    g = _Geom(case.B, case.C, case.T, case.L)
    for j in range(case.B):
        for space in SPACES:
            img, con = layer_rows(m, g, j, space)
            assert img.dtype == con.dtype == (torch.bfloat16 if space == "value" else torch.float32)
            z, S = H.head_logits(img, con, NH)
            e_z = H.Z_COEF * H.U * S
            wts, e_w = H.head_weights(z, e_z, norm)
            mean, e_mean = H.mean_and_bound(wts, e_w)
            heads, raw = (getattr(reqs[j], f) for f in FIELDS[space])
            for name, got, ref, e in (("heads", heads, wts, e_w), ("raw", raw, mean, e_mean)):
                o = w * ref                                     # (onto zeros: weight x map, one rounding of the product)
                ratio, n_over = H.excess(got, o, w * e + 2 * H.U * o.abs(), "f32")
                print(f"\n  item {j} {space} {norm} {name}: max err / bound = {ratio:.3f}")
                assert n_over == 0, (j, space, name, ratio)
            assert float(heads.abs().max()) > 0


def oracle_head_maps(case, d_o, layer, space, rounded):
    """fp64 [NH, C, L] logits per head from the oracle's dict vectors of ``layer`` (``rounded``: the vectors rounded to
    bf16 first, the storage of the activations the route forms them from)."""
    li = layer
    if space == "output":
        con, img = d_o["output_space_concept_vectors"][li, 0], d_o["output_space_image_vectors"][li, 0]   # [tokens, H]
    else:
        con = d_o["cross_attention_concept_vectors"][li, 0].permute(1, 0, 2).reshape(case.C, -1)         # [heads, C, 128]
        img = d_o["cross_attention_image_vectors"][li, 0].permute(1, 0, 2).reshape(case.L, -1)
    if rounded:
        con, img = M.bf(con.float()), M.bf(img.float())
    return H.head_logits(img.float(), con.float(), M.HIDDEN // 128)[0]


# The map vectors themselves are kept in fp32 on this route (ATT32 / ATTI32 / QPRE), so rounding the oracle's vectors to
# THAT storage changes nothing and a gate built on it would be zero.  The rounding that the route does make is bf16, on the
# activations these vectors are formed from (the GEMM operands, q / k / v in QKV, the dict's own dtype), so the reference
# error is that of the oracle's vectors rounded to bf16, and the gate is 1.5 x it.  Both figures are printed (pytest -s).
# Measured on MI355X: output |model - oracle| 1.708e-03 against 1.338e-03, ratio 1.28; cross 8.163e-05 against 2.042e-03,
# ratio 0.04: both inside the gate.
# (a) is the check that binds: it holds the launch to the very rows the layer wrote.
@pytest.mark.parametrize("space", ["output", "cross"])
def test_b_against_the_fp32_oracle(space):
    case = case_of(1, (1,))
    m = TM.build(case)
    NH = m.params.num_heads
    reqs = requests(case, (space,), 1.0, None, NH=NH)
    run_model(m, case, reqs, stop=True)
    _, d_o = TM.oracle({}, case, 0)
    ref = oracle_head_maps(case, d_o, 1, space, rounded=False)
    ref_r = oracle_head_maps(case, d_o, 1, space, rounded=True)
    got = getattr(reqs[0], FIELDS[space][0]).double().cpu()
    err_model, err_round = float((got - ref).abs().max()), float((ref_r - ref).abs().max())
    print(f"\n  {space}: |model - oracle| {err_model:.3e} on logits up to {float(ref.abs().max()):.3e}; |oracle vectors rounded "
          f"to bf16 - oracle| {err_round:.3e}; ratio {err_model / err_round:.2f} (gate {MARGIN})")
    assert err_round > 0
    assert err_model <= MARGIN * err_round, (space, err_model, err_round)


def test_c_head_maps_leave_everything_else_bit_for_bit():
    case = case_of(2, (0, 1))
    m = TM.build(case)
    w = 1.0 / len(case.layers)
    base = requests(case, (), w)
    p0 = run_model(m, case, base, stop=False)
    quiet = requests(case, ("cross", "value"), w, L.NORM_SOFTMAX)
    p1 = run_model(m, case, quiet, stop=False)
    every = requests(case, SPACES, w)
    p2 = run_model(m, case, every, stop=False)
    assert torch.equal(p0, p1) and torch.equal(p0, p2), "the prediction moved"
    for a, b, c in zip(base, quiet, every):
        assert torch.equal(a.cross_space, b.cross_space) and torch.equal(a.cross_space, c.cross_space)
        assert torch.equal(a.out_space, b.out_space), "cross / value head maps moved the output-space concept maps"
        assert float(b.heads_value.abs().max()) > 0 and float(c.heads_out.abs().max()) > 0
    assert m.epilogue_logits is True


def test_d_the_shift_of_the_output_space_concept_maps_when_output_is_asked():
    """Asking for "output" head maps moves the forward to the fp32 image rows' route (epilogue_logits = False for its
    duration), which sums a logit's products in another order than the attention epilogue's per-head partials.  Both
    orders lie within rowop_cases' logit bound 2 (dim / 64 + 6 + 1) U S of the exact logit of the same rows, and a
    softmax moves by at most twice its logits' shift: the gate is 2 x 2 x that bound, from the rows the layer left.
    Measured on MI355X: 1.788e-07 and 2.086e-07 for the two items (gates 1.653e-05 and 1.865e-05, maps up to 0.59)."""
    case = case_of(2, (1,))
    m = TM.build(case)
    base = requests(case, (), 1.0)
    run_model(m, case, base, stop=True)
    asked = requests(case, ("output",), 1.0)
    run_model(m, case, asked, stop=True)
    g = _Geom(case.B, case.C, case.T, case.L)
    for j, (a, b) in enumerate(zip(base, asked)):
        img, con = layer_rows(m, g, j, "output")
        S = con.double().abs() @ img.double().abs().T
        e_z = 2 * (m.hidden_size / 64 + 6 + 1) * H.U * float(S.max())
        shift = float((a.out_space - b.out_space).abs().max())
        print(f"\n  item {j}: output-space concept maps with head_maps 'output': max shift {shift:.3e} (gate {4 * e_z:.3e}, "
              f"maps up to {float(a.out_space.abs().max()):.3e})")
        assert shift <= 4 * e_z
        assert torch.equal(a.cross_space, b.cross_space)


def test_c_three_items_per_forward_equal_their_single_item_calls():
    case = case_of(3, (0, 1))
    m = TM.build(case)
    w = 0.5
    together = requests(case, SPACES, w, L.NORM_ENTMAX15)
    p = run_model(m, case, together, stop=False)
    one = case_of(1, (0, 1))
    for j in range(3):
        solo = requests(one, SPACES, w, L.NORM_ENTMAX15)
        pj = run_model(m, one, solo, stop=False, idx=[j])
        assert torch.equal(p[j], pj[0]), j
        for name in ("out_space", "cross_space") + tuple(f for s in SPACES for f in FIELDS[s]):
            assert torch.equal(getattr(together[j], name), getattr(solo[0], name)), (j, name)


def test_normalize_concepts_against_a_torch_restatement():
    from conceptattention_amd.heatmaps import linear_normalization
    case = case_of(1, (1,))
    m = TM.build(case)
    NH = m.params.num_heads
    reqs = requests(case, SPACES, 1.0, None, NH=NH, normalize=True)
    run_model(m, case, reqs, stop=True)
    g = _Geom(case.B, case.C, case.T, case.L)
    for space in SPACES:
        img, con = layer_rows(m, g, 0, space)
        con = linear_normalization(con.float(), dim=0)
        z, S = H.head_logits(img, con, NH)
        mean, e_mean = H.mean_and_bound(z, H.Z_COEF * H.U * S)
        ratio, n_over = H.excess(getattr(reqs[0], FIELDS[space][1]), mean, e_mean + 2 * H.U * mean.abs(), "f32")
        assert n_over == 0, (space, ratio)


def test_e_the_refusals_are_value_errors():
    case = case_of(1, (1,))
    m = TM.build(case)
    with pytest.raises(ValueError, match="head maps: .*return_vectors=False"):
        run_model(m, case, requests(case, ("cross",), 1.0), stop=True, return_vectors=True)
    with pytest.raises(ValueError, match="head maps: the ablation joint_attention_kwargs"):
        run_model(m, case, requests(case, ("value",), 1.0), stop=True,
                  joint_attention_kwargs={"concept_self_attention": False})
    with pytest.raises(ValueError, match="head maps: head_norm"):
        run_model(m, case, requests(case, ("value",), 1.0, head_norm=L.NORM_NONE), stop=True)
    m.capture_independent_image = True
    try:
        with pytest.raises(ValueError, match="head maps: capture_independent_image=True"):
            run_model(m, case, requests(case, ("output",), 1.0), stop=True)
        run_model(m, case, requests(case, ("cross", "value"), 1.0), stop=True)        # (these two are covered)
    finally:
        m.capture_independent_image = False
    trace = StepTrace()
    reqs = requests(case, ("cross",), 1.0)
    run_model(m, case, reqs, stop=True, trace=trace)
    item = TM.dev_item(case, 0)
    with pytest.raises(ValueError, match="requery: per-head maps are not part of a re-query"):
        m.requery([trace], item["concepts"], item["concept_ids"], requests(case, ("cross",), 1.0))
    assert m.epilogue_logits is True


def test_no_head_request_means_no_launch(monkeypatch):
    case = case_of(2, (0, 1))
    m = TM.build(case)
    calls = []
    real = ops.head_maps
    monkeypatch.setattr(ops, "head_maps", lambda *a, **k: (calls.append(len(a[0])), real(*a, **k))[1])
    run_model(m, case, requests(case, (), 1.0), stop=True)
    assert calls == []
    run_model(m, case, requests(case, SPACES, 1.0), stop=True)
    assert calls == [6, 6]                                   # one launch per captured layer: 2 items x 3 spaces
