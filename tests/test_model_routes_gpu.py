"""Every model-level route of HipFluxDiT's forward on the tiny geometry (tests/model_route_cases.py), on the GPU:

  a. each case against the fp32 oracle (oracle/flux_oracle.py; fp8 cases against the bf16 run of the same case), with the
     tiny-model gates of tests/test_model_gpu.py, and the attention launches it makes against the table's count;
  b. every B = 3 case, item by item, bit-identical to B = 1 forwards;
  c. equivalences that are exact by construction;
  d. a forward after a change of route or shape on a live model equals the forward of a freshly built model;
  e. nothing but the requested accumulators and table rows is written.
"""
from dataclasses import dataclass, replace

import pytest
import torch

pytestmark = pytest.mark.gpu

import model_route_cases as M  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from conceptattention_amd.flux_dit import DICT_KEYS, FluxWeights, HeatmapRequest, HipFluxDiT, _Geom  # noqa: E402
from oracle import flux_oracle as O  # noqa: E402
from oracle import sparse_norms  # noqa: E402

DEV = "cuda:0"
SPACES = (("out_space", "output_space", M.OUT_MAP_GATE), ("cross_space", "cross_attention", M.CROSS_MAP_GATE))
_WEIGHTS, _DEV_ITEMS = {}, {}
WORST = {}   # route family -> (max err / gate, case, output) over the module, printed by the last (a) test


def maxabs(a, b):
    return (torch.as_tensor(a).float().cpu() - torch.as_tensor(b).float().cpu()).abs().max().item()


# ------------------------------------------------------------------------------------------------------- plumbing
def weights(case) -> FluxWeights:
    """Device weights per geometry, shared by the module's models (as replicas on other streams share them)."""
    key = (case.guidance_embed, case.singles)
    if key not in _WEIGHTS:
        w = FluxWeights(M.params(case), DEV)
        w.load_state_dict(M.state_dict(case))
        _WEIGHTS[key] = w
    return _WEIGHTS[key]


def configure(m, case):
    s = case.full_settings()
    m.set_precision(s["precision"], s["keep_bf16_layers"])
    for k in HipFluxDiT.ROUTE_SETTINGS:
        if k not in ("precision", "keep_bf16_layers"):
            setattr(m, k, s[k])
    return m


def build(case) -> HipFluxDiT:
    return configure(HipFluxDiT(M.params(case), DEV, weights=weights(case)), case)


def dev_item(case, j) -> dict:
    key = (case.C, case.T, case.side, j)
    if key not in _DEV_ITEMS:
        inp = M.item_inputs(case, j)
        d = {k: v.to(DEV) for k, v in inp.items() if torch.is_tensor(v)}
        d["img"] = O.patchify(inp["latent"]).to(DEV)
        _DEV_ITEMS[key] = d
    return dict(_DEV_ITEMS[key], t=M.ITEM_TIMESTEPS[j], guidance=M.ITEM_GUIDANCE[j])


@dataclass
class Out:
    pred: torch.Tensor
    vec: dict
    reqs: list
    x_txt: torch.Tensor      # final residual rows [B, T, H] / [B, L, H]
    x_img: torch.Tensor


def zero_requests(case, n):
    if case.layers is None:
        return None
    z = lambda: torch.zeros(case.C, case.L, device=DEV)  # noqa: E731
    return [HeatmapRequest(tuple(case.layers), 1.0 / len(case.layers), z(), z(), norm=case.norm) for _ in range(n)]


def forward(m, case, idx=None, items=None, reqs="zeros") -> Out:
    """One forward of ``case`` over its items (``idx``: a subset as its own batch; ``items``: other inputs)."""
    if items is None:
        items = [dev_item(case, j) for j in (range(case.B) if idx is None else idx)]
    B = len(items)
    cat = lambda k: torch.cat([it[k] for it in items], 0)  # noqa: E731
    if reqs == "zeros":
        reqs = zero_requests(case, B)
    C = items[0]["concepts"].shape[1]
    pred, d = m(img=cat("img"), img_ids=cat("img_ids"), txt=cat("txt"), txt_ids=cat("txt_ids"), concepts=cat("concepts"),
                concept_ids=cat("concept_ids"), concept_vec=cat("concept_vec"), y=cat("vec"),
                timesteps=torch.tensor([it["t"] for it in items], device=DEV),
                guidance=torch.tensor([it["guidance"] for it in items], device=DEV) if case.guidance_embed else None,
                joint_attention_kwargs=case.jak, return_vectors=case.return_vectors, heatmaps=reqs)
    g = _Geom(B, C, case.T, case.L)
    H = m.hidden_size
    out = Out(pred, d, reqs, m.X[g.oT:g.oI].view(B, case.T, H).clone(), m.X[g.oI:g.n].view(B, case.L, H).clone())
    torch.cuda.synchronize()
    return out


def assert_same(a: Out, b: Out, ja=None, jb=None, what=""):
    """Outputs of item ``ja`` of a and item ``jb`` of b (None: all items) are bit-identical."""
    pick = lambda t, j, dim=0: t if j is None else t.select(dim, j)  # noqa: E731
    assert a.pred.dtype == b.pred.dtype
    assert torch.equal(pick(a.pred, ja), pick(b.pred, jb)), f"{what}: pred"
    assert torch.equal(pick(a.x_txt, ja), pick(b.x_txt, jb)), f"{what}: final text rows"
    assert torch.equal(pick(a.x_img, ja), pick(b.x_img, jb)), f"{what}: final image rows"
    assert a.vec.keys() == b.vec.keys()
    for k in a.vec:
        assert torch.equal(pick(a.vec[k], ja, 1), pick(b.vec[k], jb, 1)), f"{what}: {k}"
    assert (a.reqs is None) == (b.reqs is None)
    if a.reqs is not None:
        ra = a.reqs if ja is None else [a.reqs[ja]]
        rb = b.reqs if jb is None else [b.reqs[jb]]
        assert len(ra) == len(rb)
        for x, y in zip(ra, rb):
            assert torch.equal(x.out_space, y.out_space), f"{what}: output-space accumulator"
            assert torch.equal(x.cross_space, y.cross_space), f"{what}: cross-space accumulator"


@pytest.fixture(scope="module")
def oracle_cache():
    return {}


def oracle(cache, case, j):
    """(pred, vector stacks) of the fp32 oracle for item j: computed once per (inputs, ablation), never modified."""
    key = M.oracle_key(case, j)
    if key not in cache:
        inp = M.item_inputs(case, j)
        with torch.no_grad():
            cache[key] = O.dit_forward(
                M.state_dict(case), M.params(case), O.patchify(inp["latent"]), inp["img_ids"], inp["txt"], inp["txt_ids"],
                inp["concepts"], inp["concept_ids"], inp["concept_vec"], torch.tensor([inp["t"]]), inp["vec"],
                None if inp["guidance"] is None else torch.tensor([inp["guidance"]]), joint_attention_kwargs=case.jak)
    return cache[key]


def reference_maps(case, d_o, space) -> torch.Tensor:
    """[C, L] mean over the case's layers of norm-over-concepts(logits) from the oracle's vectors."""
    img, con = d_o[f"{space}_image_vectors"][None], d_o[f"{space}_concept_vectors"][None]
    if case.norm == L.NORM_SOFTMAX:
        return O.compute_heatmaps(img, con, list(case.layers), [0]).reshape(case.C, case.L)
    fn = {L.NORM_SPARSEMAX: sparse_norms.sparsemax, L.NORM_ENTMAX15: sparse_norms.entmax15}[case.norm]
    logits = O.heatmap_logits(img, con)[0, list(case.layers), 0]          # [layers, C, patches]
    return torch.from_numpy(fn(logits.double().numpy(), axis=1).mean(0)).float()


def family(case) -> str:
    r = M.route_of(case, M.captured_layer(case))
    if case.fp8:
        return "fp8 (vs bf16 run)"
    if r.indep:
        return "indep"
    if not r.split:
        return "bf16 residual"
    if case.layers is None:
        return "vectors only"
    return "use_part" if r.use_part else ("f32img, C = 9" if case.C == 9 else "f32img")


def note(case, name, err, gate):
    r = err / gate
    print(f"  {case.name:44s} {name:34s} max err {err:.3e} / gate {gate:.3e} = {r:.3f}")
    f = family(case)
    if r > WORST.get(f, (0,))[0]:
        WORST[f] = (r, case.name, name)
    return r


# ------------------------------------------------------------------------------------ a. against the oracle
@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_case_against_the_oracle(case, oracle_cache, monkeypatch):
    launches = []
    real = ops.attention
    monkeypatch.setattr(ops, "attention", lambda probs, *a, **k: (launches.append(len(probs)), real(probs, *a, **k))[1])
    out = forward(build(case), case)
    monkeypatch.undo()
    assert launches == M.expected_attention_launches(case), (launches, [M.route_of(case, i) for i in range(M.DEPTH)])
    B, C, Li, H = case.B, case.C, case.L, M.HIDDEN
    assert out.pred.shape == (B, Li, 64)
    assert out.pred.dtype == case.full_settings()["residual_dtype"]
    assert set(out.vec) == (set(DICT_KEYS) if case.return_vectors else set())
    if case.return_vectors:
        assert out.vec["output_space_concept_vectors"].shape == (M.DEPTH, B, C, H)
        assert out.vec["output_space_image_vectors"].shape == (M.DEPTH, B, Li, H)
        assert out.vec["cross_attention_concept_vectors"].shape == (M.DEPTH, B, 2, C, 128)
        assert out.vec["cross_attention_image_vectors"].shape == (M.DEPTH, B, 2, Li, 128)
    print(f"\n[measured] {case.name}: {' | '.join(str(M.route_of(case, i)) for i in range(M.DEPTH))}")
    ratios = []
    if case.fp8:
        # no oracle for e4m3 operands: the bf16 run of the same case, the gates of test_tiny_model_fp8_mode_tracks_bf16
        twin = case.bf16_twin()
        ref = forward(build(twin), twin)
        for j in range(B):
            a, b = out.pred[j].float(), ref.pred[j].float()
            rel = ((a - b).norm() / b.norm()).item()
            assert rel > 0, "the fp8 route computed the bf16 result: it did not run"
            ratios.append(note(case, f"item {j} pred rel-rms vs bf16", rel, M.FP8_PRED_REL_RMS))
            for attr, _, _ in SPACES if case.layers is not None else ():
                e = maxabs(getattr(out.reqs[j], attr), getattr(ref.reqs[j], attr))
                ratios.append(note(case, f"item {j} {attr} vs bf16", e, M.FP8_MAP_GATE))
        for k in out.vec:
            assert out.vec[k].shape == ref.vec[k].shape and out.vec[k].dtype == ref.vec[k].dtype
            assert torch.isfinite(out.vec[k].float()).all(), k
    else:
        for j in range(B):
            pred_o, d_o = oracle(oracle_cache, case, j)
            gate = M.PRED_GATE * max(pred_o.abs().max().item(), 1.0)
            ratios.append(note(case, f"item {j} pred", maxabs(out.pred[j], pred_o[0]), gate))
            for k in out.vec:
                gate = M.VEC_GATE * max(d_o[k].abs().max().item(), 1.0)
                ratios.append(note(case, f"item {j} {k}", maxabs(out.vec[k][:, j], d_o[k][:, 0]), gate))
            for attr, space, gate in SPACES if case.layers is not None else ():
                acc = getattr(out.reqs[j], attr)
                ratios.append(note(case, f"item {j} {attr}", maxabs(acc, reference_maps(case, d_o, space)), gate))
                assert abs(acc.sum(0) - 1).max().item() < 1e-5, (attr, "the weights over the concepts sum to 1")
    assert max(ratios) < 1, f"{case.name}: max err / gate {max(ratios):.3f}"
    if case is M.CASES[-1]:
        print("\n[measured] largest max err / gate per route family:")
        for f, (r, name, what) in sorted(WORST.items()):
            print(f"  {f:22s} {r:.3f}  ({name}: {what})")


# ------------------------------------------------------------------------------------ b. batch invariance
@pytest.mark.parametrize("case", [c for c in M.CASES if c.B > 1], ids=lambda c: c.name)
def test_batched_case_is_bit_identical_to_one_item_at_a_time(case):
    batched = forward(build(case), case)
    m1 = build(case)
    for j in range(case.B):
        assert_same(batched, forward(m1, case, idx=[j]), j, 0, f"{case.name} item {j}")


# ------------------------------------------------------------------------------------ c. exact equivalences
@pytest.mark.parametrize("name", ["noepi", "indep", "cover_bf16res_qkbf16_noepi", "noepi_b3", "noepi_entmax15_c8"])
def test_fused_and_three_launch_heat_maps_are_the_same_bits(name):
    """fused_heatmaps True / False from the same fp32 rows (no partial logits from the attention epilogue, whose
    summation order is another: epilogue_logits = False, or capture_independent_image): ca_heatmap_fused is
    heatmap_logits + heatmap_softmax_accumulate per problem."""
    case = M.BY_NAME[name]
    assert not M.route_of(case, 1).use_part and M.route_of(case, 1).f32img
    assert case.full_settings()["fused_heatmaps"]
    other = replace(case, name=name + "~unfused", settings=dict(case.settings, fused_heatmaps=False))
    assert M.route_of(other, 1) == M.route_of(case, 1)
    assert_same(forward(build(case), case), forward(build(other), other), what=name)


def test_fp8_mode_with_every_double_block_kept_is_the_bf16_forward():
    a = replace(M.BY_NAME["default"], name="default~singles0", singles=0)
    b = replace(a, name="fp8~keepall", settings=dict(precision="fp8", keep_bf16_layers=frozenset(range(M.DEPTH))))
    assert not any(M.route_of(b, i).fp8 for i in range(M.DEPTH))
    assert_same(forward(build(a), a), forward(build(b), b), what="fp8 with all double blocks kept vs bf16")


@pytest.mark.parametrize("name", ["indep", "indep_qkall", "indep_c9", "indep_s208", "indep_b3", "fp8_fp8qkv_indepoff"])
def test_independent_capture_returns_the_same_latent_for_every_captured_set(name):
    """capture_independent_image: pred and the final text / image rows do not depend on which layers' maps are asked
    for (the tiny version of test_full_depth_gpu's independence test), and a layer's maps not on the other layers.
    In fp8 mode this holds with fp8_bf16_qkv_when_captured = False only: otherwise a captured layer's qkv projection
    runs in another number format than an uncaptured layer's, and k and v feed the image rows (the case indep_fp8 is
    therefore held to the oracle-side gates alone)."""
    base = replace(M.BY_NAME[name], return_vectors=False)
    outs = {}
    for layers in (None, (1,), (0, 1)):
        case = replace(base, layers=layers)
        m = build(case)
        if layers is None:   # a forward that returns pred alone
            outs[layers] = forward(m, replace(case, return_vectors=False), reqs=None)
        else:
            reqs = [HeatmapRequest(layers, 1.0, None, None,
                                   per_layer_out=torch.zeros(len(layers), case.C, case.L, device=DEV),
                                   per_layer_cross=torch.zeros(len(layers), case.C, case.L, device=DEV))
                    for _ in range(case.B)]
            outs[layers] = forward(m, case, reqs=reqs)
    for layers in ((1,), (0, 1)):
        assert torch.equal(outs[layers].pred, outs[None].pred), layers
        assert torch.equal(outs[layers].x_txt, outs[None].x_txt) and torch.equal(outs[layers].x_img, outs[None].x_img)
    for a, b in zip(outs[(1,)].reqs, outs[(0, 1)].reqs):
        assert torch.equal(a.per_layer_out[0], b.per_layer_out[1])
        assert torch.equal(a.per_layer_cross[0], b.per_layer_cross[1])
        assert b.per_layer_out[0].abs().max() > 0 and a.per_layer_out[0].abs().max() > 0


ROUTE_SETTINGS_SEEN = {}   # the first case with each distinct set of settings -> the settings
for _c in M.CASES:
    if _c.settings not in ROUTE_SETTINGS_SEEN.values():
        ROUTE_SETTINGS_SEEN[_c.name] = _c.settings


@pytest.mark.parametrize("settings_of", list(ROUTE_SETTINGS_SEEN))
def test_image_and_text_rows_ignore_the_concepts(settings_of):
    """The concept stream only reads the image keys / values: under every route, pred, the final text and image rows
    and the image rows' vectors do not change by a bit when the concepts are permuted or their count changes (1, 3, 9:
    the count also moves the layer between the partial-logits and the fp32-rows route); permuting the concepts permutes
    their own vectors (the q rows exactly; the attention rows to one bf16 step: the key order differs)."""
    settings = ROUTE_SETTINGS_SEEN[settings_of]
    base = dev_item(M.Case("x", C=9), 0)
    perm = [2, 0, 1]
    outs = {}
    for tag, pick in (("c3", [0, 1, 2]), ("c3_perm", perm), ("c1", [4]), ("c9", list(range(9)))):
        case = M.Case(tag, dict(settings), C=len(pick))
        item = dict(base, concepts=base["concepts"][:, pick].contiguous(), concept_ids=base["concept_ids"][:, :len(pick)])
        outs[tag] = forward(build(case), case, items=[item])
    ref = outs["c3"]
    for tag in ("c3_perm", "c1", "c9"):
        o = outs[tag]
        assert torch.equal(o.pred, ref.pred), f"pred changed ({tag})"
        assert torch.equal(o.x_txt, ref.x_txt), f"text rows changed ({tag})"
        assert torch.equal(o.x_img, ref.x_img), f"image rows changed ({tag})"
        for k in ("output_space_image_vectors", "cross_attention_image_vectors"):
            assert torch.equal(o.vec[k], ref.vec[k]), f"{k} changed ({tag})"
    p = outs["c3_perm"]
    # layer 0: the concept rows enter it as the same values; later layers inherit the one-step differences
    assert torch.equal(p.vec["cross_attention_concept_vectors"][0], ref.vec["cross_attention_concept_vectors"][0][:, :, perm])
    a, b = p.vec["output_space_concept_vectors"][0].float(), ref.vec["output_space_concept_vectors"][0][:, perm].float()
    assert (a - b).abs().max().item() <= 2.0 ** -7 * max(b.abs().max().item(), 1.0)


# ------------------------------------------------------------------------------------ d. no state left behind
CHAINS = [
    ("indep", "default"), ("default", "indep"),
    ("fp8", "default"), ("default", "fp8"), ("indep_fp8", "indep"),
    ("c9", "default"), ("indep_c9", "indep"), ("default", "c9"),
    ("default", "s208", "default"), ("indep_s208", "indep", "indep_s208"), ("fp8", "fp8_s208", "fp8"),
    ("default_b3", "default"), ("indep_b3", "indep"), ("fp8_b3", "fp8"), ("default", "default_b3"),
    ("noepi", "default"), ("default", "noepi"), ("unfused", "indep"),
    ("bf16res", "default"), ("default", "bf16res"),
    ("vectorsonly", "mapsonly"), ("layer0only", "default"), ("qkall", "qkbf16"),
    ("default_neither", "indep_crossonly"), ("fp8_fp8qkv", "fp8"), ("fp8_keep1", "fp8_c9"),
    ("indep_sparsemax", "default"),
]


@pytest.mark.parametrize("chain", CHAINS, ids="->".join)
def test_forward_after_a_route_change_equals_a_fresh_model(chain):
    """One model instance runs the chain's cases in order, its settings switched between them as
    pipeline._stream_models does; the last forward returns the bits of the same case on a freshly built model."""
    cases = [M.BY_NAME[n] for n in chain]
    assert all(a != b for a, b in zip(cases, cases[1:]))
    assert len({(c.guidance_embed, c.singles) for c in cases}) == 1, "one model: one geometry"
    m = build(cases[0])
    for c in cases:
        out = forward(configure(m, c), c)
    assert_same(out, forward(build(cases[-1]), cases[-1]), what="->".join(chain))


# ------------------------------------------------------------------------------------ e. nothing else written
def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("name", ["default", "noepi", "unfused", "indep", "c9", "fp8", "indep_fp8", "bf16res"])
def test_only_the_requested_accumulators_and_table_rows_are_written(name):
    """Three items with three different requests in one forward: item 0 layers (0, 1) with both accumulators and both
    per-layer tables; item 1 layer 1 and a table row for a layer that does not exist, no cross-space accumulator; item 2
    names no layer of the model.  Every accumulator lies between guard rows.  Requested tensors start from a known
    pattern, the others and the guards from NaN."""
    base = replace(M.BY_NAME[name], B=3, return_vectors=False)
    C, Li = base.C, base.L
    pattern = (1.0 + (torch.arange(C * Li, device=DEV) % 7) / 8).view(C, Li)

    def guarded(fill, rows=C):
        buf = torch.full((rows + 2, Li), float("nan"), device=DEV)
        if fill is not None:
            buf[1:-1] = fill
        return buf

    def requests(items):
        bufs, reqs = {}, []
        for j in items:
            b = {k: guarded(pattern if j < 2 else None) for k in ("out", "cross")}
            b["t_out"] = guarded(pattern.repeat(2, 1) if j == 0 else None, 2 * C)
            b["t_cross"] = guarded(pattern.repeat(2, 1) if j == 0 else None, 2 * C)
            if j == 1:
                b["t_out"][1:1 + C] = pattern
            layers = ((0, 1), (1, 7), (7, 8))[j]
            reqs.append(HeatmapRequest(layers, 0.5 if j == 0 else 1.0, b["out"][1:-1], None if j == 1 else b["cross"][1:-1],
                                       per_layer_out=b["t_out"][1:-1].view(2, C, Li),
                                       per_layer_cross=None if j == 1 else b["t_cross"][1:-1].view(2, C, Li),
                                       per_layer_weight=0.25))
            bufs[j] = b
        return bufs, reqs

    before, _ = requests(range(3))
    bufs, reqs = requests(range(3))
    m1 = build(base)
    forward(m1, base, reqs=reqs)
    for j in range(3):
        for k, t in bufs[j].items():   # guard rows, whoever owns them
            assert torch.equal(_bits(t[0]), _bits(before[j][k][0])) and torch.equal(_bits(t[-1]), _bits(before[j][k][-1])), (j, k)
    for k, t in bufs[2].items():       # item 2: no layer of its request ran
        assert torch.equal(_bits(t), _bits(before[2][k])), k
    assert torch.equal(_bits(bufs[1]["cross"]), _bits(before[1]["cross"]))          # not part of item 1's request
    assert torch.equal(_bits(bufs[1]["t_cross"]), _bits(before[1]["t_cross"]))
    assert torch.equal(_bits(bufs[1]["t_out"][1 + C:]), _bits(before[1]["t_out"][1 + C:]))   # the row of layer 7
    # what was requested: the pattern plus the maps of a zero-filled run that asks every item for both layers (the same
    # captured layers, so the same residual stream; weights are powers of two, so w * p scales exactly)
    z = lambda *shape: torch.zeros(*shape, device=DEV)  # noqa: E731
    full = [HeatmapRequest((0, 1), 0.5, z(C, Li), z(C, Li), per_layer_out=z(2, C, Li), per_layer_cross=z(2, C, Li),
                           per_layer_weight=0.25) for _ in range(3)]
    forward(m1, base, reqs=full)
    # a rounding of pattern + w * p at |value| < 4 per layer (half an ulp of 2^-22 each, two layers at the most) where
    # the zero-filled run rounds at |w * p| <= 1
    tol = 2.0 ** -21
    close = lambda got, want: (got - want).abs().max().item() <= tol  # noqa: E731
    for f in full:
        assert abs(f.out_space.sum(0) - 1).max().item() < 1e-5 and abs(f.cross_space.sum(0) - 1).max().item() < 1e-5
        assert abs(f.per_layer_out.sum(1) - 0.25).max().item() < 1e-5
    assert close(reqs[0].out_space, pattern + full[0].out_space)
    assert close(reqs[0].cross_space, pattern + full[0].cross_space)
    assert close(reqs[0].per_layer_out, pattern + full[0].per_layer_out)
    assert close(reqs[0].per_layer_cross, pattern + full[0].per_layer_cross)
    assert close(reqs[1].out_space, pattern + 4 * full[1].per_layer_out[1])          # layer 1 alone, weight 1
    assert close(reqs[1].per_layer_out[0], pattern + full[1].per_layer_out[1])
