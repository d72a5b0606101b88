"""The model-level case table without a GPU (tests/model_route_cases.py): every LayerRoute that HipFluxDiT._layer_route
can return is the route of some layer of some case, case names say what their routes are, and no route of any admitted
batch puts more attention problems into one launch than the kernel's table holds."""
import itertools

import pytest

import model_route_cases as M
from conceptattention_amd import _lib as L
from conceptattention_amd.flux_dit import HipFluxDiT, LayerRoute


def flags(route) -> str:
    return " ".join(f for f, v in zip(LayerRoute._fields, route) if v) or "(uncaptured, bf16 q / k)"


def test_table_speaks_about_the_models_settings():
    assert set(M.DEFAULTS) == set(M.SETTING_VALUES) == set(HipFluxDiT.ROUTE_SETTINGS)
    for k, vals in M.SETTING_VALUES.items():
        assert vals[0] == M.DEFAULTS[k] and len(set(vals)) == len(vals) >= 2, k
    assert len(M.BY_NAME) == len(M.CASES)
    for c in M.CASES:
        assert set(c.settings) <= set(M.DEFAULTS), c.name
        assert all(c.settings[k] != M.DEFAULTS[k] for k in c.settings), c.name
        assert c.C in (1, 3, 8, 9) and c.T == 8 and c.side in (256, 208) and c.B in (1, 3) and c.singles in (0, 1), c.name
        assert c.B <= len(M.ITEM_SEEDS) and c.B <= M.MAX_ITEMS
        assert c.layers is None or (c.layers and set(c.layers) <= set(range(M.DEPTH))), c.name
        assert c.return_vectors or c.layers, c.name     # every case returns something beside pred
    assert M.Case("x", side=208).L == 169 and M.Case("x").L == 256


def test_every_reachable_route_is_executed_by_a_case():
    """All ROUTE_SETTINGS values x C in {1, 8, 9} x return_vectors x {no maps, maps of another layer, maps of this
    layer}: every distinct LayerRoute is the route of a layer of a case.  No exclusions."""
    reach = M.reachable_routes()
    by_route = {}
    for c in M.CASES:
        for i in range(M.DEPTH):
            by_route.setdefault(M.route_of(c, i), []).append(f"{c.name}[layer {i}]")
    print(f"\n{len(reach)} distinct reachable routes:")
    for r in sorted(reach, reverse=True):
        print(f"  {flags(r):60s} <- {', '.join(by_route.get(r, ['NONE'])[:3])}")
    missing = [flags(r) for r in reach if r not in by_route]
    assert not missing, missing
    assert set(by_route) <= set(reach), "a case reaches a route the enumeration does not know"
    assert len(reach) == 42


def test_the_issues_cases_are_in_the_table():
    """The settings, pairs, ablations, return forms, norms and sides the table was asked to hold, by what they ARE."""
    def has(**want):
        def ok(c):
            s = c.full_settings()
            for k, v in want.items():
                got = s[k] if k in s else getattr(c, k)
                if got != v:
                    return False
            return True
        return [c for c in M.CASES if ok(c)]
    base = dict(layers=(1,), return_vectors=True)
    for k, vals in M.SETTING_VALUES.items():
        if k in ("bf16_timesteps", "fp32_latent", "keep_bf16_layers", "fp8_bf16_qkv_when_captured"):
            continue   # (the first two select no route; the last two act in fp8 mode only: below)
        for v in vals[1:]:
            assert has(**base, **{k: v}), (k, v)
    assert has(**base, precision="fp8", fp8_bf16_qkv_when_captured=False)
    assert has(**base, precision="fp8", keep_bf16_layers=frozenset({1}))
    ind = dict(base, capture_independent_image=True)
    assert has(**ind, qk_f16="all") and has(**ind, C=9) and has(**ind, precision="fp8") and has(**ind, B=3)
    assert has(**ind, residual_dtype=M.torch.bfloat16)
    assert has(**base, precision="fp8", C=9) and has(**base, epilogue_logits=False, B=3)
    for route in (dict(C=3), dict(capture_independent_image=True), dict(C=9), dict(precision="fp8")):
        for cross, self_ in itertools.product((True, False), repeat=2):
            assert has(**base, **route, cross=cross, self_=self_, B=1), (route, cross, self_)
        assert [c for c in has(**base, **route, B=3) if not (c.cross and c.self_)], route
    assert has(return_vectors=False, layers=(1,)) and has(return_vectors=True, layers=None)
    assert has(return_vectors=False, layers=(0,))
    for norm in (L.NORM_SPARSEMAX, L.NORM_ENTMAX15):
        assert [c for c in has(norm=norm) if c.settings or c.C == 9], norm
    for route in ({}, dict(capture_independent_image=True), dict(precision="fp8")):
        assert has(side=208, **route), route


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_case_names_say_what_the_routes_are(case):
    r = M.route_of(case, M.captured_layer(case))
    tokens = case.name.split("_")
    for t in tokens:
        rule = M.ROUTE_TOKENS.get(t) or M.IMPLIED_TOKENS.get(t)
        assert rule is not None, f"{case.name}: token {t!r} has no rule"
        assert rule(case, r), f"{case.name}: {t!r} does not hold on {r}"
    for t, rule in M.ROUTE_TOKENS.items():
        assert (t in tokens) == bool(rule(case, r)), f"{case.name}: {t!r} must be named exactly when it holds ({r})"


def test_attention_problems_per_launch_fit_the_kernels_table():
    """_double_block puts at most 3 B problems into one ops.attention launch (concept rows, main, the map side of
    capture_independent_image) and HipFluxDiT.__call__ admits B <= 5: 15 <= ATTN_MAX_PROBLEMS, on every reachable route
    and ablation.  (The forward therefore has no second launch for an overflow.)"""
    assert M.MAX_ITEMS == 5
    worst = 0
    for route in M.reachable_routes():
        for cross, self_ in itertools.product((True, False), repeat=2):
            for B in range(1, M.MAX_ITEMS + 1):
                worst = max(worst, *M.attention_launches(route, B, cross, self_))
    assert worst == 3 * M.MAX_ITEMS <= L.ATTN_MAX_PROBLEMS
    for c in M.CASES:
        launches = M.expected_attention_launches(c)
        assert max(launches) <= L.ATTN_MAX_PROBLEMS and min(launches) >= 1, c.name
    # the forward holds the launch to the same limit itself
    import inspect
    src = inspect.getsource(HipFluxDiT._double_block)
    assert src.count("ops.attention(") == 3 and "ATTN_MAX_PROBLEMS" not in src
