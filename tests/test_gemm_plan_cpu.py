"""ca_gemm_plan without a GPU: the routes of the model's grouped launches on a 256-CU MI355X, the coverage of those
routes by the GPU case table (tests/gemm_route_cases.py), argument errors, and the CPU-side proof that every bound of
the GPU cases rejects a realistic kernel slip."""
import pytest

import __graft_entry__ as entry
import gemm_route_cases as G
from conceptattention_amd import _lib as L
from conceptattention_amd import ops

H = 3072
N_CU = 256
Q, R, GE = L.EPI_QKV_NORM_ROPE, L.EPI_GATE_RESIDUAL, L.EPI_GELU_TANH


@pytest.fixture(scope="module", autouse=True)
def lib():
    entry.build()
    return L.load()


def model_launches(B, C):
    """The grouped GEMM launches of one double and one single block at B items per forward and C concepts (the
    residual stream in fp32): name -> problems."""
    img, ctx, rows = B * 4096, B * (256 + C), B * 4352
    return {"qkv": [dict(M=img, N=3 * H, K=H, epi=Q, n_split=3 * H), dict(M=ctx, N=3 * H, K=H, epi=Q, n_split=3 * H)],
            "proj": [dict(M=img, N=H, K=H, epi=R, f32=True), dict(M=ctx, N=H, K=H, epi=R, f32=True)],
            "mlp.0": [dict(M=img, N=4 * H, K=H, epi=GE), dict(M=ctx, N=4 * H, K=H, epi=GE)],
            "mlp.2": [dict(M=img, N=H, K=4 * H, epi=R, f32=True), dict(M=ctx, N=H, K=4 * H, epi=R, f32=True)],
            "linear1": [dict(M=rows, N=7 * H, K=H, epi=Q, n_split=3 * H)],
            "linear2": [dict(M=rows, N=H, K=5 * H, epi=R, f32=True)]}


def thin_form(info):
    if info["thin_mf"]:
        return (info["thin_mf"], info["thin_nw"])
    return "walk" if info["thin_tiles"] else None


def model_plan(fp8, B, C, name):
    return G.plan_raw(model_launches(B, C)[name], L.TILE_PP_256x256 if fp8 else L.TILE_AUTO, fp8, N_CU)


# (fp8, B, C) -> launch -> (persistent, thin form) on 256 CUs; every launch is on the 256 x 256 ping-pong tile
W, T21, T24, T41, T44 = "walk", (2, 1), (2, 4), (4, 1), (4, 4)
MODEL_TABLE = {
    (False, 1, 4): dict(qkv=(1, W), proj=(0, W), **{"mlp.0": (1, W), "mlp.2": (0, W)}, linear1=(1, None), linear2=(0, None)),
    (False, 1, 8): dict(qkv=(1, W), proj=(0, W), **{"mlp.0": (1, W), "mlp.2": (0, W)}, linear1=(1, None), linear2=(0, None)),
    (False, 5, 4): dict(qkv=(1, T24), proj=(1, T21), **{"mlp.0": (1, T21), "mlp.2": (1, T21)}, linear1=(1, None),
                        linear2=(1, None)),
    (False, 5, 8): dict(qkv=(1, T44), proj=(1, T41), **{"mlp.0": (1, T41), "mlp.2": (1, T41)}, linear1=(1, None),
                        linear2=(1, None)),
    (True, 1, 4): dict(qkv=(1, W), proj=(0, W), **{"mlp.0": (1, W), "mlp.2": (0, W)}, linear1=(1, None), linear2=(0, None)),
    (True, 1, 8): dict(qkv=(1, W), proj=(0, W), **{"mlp.0": (1, W), "mlp.2": (0, W)}, linear1=(1, None), linear2=(0, None)),
    (True, 5, 4): dict(qkv=(1, W), proj=(1, W), **{"mlp.0": (1, W), "mlp.2": (1, W)}, linear1=(1, None), linear2=(1, None)),
    (True, 5, 8): dict(qkv=(1, W), proj=(1, W), **{"mlp.0": (1, W), "mlp.2": (1, W)}, linear1=(1, None), linear2=(1, None)),
}


@pytest.mark.parametrize("key", list(MODEL_TABLE), ids=lambda k: f"{'fp8' if k[0] else 'bf16'}-B{k[1]}-C{k[2]}")
def test_model_launch_routes_are_pinned(key):
    fp8, B, C = key
    for name, (persistent, thin) in MODEL_TABLE[key].items():
        info = model_plan(fp8, B, C, name)
        assert info["tile"] == L.TILE_PP_256x256, (name, info)
        assert info["kernel"] == (L.GEMM_KERNEL_PP_FP8 if fp8 else L.GEMM_KERNEL_PP), (name, info)
        assert (info["persistent"], thin_form(info)) == (persistent, thin), (name, info)
        if info["persistent"]:
            assert info["grid"] == N_CU, (name, info)
        else:
            assert info["grid"] == info["main_tiles"] + info["thin_tiles"], (name, info)
    # the 5-item mlp.0 launch of the issue: (80 + 5) x 48 = 4080 main tiles, 48 thin ones, 4080 % 256 + 48 > 256
    info = model_plan(False, 5, 4, "mlp.0")
    assert (info["main_tiles"], info["thin_grid_x"], info["thin_groups"]) == (4080, 4 * 96, 1)


def _combo_of_case(case):
    r, e = G.ROUTES[case.route], G.EPIS[case.epi]
    thin = r.thin if r.kernel != L.GEMM_KERNEL_CLASSIC else None
    return (r.kernel, thin, e["epi"], "f32" if e["f32"] else "bf16", "fp8" if r.fp8 else "bf16")


def test_every_model_route_is_in_the_gpu_case_table():
    """Each (kernel, thin form, epilogue, out dtype, precision) of the model's launches has a GPU case: a router
    change that sends the model down a new path fails here until the matrix covers it."""
    covered = {_combo_of_case(c) for c in G.CASES}
    for fp8, B, C in MODEL_TABLE:
        for name, probs in model_launches(B, C).items():
            info = model_plan(fp8, B, C, name)
            for p in probs:
                combo = (info["kernel"], thin_form(info), p["epi"], "f32" if p.get("f32") else "bf16",
                         "fp8" if fp8 else "bf16")
                assert combo in covered, (fp8, B, C, name, combo)


def test_case_table_covers_every_route_and_epilogue():
    routes = {c.route for c in G.CASES}
    assert routes == set(G.ROUTES)
    for r in G.ROUTES:
        assert {c.epi for c in G.CASES if c.route == r} == {e for e in G.EPIS if G.compatible(r, e)}, r
    assert {c.K for c in G.CASES} == {128, 3072}


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.id)
def test_every_case_reaches_its_route_on_a_256_cu_part(case):
    assert G.find_shape(case.route, case.epi, case.K, N_CU) is not None, case.id


def test_plan_follows_the_cu_count():
    """Persistence needs n_cu % 8 == 0 and more tiles than CUs; the thin-row decision depends on the CU count."""
    shape = [dict(M=3 * 256 + 20, N=256 * 65, K=128, epi=L.EPI_BIAS)]
    own = G.plan_raw(shape, L.TILE_PP_256x256, False, 256)
    assert thin_form(own) == (2, 1) and not own["persistent"]
    walk = G.plan_raw(shape, L.TILE_PP_256x256, False, 512)       # 195 % 512 + 65 <= 512: rides in the walk
    assert thin_form(walk) == "walk" and walk["thin_tiles"] == 65
    big = [dict(M=4 * 256, N=256 * 80, K=128, epi=L.EPI_BIAS)]
    assert G.plan_raw(big, L.TILE_PP_256x256, False, 256)["persistent"] == 1
    assert G.plan_raw(big, L.TILE_PP_256x256, False, 252)["persistent"] == 0   # 252 % 8 != 0
    # the classic kernel never walks persistently, whatever the tile count
    info = G.plan_raw(big, L.TILE_256x256, False, 256)
    assert info["kernel"] == L.GEMM_KERNEL_CLASSIC and not info["persistent"] and info["grid"] == 320


def test_plan_of_tile_auto_is_the_auto_tile():
    shape = [dict(M=4096, N=128, K=3072, epi=L.EPI_BIAS)]
    arr = (L.GemmProblem * 1)()
    G._raw_problem(arr[0], **shape[0])
    assert G.plan_raw(shape, L.TILE_AUTO, False, N_CU)["tile"] == L.load().ca_gemm_auto_tile(arr, 1)


def _plan_error(fp8=False, tile=L.TILE_PP_256x256, **over):
    arr = (L.GemmProblem * 1)()
    base = dict(M=300, N=768, K=128, epi=L.EPI_GATE_RESIDUAL)
    qkv = over.pop("qkv", False)
    if qkv:
        base.update(epi=L.EPI_QKV_NORM_ROPE, n_split=768, qpre=over.pop("qpre", None))
    G._raw_problem(arr[0], fp8=fp8, **base)
    for k, v in over.items():
        setattr(arr[0], k, v)
    with pytest.raises(ValueError, match="ca_gemm_plan"):
        ops.gemm_plan(arr, tile=tile, n_cu=N_CU, fp8=fp8)


def test_plan_rejects_what_the_launch_rejects():
    _plan_error(gate_stride=6, gate_item_rows=4)                       # gate_stride % 4
    _plan_error(gate_stride=8, gate_item_rows=0)                       # gate_item_rows < 1
    _plan_error(gate_stride=8, gate_item_rows=4, gate_rows=100, gate2=G._FAKE, gate2_item_rows=0)
    _plan_error(fp8=True, qkv=True, qpre=3)                            # qpre_f32 = 3 with fp8
    _plan_error(epilogue=L.EPI_GELU_TANH, out_f32=1)                   # out_f32 with GELU
    _plan_error(qkv=True, tile=L.TILE_PP_256x128)                      # QKV_NORM_ROPE off the 256 x 256 tile
    _plan_error(qkv=True, tile=L.TILE_256x256)
    _plan_error(fp8=True, tile=L.TILE_PP_256x128)                      # fp8 has the 256 x 256 tile only
    _plan_error(A=None)                                                # null operand
    _plan_error(K=96)                                                  # K % 64
    arr = (L.GemmProblem * 1)()
    G._raw_problem(arr[0], M=300, N=768, K=128, epi=L.EPI_BIAS)
    info = L.GemmPlanInfo()
    assert L.load().ca_gemm_plan(arr, 1, L.TILE_PP_256x256, 0, -1, info) == -1      # n_cu < 0
    assert L.load().ca_gemm_plan(arr, 1, L.TILE_PP_256x256, 2, N_CU, info) == -1    # fp8 not 0 / 1
    assert L.load().ca_gemm_plan(arr, 1, L.TILE_PP_256x256, 0, N_CU, None) == -1
    assert L.load().ca_gemm_plan(arr, 1, L.TILE_PP_256x256, 0, N_CU, info) == 0


@pytest.mark.parametrize("slip", list(G.SLIPS))
def test_bounds_reject_a_realistic_kernel_slip(slip):
    """The fp64 reference rounded as the kernel stores it passes every bound of its case; the named slip (computed
    exactly, then rounded the same way) puts elements of the output that carries it over the bound."""
    faithful_ok, n_over = G.discrimination(slip)
    assert faithful_ok, f"{slip}: the bound rejects a faithful result"
    assert n_over > 0, f"{slip}: the bound does not see the slip"
