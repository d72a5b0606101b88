"""The autoencoder kernels' case table without a GPU (tests/vae_cases.py): every launch form of ca_vae.hip and every
entry point it defines is named by a GPU case, the table hits the edges listed below, the faithful fp32 emulation is
inside every bound and every bound rejects a named kernel slip."""
import ctypes
import os
import re

import pytest
import torch

import vae_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "conceptattention_amd", "csrc", "ca_vae.hip")
HEADER = os.path.join(ROOT, "include", "conceptattn.h")


def _norm(name: str) -> str:
    return re.sub(r"\s+", "", name)


def launch_forms() -> list:
    """The kernel of every hipLaunchKernelGGL( call of ca_vae.hip's host half (the entry points)."""
    src = re.sub(r"//[^\n]*", "", open(SRC).read())
    return [_norm(k) for k in re.findall(r"hipLaunchKernelGGL\(\s*(ca_\w+_kernel\b(?:<[^>]*>)?)", src)]


def entry_points() -> set:
    return set(re.findall(r'extern\s+"C"\s+int\s+(ca_\w+)\s*\(', open(SRC).read()))


def test_launch_sites_are_parsed():
    forms = launch_forms()
    assert len(forms) == 8, forms
    assert len(set(forms)) == 8, forms           # every launch site a distinct instantiation
    assert open(SRC).read().count("hipLaunchKernelGGL(") == 8


def test_every_launch_form_has_a_case():
    named = {_norm(k) for c in V.CASES for k in c.kernels}
    missing = [f for f in launch_forms() if f not in named]
    assert not missing, f"launch forms of ca_vae.hip without a GPU case in tests/vae_cases.py: {missing}"
    stale = named - set(launch_forms())
    assert not stale, f"cases name kernels ca_vae.hip does not launch: {stale}"
    for c in V.CASES:                            # a GroupNorm case names both of its launches, of one input type
        if c.op == "gn":
            t = "float" if c.shape["xdt"] == "f32" else "bf16"
            assert [_norm(k) for k in c.kernels] == [f"ca_gn_stats_kernel<{t}>", f"ca_gn_apply_kernel<{t}>"], c.id
        if c.op == "conv":                       # the dispatch of ca_conv3x3_nhwc: CoutPad <= 32
            assert c.kernel == ("ca_conv_kernel<1>" if V.ceil_to(c.shape["cout"], 16) <= 32 else "ca_conv_kernel<4>")


def test_every_entry_point_has_a_case():
    header = open(HEADER).read()
    entries = entry_points()
    assert len(entries) == 4, entries
    for e in entries:
        assert re.search(r"\bint\s+%s\s*\(" % e, header), f"{e} is not declared in include/conceptattn.h"
    covered = {c.entry for c in V.CASES}
    assert entries == covered, entries ^ covered


@pytest.mark.parametrize("entry", sorted(entry_points()))
def test_a_rejected_call_is_reported_under_the_called_entry_points_name(entry):
    """Every entry point refuses a NULL first pointer before it touches the GPU, under its own name."""
    import __graft_entry__ as graft
    from conceptattention_amd import _lib as L
    graft.build()
    lib = L.load()
    args = [0.0 if t is ctypes.c_float else 0 if t in (ctypes.c_int32, ctypes.c_int64) else None
            for t in L.SIGNATURES[entry][1]]
    assert args[0] is None, entry
    assert getattr(lib, entry)(*args) == -1, entry
    assert lib.ca_last_error().decode().startswith(entry + ": "), lib.ca_last_error()


def test_case_ids_are_unique_and_inputs_are_built_on_the_cpu():
    assert len(V.BY_ID) == len(V.CASES)
    assert len({c.seed for c in V.CASES}) == len(V.CASES)
    for c in V.CASES:
        for v in V.make_inputs(c).values():
            assert v.device.type == "cpu", c.id
    from conceptattention_amd import ops
    for hw in (1, 511, 512, 1023, 1024, 1025, 4096, 40000, 70000, 10 ** 6):
        assert V.groupnorm_chunks(hw) == ops.groupnorm_chunks(hw)


def test_edges_the_cases_must_hit():
    cv = [c.shape for c in V.CASES if c.op == "conv"]
    k1 = [c.shape for c in V.CASES if c.kernel == "ca_conv_kernel<1>"]
    k4 = [c.shape for c in V.CASES if c.kernel == "ca_conv_kernel<4>"]
    assert {s["cout"] for s in k1} >= {3, 16, 20, 32}
    assert {s["cout"] for s in k4} >= {35, 36, 48, 80, 130, 132, 160}
    vec = V.conv_vector_epilogue
    assert any(s["cout"] % 4 == 0 and s["ldo"] % 4 and not vec(s) for s in cv)
    assert any(s["cout"] % 4 == 0 and s["ldo"] % 4 == 0 and s["resid"] == "separate" and s["ldr"] % 4 for s in cv)
    assert set(V.SCALAR_TWINS) == {c.id for c in V.CASES if c.op == "conv" and c.shape["cout"] % 4 == 0
                                   and not vec(c.shape)}
    assert all(vec(t.shape) for t in V.SCALAR_TWINS.values())
    assert any(s["ldx"] == 40 and s["cin"] == 32 for s in cv)
    assert any(s["ldo"] > s["cout"] and s["out"] == "f32" for s in cv)
    assert any(s["ldo"] > s["cout"] and s["out"] == "bf16" for s in cv)
    assert any(s["ldo"] > s["cout"] and vec(s) for s in cv)
    assert any(s["resid"] == "separate" and s["ldr"] != s["ldo"] for s in cv)
    assert any(not s["bias"] and s["resid"] == "none" for s in cv)
    assert any(not s["bias"] and s["resid"] != "none" for s in cv)
    assert any(s["resid"] == "in place" and s["out"] == "f32" for s in k1)
    assert any(s["resid"] == "in place" and s["out"] == "f32" for s in k4)
    assert any(s["mode"] == "k1" and s["cin"] == 32 for s in cv)
    assert any(s["mode"] == "k1" and s["out"] == "bf16" for s in cv)
    assert any(s["mode"] == "s1" and s["cin"] == 512 for s in cv)
    hw = lambda mode: {(s["H"], s["W"]) for s in cv if s["mode"] == mode}      # noqa: E731
    assert hw("s2") >= {(2, 2), (3, 3), (16, 16), (33, 17)}
    assert hw("up") >= {(1, 1), (5, 7)}
    assert hw("s1") >= {(1, 1), (33, 1), (1, 17)}
    M = {V.conv_geometry(s)[5] for s in cv}
    assert min(M) < 64 and {128, 129} <= M
    assert any(s["B"] == 2 and (s["H"], s["W"]) == (8, 8) and V.conv_geometry(s)[5] == 128 for s in cv)
    assert any(s["B"] == 3 and V.conv_geometry(s)[5] < 128 for s in cv)       # image boundaries inside one tile
    assert all(s["H"] <= 33 and s["W"] <= 17 or V.conv_geometry(s)[5] == 129 for s in cv)
    legacy = {(s["H"], s["W"], s["cin"], s["cout"], s["mode"], s["resid"] == "separate", s["out"] == "f32")
              for s in cv if s["bias"] and s["ldo"] == s["cout"] and s["ldx"] == V.ceil_to(s["cin"], 32)
              and s["ldr"] in (None, s["cout"]) and s["B"] == 2}
    assert legacy >= set(V.LEGACY_CONV) and len(set(V.LEGACY_CONV)) == 16

    gn = [c.shape for c in V.CASES if c.op == "gn"]
    for xdt in ("f32", "bf16"):
        assert {s["C"] for s in gn if s["xdt"] == xdt} >= {32, 64, 128, 256, 512, 1024}, xdt
    assert {s["HW"] for s in gn} >= {1, 7, 511, 512, 1023, 1024, 1025, 4096, 70000}
    rstep = lambda s: 256 // (s["C"] // 4)                                     # noqa: E731
    assert any(s["HW"] < rstep(s) for s in gn) and any(s["HW"] > rstep(s) and s["HW"] % rstep(s) for s in gn)
    assert {s["B"] for s in gn} >= {1, 2, 3}
    assert {(s["n_chunks"], s["HW"]) for s in gn} >= {(1, 4096), (1024, 1000), (7, 5)}
    assert any(s["C"] == 1024 and s["HW"] == 40000 and s["B"] == 1 and s["HW"] // 8 > 4096 for s in gn)
    assert any(s["xdt"] == "f32" and s["ldx"] > s["C"] and s["ldx"] % 4 == 0 and s["ldy"] > s["C"] for s in gn)
    assert any(s["xdt"] == "bf16" and s["ldx"] > s["C"] and s["ldx"] % 8 == 0 and s["ldy"] > s["C"] for s in gn)
    assert any(s["const"] and s["C"] == 128 and s["HW"] == 600 for s in gn)
    assert {s["mean"] for s in gn} >= {100.0, 1000.0}
    assert any(s["swish"] for s in gn) and any(not s["swish"] for s in gn)

    sm = [c.shape for c in V.CASES if c.op == "softmax"]
    assert {s["n"] for s in sm} >= {1, 63, 64, 65, 255, 256, 257, 1000}
    assert {s["rows"] for s in sm} >= {1, 5}
    assert any(s["lds"] != s["ldp"] for s in sm) and any(s["ldp"] - s["n"] > 256 for s in sm)
    assert {s["scale"] for s in sm} >= {0.125, 512 ** -0.5}
    assert any(s["rows"] >= 5 for s in sm)       # rows 1, 2, 3: equal scores, one score 60 nats above, all near -1e4
    inp = V.make_inputs(V.BY_ID["softmax_n257"])
    sc = inp["s"][:, :257]
    assert bool((sc[1] == sc[1, 0]).all()) and bool((sc[3] < -9990).all())
    assert (sc[2].max() - sc[2].sort().values[-2]).item() * 0.125 >= 60

    af = [c.shape for c in V.CASES if c.op == "affine"]
    assert {(s["out"], s["lv"]) for s in af} == {("bf16", False), ("bf16", True), ("f32", False), ("f32", True)}
    assert any(s["C"] < s["ldx"] for s in af)
    assert {s["out"] for s in af if s["C"] < s["ldo"]} == {"bf16", "f32"}
    assert any(s["view"] and s["lv"] for s in af)
    assert {s["rows"] * s["C"] for s in af} >= {1, 255, 257}
    big = [s for s in af if s["rows"] * s["C"] > 65536 * 1024]
    assert [(s["rows"], s["C"], s["a"], s["b"], s["lv"]) for s in big] == [(2 ** 22 + 3, 17, 1.0, 0.0, False)]
    assert any(s["a"] == 1 / V.SCALE_FACTOR and s["b"] == V.SHIFT_FACTOR for s in af)
    assert {s["out"] for s in af if s["a"] == 1.0 and s["b"] == 0.0 and not s["lv"]} == {"bf16", "f32"}   # kind exact


def test_slips_the_table_must_hold():
    slips = {(V.BY_ID[cid].op, slip) for cid, slip, _ in V.SLIPS.values()}
    assert slips >= {("conv", s) for s in ("s2_pad_leading_edge", "up_parity", "taps_transposed", "last_k_step_dropped",
                                           "bias_missing_in_scalar_tail", "resid_read_with_ldo",
                                           "bf16_store_truncates")}
    assert slips >= {("gn", s) for s in ("one_pass_variance", "unbiased_variance", "last_chunk_rows_dropped",
                                         "empty_chunk_merged", "group_index_ignores_cpg", "bf16_store_truncates")}
    assert slips >= {("softmax", s) for s in ("no_max_subtraction", "log2e_missing", "padding_not_zeroed")}
    assert slips >= {("affine", s) for s in ("std_is_exp_logvar", "shift_before_scale", "padding_columns_written")}


@pytest.mark.parametrize("case", [c for c in V.CASES if not c.shape.get("big")], ids=lambda c: c.id)
def test_faithful_emulation_passes_every_bound(case):
    """The same operation in fp32 on the CPU, stored as the kernel stores it, has no element over a bound (the bounds
    are not so tight that a correct kernel fails them on rounding alone).  The convolution twice: torch's fp32
    convolution, and the tap walk the slips are applied to.  Not run: the 71M-element affine case."""
    inp = V.make_inputs(case)
    ref = V.reference(case, inp)
    for name, (r, _, _) in ref.items():
        assert bool(torch.isfinite(r).all()), (case.id, name)
    for form in [None] + (["taps"] if case.op == "conv" else []):
        over = V.over_bounds(case, inp, V.emulate(case, inp, form), ref)
        assert not any(over.values()), (case.id, form, over)


@pytest.mark.parametrize("slip", list(V.SLIPS))
def test_bounds_reject_a_named_kernel_slip(slip):
    faithful_ok, n_over = V.discrimination(slip)
    assert faithful_ok, f"{slip}: the bound rejects a faithful result"
    assert n_over > 0, f"{slip}: the bound does not see the slip"


def test_half_ulp_store_and_truncation():
    """The bf16 kind allows half an ulp on top of the bound before the store: round to nearest passes, a truncating
    store fails wherever the dropped bits are more than half an ulp."""
    ref = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -10, 1 + 2.0 ** -10, -(3 + 2.0 ** -7 + 2.0 ** -9)], dtype=torch.float64)
    zero = torch.zeros_like(ref)
    assert V.excess(ref.float().to(torch.bfloat16), ref, zero, "bf16")[1] == 0
    assert V.trunc_bf16(ref.float()).tolist() == [1.0, 1.0, -3.0]
    assert V.excess(V.trunc_bf16(ref.float()), ref, zero, "bf16")[1] == 2
    assert V.excess(torch.tensor([float("nan")]), ref[:1], zero[:1], "bf16")[1] == 1     # never written
