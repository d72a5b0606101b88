"""The row kernels' case table without a GPU (tests/rowop_cases.py): every launch form of ca_rowops.hip and every row
entry point of include/conceptattn.h is named by a GPU case, and every bound rejects a named kernel slip."""
import ctypes
import os
import re

import pytest
import torch

import rowop_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "conceptattention_amd", "csrc", "ca_rowops.hip")
HEADER = os.path.join(ROOT, "include", "conceptattn.h")


def _norm(name: str) -> str:
    return re.sub(r"\s+", "", name)


def launch_forms() -> list:
    """The kernel of every launch of ca_rowops.hip: each instantiation its host half (the unit's second anonymous
    namespace and the entry points after it) hands to launch(), directly, through a dispatch lambda or from a table.
    Not a launch: the kernels named for ca_raise_lds_limit (cast to const void *) and inside decltype."""
    src = open(SRC).read()
    host = re.sub(r"//[^\n]*", "", src[src.rindex("\nnamespace {"):])
    assert "launch(" in host and "__global__" not in host
    return [_norm(s) for s in re.findall(r"(?<!\(const void \*\))(?<!decltype\(&)\b(ca_\w+_kernel\b(?:<[^>]*>)?)", host)]


def row_entry_points() -> set:
    """The extern "C" entry points defined in ca_rowops.hip (every one of them launches a row kernel)."""
    return set(re.findall(r'extern\s+"C"\s+int\s+(ca_\w+)\s*\(', open(SRC).read()))


def test_launch_sites_are_parsed():
    forms = launch_forms()
    assert len(forms) == 35, forms
    assert len(set(forms)) == 35, forms          # every launch site a distinct instantiation


def test_every_launch_form_has_a_case():
    named = {_norm(c.kernel) for c in R.CASES}
    missing = [f for f in launch_forms() if f not in named]
    assert not missing, f"launch forms of ca_rowops.hip without a GPU case in tests/rowop_cases.py: {missing}"
    stale = named - set(launch_forms())
    assert not stale, f"cases name kernels ca_rowops.hip does not launch: {stale}"


def test_every_row_entry_point_has_a_case():
    header = open(HEADER).read()
    entries = row_entry_points()
    assert len(entries) >= 19, entries
    for e in entries:
        assert re.search(r"\bint\s+%s\s*\(" % e, header), f"{e} is not declared in include/conceptattn.h"
    covered = {c.entry for c in R.CASES}
    assert entries <= covered, f"row entry points without a case: {sorted(entries - covered)}"
    assert covered <= entries, sorted(covered - entries)


@pytest.mark.parametrize("entry", sorted(row_entry_points()))
def test_a_rejected_call_is_reported_under_the_called_entry_points_name(entry):
    """Every row entry point refuses a NULL first pointer before it touches the GPU, and the text ca_last_error() then
    returns begins with the name of the entry point that was CALLED -- also where two entry points share one body
    (ca_qpre_finish_rope_f32 once reported as ca_qpre_finish_f32)."""
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
    assert len(R.BY_ID) == len(R.CASES)
    for c in R.CASES:
        inp = R.make_inputs(c)
        for v in inp.values():
            for t in (v if isinstance(v, list) else [v]):
                assert t.device.type == "cpu", c.id


def test_edges_the_cases_must_hit():
    ln = [c.shape for c in R.CASES if c.op == "ln"]
    assert {s["H"] for s in ln} >= {8, 264, 3072, 4096}
    assert {s["M"] for s in ln} >= {1, 7, 8, 9, 777}
    assert {len(s["segs"]) for s in ln} >= {1, 3, 15, 16}
    assert any(s["ldx"] > s["H"] and s["ldo"] > s["H"] for s in ln)
    assert any(s["ldlo"] > s["H"] for s in ln if s["out"] == "split")
    gemv = [c.shape for c in R.CASES if c.op == "gemv"]
    assert {s["nv"] for s in gemv} == set(range(1, 9))
    assert {s["K"] for s in gemv} >= {8, 264, 2056, 4096}
    assert any(s["N"] > 65536 for s in gemv) and any(s["N"] % 16 for s in gemv)
    assert any(not s["bias"] for s in gemv) and any(s["acc"] for s in gemv) and any(s["silu"] for s in gemv)
    assert any(s["nv"] >= 5 and s["nv"] * s["K"] * 4 > 64 * 1024 for s in gemv)       # the LDS opt-in
    lg = [c.shape for c in R.CASES if c.op == "logits"]
    assert {s["C"] for s in lg} >= {1, 3, 5, 8, 11} and {s["L"] for s in lg} >= {1, 2, 257}
    assert any(s["L"] > 4096 for s in lg) and {s["dim"] for s in lg} >= {8, 264, 3072, 4096}
    sp = [c.shape for c in R.CASES if c.op == "split"]
    assert any(s["rows"] * s["K"] > 2 ** 20 for s in sp if s["silu"])
    assert any(s["rows"] * s["K"] > 2 ** 20 for s in sp if not s["silu"])
    assert any(s["K"] % 8 for s in sp)
    cb = [c.shape for c in R.CASES if c.op == "combine"]
    assert any(s["nv"] * s["N"] > 2 ** 21 for s in cb) and any(not s["bias"] for s in cb)
    assert {c.shape["C"] for c in R.CASES if c.op == "norm"} >= {1, 8, 9, 16}
    qk = [c.shape for c in R.CASES if c.op == "qk"]
    assert {s["heads"] for s in qk} >= {1, 3, 24} and any(len(s["segs"]) == 16 for s in qk)
    assert any(s["M"] * 2 * s["heads"] % 16 for s in qk)
    assert any(s["ld"] > 3 * s["heads"] * 128 for s in qk)
    ax = [c.shape for c in R.CASES if c.op == "axpy"]
    assert any(s["n"] < 8 for s in ax) and any(s["n"] % 8 for s in ax if s["n"] > 8)
    assert {c.shape["form"] for c in R.CASES if c.op == "fused"} == {"part", "bf16", "f32"}


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_faithful_emulation_passes_every_bound(case):
    """The fp64 reference stored as the kernel stores it is within every bound of the case (the bounds are not so
    tight that a correct kernel fails them on rounding alone)."""
    inp = R.make_inputs(case)
    for name, (ref, pre, kind) in R.reference(case, inp).items():
        assert bool(torch.isfinite(ref).all()), (case.id, name)
        _, n_over = R.excess(R.rounded_like_output(ref, kind), ref, pre, kind)
        assert n_over == 0, (case.id, name)


@pytest.mark.parametrize("slip", list(R.SLIPS))
def test_bounds_reject_a_named_kernel_slip(slip):
    """The faithful result passes every bound of its case; the named slip (emulated in fp64, or in fp32 where the
    kernel works in fp32, then stored the same way) puts elements of the output that carries it over the bound."""
    faithful_ok, n_over = R.discrimination(slip)
    assert faithful_ok, f"{slip}: the bound rejects a faithful result"
    assert n_over > 0, f"{slip}: the bound does not see the slip"


def test_fp8_tie_rule():
    """RNE to e4m3 on exact ties goes to the even mantissa; the tie band admits both neighbours only inside it."""
    r = torch.tensor([1.0625, 1.1875, -1.0625, 3.0], dtype=torch.float64)
    assert R.e4m3(r).tolist() == [1.0, 1.25, -1.0, 3.0]
    assert R.trunc_e4m3(r).tolist() == [1.0, 1.125, -1.0, 3.0]
    got = torch.tensor([1.125, 1.125, -1.125, 3.0], dtype=torch.float64)
    _, n = R.excess(got, r, torch.full_like(r, 1e-6), "fp8")
    assert n == 0                                   # within 1e-6 of a tie either neighbour is RNE of a point in band
    _, n = R.excess(got, r, torch.zeros_like(r), "fp8")
    assert n == 3                                   # exactly on the tie: only the even one
