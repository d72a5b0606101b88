"""What tests/test_stream_contract_gpu.py rests on, without a GPU: the probes cover every entry point of
include/conceptattn.h that takes a stream, ca_last_error() is per thread, and the bookkeeping of the two allocators of
tests/stream_gate.py."""
import os
import re
import threading

import pytest
import torch

import __graft_entry__ as entry
import address_range_cases as C
import gemm_route_cases as G
import stream_contract_cases as P
import stream_gate as SG
from conceptattention_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return L.load()


# ------------------------------------------------------------------------------------------------------ coverage
def test_every_entry_point_that_takes_a_stream_is_probed():
    declared = P.stream_entry_points()
    # the parser agrees with the binding: a ca_stream_t is the last argument, a c_void_p, of exactly these
    assert len(declared) >= 40 and declared <= set(L.SIGNATURES)
    assert declared.isdisjoint(P.NO_STREAM)
    probed = {e for p in P.PROBES for e in p.entries}
    print(f"\n  {len(declared)} entry points take a stream; {len(P.PROBES)} probes name {len(probed)}")
    assert probed == declared, f"not probed: {sorted(declared - probed)}; not in the header: {sorted(probed - declared)}"


def test_the_parser_sees_a_new_declaration(tmp_path):
    text = open(P.HEADER).read()
    new = tmp_path / "conceptattn.h"
    new.write_text(text + "\nint ca_new_thing_f32(const float *x, int32_t n,\n                     ca_stream_t stream);\n"
                          "int ca_no_stream(const float *x /* not a ca_stream_t */, int32_t n);\n")
    assert P.stream_entry_points(str(new)) == P.stream_entry_points() | {"ca_new_thing_f32"}


def test_the_probe_table_has_what_the_issue_lists():
    ids = [p.id for p in P.PROBES]
    assert len(ids) == len(set(ids))
    gemm = [p for p in P.PROBES if p.family == "gemm"]
    assert [p.arg[0] for p in gemm] == list(G.ROUTES)                                     # every route
    assert {p.arg[1] for p in gemm} == set(C.GEMM_EPIS)                                   # all four epilogues
    assert all(G.compatible(*p.arg) for p in gemm)
    assert any(isinstance(G.ROUTES[p.arg[0]].thin, tuple) for p in gemm)                  # the thin-row second launch
    assert {p.entries[0] for p in gemm} == {"ca_gemm_bf16", "ca_gemm_fp8"}
    assert [p.id for p in P.PROBES if p.family == "attn"] == [f"attn-{k}" for k in C.ATTN_PLACEMENT]
    import rowop_cases as R
    import vae_cases as V
    for fam, cases in (("rowop", R.CASES), ("vae", V.CASES)):
        forms = {(c.entry, c.kernel) for c in cases}
        by_id = {c.id: c for c in cases}
        got = [(by_id[p.arg].entry, by_id[p.arg].kernel) for p in P.PROBES if p.family == fam]
        assert set(got) == forms and len(got) == len(forms), fam                          # every launch form once
    text = {p.arg[0] for p in P.PROBES if p.family == "text"}
    assert text == set(C.TEXT_PLACEMENT)
    assert any(p.id == "text-ca_layernorm_f32in-rows" and p.wrapper is None for p in P.PROBES)
    assert {p.arg for p in P.PROBES if p.family == "render"} == set(P.RENDER_CASES.values())
    assert {p.family for p in P.PROBES} == {"gemm", "attn", "rowop", "vae", "text", "segtab", "mseg", "render"}


def test_waits_by_design_and_integration_md_name_the_same_wrappers():
    probed = {p.wrapper for p in P.PROBES if p.wrapper}
    assert probed == set(P.WAITS_BY_DESIGN)
    for p in P.PROBES:
        if p.wrapper:
            assert any(q.direct and q.entries == p.entries and q.wrapper is None for q in P.PROBES), p.id
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"Wrappers that wait:(.*?)\n\n", doc, flags=re.S)
    assert m, "INTEGRATION.md: the 'Wrappers that wait:' lines are missing"
    named = set(re.findall(r"`ops\.([a-z_]+(?:\(row_idx=\.\.\.\))?)`", m.group(1)))
    assert named == set(P.WAITS_BY_DESIGN), named ^ set(P.WAITS_BY_DESIGN)


# ------------------------------------------------------------------------------------------- error text per thread
def test_ca_last_error_is_per_thread(lib):
    """Two threads each provoke a different rejected call (the argument checks need no device), meet at a barrier, then
    read ca_last_error(): each sees its own message; a third thread that made no call sees neither."""
    barrier = threading.Barrier(3)
    seen, rcs = {}, {}

    def gemm():
        rcs["gemm"] = lib.ca_gemm_bf16(None, 1, 0, None)
        barrier.wait(timeout=30)
        seen["gemm"] = lib.ca_last_error()

    def fused():
        arr = (L.HeatmapProblem * 1)()
        rcs["fused"] = lib.ca_heatmap_fused(arr, 1, 64, 9, 256, 0, None)
        barrier.wait(timeout=30)
        seen["fused"] = lib.ca_last_error()

    def idle():
        barrier.wait(timeout=30)
        seen["idle"] = lib.ca_last_error()
    threads = [threading.Thread(target=f) for f in (gemm, fused, idle)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert rcs == {"gemm": -1, "fused": -1} and set(seen) == {"gemm", "fused", "idle"}, (rcs, seen)
    assert b"ca_gemm" in seen["gemm"] and b"ca_heatmap_fused" not in seen["gemm"], seen
    assert b"ca_heatmap_fused" in seen["fused"] and b"ca_gemm" not in seen["fused"], seen
    assert b"ca_gemm" not in seen["idle"] and b"ca_heatmap_fused" not in seen["idle"], seen


# ----------------------------------------------------------------------------------------------- the allocators
def _recorded():
    rec = SG.Recording("cpu")
    a = rec.to(torch.arange(6, dtype=torch.float32).view(2, 3), {"a": None})
    o = rec.full((4, 5), 7.0, torch.bfloat16, {"o": None})
    i = rec.to(torch.tensor([3, 1, 2], dtype=torch.int32))
    return rec, a, o, i


def test_recording_keeps_the_calls_in_order_and_a_pristine_copy():
    rec, a, o, i = _recorded()
    assert [c[0] for c in rec.calls] == ["to", "full", "to"]
    assert rec.calls[1][1:] == ((4, 5), 7.0, torch.bfloat16)
    assert tuple(o.shape) == (4, 5) and o.dtype == torch.bfloat16 and bool((o == 7).all())
    a.add_(1)                                                     # what a kernel does to an in-place operand
    assert torch.equal(rec.calls[0][1], torch.arange(6, dtype=torch.float32).view(2, 3)), "the recorded payload moved"
    assert torch.equal(rec.calls[2][1], i) and rec.t_first is not None


def test_gated_refuses_a_call_that_differs_from_the_recorded_one():
    """(the checks come before any device work, so they run here)"""
    rec, _, _, _ = _recorded()
    for bad, what in ((lambda g: g.to(torch.zeros(2, 4)), "shape"),
                      (lambda g: g.to(torch.zeros(2, 3, dtype=torch.float64)), "dtype"),
                      (lambda g: g.full((2, 3), 0.0, torch.float32), "kind")):
        with pytest.raises(AssertionError, match="call 0"):
            bad(SG.Gated(rec))
    g = SG.Gated(rec)
    g.k = 1
    with pytest.raises(AssertionError, match="call 1"):
        g.full((4, 5), 7.0, torch.float32)                        # dtype of a full()
    g.k = 1
    with pytest.raises(AssertionError, match="fill"):
        g.full((4, 5), 8.0, torch.bfloat16)
    g.k = 3
    with pytest.raises(AssertionError, match="only 3 calls"):
        g.to(torch.zeros(1))
    g.k = 2
    with pytest.raises(AssertionError, match="2 allocator calls"):
        g.release()


def test_poison_per_dtype():
    for dt in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
        assert SG.poison_kind(dt, True) == SG.poison_kind(dt, False) == "nan"
    for dt in (torch.int32, torch.int64):
        assert SG.poison_kind(dt, True) == "index" and SG.poison_kind(dt, False) == "bytes"
    for dt in (torch.uint8, torch.int8, torch.int16):
        assert SG.poison_kind(dt, True) == SG.poison_kind(dt, False) == "bytes"
    assert SG.POISON_BYTE == 0xA5
    ids = torch.tensor([3, 1, 2], dtype=torch.int32)              # the index poison: the same ids, one place on
    assert torch.equal(torch.roll(ids, 1), torch.tensor([2, 3, 1], dtype=torch.int32))
