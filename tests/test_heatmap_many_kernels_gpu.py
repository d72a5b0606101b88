"""ca_heatmap_many on the device, every case of tests/heatmap_many_cases.py: bit equality with the three-launch form
(ops.heatmap_logits + ops.heatmap_norm_accumulate) at every C and with ops.heatmap_fused at C <= 8, every value inside
the derived bound of the fp64 reference, a second launch over the same inputs giving the same bits; and the sparse
weighting kernels at 17, 24 and 32 concepts against the same reference and bounds.

Every buffer a launch sees is cut out of a larger allocation with GUARD elements of NaN on both sides, outputs start as
NaN, and the vectors' padding columns hold NaN: an element never written fails its bound, and a guard or a padding column
must come back byte for byte.  Then one capture-and-replay check and one launch with all operands at bit 31, shaped like
tests/test_stream_contract_gpu.py's and tests/test_address_range_gpu.py's.  max err / bound is printed (pytest -s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import heatmap_many_cases as H  # noqa: E402
import placement as PL  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
NAN = float("nan")
GUARD = 64          # elements on either side of every buffer
MANY = [c for c in H.CASES if c.op == "many"]
SPARSE = [c for c in H.CASES if c.op == "norm"]


class Guarded:
    """Buffers with GUARD NaN elements in front and behind (16-byte aligned starts), checked after the launches."""

    def __init__(self):
        self.whole = []

    def _cut(self, shape, dtype):
        n = 1
        for d in shape:
            n *= d
        w = torch.full((n + 2 * GUARD,), NAN, device=DEV, dtype=dtype)
        self.whole.append((w, n))
        return w[GUARD:GUARD + n].view(shape)

    def to(self, t, roles=None):
        v = self._cut(tuple(t.shape), t.dtype)
        v.copy_(t)
        return v

    def full(self, shape, fill, dtype, roles=None):
        v = self._cut(tuple(shape), dtype)
        v.fill_(fill)
        return v

    def check_guards(self):
        for w, n in self.whole:
            assert bool(torch.isnan(w[:GUARD]).all()) and bool(torch.isnan(w[GUARD + n:]).all()), "guard elements written"


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def place(case, inp, al):
    """The device operands of every problem: vectors (whole padded buffers), accumulators' start values, NaN logits."""
    s = case.shape
    dev = []
    for i, pr in enumerate(inp["probs"]):
        tag = "" if i == len(inp["probs"]) // 2 else f"[{i}]"
        d = dict(img=al.to(pr["img"], {"img" + tag: None}), con=al.to(pr["con"], {"con" + tag: None}))
        if "acc" in H.OUTS[s["outs"]]:
            d["acc"] = al.to(pr["acc0"], {"acc" + tag: None})
        if "acc2" in H.OUTS[s["outs"]]:
            d["acc2"] = al.to(pr["acc20"], {"acc2" + tag: None})
        if "logits" in H.OUTS[s["outs"]]:
            d["logits"] = al.full((s["C"], s["L"]), NAN, torch.float32, {"logits" + tag: None})
        dev.append(d)
    return dev


def problems(case, dev):
    dim = case.shape["dim"]
    return [ops.Heatmap(d["img"][:, :dim], d["con"][:, :dim], acc=d.get("acc"), weight=H.W1, acc2=d.get("acc2"),
                        weight2=H.W2, logits=d.get("logits")) for d in dev]


def outputs(dev):
    return [{k: v for k, v in d.items() if k in ("acc", "acc2", "logits")} for d in dev]


def run_many(case, inp, al, entry=None):
    dev = place(case, inp, al)
    before = [(d["img"].clone(), d["con"].clone()) for d in dev]
    (entry or ops.heatmap_many)(problems(case, dev), norm=L.NORMS[case.shape["norm"]])
    torch.cuda.synchronize()
    al.check_guards()
    for d, (i0, c0) in zip(dev, before):                       # the inputs and their NaN padding: byte for byte
        assert torch.equal(_bytes(d["img"]), _bytes(i0)) and torch.equal(_bytes(d["con"]), _bytes(c0))
    return outputs(dev)


def run_three_launch(case, inp, al):
    """The parity reference: per problem one ops.heatmap_logits, then one ops.heatmap_norm_accumulate per accumulator."""
    s = case.shape
    dev = place(case, inp, al)
    norm = L.NORMS[s["norm"]]
    for d in dev:
        lg = d["logits"] if "logits" in d else al.full((s["C"], s["L"]), NAN, torch.float32)
        ops.heatmap_logits(d["img"][:, :s["dim"]], d["con"][:, :s["dim"]], lg)
        if "acc" in d:
            ops.heatmap_norm_accumulate(lg, d["acc"], H.W1, norm)
        if "acc2" in d:
            ops.heatmap_norm_accumulate(lg, d["acc2"], H.W2, norm)
    torch.cuda.synchronize()
    return outputs(dev)


def assert_same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert set(x) == set(y)
        for k in x:
            assert torch.equal(_bytes(x[k]), _bytes(y[k])), f"{what}: problem {i} {k} differs"


@pytest.mark.parametrize("case", MANY, ids=lambda c: c.id)
def test_many_against_the_three_launch_form_the_fused_form_and_fp64(case):
    inp = H.make_inputs(case)
    got = run_many(case, inp, Guarded())
    ref = H.reference(case, inp, dev=DEV)
    worst, n_over = H.over_the_bound(case, inp, got, ref)
    print(f"\n  {case.id}: {case.kernel}  max err / bound = {worst:.3f}")
    assert_same_bits(got, run_many(case, inp, Guarded()), "second launch")
    assert_same_bits(got, run_three_launch(case, inp, Guarded()), "three-launch form")
    if case.shape["C"] <= 8:
        assert_same_bits(got, run_many(case, inp, Guarded(), entry=ops.heatmap_fused), "ca_heatmap_fused")
    assert n_over == 0, f"{case.id}: {n_over} elements over the bound (NaN = never written), max err / bound {worst:.3g}"


@pytest.mark.parametrize("case", SPARSE, ids=lambda c: c.id)
def test_sparse_weighting_at_17_24_and_32_concepts(case):
    s = case.shape
    inp = H.make_inputs(case)
    al = Guarded()
    lg, acc = al.to(inp["logits"]), al.to(inp["acc0"])
    ops.heatmap_norm_accumulate(lg, acc, s["w"], norm=L.NORMS[s["norm"]])
    torch.cuda.synchronize()
    al.check_guards()
    assert torch.equal(_bytes(lg), _bytes(inp["logits"].to(DEV)))
    (ref,) = H.reference(case, inp, dev=DEV)
    worst, n_over = H.over_the_bound(case, inp, [{"acc": acc}], [ref])
    print(f"\n  {case.id}: {case.kernel}  max err / bound = {worst:.3f}")
    assert n_over == 0, f"{case.id}: {n_over} elements over the bound, max err / bound {worst:.3g}"


def test_more_than_32_concepts_are_refused_by_the_sparse_norms_only():
    z = torch.zeros(33, 40, device=DEV)
    acc = torch.zeros(33, 40, device=DEV)
    with pytest.raises(ValueError, match="33"):
        ops.heatmap_norm_accumulate(z, acc, 1.0, norm=L.NORM_SPARSEMAX)
    ops.heatmap_norm_accumulate(z, acc, 1.0, norm=L.NORM_SOFTMAX)
    torch.cuda.synchronize()
    assert torch.allclose(acc, torch.full_like(acc, 1.0 / 33), rtol=1e-6, atol=0)
    # ops.heatmap_softmax_accumulate keeps the limit it always had with a sparse norm, and is the same launch below it
    with pytest.raises(ValueError, match="17"):
        ops.heatmap_softmax_accumulate(z[:17].contiguous(), acc[:17].contiguous(), 1.0, norm=L.NORM_ENTMAX15)
    g = torch.Generator().manual_seed(3)
    z16 = torch.randn(16, 40, generator=g).to(DEV)
    a, b = torch.zeros(16, 40, device=DEV), torch.zeros(16, 40, device=DEV)
    ops.heatmap_softmax_accumulate(z16, a, 0.5, norm=L.NORM_SPARSEMAX)
    ops.heatmap_norm_accumulate(z16, b, 0.5, norm=L.NORM_SPARSEMAX)
    assert torch.equal(a, b)
    assert ops.heatmap_many_fits(32, 3072) and ops.heatmap_many_fits(1, 4096)
    assert not ops.heatmap_many_fits(33, 3072) and not ops.heatmap_many_fits(12, 4104) and not ops.heatmap_many_fits(0, 8)


def test_heatmap_many_runs_on_its_stream_and_returns_before_it_drains():
    """The stream contract's probe (tests/test_stream_contract_gpu.py::test_runs_on_its_stream_and_returns_before_it_drains),
    for ca_heatmap_many: a warm-up on the current stream, then the same launch on a second stream behind a gate kernel: the
    call returns while the gate still runs, and gives the warm-up's bytes."""
    import stream_contract_cases as P
    import stream_gate as SG
    from test_stream_contract_gpu import _raw
    case = H.BY_ID["many_C17_L257_dim264_sparsemax_n16_all"]
    inp = H.make_inputs(case)

    def run(al):
        dev = place(case, inp, al)
        ops.heatmap_many(problems(case, dev), norm=L.NORMS[case.shape["norm"]])
        torch.cuda.synchronize()
        return {f"{i}.{k}": v.clone() for i, g in enumerate(outputs(dev)) for k, v in g.items()}
    rec = SG.Recording(DEV)
    with SG.watching() as warm_calls:
        want = run(rec)
    assert warm_calls and rec.t_first is not None
    torch.cuda.synchronize()
    gate = SG.Gate()
    al = SG.Gated(rec, gate)
    s2 = torch.cuda.Stream()
    assert s2.cuda_stream != 0 and s2 != torch.cuda.current_stream()
    try:
        with torch.cuda.stream(s2), SG.watching(gate) as calls:
            got = run(al)
    finally:
        torch.cuda.synchronize()
    al.release()
    seen = [(n, running) for n, running, _ in calls if n not in P.NO_STREAM]
    assert tuple(n for n, _ in seen) == ("ca_heatmap_many",), seen
    assert all(running for _, running in seen), "ca_heatmap_many returned only after the gate had finished"
    assert set(got) == set(want)
    for k in want:
        assert _raw(got[k]) == _raw(want[k]), f"{k} behind the gate != the warm-up run"


def test_replay_heatmap_many_with_the_accumulator_reset_inside_the_capture():
    from test_stream_contract_gpu import BF, _like, _rand, _replay_check
    Lp, Cc, dim = 300, 12, 256
    sets = [dict(img=_rand((Lp, dim), s, 1.0, BF), con=_rand((Cc, dim), s + 1, 0.2, BF), acc0=_rand((Cc, Lp), s + 2))
            for s in (7, 17)]
    st = _like(sets[0])
    outs = dict(acc=torch.empty(Cc, Lp, device=DEV), logits=torch.empty(Cc, Lp, device=DEV))

    def call():
        outs["acc"].copy_(st["acc0"])            # the accumulator's reset: inside the capture
        ops.heatmap_many([ops.Heatmap(st["img"], st["con"], acc=outs["acc"], weight=0.5, logits=outs["logits"])],
                         norm=L.NORM_SPARSEMAX)
    _replay_check("heatmap_many", sets, st, outs, call)


def test_all_operands_at_bit_31():
    """Every buffer of a 16-problem launch below a multiple of 4 GiB with bit 31 of all its addresses set: the same bits
    as from ordinary allocations."""
    case = H.BY_ID["many_C17_L257_dim264_sparsemax_n16_all"]
    inp = H.make_inputs(case)
    plain = run_many(case, inp, Guarded())
    arena = PL.Arena(DEV)
    try:
        pl = arena.placer()
        got = run_many(case, inp, pl)
        for start, n in pl.placed.values():
            assert start >> 31 & 1 and (start + n - 1) >> 31 & 1, hex(start)
        assert_same_bits(got, plain, "bit-31 placement")
    finally:
        arena.buf = None
        torch.cuda.empty_cache()
