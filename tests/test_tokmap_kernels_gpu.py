"""ca_token_maps on the device, every case of tests/tokmap_cases.py: the accumulators and lse against the fp64 reference
inside the derived bound, the same bits from a second launch and over a garbage workspace, each accumulator alone, a
problem alone against the same problem inside a 5-problem and a 16-problem launch and among 17 through the wrapper, NaN
rows, and the stream contract (order, no host wait, graph replay).

Every buffer a launch sees is cut out of a larger allocation with guard elements on both sides; whatever a launch may not
read is NaN (tokmap_cases.make_inputs), lse starts as NaN: an element never written fails its bound, and a guard must come
back as it was.  max err / bound is printed per case and per family (pytest -s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import tokmap_cases as T  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
NAN = float("nan")
GUARD = 64          # elements on either side of every buffer
WORST = {}          # family -> (largest max err / bound over the maps, over acc from its non-zero start, over lse)


class Guarded:
    """Buffers with GUARD elements in front and behind (NaN; the NaN bit pattern / 0x5A for the integer types)."""

    def __init__(self):
        self.whole = []

    def _cut(self, shape, dtype):
        n = 1
        for d in shape:
            n *= d
        fill = NAN if dtype.is_floating_point else (T.NAN_BITS if dtype == torch.int16 else 0x5A)
        w = torch.full((n + 2 * GUARD,), fill, device=DEV, dtype=dtype)
        self.whole.append((w, n, fill))
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
        for w, n, fill in self.whole:
            for g in (w[:GUARD], w[GUARD + n:]):
                assert bool(torch.isnan(g).all() if fill != fill else (g == fill).all()), "guard elements written"


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def place(case, al, outs=("acc", "acc2", "lse"), tag="", edit=None):
    """The device operands of one problem.  ``edit(buffers)`` may change the host copies of the input buffers first."""
    inp = T.make_inputs(case)
    host = {k: v.clone() for k, v in inp["buffers"].items()}
    if edit:
        edit(host)
    bufs = {name: al.to(b, {name + tag: None}) for name, b in host.items()}
    d = dict(bufs=bufs, before={k: v.clone() for k, v in bufs.items()})
    for name in ("q", "k0", "k1"):
        d[name] = T.view(case, bufs, name).view(torch.bfloat16)
    if "acc" in outs:
        d["acc"] = al.to(inp["acc0"], {"acc" + tag: None})
    if "acc2" in outs:
        d["acc2"] = al.to(inp["acc20"], {"acc2" + tag: None})
    if "lse" in outs:
        d["lse"] = al.full((case.heads, case.nq), NAN, torch.float32, {"lse" + tag: None})
    return d


def problem(case, d):
    return ops.TokenMaps(d["q"], d["k0"], d["k1"] if case.n1 else None, case.n_tok, acc=d.get("acc"), weight=T.W1,
                         acc2=d.get("acc2"), weight2=T.W2, lse=d.get("lse"))


def outputs(d):
    return {k: d[k] for k in ("acc", "acc2", "lse") if k in d}


def run(cases, al, outs=("acc", "acc2", "lse"), workspace=None, edit=None):
    """One ops.token_maps call over ``cases`` (they share heads, storage type and scale); -> the outputs per problem."""
    c0 = cases[0]
    assert all((c.heads, c.f16, c.prescaled) == (c0.heads, c0.f16, c0.prescaled) for c in cases)
    dev = [place(c, al, outs, tag=f"[{i}]", edit=edit) for i, c in enumerate(cases)]
    ops.token_maps([problem(c, d) for c, d in zip(cases, dev)], c0.heads, c0.scale_log2, qk_f16=c0.f16, workspace=workspace)
    torch.cuda.synchronize()
    al.check_guards()
    for d in dev:                                               # the inputs and all their NaN surroundings: byte for byte
        for k, v in d["bufs"].items():
            assert torch.equal(_bytes(v), _bytes(d["before"][k])), f"input buffer {k} changed"
    return [outputs(d) for d in dev]


def assert_same_bits(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(_bytes(a[k]), _bytes(b[k])), f"{what}: {k} differs"


_SINGLE = {}


def single(case):
    """The outputs of a case launched alone (computed once; read-only)."""
    if case.id not in _SINGLE:
        _SINGLE[case.id] = run([case], Guarded())[0]
    return _SINGLE[case.id]


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_every_case_against_fp64(case):
    inp = T.make_inputs(case)
    got = single(case)
    maps, lse, bound = T.reference(case)
    worst = {}
    # the maps themselves: acc2 starts at zero and has weight 1, so it holds fma(1, map, 0) = the map, bit for bit, and is
    # held to the map's own bound with nothing added (a zero or a doubled cold-text cell fails here)
    assert T.W2 == 1.0 and not bool(inp["acc20"].any())
    worst["maps"] = T.over_the_bound(got["acc2"], maps, bound.maps)
    # the accumulate semantics: acc += weight * map from a non-zero start, one fused multiply-add on top
    a0 = inp["acc0"]
    worst["acc"] = T.over_the_bound(got["acc"], a0.double() + T.W1 * maps, T.acc_bound(T.W1, a0, maps, bound.maps))
    worst["lse"] = T.over_the_bound(got["lse"], lse, bound.lse)
    print(f"\n  {case.id}: max err / bound  maps {worst['maps'][0]:.3f}  acc {worst['acc'][0]:.3f}  lse {worst['lse'][0]:.3f}")
    old = WORST.get(case.family, (0.0, 0.0, 0.0))
    WORST[case.family] = tuple(max(o, worst[k][0]) for o, k in zip(old, ("maps", "acc", "lse")))
    assert_same_bits(got, run([case], Guarded())[0], "second launch")
    for name, (ratio, n_over) in worst.items():
        assert n_over == 0, f"{case.id}: {name}: {n_over} elements over the bound (NaN = never written), max err / bound {ratio:.3g}"


def test_print_the_largest_ratio_per_family():
    for case in T.CASES:                                        # (cached when the cases above ran in this process)
        if case.family not in WORST:
            test_every_case_against_fp64(case)
    print()
    for fam in T.FAMILIES:
        print(f"  {fam:14s} largest max err / bound: maps {WORST[fam][0]:.3f}  acc (non-zero start) {WORST[fam][1]:.3f}  "
              f"lse {WORST[fam][2]:.3f}")
    assert set(WORST) == set(T.FAMILIES)


ACC_CASE = next(c for c in T.CASES if c.family == "unit" and c.heads == 3)


@pytest.mark.parametrize("outs", [("acc",), ("acc2",), ("acc", "lse"), ("acc", "acc2")], ids="+".join)
def test_each_accumulator_alone_and_a_non_zero_start(outs):
    """acc += weight * map from a non-zero start (tokmap_cases' acc0 is N(0, 0.1)), whichever outputs are asked for."""
    both = single(ACC_CASE)
    got = run([ACC_CASE], Guarded(), outs=outs)[0]
    assert set(got) == set(outs)
    assert_same_bits(got, {k: both[k] for k in outs}, "+".join(outs))
    inp = T.make_inputs(ACC_CASE)
    assert float(inp["acc0"].abs().min()) > 0 and not torch.equal(both["acc"].cpu(), inp["acc0"])


def test_a_garbage_workspace_changes_nothing_and_stays_untouched():
    al = Guarded()
    ws = al.full((4096,), 0xA5, torch.uint8)
    got = run([ACC_CASE], al, workspace=ws)[0]
    assert bool((ws == 0xA5).all()), "the workspace was written beyond ca_token_maps_workspace_bytes() = 0"
    assert_same_bits(got, single(ACC_CASE), "garbage workspace")
    assert ops.token_maps_workspace_bytes([problem(ACC_CASE, place(ACC_CASE, Guarded()))], ACC_CASE.heads) == 0


@pytest.mark.parametrize("n", [5, 16, 17])
def test_a_problem_alone_has_the_bits_it_has_inside_a_launch(n):
    """Problems of different shapes (nq, n0, n_tok, n1, layout) in one launch: each has the bits of its own launch; 17 go
    through the wrapper's split."""
    pool = [c for c in T.CASES if (c.heads, c.f16, c.prescaled) == (2, False, False)]
    assert len(pool) >= 5 and len({(c.nq, c.n0, c.n1) for c in pool}) >= 4
    pool.sort(key=lambda c: -c.n0 * c.nq)                       # the largest first: the grid is sized for problem 0 alone
    cases = [pool[i % len(pool)] for i in range(n)][::-1 if n == 16 else 1]
    got = run(cases, Guarded())
    for i, (c, g) in enumerate(zip(cases, got)):
        assert_same_bits(g, single(c), f"problem {i} ({c.id}) of {n}")


@pytest.mark.parametrize("f16", [False, True])
def test_nan_rows(f16):
    case = next(c for c in T.CASES if c.family == "unit" and c.heads == 3 and c.f16 == f16 and c.n_tok < c.n0)
    W = case.heads * 128
    clean = single(case)

    def put(name, row, col):
        def edit(host):
            b, r0, _, c0 = T.make_inputs(case)["views"][name]
            host[b][r0 + row, c0 + col] = T.NAN_BITS
        return edit
    # a NaN in head 1 of query row 3: that row's cells and that head's lse, nothing else
    got = run([case], Guarded(), edit=put("q", 3, 128 + 5))[0]
    for k in ("acc", "acc2"):
        assert bool(torch.isnan(got[k][:, 3]).all())
        keep = [i for i in range(case.nq) if i != 3]
        assert torch.equal(_bytes(got[k][:, keep]), _bytes(clean[k][:, keep]))
    nan_lse = torch.isnan(got["lse"])
    assert bool(nan_lse[1, 3]) and int(nan_lse.sum()) == 1
    # a NaN in a key row (an image key, then a text key past n_tok): every cell
    for name, row in (("k1", case.n1 - 1), ("k0", case.n0 - 1)):
        got = run([case], Guarded(), edit=put(name, row, W - 1))[0]
        assert bool(torch.isnan(got["acc"]).all()) and bool(torch.isnan(got["acc2"]).all())
        assert bool(torch.isnan(got["lse"][case.heads - 1]).all()) and not bool(torch.isnan(got["lse"][0]).any())


STREAM_CASES = [c for c in T.CASES if (c.heads, c.f16, c.prescaled) == (2, False, False)][:3]


def test_token_maps_runs_on_its_stream_and_returns_before_it_drains():
    """The stream contract's probe (tests/test_stream_contract_gpu.py::test_runs_on_its_stream_and_returns_before_it_drains)
    for ca_token_maps: a warm-up on the current stream, then the same launch on a second stream behind a gate kernel: the
    call returns while the gate still runs, and gives the warm-up's bytes."""
    import stream_contract_cases as P
    import stream_gate as SG
    from test_stream_contract_gpu import _raw

    def go(al):
        dev = [place(c, al, tag=f"[{i}]") for i, c in enumerate(STREAM_CASES)]
        ops.token_maps([problem(c, d) for c, d in zip(STREAM_CASES, dev)], 2, T.SCALE_LOG2)
        torch.cuda.synchronize()
        return {f"{i}.{k}": v.clone() for i, d in enumerate(dev) for k, v in outputs(d).items()}
    rec = SG.Recording(DEV)
    with SG.watching() as warm_calls:
        want = go(rec)
    assert warm_calls and rec.t_first is not None
    torch.cuda.synchronize()
    gate = SG.Gate()
    al = SG.Gated(rec, gate)
    s2 = torch.cuda.Stream()
    assert s2.cuda_stream != 0 and s2 != torch.cuda.current_stream()
    try:
        with torch.cuda.stream(s2), SG.watching(gate) as calls:
            got = go(al)
    finally:
        torch.cuda.synchronize()
    al.release()
    seen = [(n, running) for n, running, _ in calls if n not in P.NO_STREAM]
    assert tuple(n for n, _ in seen) == ("ca_token_maps",), seen
    assert all(running for _, running in seen), "ca_token_maps returned only after the gate had finished"
    assert set(got) == set(want)
    for k in want:
        assert _raw(got[k]) == _raw(want[k]), f"{k} behind the gate != the warm-up run"


def test_replay_token_maps_with_the_accumulator_reset_inside_the_capture():
    from test_stream_contract_gpu import BF, _like, _rand, _replay_check
    nq, n0, n1, heads, n_tok = 70, 24, 70, 2, 20
    W = heads * 128
    sets = [dict(qkv=_rand((n0 + n1, 3 * W), s, 1.0, BF), acc0=_rand((n_tok, nq), s + 1)) for s in (5, 15)]
    st = _like(sets[0])
    outs = dict(acc=torch.empty(n_tok, nq, device=DEV), lse=torch.empty(heads, nq, device=DEV))

    def call():
        outs["acc"].copy_(st["acc0"])            # the accumulator's reset: inside the capture
        qkv = st["qkv"]
        ops.token_maps([ops.TokenMaps(qkv[n0:, :W], qkv[:n0, W:2 * W], qkv[n0:, W:2 * W], n_tok, acc=outs["acc"], weight=0.5,
                                      lse=outs["lse"])], heads, T.SCALE_LOG2)
    _replay_check("token_maps", sets, st, outs, call)
