"""ca_propagate_maps on the device, every case of tests/propmap_cases.py: the accumulators against the fp64 reference
inside the derived bound, the same bits from a second launch and over a garbage workspace, a problem alone against the same
problem among 16 (and among 17 through the wrapper's split), a query row at rows 0, 17 and 200, the three NaN rules, a
constant map, and the cross-checks against ca_query_maps.

Every buffer a launch sees is cut out of a larger allocation with guard elements on both sides; whatever a launch may not
read is NaN (propmap_cases.make_inputs): a guard must come back as it was, and a NaN that was read shows in the outputs.
max err / bound is printed per case and per family (pytest -s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import propmap_cases as P  # noqa: E402
import querymap_cases as Q  # noqa: E402
import tokmap_cases as T  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
NAN = float("nan")
GUARD = 64          # elements on either side of every buffer
WORST = {}          # family -> (largest max err / bound over the maps, over acc from its non-zero start)


def test_the_library_exports_the_entry():
    lib = L.load()
    assert hasattr(lib, "ca_propagate_maps") and hasattr(lib, "ca_propagate_maps_workspace_bytes")
    assert callable(ops.propagate_maps) and callable(ops.propagate_maps_workspace_bytes)


class Guarded:
    """Buffers with GUARD elements in front and behind (NaN; the NaN bit pattern / 0x5A for the integer types)."""

    def __init__(self):
        self.whole = []

    def _cut(self, shape, dtype):
        n = 1
        for d in shape:
            n *= d
        fill = NAN if dtype.is_floating_point else (P.NAN_BITS if dtype == torch.int16 else 0x5A)
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


def place(case, al, outs=("acc", "acc2"), tag="", edit=None):
    """The device operands of one problem; ``tag`` marks the problem in the allocator's roles.  ``edit(buffers)`` may change
    the host copies of the input buffers first."""
    inp = P.make_inputs(case)
    host = {k: v.clone() for k, v in inp["buffers"].items()}
    if edit:
        edit(host)
    bufs = {name: al.to(b, {name + tag: None}) for name, b in host.items()}
    d = dict(bufs=bufs, before={k: v.clone() for k, v in bufs.items()})
    for name in ("q", "k0", "k1"):
        d[name] = P.view(case, bufs, name).view(torch.bfloat16)
    d["v"] = P.view(case, bufs, "v")
    if "acc" in outs:
        d["acc"] = al.to(inp["acc0"], {"acc" + tag: None})
    if "acc2" in outs:
        d["acc2"] = al.to(inp["acc20"], {"acc2" + tag: None})
    return d


def problem(case, d):
    return ops.PropagateMaps(d["q"], d["k0"] if case.n0 else None, d["k1"], d["v"], acc=d.get("acc"), weight=P.W1,
                             acc2=d.get("acc2"), weight2=P.W2)


def run(cases, al, outs=("acc", "acc2"), workspace=None, edit=None):
    """One ops.propagate_maps call over ``cases`` (they share heads, storage type and scale); -> the outputs per problem."""
    c0 = cases[0]
    assert all((c.heads, c.f16, c.prescaled) == (c0.heads, c0.f16, c0.prescaled) for c in cases)
    dev = [place(c, al, outs, tag=f"[{i}]", edit=edit) for i, c in enumerate(cases)]
    ops.propagate_maps([problem(c, d) for c, d in zip(cases, dev)], c0.heads, c0.scale_log2, qk_f16=c0.f16, workspace=workspace)
    torch.cuda.synchronize()
    al.check_guards()
    for d in dev:                                               # the inputs and all their NaN surroundings: byte for byte
        for k, v in d["bufs"].items():
            assert torch.equal(_bytes(v), _bytes(d["before"][k])), f"input buffer {k} changed"
    return [{k: d[k] for k in ("acc", "acc2") if k in d} for d in dev]


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


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c.id)
def test_every_case_against_fp64(case):
    got = single(case)
    # acc2 starts at zero and has weight 1, so it holds fma(1, out, 0) = the propagated map, bit for bit, and is held to the
    # map's own bound; acc += weight * out from N(0, 0.1): one fused multiply-add on top
    worst = P.check_outputs(case, got)
    print(f"\n  {case.id}: max err / bound  " + "  ".join(f"{k} {v[0]:.3f}" for k, v in worst.items()))
    old = WORST.get(case.family, (0.0, 0.0))
    WORST[case.family] = tuple(max(o, worst[k][0]) for o, k in zip(old, ("maps", "acc")))
    assert_same_bits(got, run([case], Guarded())[0], "second launch")
    for name, (ratio, n_over) in worst.items():
        assert n_over == 0, f"{case.id}: {name}: {n_over} elements over the bound (NaN = never written), max err / bound {ratio:.3g}"


def test_print_the_largest_ratio_per_family():
    for case in P.CASES:                                        # (cached when the cases above ran in this process)
        if case.family not in WORST:
            test_every_case_against_fp64(case)
    print()
    for fam in P.FAMILIES:
        print(f"  {fam:14s} largest max err / bound: maps {WORST[fam][0]:.3f}  acc (non-zero start) {WORST[fam][1]:.3f}")
    assert set(WORST) == set(P.FAMILIES)


ACC_CASE = next(c for c in P.CASES if c.heads == 3 and c.nq == 65 and c.n0 > 0 and not c.f16)


@pytest.mark.parametrize("outs", [("acc",), ("acc2",)])
def test_each_accumulator_alone_has_the_bits_it_has_beside_the_other(outs):
    both = single(ACC_CASE)
    got = run([ACC_CASE], Guarded(), outs=outs)[0]
    assert set(got) == set(outs)
    assert_same_bits(got, {k: both[k] for k in outs}, str(outs))
    inp = P.make_inputs(ACC_CASE)
    assert float(inp["acc0"].abs().min()) > 0 and not torch.equal(both["acc"].cpu(), inp["acc0"])


def test_a_garbage_workspace_changes_nothing_and_is_written_inside_its_size_only():
    al = Guarded()
    c = ACC_CASE
    need = ops.propagate_maps_workspace_bytes([problem(c, place(c, Guarded()))], c.heads)
    assert need == (c.heads * c.C * c.nq * 4 + 15) // 16 * 16
    ws = al.full((need + 4096,), 0xA5, torch.uint8)
    got = run([c], al, workspace=ws[:need])[0]
    assert bool((ws[need:] == 0xA5).all()), "the workspace was written beyond ca_propagate_maps_workspace_bytes()"
    assert_same_bits(got, single(c), "garbage workspace")
    with pytest.raises(ValueError, match="workspace too small"):
        run([c], Guarded(), workspace=ws[:need - 16])


@pytest.mark.parametrize("n", [16, 17])
def test_a_problem_alone_has_the_bits_it_has_inside_a_launch(n):
    """Problems of different shapes (nq, n0, n1, C, strides) in one launch: each has the bits of its own launch; 17 go
    through the wrapper's split."""
    key = max({(c.heads, c.f16, c.prescaled) for c in P.CASES},
              key=lambda k: len([c for c in P.CASES if (c.heads, c.f16, c.prescaled) == k and c.nq <= 200]))
    pool = [c for c in P.CASES if (c.heads, c.f16, c.prescaled) == key and c.nq <= 200]
    assert len(pool) >= 3 and len({(c.nq, c.n0, c.n1, c.C) for c in pool}) >= 3, pool
    pool.sort(key=lambda c: -c.C * c.nq)                        # the largest first: the grid is sized for the largest
    cases = [pool[i % len(pool)] for i in range(n)][::-1 if n == 16 else 1]
    got = run(cases, Guarded())
    for i, (c, g) in enumerate(zip(cases, got)):
        assert_same_bits(g, single(c), f"problem {i} ({c.id}) of {n}")


@pytest.mark.parametrize("f16", [False, True])
def test_a_query_row_has_the_same_bits_at_rows_0_17_and_200(f16):
    """The same q row at rows 0, 17 and 200 of a 216-row problem (another row block, another group of 16, another lane): the
    three columns of the output are equal bit for bit, and differ from their neighbours."""
    heads, n0, n1, C = 3, 77, 200, 5
    W = heads * 128
    g = T._gen(f"propmap.row200.{f16}")
    q = torch.randn(216, W, generator=g)
    q[200] = q[17] = q[0]
    k = torch.randn(n0 + n1, W, generator=g)
    v = torch.randn(C, n1, generator=g).to(DEV)
    qd = P.to_bits(q, f16).to(DEV).view(torch.bfloat16)
    kd = P.to_bits(k, f16).to(DEV).view(torch.bfloat16)
    acc2 = torch.zeros(C, 216, device=DEV)
    ops.propagate_maps([ops.PropagateMaps(qd, kd[:n0], kd[n0:], v, acc2=acc2, weight2=1.0)], heads, P.SCALE_LOG2, qk_f16=f16)
    torch.cuda.synchronize()
    for r in (17, 200):
        assert torch.equal(_bytes(acc2[:, r]), _bytes(acc2[:, 0]))
    assert not torch.equal(acc2[:, 1], acc2[:, 0]) and not torch.equal(acc2[:, 201], acc2[:, 200])
    assert bool(torch.isfinite(acc2).all())


@pytest.mark.parametrize("f16", [False, True])
def test_nan_rules(f16):
    case = next(c for c in P.CASES if c.f16 == f16 and c.n0 > 0 and c.nq >= 15 and c.C >= 5 and c.n1 >= 31 and c.heads >= 2
                and c.vkind in ("softmax", "normal"))
    W = case.heads * 128
    clean = single(case)
    assert bool(torch.isfinite(clean["acc"]).all())

    def put(name, row, col, value=P.NAN_BITS):
        def edit(host):
            host[name][row, col] = value
        return edit
    # a NaN in head 1 of query row 3: that query's cells in every map row, nothing else
    got = run([case], Guarded(), edit=put("q", 3, 128 + 5))[0]
    keep = [i for i in range(case.nq) if i != 3]
    for k in ("acc", "acc2"):
        assert bool(torch.isnan(got[k][:, 3]).all())
        assert torch.equal(_bytes(got[k][:, keep]), _bytes(clean[k][:, keep]))
    # a NaN in a key row (a valued key, then a leading key): every cell
    for name, row in (("k1", case.n1 - 1), ("k0", case.n0 - 1)):
        got = run([case], Guarded(), edit=put(name, row, W - 1))[0]
        assert bool(torch.isnan(got["acc"]).all()) and bool(torch.isnan(got["acc2"]).all())
    # a NaN in v[2, j]: row 2, and the other rows keep their bits
    got = run([case], Guarded(), edit=put("v", 2, case.n1 // 2, NAN))[0]
    rest = [r for r in range(case.C) if r != 2]
    for k in ("acc", "acc2"):
        assert bool(torch.isnan(got[k][2]).all())
        assert torch.equal(_bytes(got[k][rest]), _bytes(clean[k][rest]))


def test_a_constant_map_without_leading_keys_returns_the_constant():
    hit = 0
    for case in P.CASES:
        if case.vkind != "const" or case.n0:
            continue
        _, bound = P.reference(case)
        got = single(case)["acc2"].double().cpu()
        assert bool(((got - P.CONST).abs() <= bound).all()), (case.id, float(((got - P.CONST).abs() / bound).max()))
        hit += 1
    assert hit >= 1


# ---- cross-checks against ca_query_maps: out = map . v^T, with map the [nq, n1] head-mean probabilities ca_query_maps
# emits.  A one-hot v (one key per map row) picks the map's column of that key; a general v is the fp64 product of the
# emitted map with v^T, inside the two bounds added (query_maps' bound carried through the product with |v|).
CROSS = [c for c in P.CASES if c.nq <= 512 and c.heads <= 5 and (c.vkind == "onehot" or c.n1 <= 129)]


def _query_map(case):
    inp = P.make_inputs(case)
    d = {n: P.view(case, inp["buffers"], n).contiguous().to(DEV).view(torch.bfloat16) for n in ("q", "k1")}
    k0 = torch.cat([P.view(case, inp["buffers"], "k0"), P.view(case, inp["buffers"], "k1")]).to(DEV).view(torch.bfloat16)
    acc2 = torch.zeros(case.nq, case.n1, device=DEV)
    ops.query_maps([ops.QueryMaps(d["q"], k0[:case.n0] if case.n0 else None, k0[case.n0:], acc2=acc2, weight2=1.0)],
                   case.heads, case.scale_log2, qk_f16=case.f16)
    torch.cuda.synchronize()
    q, k, _ = P.operands(case)
    return acc2.double().cpu(), Q.reference_qk(q, k, case.n0, case.scale_log2)[2].maps


@pytest.mark.parametrize("case", CROSS, ids=lambda c: c.id)
def test_the_output_is_query_maps_times_v(case):
    assert any(c.vkind == "onehot" for c in CROSS) and any(c.vkind != "onehot" for c in CROSS)
    got = single(case)["acc2"]
    qmap, qbound = _query_map(case)
    v = P.operands(case)[2]
    _, bound = P.reference(case)
    if case.vkind == "onehot":                      # (keys shared by two map rows add up: the product below covers both)
        cols = [P.onehot_key(case, r) for r in range(case.C)]
        if len(set(cols)) == len(cols):
            assert torch.equal((qmap @ v.T).T, qmap[:, cols].T)
    want = (qmap @ v.T).T
    worst, n_over = P.over_the_bound(got, want, bound + (qbound @ v.abs().T).T)
    print(f"\n  {case.id}: |propagate_maps - query_maps v^T| / (bound + bound)  {worst:.3f}")
    assert n_over == 0, (case.id, worst)
