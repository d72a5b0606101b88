"""ca_query_maps on the device, every case of tests/querymap_cases.py: the accumulators and lse against the fp64 reference
inside the derived bound, the same bits from a second launch and over a garbage workspace, a problem alone against the
same problem among 16 (and among 17 through the wrapper's split), a query row at row 0 and at row 200, NaN rows, and the
cross-checks against ca_token_maps on swapped roles.

Every buffer a launch sees is cut out of a larger allocation with guard elements on both sides; whatever a launch may not
read is NaN (querymap_cases.make_inputs), lse starts as NaN: an element never written fails its bound, and a guard must
come back as it was.  max err / bound is printed per case and per family (pytest -s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import querymap_cases as Q  # noqa: E402
import tokmap_cases as T  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
NAN = float("nan")
GUARD = 64          # elements on either side of every buffer
WORST = {}          # family -> (largest max err / bound over the maps, over acc from its non-zero start, over lse)


def test_the_library_exports_the_entry():
    lib = L.load()
    assert hasattr(lib, "ca_query_maps") and hasattr(lib, "ca_query_maps_workspace_bytes")
    assert callable(ops.query_maps) and callable(ops.query_maps_workspace_bytes)


class Guarded:
    """Buffers with GUARD elements in front and behind (NaN; the NaN bit pattern / 0x5A for the integer types)."""

    def __init__(self):
        self.whole = []

    def _cut(self, shape, dtype):
        n = 1
        for d in shape:
            n *= d
        fill = NAN if dtype.is_floating_point else (Q.NAN_BITS if dtype == torch.int16 else 0x5A)
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


def place(case, al, outs=None, tag="", edit=None):
    """The device operands of one problem.  ``edit(buffers)`` may change the host copies of the input buffers first."""
    outs = case.outs if outs is None else outs
    inp = Q.make_inputs(case)
    host = {k: v.clone() for k, v in inp["buffers"].items()}
    if edit:
        edit(host)
    bufs = {name: al.to(b, {name + tag: None}) for name, b in host.items()}
    d = dict(bufs=bufs, before={k: v.clone() for k, v in bufs.items()})
    for name in ("q", "k0", "k1"):
        d[name] = Q.view(case, bufs, name).view(torch.bfloat16)
    if "acc" in outs:
        d["acc"] = al.to(inp["acc0"], {"acc" + tag: None})
    if "acc2" in outs:
        d["acc2"] = al.to(inp["acc20"], {"acc2" + tag: None})
    if "lse" in outs:
        d["lse"] = al.full((case.heads, case.nq), NAN, torch.float32, {"lse" + tag: None})
    return d


def problem(case, d):
    return ops.QueryMaps(d["q"], d["k0"] if case.n0 else None, d["k1"], acc=d.get("acc"), weight=Q.W1, acc2=d.get("acc2"),
                         weight2=Q.W2, lse=d.get("lse"))


def outputs(d):
    return {k: d[k] for k in ("acc", "acc2", "lse") if k in d}


def run(cases, al, outs=None, workspace=None, edit=None):
    """One ops.query_maps call over ``cases`` (they share heads, storage type and scale); -> the outputs per problem."""
    c0 = cases[0]
    assert all((c.heads, c.f16, c.prescaled) == (c0.heads, c0.f16, c0.prescaled) for c in cases)
    dev = [place(c, al, outs, tag=f"[{i}]", edit=edit) for i, c in enumerate(cases)]
    ops.query_maps([problem(c, d) for c, d in zip(cases, dev)], c0.heads, c0.scale_log2, qk_f16=c0.f16, workspace=workspace)
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


@pytest.mark.parametrize("case", Q.CASES, ids=lambda c: c.id)
def test_every_case_against_fp64(case):
    got = single(case)
    assert set(got) == set(case.outs)
    # acc2 starts at zero and has weight 1, so it holds fma(1, map, 0) = the map, bit for bit, and is held to the map's own
    # bound (a zero or a doubled cold cell fails here); acc += weight * map from N(0, 0.1): one fused multiply-add on top
    worst = Q.check_outputs(case, got)
    print(f"\n  {case.id}: max err / bound  " + "  ".join(f"{k} {v[0]:.3f}" for k, v in worst.items()))
    old = WORST.get(case.family, (0.0, 0.0, 0.0))
    WORST[case.family] = tuple(max(o, worst.get(k, (0.0, 0))[0]) for o, k in zip(old, ("maps", "acc", "lse")))
    assert_same_bits(got, run([case], Guarded())[0], "second launch")
    for name, (ratio, n_over) in worst.items():
        assert n_over == 0, f"{case.id}: {name}: {n_over} elements over the bound (NaN = never written), max err / bound {ratio:.3g}"


def test_print_the_largest_ratio_per_family():
    for case in Q.CASES:                                        # (cached when the cases above ran in this process)
        if case.family not in WORST:
            test_every_case_against_fp64(case)
    print()
    for fam in Q.FAMILIES:
        print(f"  {fam:14s} largest max err / bound: maps {WORST[fam][0]:.3f}  acc (non-zero start) {WORST[fam][1]:.3f}  "
              f"lse {WORST[fam][2]:.3f}")
    assert set(WORST) == set(Q.FAMILIES)


ACC_CASE = next(c for c in Q.CASES if c.family == "unit" and c.heads == 3 and c.n0 == 77 and c.outputs == Q.OUTPUTS[0] and not c.f16)


@pytest.mark.parametrize("outputs_", Q.OUTPUTS[1:])
def test_each_accumulator_alone_has_the_bits_it_has_beside_the_other(outputs_):
    """The cases with one accumulator, or without lse, share their operands' shapes with ACC_CASE but not its seed; here
    ACC_CASE itself is run with each output set: whatever is asked for has the bits of the run that asked for everything."""
    outs = tuple(outputs_.split("+"))
    both = single(ACC_CASE)
    got = run([ACC_CASE], Guarded(), outs=outs)[0]
    assert set(got) == set(outs)
    assert_same_bits(got, {k: both[k] for k in outs}, outputs_)
    inp = Q.make_inputs(ACC_CASE)
    assert float(inp["acc0"].abs().min()) > 0 and not torch.equal(both["acc"].cpu(), inp["acc0"])


def test_a_garbage_workspace_changes_nothing_and_is_written_inside_its_size_only():
    al = Guarded()
    need = ops.query_maps_workspace_bytes([problem(ACC_CASE, place(ACC_CASE, Guarded()))], ACC_CASE.heads)
    assert need == (ACC_CASE.heads * ACC_CASE.nq * 8 + 15) // 16 * 16
    ws = al.full((need + 4096,), 0xA5, torch.uint8)
    got = run([ACC_CASE], al, workspace=ws[:need])[0]
    assert bool((ws[need:] == 0xA5).all()), "the workspace was written beyond ca_query_maps_workspace_bytes()"
    assert_same_bits(got, single(ACC_CASE), "garbage workspace")
    with pytest.raises(ValueError, match="workspace too small"):
        run([ACC_CASE], Guarded(), workspace=ws[:need - 16])


@pytest.mark.parametrize("n", [16, 17])
def test_a_problem_alone_has_the_bits_it_has_inside_a_launch(n):
    """Problems of different shapes (nq, n0, n1, layout) in one launch: each has the bits of its own launch; 17 go through
    the wrapper's split."""
    pool = [c for c in Q.CASES if (c.heads, c.f16, c.prescaled) == (2, False, False) and c.nq <= 77]
    assert len(pool) >= 5 and len({(c.nq, c.n0, c.n1) for c in pool}) >= 4
    pool.sort(key=lambda c: -c.n1 * c.nq)                       # the largest first: the grid is sized for the largest
    cases = [pool[i % len(pool)] for i in range(n)][::-1 if n == 16 else 1]
    got = run(cases, Guarded())
    for i, (c, g) in enumerate(zip(cases, got)):
        assert_same_bits(g, single(c), f"problem {i} ({c.id}) of {n}")


@pytest.mark.parametrize("f16", [False, True])
def test_a_query_row_has_the_same_bits_at_row_0_and_at_row_200(f16):
    """The same q row at rows 0, 17 and 200 of a 216-row problem (another row block, another lane): the three rows of the map
    and of lse are equal bit for bit, and differ from their neighbours."""
    heads, n0, n1 = 3, 77, 200
    W = heads * 128
    g = T._gen(f"querymap.row200.{f16}")
    q = torch.randn(216, W, generator=g)
    q[200] = q[17] = q[0]
    k = torch.randn(n0 + n1, W, generator=g)
    qd = Q.to_bits(q, f16).to(DEV).view(torch.bfloat16)
    kd = Q.to_bits(k, f16).to(DEV).view(torch.bfloat16)
    acc2 = torch.zeros(216, n1, device=DEV)
    lse = torch.full((heads, 216), NAN, device=DEV)
    ops.query_maps([ops.QueryMaps(qd, kd[:n0], kd[n0:], acc2=acc2, weight2=1.0, lse=lse)], heads, Q.SCALE_LOG2, qk_f16=f16)
    torch.cuda.synchronize()
    for r in (17, 200):
        assert torch.equal(_bytes(acc2[r]), _bytes(acc2[0])) and torch.equal(_bytes(lse[:, r]), _bytes(lse[:, 0]))
    assert not torch.equal(acc2[1], acc2[0]) and not torch.equal(acc2[201], acc2[200])
    assert bool(torch.isfinite(acc2).all()) and bool(torch.isfinite(lse).all())


@pytest.mark.parametrize("f16", [False, True])
def test_nan_rows(f16):
    case = next(c for c in Q.CASES if c.family == "unit" and c.heads == 3 and c.f16 == f16 and c.n0 == 77 and c.outputs == Q.OUTPUTS[0])
    W = case.heads * 128
    clean = single(case)

    def put(name, row, col):
        def edit(host):
            b, r0, _, c0 = Q.make_inputs(case)["views"][name]
            host[b][r0 + row, c0 + col] = Q.NAN_BITS
        return edit
    # a NaN in head 1 of query row 3: that row's cells and that head's lse, nothing else
    got = run([case], Guarded(), edit=put("q", 3, 128 + 5))[0]
    for k in ("acc", "acc2"):
        assert bool(torch.isnan(got[k][3]).all())
        keep = [i for i in range(case.nq) if i != 3]
        assert torch.equal(_bytes(got[k][keep]), _bytes(clean[k][keep]))
    nan_lse = torch.isnan(got["lse"])
    assert bool(nan_lse[1, 3]) and int(nan_lse.sum()) == 1
    # a NaN in a key row (an emitted key, then a leading key): every cell
    for name, row in (("k1", case.n1 - 1), ("k0", case.n0 - 1)):
        got = run([case], Guarded(), edit=put(name, row, W - 1))[0]
        assert bool(torch.isnan(got["acc"]).all()) and bool(torch.isnan(got["acc2"]).all())
        assert bool(torch.isnan(got["lse"][case.heads - 1]).all()) and not bool(torch.isnan(got["lse"][0]).any())


# ---- cross-checks against ca_token_maps.  A softmax does not care in which order its keys come, so with the emitted keys
# handed to ca_token_maps as its (at most 512) text keys and the leading keys as its image keys,
#     query_maps(q, k0 = A, k1 = B).map[i, j]  ==  token_maps(q, k0 = B, k1 = A, n_tok = |B|).map[j, i],
# each inside its own derived bound, so their difference inside the two bounds added; lse likewise.
CROSS = [c for c in Q.CASES if c.n1 <= 512 and c.nq <= 77 and c.outputs == Q.OUTPUTS[0]
         and (c.n0 == 0 or c.family in ("cold_text", "ties") or c.n1 in (1, 15, 64))]


@pytest.mark.parametrize("case", CROSS, ids=lambda c: c.id)
def test_the_map_is_token_maps_on_swapped_roles_transposed(case):
    assert any(c.n0 == 0 for c in CROSS) and any(c.n0 > 0 for c in CROSS)
    got = single(case)
    inp = Q.make_inputs(case)
    dev = {"q": Q.view(case, inp["buffers"], "q").contiguous().to(DEV).view(torch.bfloat16)}
    # (the emitted rows, then the leading rows, in one allocation: one row stride, whatever the row counts)
    keys = torch.cat([Q.view(case, inp["buffers"], n) for n in ("k1", "k0")]).to(DEV).view(torch.bfloat16)
    dev["k1"], dev["k0"] = keys[:case.n1], keys[case.n1:]
    acc2 = torch.zeros(case.n1, case.nq, device=DEV)
    lse = torch.full((case.heads, case.nq), NAN, device=DEV)
    ops.token_maps([ops.TokenMaps(dev["q"], dev["k1"], dev["k0"] if case.n0 else None, case.n1, acc2=acc2, weight2=1.0, lse=lse)],
                   case.heads, case.scale_log2, qk_f16=case.f16)
    torch.cuda.synchronize()
    q, k = Q.operands(case)
    _, _, tb = T.reference_qk(q, torch.cat([k[case.n0:], k[:case.n0]]), case.n1, case.scale_log2)
    maps, _, qb = Q.reference(case)
    worst, n_over = Q.over_the_bound(got["acc2"], acc2.T.double().cpu(), qb.maps + tb.maps.T)
    worst_lse, n_lse = Q.over_the_bound(got["lse"], lse.double().cpu(), qb.lse + tb.lse)
    print(f"\n  {case.id}: |query_maps - token_maps^T| / (bound + bound)  maps {worst:.3f}  lse {worst_lse:.3f}")
    assert n_over == 0 and n_lse == 0, (case.id, worst, worst_lse)


def test_without_leading_keys_the_rows_sum_to_one_inside_the_bound():
    hit = 0
    for case in Q.CASES:
        if case.n0 or "acc2" not in case.outs:
            continue
        _, _, bound = Q.reference(case)
        rows = single(case)["acc2"].double().cpu().sum(1)
        tol = bound.maps.sum(1)
        assert bool(((rows - 1).abs() <= tol).all()), (case.id, float(((rows - 1).abs() / tol).max()))
        hit += 1
    assert hit >= 4
