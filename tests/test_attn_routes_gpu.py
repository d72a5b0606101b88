"""Every launch form of the attention kernels (tests/attn_cases.py) through ops.attention, against an fp64 reference of
the same attention on the same inputs with derived bounds, and bit for bit where the kernels promise it.

Every output and its padding is filled with NaN before the launch: the bf16 rows and the rows between the two query
segments, the fp32 copy (one row and the columns past heads * 128 beyond the problem), hm_part with its columns
c >= hm_C.  An element the kernel never writes fails its bound; every byte it does not own must come back unchanged,
as must the inputs.  max err / bound is printed per case and output (pytest -s).

On MI355X the file runs in about 12 s.  Largest max err / bound: bf16 outputs 0.500 (the half-ulp store), fp32
copies 0.019 on exact probes (ca_attn4, both operand types; bit-exact) and 0.801 on logits of std 8 nats, hm_part
0.045; the table is in attn_cases.py."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_cases as A  # noqa: E402
import placement  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
NAN = float("nan")
ROWS = 512          # reference row chunk


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def launch(case, inp, alloc=None):
    """Run the case; returns per problem the output buffers and the owned masks.  `alloc` (tests/placement.py) decides
    where every buffer the kernel sees lies; by default they are ordinary torch allocations."""
    al = alloc or placement.Plain(DEV)
    D = case.heads * 128
    attns, res = [], []
    for p, x in zip(case.probs, inp):
        nq1 = p.nq - p.nq0 if p.two_q else 0
        nq0 = p.nq - nq1
        qroles = {"q": placement.mid(x.gq0, nq0, x.ldq, 0, D)}
        oroles = {"out": placement.mid(x.gq0, nq0, x.ldo, 0, D)}
        if nq1:
            qroles["q1"] = placement.mid(x.gq1, nq1, x.ldq, 0, D)
            oroles["out1"] = placement.mid(x.gq1, nq1, x.ldo, 0, D)
        kroles = {"k0/v0": placement.mid(x.gk0, p.n0, x.ldkv, D, D)}
        if p.n1:
            kroles["k1/v1"] = placement.mid(x.gk1, p.n1, x.ldkv, D, D)
        qbuf, kvbuf = al.to(x.qbuf, qroles), al.to(x.kvbuf, kroles)
        gx = dataclasses.replace(x, qbuf=qbuf, kvbuf=kvbuf)
        q0, q1, k0, v0, k1, v1 = A.views(case, p, gx)
        assert nq1 == (q1.shape[0] if q1 is not None else 0)
        out = al.full((x.out_rows, x.ldo), NAN, torch.bfloat16, oroles)
        own = torch.zeros(out.shape, dtype=torch.bool, device=DEV)
        own[x.gq0:x.gq0 + nq0, :D] = True
        own[x.gq1:x.gq1 + nq1, :D] = True
        f32 = al.full((p.nq + 1, x.ldo32), NAN, torch.float32,
                      {"out_f32": placement.mid(0, p.nq, x.ldo32, 0, D)}) if p.f32 else None
        hmcon = al.to(x.hmbuf, {"hm_con": placement.mid(0, p.hm_C, x.ldhc, 0, D)}) if x.hmbuf is not None else None
        hmp = al.full((case.heads, nq1, 8), NAN, torch.float32, {"hm_part": None}) if p.hm_C else None
        attns.append(ops.Attn(q0, out[x.gq0:x.gq0 + nq0, :D], k0, v0, k1, v1,
                              out_f32=f32[:p.nq, :D] if f32 is not None else None,
                              q1=q1, out1=out[x.gq1:x.gq1 + nq1, :D] if nq1 else None,
                              hm_con=hmcon[:, :D] if hmcon is not None else None, hm_part=hmp))
        res.append(dict(x=gx, qbuf0=qbuf.clone(), kvbuf0=kvbuf.clone(), out=out, own=own, f32=f32, hmcon=hmcon,
                        hmcon0=None if hmcon is None else hmcon.clone(), hm=hmp, nq0=nq0, nq1=nq1))
    kw = dict(scale=case.scale) if case.form == "scale" else dict(q_prescaled=True, qk_f16=case.form == "qk16")
    ops.attention(attns, case.heads, **kw)
    torch.cuda.synchronize()
    return res


def rows_of(r):
    """The bf16 output rows in problem row order."""
    x = r["x"]
    D = x.D
    parts = [r["out"][x.gq0:x.gq0 + r["nq0"], :D]]
    if r["nq1"]:
        parts.append(r["out"][x.gq1:x.gq1 + r["nq1"], :D])
    return torch.cat(parts)


def check_untouched(case, res):
    for i, r in enumerate(res):
        x = r["x"]
        assert torch.equal(_bytes(x.qbuf), _bytes(r["qbuf0"])), f"{case.id}[{i}]: q buffer changed"
        assert torch.equal(_bytes(x.kvbuf), _bytes(r["kvbuf0"])), f"{case.id}[{i}]: k / v buffer changed"
        if r["hmcon"] is not None:
            assert torch.equal(_bytes(r["hmcon"]), _bytes(r["hmcon0"])), f"{case.id}[{i}]: hm_con changed"
        assert bool(r["out"][~r["own"]].isnan().all()), f"{case.id}[{i}]: bf16 bytes outside the output rows written"
        if r["f32"] is not None:
            D = x.D
            assert bool(r["f32"][-1].isnan().all()) and bool(r["f32"][:, D:].isnan().all()), \
                f"{case.id}[{i}]: out_f32 padding written"
        if r["hm"] is not None:
            C = r["hmcon"].shape[0]
            assert bool(r["hm"][..., C:].isnan().all()), f"{case.id}[{i}]: hm_part columns >= hm_C written"


RATIOS = {}


def check_bounds(case, inp, res):
    exact_bits = True
    for i, (p, x, r) in enumerate(zip(case.probs, inp, res)):
        ref, pre, hm, hm_pre = A.reference(case, p, x, dev=DEV, rows=ROWS)
        got = rows_of(r)
        fam = "probe" if case.exact else case.family if case.family != "probe" else "spiked probe"
        checks = [("out", got, ref, pre, "bf16")]
        if r["f32"] is not None:
            g32 = r["f32"][:p.nq, :x.D]
            checks.append(("out_f32", g32, ref, pre, "f32"))
            if case.exact:
                assert torch.equal(_bytes(got), _bytes(g32.bfloat16())), \
                    f"{case.id}[{i}]: bf16 output is not the RNE rounding of the fp32 copy"
                exact_bits &= bool((g32.double() == ref.float().double()).all())
        if hm is not None:
            checks.append(("hm_part", r["hm"][..., :p.hm_C], hm, hm_pre, "f32"))
        for name, g, rf, pr, kind in checks:
            ratio, n_over = A.excess(g, rf, pr, kind)
            key = (case.kernel, fam, name)
            RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
            print(f"{case.id}[{i}] {name}: max err / bound {ratio:.3f}")
            assert n_over == 0, f"{case.id}[{i}] {name}: {n_over} elements over the bound (max err / bound {ratio:.3g})"
    if case.exact and any(p.f32 for p in case.probs):
        print(f"{case.id}: fp32 copy {'bit-exact' if exact_bits else 'NOT bit-exact'} against the fp64 reference")


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.id)
def test_attention_case(case):
    inp = A.make_inputs(case)
    a4 = case.form != "scale"
    if a4:
        ops.attention_stats(reset=True)
    res = launch(case, inp)
    check_untouched(case, res)
    check_bounds(case, inp, res)
    if a4:
        st = ops.attention_stats()
        want = A.expected_stats(case)
        got = (st["recomputed_workgroups"], st["rereference_events"])
        print(f"{case.id}: counters {got}")
        for w, g, n in zip(want, got, ("recomputed_workgroups", "rereference_events")):
            if w is not None:
                assert g == w, f"{case.id}: {n} {g}, expected {w}"
        if case.family == "structured_far":
            assert got[1] > 0


WALK = [c for c in A.CASES if len(c.probs) == 16 and c.form != "scale"]


@pytest.mark.parametrize("case", WALK, ids=lambda c: c.id)
def test_launch_composition_bit_identity(case):
    """"An item's bits do not depend on the launch it shares" (ca_attn4_kernel.inc): every problem alone gives the
    bits it gives as problem k of 16, also when the 16 run as a persistent walk."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    hx = (case.heads + 7) // 8
    total = sum(8 * hx * ((p.nq + 255) // 256) for p in case.probs)     # as ca_attn_fwd_impl
    assert total == A.units(case)[0]
    walk = n_cu % 8 == 0 and total > n_cu
    assert walk == ("walk" in case.id and A.walks(case, n_cu)), (n_cu, total)
    inp = A.make_inputs(case)
    together = launch(case, inp)
    for i, (p, x) in enumerate(zip(case.probs, inp)):
        alone = launch(dataclasses.replace(case, probs=(p,)), [x])[0]
        assert torch.equal(_bytes(alone["out"]), _bytes(together[i]["out"])), f"{case.id}: problem {i} bf16 bits"
        if p.f32:
            assert torch.equal(_bytes(alone["f32"]), _bytes(together[i]["f32"])), f"{case.id}: problem {i} fp32 bits"


CROSS = [c for c in A.CASES if c.form == "pre" and c.exact]


@pytest.mark.parametrize("case", CROSS, ids=lambda c: c.id)
def test_attn4_bf16_and_f16_kernels_agree_bit_for_bit_on_exact_probes(case):
    """Exact-probe q and k are exact in bf16 and in half: ca_attn4_kernel and ca_attn4_qk16_kernel give the same bits."""
    twin = dataclasses.replace(case, form="qk16")
    a = launch(case, A.make_inputs(case))
    b = launch(twin, A.make_inputs(twin))
    for i, (ra, rb) in enumerate(zip(a, b)):
        assert torch.equal(_bytes(ra["out"]), _bytes(rb["out"])), f"{case.id}[{i}]: bf16 bits differ"
        for k in ("f32", "hm"):
            if ra[k] is not None:
                assert torch.equal(_bytes(ra[k]), _bytes(rb[k])), f"{case.id}[{i}]: {k} bits differ"


def test_attention_rejects_views_narrower_than_the_heads():
    """A q / out / k / v view narrower than num_heads * 128 inside a wider buffer is refused before any launch (the
    kernel would read and write the columns beyond the view); the buffers come back unchanged."""
    nh, n = 2, 100
    buf = torch.randn(n, 3 * nh * 128 + 64, device=DEV).bfloat16()
    out = torch.full((n, nh * 128 + 64), NAN, device=DEV, dtype=torch.bfloat16)
    b0, o0 = buf.clone(), out.clone()
    q, k, v = buf[:, :nh * 128], buf[:, nh * 128:2 * nh * 128], buf[:, 2 * nh * 128:3 * nh * 128]
    with pytest.raises(ValueError, match="out"):
        ops.attention([ops.Attn(q, out[:, :128], k, v)], nh)
    with pytest.raises(ValueError, match="k1"):
        ops.attention([ops.Attn(q, out[:, :nh * 128], k[:50], v[:50], k[50:, :128], v[50:])], nh, q_prescaled=True)
    torch.cuda.synchronize()
    assert torch.equal(_bytes(buf), _bytes(b0)) and torch.equal(_bytes(out), _bytes(o0))
    ops.attention([ops.Attn(q, out[:, :nh * 128], k, v)], nh)       # the full-width views are accepted
    torch.cuda.synchronize()
    assert bool(out[:, nh * 128:].isnan().all())


def test_print_largest_ratios():
    """(runs last in this file) the largest max err / bound per kernel, input family and output."""
    for key in sorted(RATIOS):
        print("max err / bound", *key, f"{RATIOS[key]:.3f}")
