"""The case table and the emulation of tests/fp8_edge_cases.py, without a GPU: the emulation meets the e4m3 value-range
contract (P1 .. P5, ``rows``) on every case, every named slip breaks its clause, the families are all there, and the
``launder`` slip -- the clamp the kernels had -- reproduces what an MI355X wrote for the special rows before the contract
was stated (tests/golden/text_parent_records.npz), bytes and scales: the recorded kernels fail P2."""
import os

import numpy as np
import pytest
import torch

import fp8_edge_cases as E
import t5_cases as T5
import t5_fp8_cases as F8

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_parent_records.npz")


@pytest.fixture(scope="module")
def runs():
    """case id -> (inputs, y32, emulated outputs, emulated outputs of the replaced inputs), computed once."""
    out = {}
    for c in E.CASES:
        inp = E.make_inputs(c)
        out[c.id] = (inp, E.y32(c, inp), E.emulate(c, inp), E.emulate(c, E.replaced(c, inp)))
    return out


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c.id)
def test_the_emulation_meets_the_contract(runs, case):
    inp, y, got, twin = runs[case.id]
    assert E.violations(y, got, twin) == set()
    rs, rv = E.p5_ratios(case, inp, *got)
    assert rs <= 1 and rv <= 1, (rs, rv)
    # P1: on the rows the contract leaves alone, the emulation is t5_fp8_cases.pack_row (the kernels' rule so far)
    q, s = got
    q0, s0 = F8.pack_row(y)
    old = torch.isfinite(y).all(-1) & ((y.abs().amax(-1) * torch.tensor(1 / 448.0)) >= E.FLT_MIN) | (y == 0).all(-1)
    assert (old.any() or case.variant != "x") and torch.equal(q[old], q0[old]) and torch.equal(s[old], s0[old])


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c.id)
def test_the_replaced_inputs_are_the_row_with_its_nan_elements_zero(runs, case):
    """What lets the GPU test state P3 with two launches: on every NaN row that has other non-zero elements, the y of the
    replaced inputs is the y of the inputs with 0 at the NaN positions, bit for bit; every clean row is untouched."""
    inp, y, _, _ = runs[case.id]
    y2 = E.y32(case, E.replaced(case, inp))
    _, _, elementwise, clean = E.row_kinds(y)
    nan = torch.isnan(y)
    want = torch.where(nan, torch.zeros_like(y), y)
    for rows in (elementwise, clean):
        assert torch.equal(y2[rows].abs().view(torch.int32), want[rows].abs().view(torch.int32))
        assert torch.equal(torch.signbit(y2[rows])[~nan[rows]], torch.signbit(want[rows])[~nan[rows]])
    assert torch.isfinite(y2[clean]).all()


@pytest.mark.parametrize("slip", sorted(E.SLIPS))
def test_every_slip_breaks_its_clause(runs, slip):
    """On every case that reaches the clause: an infinite y for P4 (a NaN or an inf in the x of a norm gives NaN only), a
    clean row behind a special one for ``rows`` and a clean tiny row for P5 (the weight variants have no clean row)."""
    clause, seen = E.SLIPS[slip], set()
    for c in E.CASES:
        inp, y, _, _ = runs[c.id]
        if slip == "inf_to_max" and not E.row_kinds(y)[0].any() or slip in ("leak", "no_floor") and c.variant != "x":
            continue
        bad = E.violations(y, E.emulate(c, inp, slip), E.emulate(c, E.replaced(c, inp), slip))
        assert clause in bad, (c.id, slip, bad)
        seen.add(c.producer)
    assert seen == set(E.PRODUCERS)


def test_family_shares():
    for c in E.CASES:
        inp = E.make_inputs(c)
        y = E.y32(c, inp)
        fams = c.families
        assert len(fams) == E.N_ROWS and set(fams) == set(E.FAMILIES), c.id
        assert 8 <= E.N_ROWS <= 12
        for r, f in enumerate(fams):
            if c.variant != "x":
                continue
            row = y[r]
            norm = c.producer in ("ln_fp8", "ln_f32in_fp8", "t5_rmsnorm_fp8")     # a NaN in x takes the whole row
            if f == "plain":
                assert torch.isfinite(row).all() and row.abs().max() * (1 / 448.0) >= E.FLT_MIN
            elif f == "zero":
                assert (row == 0).all()
            elif f == "tiny":
                a = row.abs()
                assert torch.isfinite(row).all() and 0 < a.max() / 448.0 < E.FLT_MIN
                assert (a[a > 0] >= E.FLT_MIN).all() and (a == 0).float().mean() >= (0.25 if c.width > 8 else 0.125)
            elif f in ("pinf", "ninf") and not norm:
                cols = E.special_columns(c.producer, c.width)
                assert torch.isinf(row[cols]).all() and torch.isfinite(row).sum() == c.width - len(cols)
                assert (row[cols] > 0).all() == (f == "pinf")
            elif f == "all_nan" or norm:
                assert torch.isnan(row).any()
                if c.producer != "t5_rmsnorm_fp8" or f not in ("pinf", "ninf"):
                    assert torch.isnan(row).all() == (norm or f == "all_nan")
            else:
                cols = E.special_columns(c.producer, c.width)
                assert torch.isnan(row[cols]).all() and torch.isnan(row).sum() == len(cols)
    # the tiny set itself: normal numbers of 2^-125 .. 2^-120 and zeros, a third of them
    t = E.tiny_values((64, 4096), "shares")
    a = t.abs()
    assert set(torch.log2(a[a > 0]).tolist()) == {-125.0, -124.0, -123.0, -122.0, -121.0, -120.0}
    assert (a == 0).float().mean() >= 1 / 3 - 0.01 and (t < 0).any() and (t > 0).any()
    # the signalling pattern survives the way into the inputs
    c = E.Case("quantize_rows", 264, False)
    assert int(E.make_inputs(c)["x"].view(torch.int16)[5, 0]) == 0x7F81
    c = E.Case("t5_rmsnorm_fp8", 264, False)
    assert int(E.make_inputs(c)["x"].view(torch.int32)[5, 0]) == 0x7F810000


# outputs 89, 90 (t5_rmsnorm_fp8 specials: bytes, scales) and 94, 95 (gated_mul_fp8 specials) of the ``rows`` family, in the
# order tests/test_text_parent_records_gpu.py yields them (both are stored whole)
RECORDED = {"t5_rmsnorm_fp8": (89, 90), "gated_mul_fp8": (94, 95)}
FLT_MAX, BF16_MAX = 3.4028234663852886e38, 3.3895313892515355e38


def _special_rows(x, big):
    x = x.clone()
    x[0] = 0
    x[1, 3], x[2, x.shape[1] // 2], x[3, x.shape[1] - 1] = E.INF, E.NAN, big
    return x


@pytest.mark.parametrize("producer", sorted(RECORDED))
def test_the_launder_slip_is_what_the_device_wrote(producer):
    rec = np.load(FIXTURE)
    lens, data = rec["rows.len"], rec["rows.bytes"]
    ends = np.cumsum(lens)
    iq, isc = RECORDED[producer]
    assert lens[iq] == 5 * 264 and lens[isc] == 5 * 4
    q_dev = torch.from_numpy(data[ends[iq] - lens[iq]:ends[iq]].copy()).reshape(5, 264)
    s_dev = torch.from_numpy(data[ends[isc] - lens[isc]:ends[isc]].copy()).view(torch.float32)
    if producer == "t5_rmsnorm_fp8":
        x, w = T5.row_inputs(264, 5)
        y = F8.rmsnorm_y32(_special_rows(x, FLT_MAX), w)
    else:
        g, u = T5.gate_inputs(264, 5)
        y = _special_rows(g, BF16_MAX).to(torch.bfloat16).float() * u.to(torch.bfloat16).float()
    q, s = E.pack_rows(y, "launder")
    for r in (1, 2):
        assert torch.equal(q[r], q_dev[r]), (producer, r)
        assert torch.equal(s[r:r + 1].view(torch.int32), s_dev[r:r + 1].view(torch.int32)), (producer, r)
    assert (q_dev[2] == 0xFE).any() and not E.is_nan_byte(q_dev).any()       # the NaN left as -448: the parent fails P2
    good = E.pack_rows(y)
    assert "P2" in E.violations(y, (q_dev, s_dev), good) and "P2" not in E.violations(y, good, good)
