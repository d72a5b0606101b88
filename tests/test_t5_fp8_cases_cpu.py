"""CPU checks of tests/t5_fp8_cases.py: the fp32 emulation of each e4m3 producer sits inside its derived bounds on every
case the GPU test runs, each named slip leaves them, and the two new entry points reject bad arguments without a GPU."""
import ctypes
import math

import pytest
import torch

import __graft_entry__ as entry
import t5_fp8_cases as F
from conceptattention_amd import _lib as L


def _rms(H, rows, first=0, slip=None, scale_of=None):
    x, w, fam = F.rms_inputs(H, rows, first)
    q, s = F.rmsnorm_fp8_emulated(x, w, slip=slip, scale_of=scale_of)
    return q, s, F.rmsnorm_y64(x, w), F.y_rel_rmsnorm(H), fam


def _gate(C, rows, first=0, slip=None, scale_of=None):
    g, u, fam = F.gate_inputs(C, rows, first)
    q, s = F.gated_mul_fp8_emulated(g, u, slip=slip, scale_of=scale_of)
    return q, s, F.gated_y64(g, u), 0.0, fam


def _check_inside(q, s, y64, y_rel, fam):
    rs, rv = F.ratios(q, s, y64, y_rel)
    assert rs <= 1.0 and rv <= 1.0, (rs, rv)
    for r, f in enumerate(fam):
        if f == "zero":
            assert float(s[r]) == 1.0 and not (q[r] & 0x7F).any()        # scale 1, bytes +-0
        if f == "outlier":   # the case is what it says: one byte at the maximum, a good part of the rest subnormal or 0
            assert int(((q[r] & 0x7F) == 0x7E).sum()) == 1
            if q.shape[1] >= 256:    # (a share of the 7 other bytes of a minimum-width row is no statistic)
                assert float(((q[r] & 0x78) == 0).double().mean()) > 0.15


@pytest.mark.parametrize("H,rows", sorted({(H, rows) for H, rows, _ in F.RMS_CASES}))
def test_rmsnorm_emulation_sits_inside_the_bounds(H, rows):
    for first in ((0, 1, 2) if rows == 1 else (0,)):
        _check_inside(*_rms(H, rows, first))


@pytest.mark.parametrize("C,rows", F.GATE_CASES)
def test_gated_mul_emulation_sits_inside_the_bounds(C, rows):
    for first in ((0, 1, 2) if rows == 1 else (0,)):
        _check_inside(*_gate(C, rows, first))


def test_the_ragged_and_minimum_widths_are_cases_and_the_wrap_cases_exceed_their_cap():
    for rows in (1, 7):
        assert {(2056, rows), (8, rows)} <= set(F.GATE_CASES)
        assert {(H, rows, s) for H in (2056, 8) for s in (False, True)} <= set(F.RMS_CASES)
    assert 2056 % 2048 == 8 and 2056 > 2048
    assert F.ROW_GRID_CAP == 65536 and set(F.WRAP_CASES) == {"t5_rmsnorm_fp8", "gated_mul_fp8"}
    for op, (units, cap, per_wg, case) in F.WRAP_CASES.items():
        assert cap + per_wg <= units < cap + cap // 4 and case["rows"] == units, op


@pytest.mark.parametrize("slip", F.SLIPS)
@pytest.mark.parametrize("make,size", [(_rms, 256), (_rms, 4096), (_gate, 512), (_gate, 10240)])
def test_every_slip_leaves_a_bound(make, size, slip):
    """The two scale slips leave the scale bound (by orders of magnitude: 2^-9 and 448 / 240 against a few u), the
    rounding slip the value bound (an error of up to a whole step against half of one)."""
    q, s, y64, y_rel, _ = make(size, 5, slip=slip)
    rs, rv = F.ratios(q, s, y64, y_rel)
    if slip == "truncate":
        assert rs <= 1.0 and rv > 1.5, (rs, rv)
    else:
        assert rs > 100.0, (rs, rv)


@pytest.mark.parametrize("make,size", [(_rms, 256), (_gate, 512)])
def test_missing_saturation_shows_where_the_scale_misses_the_maximum(make, size):
    """t5_fp8_cases' docstring: with the row's true maximum in the scale no element exceeds 448 (1 + 3 u) and the clamp
    never acts; with the outlier left out of the maximum it must hold the store at +-448 (finite), and without it the
    byte is NaN."""
    rows = 6
    q, s, y64, y_rel, fam = make(size, rows)
    z = F.dequant(q, s) / s.double()[:, None]
    assert float(z.abs().max()) == 448.0                                        # the kernels' own scale: 448 exactly
    q2, *_ = make(size, rows, slip="no_saturation")
    assert torch.equal(q2, q)                                                   # ... and the clamp changes no byte there
    mask = y64.abs() < y64.abs().amax(-1, keepdim=True)                          # the maximum left out of the scale
    mask[[r for r, f in enumerate(fam) if f != "outlier"]] = True
    qs, ss, *_ = make(size, rows, scale_of=mask)
    qn, sn, *_ = make(size, rows, slip="no_saturation", scale_of=mask)
    sat = F.dequant(qs, ss)
    assert torch.isfinite(sat).all()
    for r, f in enumerate(fam):
        if f == "outlier":
            assert float(sat[r].abs().max()) == 448.0 * float(ss[r])            # held at the largest finite value
    assert F.ratios(qn, sn, y64, y_rel) == (math.inf, math.inf)                 # NaN bytes without the clamp
    assert torch.isnan(F.dequant(qn, sn)).sum() == sum(f == "outlier" for f in fam)


def test_model_emulation_without_fp8_projections_is_the_fp64_restatement():
    import t5_ref
    from conceptattention_amd.params import tiny_t5_params
    from conceptattention_amd.t5 import synthetic_t5_state_dict
    p = tiny_t5_params(**t5_ref.CASES["long"][0])
    sd = synthetic_t5_state_dict(p, 0)
    ids = t5_ref.case_ids("long")[:1, :64].contiguous()
    ref = t5_ref.encoder(sd, ids, p.num_heads, p.num_layers)
    assert torch.equal(F.encoder_fp8_emulated(sd, ids, p.num_heads, p.num_layers, fp8=()), ref)
    full = F.encoder_fp8_emulated(sd, ids, p.num_heads, p.num_layers)
    part = F.encoder_fp8_emulated(sd, ids, p.num_heads, p.num_layers, fp8=("o",))
    err = lambda t: float(((t - ref) ** 2).mean().sqrt() / (ref ** 2).mean().sqrt())   # noqa: E731
    assert 0 < err(part) < err(full) < 0.2                                      # quantisation is there, and it adds up


# ---------------------------------------------------------------------------------------------------------- rejection
@pytest.fixture(scope="module")
def lib():
    entry.build()
    return L.load()


def test_argument_rejection_of_the_two_entries_needs_no_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15            # a 16-byte aligned non-null address; nothing is ever launched

    def rms(**kw):
        a = dict(x=p, ldx=256, w=p, out=p, ldo=256, scale=p, rows=1, H=256, eps=1e-6)
        a.update(kw)
        return lib.ca_t5_rmsnorm_f32in_fp8(a["x"], a["ldx"], a["w"], a["out"], a["ldo"], a["scale"], a["rows"], a["H"],
                                           a["eps"], None)
    for bad in (dict(x=None), dict(w=None), dict(out=None), dict(scale=None), dict(rows=0), dict(H=0), dict(H=252),
                dict(ldx=248), dict(ldx=258, H=248), dict(ldo=248), dict(ldo=260), dict(eps=0.0), dict(x=p + 4),
                dict(w=p + 8), dict(out=p + 4), dict(scale=p + 2)):
        assert rms(**bad) == -1, bad
        assert b"ca_t5_rmsnorm_f32in_fp8" in lib.ca_last_error()

    def gate(**kw):
        a = dict(g=p, ldg=512, u=p, ldu=512, out=p, ldo=512, scale=p, rows=1, C=512)
        a.update(kw)
        return lib.ca_gated_mul_fp8(a["g"], a["ldg"], a["u"], a["ldu"], a["out"], a["ldo"], a["scale"], a["rows"],
                                    a["C"], None)
    for bad in (dict(g=None), dict(u=None), dict(out=None), dict(scale=None), dict(rows=0), dict(C=0), dict(C=508),
                dict(ldg=504), dict(ldu=516), dict(ldo=504), dict(ldo=516), dict(g=p + 8), dict(u=p + 2),
                dict(out=p + 4), dict(scale=p + 1)):
        assert gate(**bad) == -1, bad
        assert b"ca_gated_mul_fp8" in lib.ca_last_error()


def test_wrappers_reject_bad_tensors_before_any_launch():
    from conceptattention_amd import ops
    x, w = torch.zeros(4, 256), torch.ones(256)
    q, s = torch.zeros(4, 256, dtype=torch.uint8), torch.zeros(4)
    b = torch.zeros(4, 256, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.t5_rmsnorm_fp8(x, w, q, s)              # not on the device
    with pytest.raises(ValueError):
        ops.gated_mul_fp8(b, b, q, s)
