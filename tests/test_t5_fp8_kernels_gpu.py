"""The two e4m3 producers of ca_t5.hip (ca_t5_rmsnorm_f32in_fp8, ca_gated_mul_fp8) on the GPU against their fp64
statements, inside the derived bounds of tests/t5_fp8_cases.py.  Every output plane is pre-filled with a NaN byte
pattern (0x7F) and every scale vector with NaN, so an element no thread wrote shows; the padding columns of a strided
plane must still hold the pattern afterwards.

Measured on an MI355X (largest printed error / bound over all cases): rmsnorm scale 0.112, value 0.985; gated product
scale 0.398, value 0.985 (0.985 = 1 / (1 + 2^-6): an e4m3 tie, half a step exactly); no byte differed from the CPU
emulation's.  The later cases (grid wrap, widths 2056 and 8): t5_fp8_cases.py has the figures.

The run_* helpers take an optional allocator (tests/placement.py), as test_vae_routes_gpu.run_checked does:
tests/test_address_range_gpu.py runs the same cases with their buffers at chosen addresses and row strides."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import placement  # noqa: E402
import t5_fp8_cases as F  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
NAN_BYTE = 0x7F
RATIOS = {}          # (kernel, "scale" | "value") -> the largest error / bound seen


def _al(alloc):
    return alloc or placement.Plain(DEV)


def _widened(t, ld):
    out = torch.zeros((t.shape[0], ld), dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def _planes(al, rows, cols, pad):
    full = al.full((rows, cols + pad), NAN_BYTE, torch.uint8, {"out": None})
    scale = al.full((rows,), NAN, torch.float32, {"out_scale": None})
    return full, full[:, :cols], scale


def _check(name, key, q, scale, y64, y_rel, fam, emulated):
    q, scale = q.cpu(), scale.cpu()
    rs, rv = F.ratios(q, scale, y64, y_rel)          # (inf, inf) where a scale or a byte is not finite: a row nobody wrote
    eq, es = emulated
    differ = int(((q != eq) & ~(((q & 0x7F) == 0) & ((eq & 0x7F) == 0))).sum())
    print(f"{name}: scale err / bound {rs:.3f}, value err / bound {rv:.3f}, {differ} of {q.numel()} bytes differ from "
          f"the emulation")
    RATIOS[(key, "scale")], RATIOS[(key, "value")] = max(RATIOS.get((key, "scale"), 0.0), rs), max(RATIOS.get((key, "value"), 0.0), rv)
    assert rs <= 1.0 and rv <= 1.0, (name, rs, rv)
    amax = y64.abs().amax(-1)
    want = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)).float()
    assert torch.allclose(scale, want, rtol=1e-6, atol=0), name               # as tests/test_fp8_gpu.py compares scales
    zero = torch.tensor([f == "zero" for f in fam])
    assert (scale[zero] == 1.0).all() and not (q[zero] & 0x7F).any(), name


@functools.lru_cache(maxsize=2)
def _rms_problem(H, rows, first):
    x, w, fam = F.rms_inputs(H, rows, first)
    return x, w, fam, F.rmsnorm_y64(x, w), F.rmsnorm_fp8_emulated(x, w)


def run_rmsnorm_fp8(case, alloc=None, first=0):
    H, rows, strided = case
    al = _al(alloc)
    x, w, fam, y64, emulated = _rms_problem(H, rows, first)
    pad = 64 if strided else 0
    xs, wd = al.to(_widened(x, H + pad), {"x": None}), al.to(w, {"w": None})
    full, q, scale = _planes(al, rows, H, 2 * pad)
    ops.t5_rmsnorm_fp8(xs[:, :H], wd, q, scale, F.EPS)
    torch.cuda.synchronize()
    _check(f"t5_rmsnorm_fp8 {H}x{rows}{' strided' if strided else ''} {fam[0]}", "rmsnorm_fp8", q, scale, y64,
           F.y_rel_rmsnorm(H), fam, emulated)
    assert (full[:, H:] == NAN_BYTE).all(), "columns beyond H were written"
    assert torch.equal(xs[:, :H].cpu(), x) and torch.equal(wd.cpu(), w), "an input changed"
    return {"out": q.clone(), "out_scale": scale.clone()}


@pytest.mark.parametrize("H,rows,strided", F.RMS_CASES)
def test_rmsnorm_fp8(H, rows, strided):
    for first in ((0, 1, 2) if rows == 1 else (0,)):
        run_rmsnorm_fp8((H, rows, strided), first=first)


def run_gated_mul_fp8(case, alloc=None, first=0):
    C, rows = case
    al = _al(alloc)
    g, u, fam = F.gate_inputs(C, rows, first)
    both = al.to(torch.cat([u, g], 1).to(BF), {"g": None, "u": None})   # the SPLIT_GELU launch's two halves as views of one buffer
    full, q, scale = _planes(al, rows, C, 64)
    ops.gated_mul_fp8(both[:, C:], both[:, :C], q, scale)
    torch.cuda.synchronize()
    _check(f"gated_mul_fp8 {C}x{rows} {fam[0]}", "gated_mul_fp8", q, scale, F.gated_y64(g, u), 0.0, fam,
           F.gated_mul_fp8_emulated(g, u))
    assert (full[:, C:] == NAN_BYTE).all(), "columns beyond C were written"
    assert torch.equal(both.cpu().float(), torch.cat([u, g], 1))          # the inputs are left alone
    return {"out": q.clone(), "out_scale": scale.clone()}


@pytest.mark.parametrize("C,rows", F.GATE_CASES)
def test_gated_mul_fp8(C, rows):
    for first in ((0, 1, 2) if rows == 1 else (0,)):
        run_gated_mul_fp8((C, rows), first=first)


def test_rmsnorm_fp8_grid_wrap():
    """rows = 65536 + 5, strided in and out: five workgroups walk a second row with `red` reused by both reductions; every
    row's scale (pre-filled with NaN) and bytes inside the bounds."""
    c = F.WRAP_CASES["t5_rmsnorm_fp8"][3]
    run_rmsnorm_fp8((c["H"], c["rows"], True))


def test_gated_mul_fp8_grid_wrap():
    c = F.WRAP_CASES["gated_mul_fp8"][3]
    run_gated_mul_fp8((c["C"], c["rows"]))


def test_zz_report():
    """The largest error / bound per kernel of this module's runs so far."""
    for key in sorted(RATIOS):
        print(f"  err / bound {key}: {RATIOS[key]:.3f}")


def test_argument_errors_one_per_check():
    x, w = torch.zeros(4, 264, device=DEV), torch.ones(256, device=DEV)
    q, s = torch.zeros(4, 264, device=DEV, dtype=torch.uint8), torch.zeros(8, device=DEV)
    b = torch.zeros(4, 528, device=DEV, dtype=BF)
    ok = lambda: ops.t5_rmsnorm_fp8(x[:, :256], w, q[:, :256], s[:4], F.EPS)   # noqa: E731
    ok()
    bad_rms = [lambda: ops.t5_rmsnorm_fp8(x[:, :256].to(BF), w, q[:, :256], s[:4]),            # x dtype
               lambda: ops.t5_rmsnorm_fp8(x[:, :256], w.to(BF), q[:, :256], s[:4]),            # weight dtype
               lambda: ops.t5_rmsnorm_fp8(x[:, :256], w, q[:, :256].to(BF), s[:4]),            # out dtype
               lambda: ops.t5_rmsnorm_fp8(x[:, :256], w, q[:, :256], s[:4].double()),          # scale dtype
               lambda: ops.t5_rmsnorm_fp8(x[:, :256], w, q[:, :248], s[:4]),                   # out shape
               lambda: ops.t5_rmsnorm_fp8(x[:, :256], w[:248], q[:, :256], s[:4]),             # weight length
               lambda: ops.t5_rmsnorm_fp8(x[:, :256], w, q[:, :256], s[:3]),                   # scale length
               lambda: ops.t5_rmsnorm_fp8(x[:, :256], w, q[:, :256], s[::2]),                  # scale not contiguous
               lambda: ops.t5_rmsnorm_fp8(x[0, :256], w, q[0, :256], s[:1]),                   # not 2-D
               lambda: ops.t5_rmsnorm_fp8(x[:, :252], w[:252], q[:, :252], s[:4]),             # H % 8
               lambda: ops.t5_rmsnorm_fp8(x[:, 2:258], w, q[:, :256], s[:4]),                  # x alignment (16 bytes)
               lambda: ops.t5_rmsnorm_fp8(x[:, :256], w, q[:, 4:260], s[:4]),                  # out8 alignment (8 bytes)
               lambda: ops.t5_rmsnorm_fp8(x[:, :256], w, torch.zeros(4, 260, device=DEV, dtype=torch.uint8)[:, :256], s[:4]),  # ldo % 8
               lambda: ops.t5_rmsnorm_fp8(torch.zeros(4, 258, device=DEV)[:, :256], w, q[:, :256], s[:4]),   # ldx % 4
               lambda: ops.t5_rmsnorm_fp8(x[:, :256], w, q[:, :256], s[:4], 0.0)]              # eps
    okg = lambda: ops.gated_mul_fp8(b[:, :256], b[:, 264:520], q[:, :256], s[:4])   # noqa: E731
    okg()
    bad_gate = [lambda: ops.gated_mul_fp8(b[:, :256].float(), b[:, 264:520], q[:, :256], s[:4]),   # g dtype
                lambda: ops.gated_mul_fp8(b[:, :256], b[:, 264:512], q[:, :256], s[:4]),           # u shape
                lambda: ops.gated_mul_fp8(b[:, :256], b[:, 264:520], q[:, :248], s[:4]),           # out shape
                lambda: ops.gated_mul_fp8(b[:, :256], b[:, 264:520], q[:, :256].float(), s[:4]),   # out dtype
                lambda: ops.gated_mul_fp8(b[:, :256], b[:, 264:520], q[:, :256], s[:5]),           # scale length
                lambda: ops.gated_mul_fp8(b[:, :252], b[:, 264:516], q[:, :252], s[:4]),           # C % 8
                lambda: ops.gated_mul_fp8(b[:, 4:260], b[:, 264:520], q[:, :256], s[:4]),          # g alignment
                lambda: ops.gated_mul_fp8(b[:, :256], b[:, 268:524], q[:, :256], s[:4]),           # u alignment
                lambda: ops.gated_mul_fp8(b[:, :256], b[:, 264:520], q[:, 4:260], s[:4]),          # out8 alignment
                lambda: ops.gated_mul_fp8(torch.zeros(4, 260, device=DEV, dtype=BF)[:, :256], b[:, 264:520], q[:, :256], s[:4]),  # ldg % 8
                lambda: ops.gated_mul_fp8(b[:, :256], b[:, 264:520], torch.zeros(4, 260, device=DEV, dtype=torch.uint8)[:, :256], s[:4])]  # ldo % 8
    for f in bad_rms + bad_gate:
        with pytest.raises(ValueError):
            f()
