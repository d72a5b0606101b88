"""The kernels of ca_t5.hip on the GPU against their fp64 statements, inside the derived bounds of tests/t5_cases.py.
Every output buffer is pre-filled with NaN, so an element no thread wrote shows; the padding columns of a strided
output and the guard rows behind an attention operand must still hold what they held.

The run_* helpers take an optional allocator (tests/placement.py), as test_vae_routes_gpu.run_checked does:
tests/test_address_range_gpu.py runs the same cases with their buffers at chosen addresses and row strides.  Each helper
checks its case and returns clones of the outputs."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import placement  # noqa: E402
import t5_cases as T  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
GUARD = 128          # rows behind the attention operands
PATTERN = 7.25       # what the guard rows of an output hold
RATIOS = {}          # kernel -> the largest max err / bound seen


def _al(alloc):
    return alloc or placement.Plain(DEV)


def _ratio(name, key, got, ref, bound):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f"{name}: unwritten or non-finite elements"
    r = float(((got - ref).abs() / bound).max())
    print(f"{name}: max err / bound {r:.3f}")
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    assert r <= 1.0, (name, r)


def _widened(t, ld, fill=0.0):
    """The host tensor t [rows, cols] as the first columns of a contiguous [rows, ld] one."""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def _guarded(alloc, rows, stride, fill, roles, guard):
    """A [rows + guard, stride] bf16 buffer holding ``fill``.  Without an allocator it ends where its (larger)
    allocation ends, as in tests/test_clip_kernels_gpu.py."""
    if alloc is None:
        n = (rows + guard) * stride
        return torch.full((4096 + n,), fill, device=DEV, dtype=BF)[4096:].view(rows + guard, stride)
    return alloc.full((rows + guard, stride), fill, BF, roles)


@functools.lru_cache(maxsize=None)
def _attn_problem(case):
    q, k, v, bias, _ = T.attn_inputs(case)
    return (q, k, v, bias) + tuple(T.attn_reference(q, k, v, bias, case.n_seq, case.heads))


def run_attention(case, alloc=None, guard=GUARD):
    """contig: four buffers with four row strides; sliced: the model's form, thirds of one projection output.  NaN guard
    rows behind n_seq * L on q, k and v (a key or value read there poisons the output), a pattern in the output's."""
    q, k, v, bias, ref, bound = _attn_problem(case)
    rows, width = q.shape
    up = [t.to(DEV, BF) for t in (q, k, v)]       # (uploaded before the first allocation: nothing behind it waits)
    if case.layout == "sliced":
        qkv = _guarded(alloc, rows, 3 * width, NAN, {"q": None, "k": None, "v": None}, guard)
        dq, dk, dv = qkv[:, :width], qkv[:, width:2 * width], qkv[:, 2 * width:]
    else:
        dq, dk, dv = (_guarded(alloc, rows, width + pad, NAN, {n: None}, guard)[:, :width]
                      for n, pad in (("q", 8), ("k", 16), ("v", 24)))
    for d, t in zip((dq, dk, dv), up):
        d[:rows] = t
    full = _guarded(alloc, rows, width + 64, PATTERN, {"out": None}, guard)
    full[:rows] = NAN
    out = full[:, :width]
    assert case.layout == "sliced" or len({t.stride(0) for t in (dq, dk, dv, out)}) == 4
    db = _al(alloc).to(bias, {"bias": None})
    ops.t5_attention(dq[:rows], dk[:rows], dv[:rows], db, out[:rows], case.n_seq, case.heads)
    torch.cuda.synchronize()
    _ratio("t5_attn " + case.name, "attention", out[:rows], ref, bound)
    assert torch.isnan(full[:rows, width:]).all(), "columns beyond heads * 64 were written"
    assert (full[rows:] == PATTERN).all(), "rows beyond n_seq * L were written"
    for d, t in ((dq, q), (dk, k), (dv, v)):
        assert torch.equal(d[:rows].cpu().float(), t) and torch.isnan(d[rows:]).all(), "an input changed"
    assert torch.equal(db.cpu(), bias)
    return {"out": out[:rows].clone()}


@pytest.mark.parametrize("case", T.ATTN_CASES, ids=lambda c: c.name)
def test_attention(case):
    run_attention(case)


@functools.lru_cache(maxsize=2)
def _rms_problem(H, rows):
    x, w = T.row_inputs(H, rows)
    return (x, w) + tuple(T.rmsnorm_reference(x, w))


def run_rmsnorm(case, alloc=None):
    H, rows, strided = case
    al = _al(alloc)
    x, w, ref, bound = _rms_problem(H, rows)
    pad = 64 if strided else 0
    xs, wd = al.to(_widened(x, H + pad), {"x": None}), al.to(w, {"w": None})
    full = al.full((rows, H + 2 * pad), NAN, BF, {"out": None})
    ops.t5_rmsnorm(xs[:, :H], wd, full[:, :H], T.EPS)
    torch.cuda.synchronize()
    _ratio(f"t5_rmsnorm {H}x{rows}{' strided' if strided else ''}", "rmsnorm", full[:, :H], ref, bound)
    assert torch.isnan(full[:, H:]).all()
    assert torch.equal(xs[:, :H].cpu(), x) and torch.equal(wd.cpu(), w), "an input changed"
    return {"out": full[:, :H].clone()}


@pytest.mark.parametrize("H,rows,strided", T.ROW_CASES)
def test_rmsnorm(H, rows, strided):
    run_rmsnorm((H, rows, strided))


def test_rmsnorm_grid_wrap():
    """rows = 65536 + 5: five workgroups walk a second row, with `red` reused (t5_cases.WRAP_CASES)."""
    c = T.WRAP_CASES["t5_rmsnorm"][3]
    run_rmsnorm((c["H"], c["rows"], True))


def run_gated_mul(case, alloc=None):
    C, rows, strided = case
    al = _al(alloc)
    g, u = T.gate_inputs(C, rows)
    ref, bound = T.gated_mul_reference(g, u)
    pad = 64 if strided else 0
    gs = al.to(_widened(g, C + pad).to(BF), {"g": None})
    us = al.to(_widened(u, C + 2 * pad).to(BF), {"u": None})
    full = al.full((rows, C + 3 * pad), NAN, BF, {"out": None})
    ops.gated_mul(gs[:, :C], us[:, :C], full[:, :C])
    got, us1 = full[:, :C].clone(), us.clone()                     # (us after the first launch; both copies in stream order)
    ops.gated_mul(gs[:, :C], us[:, :C], us[:, :C])                 # in place, as the model runs it
    torch.cuda.synchronize()
    _ratio(f"gated_mul {C}x{rows}", "gated_mul", full[:, :C], ref, bound)
    assert torch.isnan(full[:, C:]).all()
    assert torch.equal(gs[:, :C].cpu().float(), g) and torch.equal(us1[:, :C].cpu().float(), u), "an input changed"
    assert torch.equal(us[:, :C], got) and (us[:, C:] == 0).all()
    return {"out": got}


@pytest.mark.parametrize("C,rows,strided", T.GATE_CASES)
def test_gated_mul(C, rows, strided):
    run_gated_mul((C, rows, strided))


def _device_normal(shape, seed, scale):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.randn(shape, device=DEV, generator=g) * scale).to(BF)


def test_gated_mul_grid_wrap():
    """13108 x 10240: 1024 threads more than the 65536 x 256 of the capped grid, so four workgroups take a second
    element.  The whole output against the fp64 product formed on the device (gated_mul_reference's bound)."""
    c = T.WRAP_CASES["gated_mul"][3]
    C, rows, pad = c["C"], c["rows"], 64
    gs, us = _device_normal((rows, C + pad), 11, 2.0), _device_normal((rows, C + 2 * pad), 12, 2.0)
    full = torch.full((rows, C + 3 * pad), NAN, device=DEV, dtype=BF)
    ops.gated_mul(gs[:, :C], us[:, :C], full[:, :C])
    torch.cuda.synchronize()
    ref = gs[:, :C].double() * us[:, :C].double()
    bound = ref.abs() * T.BF16_U + 2.0 ** -133
    got = full[:, :C].double()
    assert torch.isfinite(got).all(), "unwritten elements"
    r = float(((got - ref).abs() / bound).max())
    print(f"gated_mul grid wrap {C}x{rows}: max err / bound {r:.3f}")
    assert r <= 1.0, r
    assert torch.equal(full[:, :C], (gs[:, :C].float() * us[:, :C].float()).to(BF))      # one rounding: the same bits
    assert torch.isnan(full[:, C:]).all()


def run_embed_rows(case, alloc=None, vocab=512):
    H, rows, strided = case
    al = _al(alloc)
    table, ids = T.embed_inputs(H, rows, vocab)
    pad = 64 if strided else 0
    ts = al.to(_widened(table, H + pad).to(BF), {"table": None})
    di = al.to(ids, {"ids": None})
    full = al.full((rows, H + 2 * pad), NAN, torch.float32, {"out": None})
    ops.embed_rows(ts[:, :H], di, full[:, :H])
    torch.cuda.synchronize()
    assert torch.equal(full[:, :H].cpu(), table[ids.long()])       # exact
    assert torch.isnan(full[:, H:]).all()
    assert torch.equal(ts[:, :H].cpu().float(), table) and torch.equal(di.cpu(), ids), "an input changed"
    return {"out": full[:, :H].clone()}, ts, full


@pytest.mark.parametrize("H,rows,strided", T.EMBED_CASES)
def test_embed_rows(H, rows, strided):
    _, ts, full = run_embed_rows((H, rows, strided))
    table, ids = T.embed_inputs(H, rows)
    for bad in (-1, table.shape[0]):
        wrong = ids.clone()
        wrong[rows // 2] = bad
        with pytest.raises(ValueError):
            ops.embed_rows(ts[:, :H], wrong, full[:, :H])


def test_embed_rows_grid_wrap():
    """32769 x 4096: 512 threads more than the capped grid holds.  Exact, against the gather on the device."""
    c = T.WRAP_CASES["embed_rows"][3]
    H, rows, pad, vocab = c["H"], c["rows"], 64, 512
    ts = _device_normal((vocab, H + pad), 13, 1.0)
    g = torch.Generator(device=DEV)
    g.manual_seed(14)
    ids = torch.randint(0, vocab, (rows,), device=DEV, generator=g, dtype=torch.int32)
    ids[0], ids[-1] = vocab - 1, 0
    full = torch.full((rows, H + 2 * pad), NAN, device=DEV)
    ops.embed_rows(ts[:, :H], ids, full[:, :H])
    torch.cuda.synchronize()
    assert torch.equal(full[:, :H], ts[:, :H].float()[ids.long()])
    assert torch.isnan(full[:, H:]).all()


def test_zz_report():
    """(runs last) the largest max err / bound per kernel of this module's runs."""
    for key in sorted(RATIOS):
        print(f"  max err / bound {key}: {RATIOS[key]:.3f}")
