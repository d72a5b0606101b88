"""The kernels of ca_t5.hip on the GPU against their fp64 statements, inside the derived bounds of tests/t5_cases.py.
Every output buffer is pre-filled with NaN, so an element no thread wrote shows; the padding columns of a strided
output must still hold it afterwards."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import t5_cases as T  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def _check(name, got, ref, bound):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f"{name}: unwritten or non-finite elements"
    r = float(((got - ref).abs() / bound).max())
    print(f"{name}: max err / bound {r:.3f}")
    assert r <= 1.0, (name, r)


@pytest.mark.parametrize("case", T.ATTN_CASES, ids=lambda c: c.name)
def test_attention(case):
    q, k, v, bias, _ = T.attn_inputs(case)
    ref, bound = T.attn_reference(q, k, v, bias, case.n_seq, case.heads)
    rows, width = q.shape
    if case.layout == "sliced":      # the model's form: thirds of one projection output, out in a wider buffer
        qkv = torch.cat([q, k, v], 1).to(DEV, BF)
        dq, dk, dv = qkv[:, :width], qkv[:, width:2 * width], qkv[:, 2 * width:]
        full = _nan((rows, width + 64), BF)
        out = full[:, :width]
    else:
        dq, dk, dv = (t.to(DEV, BF) for t in (q, k, v))
        full = out = _nan((rows, width), BF)
    ops.t5_attention(dq, dk, dv, bias.to(DEV), out, case.n_seq, case.heads)
    torch.cuda.synchronize()
    _check("t5_attn " + case.name, out, ref, bound)
    if case.layout == "sliced":
        assert torch.isnan(full[:, width:]).all(), "columns beyond heads * 64 were written"


@pytest.mark.parametrize("H,rows,strided", T.ROW_CASES)
def test_rmsnorm(H, rows, strided):
    x, w = T.row_inputs(H, rows)
    ref, bound = T.rmsnorm_reference(x, w)
    pad = 64 if strided else 0
    xs = torch.zeros(rows, H + pad, device=DEV)
    xs[:, :H] = x.to(DEV)
    full = _nan((rows, H + 2 * pad), BF)
    ops.t5_rmsnorm(xs[:, :H], w.to(DEV), full[:, :H], T.EPS)
    torch.cuda.synchronize()
    _check(f"t5_rmsnorm {H}x{rows}{' strided' if strided else ''}", full[:, :H], ref, bound)
    assert torch.isnan(full[:, H:]).all()


@pytest.mark.parametrize("C,rows,strided", [(C, r, s) for C in (512, 10240) for r in (1, 7, 1280) for s in (False, True)])
def test_gated_mul(C, rows, strided):
    g, u = T.gate_inputs(C, rows)
    ref, bound = T.gated_mul_reference(g, u)
    pad = 64 if strided else 0
    gs, us = torch.zeros(rows, C + pad, device=DEV, dtype=BF), torch.zeros(rows, C + 2 * pad, device=DEV, dtype=BF)
    gs[:, :C], us[:, :C] = g.to(DEV, BF), u.to(DEV, BF)
    full = _nan((rows, C + 3 * pad), BF)
    ops.gated_mul(gs[:, :C], us[:, :C], full[:, :C])
    torch.cuda.synchronize()
    _check(f"gated_mul {C}x{rows}", full[:, :C], ref, bound)
    assert torch.isnan(full[:, C:]).all()
    ops.gated_mul(gs[:, :C], us[:, :C], us[:, :C])                 # in place, as the model runs it
    assert torch.equal(us[:, :C], full[:, :C])


@pytest.mark.parametrize("H,rows,strided", T.ROW_CASES)
def test_embed_rows(H, rows, strided):
    table, ids = T.embed_inputs(H, rows)
    pad = 64 if strided else 0
    ts = torch.zeros(table.shape[0], H + pad, device=DEV, dtype=BF)
    ts[:, :H] = table.to(DEV, BF)
    full = _nan((rows, H + 2 * pad), torch.float32)
    ops.embed_rows(ts[:, :H], ids, full[:, :H])
    torch.cuda.synchronize()
    assert torch.equal(full[:, :H].cpu(), table[ids.long()])       # exact
    assert torch.isnan(full[:, H:]).all()
    for bad in (-1, table.shape[0]):
        wrong = ids.clone()
        wrong[rows // 2] = bad
        with pytest.raises(ValueError):
            ops.embed_rows(ts[:, :H], wrong, full[:, :H])
