"""The kernels of ca_clip.hip on the GPU against their fp64 statements, inside the derived bounds of
tests/clip_cases.py.  Every output buffer is pre-filled with NaN, so an element no thread wrote shows; padding columns
and guard rows must still hold what they held."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_cases as T  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
GUARD = 128          # rows behind the operands: more than a 32-key step or a 64-query workgroup reaches
PATTERN = 7.25       # what the guard rows of an output hold


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def _check(name, got, ref, bound):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f"{name}: unwritten or non-finite elements"
    r = float(((got - ref).abs() / bound).max())
    print(f"{name}: max err / bound {r:.3f}")
    assert r <= 1.0, (name, r)


def _at_the_end(rows, stride, fill):
    """A [rows + GUARD, stride] bf16 view that ends where its (larger) allocation ends; all of it holds ``fill``."""
    n = (rows + GUARD) * stride
    whole = torch.full((4096 + n,), fill, device=DEV, dtype=BF)
    return whole[4096:].view(rows + GUARD, stride)


@pytest.mark.parametrize("case", T.ATTN_CASES, ids=lambda c: c.name)
def test_attention(case):
    q, k, v = T.attn_inputs(case)
    ref, bound = T.attn_reference(q, k, v, case.n_seq, case.heads)
    rows, width = q.shape
    nan = float("nan")
    if case.layout == "sliced":      # the model's form: thirds of one projection output (plus 8 unused columns)
        qkv = _at_the_end(rows, 3 * width + 8, nan)
        dq, dk, dv = qkv[:, :width], qkv[:, width:2 * width], qkv[:, 2 * width:3 * width]
    else:                            # four buffers, four strides
        dq, dk, dv = (_at_the_end(rows, width + pad, nan)[:, :width] for pad in (8, 16, 24))
    for d, t in ((dq, q), (dk, k), (dv, v)):
        d[:rows] = t.to(DEV, BF)     # the GUARD rows behind n_seq * L stay NaN: a key or value read there poisons the output
    full = _at_the_end(rows, width + 64, PATTERN)
    full[:rows] = nan
    out = full[:, :width]
    assert len({dq.stride(0), out.stride(0)}) == 2 and (case.layout == "sliced" or len({t.stride(0) for t in (dq, dk, dv, out)}) == 4)
    ops.clip_attention(dq[:rows], dk[:rows], dv[:rows], out[:rows], case.n_seq, case.heads, T.SCALE)
    torch.cuda.synchronize()
    _check("clip_attn " + case.name, out[:rows], ref, bound)
    assert torch.isnan(full[:rows, width:]).all(), "columns beyond heads * 64 were written"
    assert (full[rows:] == PATTERN).all(), "rows beyond n_seq * L were written"


@pytest.mark.parametrize("H,strided", T.LN_CASES)
def test_layernorm(H, strided):
    x, w, b = T.ln_inputs(H)
    ref, bound = T.layernorm_reference(x, w, b)
    rows, pad = x.shape[0], 64 if strided else 0
    xs = torch.zeros(rows, H + pad, device=DEV)
    xs[:, :H] = x.to(DEV)
    full = _nan((rows, H + 2 * pad), BF)
    ops.layernorm(xs[:, :H], w.to(DEV), b.to(DEV), full[:, :H], T.EPS)
    torch.cuda.synchronize()
    _check(f"layernorm {H}{' strided' if strided else ''}", full[:, :H], ref, bound)
    assert torch.isnan(full[:, H:]).all()
    idx = torch.tensor(T.LN_GATHER, dtype=torch.int32)                  # out of order and repeated
    part = _nan((len(idx), H + 2 * pad), BF)
    ops.layernorm(xs[:, :H], w.to(DEV), b.to(DEV), part[:, :H], T.EPS, row_idx=idx)
    torch.cuda.synchronize()
    assert torch.equal(part[:, :H], full[idx.long().to(DEV), :H])       # the gather reads the same rows: the same bits
    assert torch.isnan(part[:, H:]).all()
    for bad in (-1, rows):
        wrong = idx.clone()
        wrong[2] = bad
        with pytest.raises(ValueError):
            ops.layernorm(xs[:, :H], w.to(DEV), b.to(DEV), part[:, :H], T.EPS, row_idx=wrong)


@pytest.mark.parametrize("C,rows,strided", T.QG_CASES)
def test_quick_gelu(C, rows, strided):
    x = T.quick_gelu_inputs(C, rows)
    ref, bound = T.quick_gelu_reference(x)
    pad = 64 if strided else 0
    xs = torch.zeros(rows, C + pad, device=DEV, dtype=BF)
    xs[:, :C] = x.to(DEV, BF)
    full = _nan((rows, C + 2 * pad), BF)
    ops.quick_gelu(xs[:, :C], full[:, :C])
    torch.cuda.synchronize()
    _check(f"quick_gelu {C}x{rows}{' strided' if strided else ''}", full[:, :C], ref, bound)
    assert torch.isnan(full[:, C:]).all()
    ops.quick_gelu(xs[:, :C], xs[:, :C])                               # in place, as the model runs it
    assert torch.equal(xs[:, :C], full[:, :C]) and (xs[:, C:] == 0).all()
    edge = torch.tensor([[-float("inf"), float("inf"), -3.0e38, 3.0e38, float("nan"), -200.0, 0.0, 1.0]], device=DEV, dtype=BF)
    got = torch.empty_like(edge)
    ops.quick_gelu(edge, got)
    g = got[0].float().cpu()
    assert g[0] == 0 and g[1] == float("inf") and g[2] == 0 and g[3] == edge[0, 3].float().cpu() and torch.isnan(g[4])
    assert g[5] == 0 and g[6] == 0 and torch.isfinite(g[[0, 2, 3, 5, 6, 7]]).all()


@pytest.mark.parametrize("H", T.EMBED_H)
def test_clip_embed(H):
    tok, pos, ids = T.embed_inputs(H)
    ref, bound = T.embed_reference(tok, pos, ids)
    rows = ids.shape[0]
    assert rows == 3 * 77
    ts = torch.zeros(tok.shape[0], H + 64, device=DEV, dtype=BF)
    ps = torch.zeros(pos.shape[0], H + 8, device=DEV, dtype=BF)
    ts[:, :H], ps[:, :H] = tok.to(DEV, BF), pos.to(DEV, BF)
    full = _nan((rows, H + 128), torch.float32)
    ops.clip_embed(ts[:, :H], ps[:, :H], ids, full[:, :H], T.EMBED_L)
    torch.cuda.synchronize()
    _check(f"clip_embed {H}", full[:, :H], ref, bound)
    assert torch.equal(full[:, :H].cpu(), T.embed_emulated(tok, pos, ids))       # one fp32 addition: the same bits
    assert torch.isnan(full[:, H:]).all()
    for bad in (-1, tok.shape[0]):
        wrong = ids.clone()
        wrong[rows // 2] = bad
        with pytest.raises(ValueError):
            ops.clip_embed(ts[:, :H], ps[:, :H], wrong, full[:, :H], T.EMBED_L)
