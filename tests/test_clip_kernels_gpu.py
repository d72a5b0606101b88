"""The kernels of ca_clip.hip on the GPU against their fp64 statements, inside the derived bounds of
tests/clip_cases.py.  Every output buffer is pre-filled with NaN, so an element no thread wrote shows; padding columns
and guard rows must still hold what they held.

The run_* helpers take an optional allocator (tests/placement.py), as test_vae_routes_gpu.run_checked does:
tests/test_address_range_gpu.py runs the same cases with their buffers at chosen addresses and row strides.  Each helper
checks its case and returns clones of the outputs."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_cases as T  # noqa: E402
import placement  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
GUARD = 128          # rows behind the operands: more than a 32-key step or a 64-query workgroup reaches
PATTERN = 7.25       # what the guard rows of an output hold
RATIOS = {}          # kernel -> the largest max err / bound seen


def _al(alloc):
    return alloc or placement.Plain(DEV)


def _nan(shape, dtype):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def _check(name, key, got, ref, bound):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f"{name}: unwritten or non-finite elements"
    r = float(((got - ref).abs() / bound).max())
    print(f"{name}: max err / bound {r:.3f}")
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    assert r <= 1.0, (name, r)


def _widened(t, ld, fill=0.0):
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def _at_the_end(alloc, rows, stride, fill, roles, guard=GUARD):
    """A [rows + guard, stride] bf16 buffer holding ``fill``.  Without an allocator it ends where its (larger)
    allocation ends."""
    if alloc is None:
        n = (rows + guard) * stride
        whole = torch.full((4096 + n,), fill, device=DEV, dtype=BF)
        return whole[4096:].view(rows + guard, stride)
    return alloc.full((rows + guard, stride), fill, BF, roles)


@functools.lru_cache(maxsize=None)
def _attn_problem(case):
    q, k, v = T.attn_inputs(case)
    return (q, k, v) + tuple(T.attn_reference(q, k, v, case.n_seq, case.heads))


def run_attention(case, alloc=None, guard=GUARD):
    q, k, v, ref, bound = _attn_problem(case)
    rows, width = q.shape
    up = [t.to(DEV, BF) for t in (q, k, v)]       # (uploaded before the first allocation: nothing behind it waits)
    if case.layout == "sliced":      # the model's form: thirds of one projection output (plus 8 unused columns)
        qkv = _at_the_end(alloc, rows, 3 * width + 8, NAN, {"q": None, "k": None, "v": None}, guard)
        dq, dk, dv = qkv[:, :width], qkv[:, width:2 * width], qkv[:, 2 * width:3 * width]
    else:                            # four buffers, four strides
        dq, dk, dv = (_at_the_end(alloc, rows, width + pad, NAN, {n: None}, guard)[:, :width]
                      for n, pad in (("q", 8), ("k", 16), ("v", 24)))
    for d, t in zip((dq, dk, dv), up):
        d[:rows] = t                 # the guard rows behind n_seq * L stay NaN: a key or value read there poisons the output
    full = _at_the_end(alloc, rows, width + 64, PATTERN, {"out": None}, guard)
    full[:rows] = NAN
    out = full[:, :width]
    assert len({dq.stride(0), out.stride(0)}) == 2 and (case.layout == "sliced" or len({t.stride(0) for t in (dq, dk, dv, out)}) == 4)
    ops.clip_attention(dq[:rows], dk[:rows], dv[:rows], out[:rows], case.n_seq, case.heads, T.SCALE)
    torch.cuda.synchronize()
    _check("clip_attn " + case.name, "attention", out[:rows], ref, bound)
    assert torch.isnan(full[:rows, width:]).all(), "columns beyond heads * 64 were written"
    assert (full[rows:] == PATTERN).all(), "rows beyond n_seq * L were written"
    for d, t in ((dq, q), (dk, k), (dv, v)):
        assert torch.equal(d[:rows].cpu().float(), t) and torch.isnan(d[rows:]).all(), "an input changed"
    return {"out": out[:rows].clone()}


@pytest.mark.parametrize("case", T.ATTN_CASES, ids=lambda c: c.name)
def test_attention(case):
    run_attention(case)


@functools.lru_cache(maxsize=2)
def _ln_problem(H, rows):
    x, w, b = T.ln_inputs(H, rows)
    return (x, w, b) + tuple(T.layernorm_reference(x, w, b))


def run_layernorm(case, alloc=None, gather=None):
    """``gather``: None, or the int32 row_idx (a host tensor); the outputs are then the gathered rows."""
    H, rows, strided = case
    al = _al(alloc)
    x, w, b, ref, bound = _ln_problem(H, rows)
    pad = 64 if strided else 0
    xs = al.to(_widened(x, H + pad), {"x": None})
    wd, bd = al.to(w, {"w": None}), al.to(b, {"b": None})
    idx = None if gather is None else al.to(gather, {"row_idx": None})
    n_out = rows if gather is None else gather.shape[0]
    full = al.full((n_out, H + 2 * pad), NAN, BF, {"out": None})
    ops.layernorm(xs[:, :H], wd, bd, full[:, :H], T.EPS, row_idx=idx)
    torch.cuda.synchronize()
    pick = slice(None) if gather is None else gather.long()
    _check(f"layernorm {H}x{rows}{' strided' if strided else ''}{' gather' if gather is not None else ''}", "layernorm",
           full[:, :H], ref[pick], bound[pick])
    assert torch.isnan(full[:, H:]).all()
    assert torch.equal(xs[:, :H].cpu(), x) and torch.equal(wd.cpu(), w) and torch.equal(bd.cpu(), b), "an input changed"
    assert idx is None or torch.equal(idx.cpu(), gather)
    return {"out": full[:, :H].clone()}, xs, wd, bd


@pytest.mark.parametrize("H,rows,strided", T.LN_CASES, ids=[T.ln_id(c) for c in T.LN_CASES])
def test_layernorm(H, rows, strided):
    got, xs, wd, bd = run_layernorm((H, rows, strided))
    idx = torch.tensor(T.ln_gather(rows), dtype=torch.int32)            # out of order and repeated
    part, _, _, _ = run_layernorm((H, rows, strided), gather=idx)
    assert torch.equal(part["out"], got["out"][idx.long().to(DEV)])     # the gather reads the same rows: the same bits
    out = _nan((len(idx), H), BF)
    for bad in (-1, rows):
        wrong = idx.clone()
        wrong[2] = bad
        with pytest.raises(ValueError):
            ops.layernorm(xs[:, :H], wd, bd, out, T.EPS, row_idx=wrong)


def test_layernorm_grid_wrap():
    """rows = 65536 + 5, strided in and out: five workgroups walk a second row with `red` reused by both reductions.
    Once row by row, once with a row_idx of the same length (a seeded permutation with repeats)."""
    c = T.WRAP_CASES["layernorm"][3]
    case = (c["H"], c["rows"], True)
    got, _, _, _ = run_layernorm(case)
    g = torch.Generator().manual_seed(77)
    idx = torch.randint(0, c["rows"], (c["rows"],), generator=g, dtype=torch.int32)
    idx[0], idx[-1] = c["rows"] - 1, 0
    part, _, _, _ = run_layernorm(case, gather=idx)
    assert torch.equal(part["out"], got["out"][idx.long().to(DEV)])


def run_quick_gelu(case, alloc=None):
    C, rows, strided = case
    al = _al(alloc)
    x = T.quick_gelu_inputs(C, rows)
    ref, bound = T.quick_gelu_reference(x)
    pad = 64 if strided else 0
    xs = al.to(_widened(x, C + pad).to(BF), {"x": None})
    full = al.full((rows, C + 2 * pad), NAN, BF, {"out": None})
    ops.quick_gelu(xs[:, :C], full[:, :C])
    got, xs1 = full[:, :C].clone(), xs.clone()                         # (xs after the first launch; both copies in stream order)
    ops.quick_gelu(xs[:, :C], xs[:, :C])                               # in place, as the model runs it
    torch.cuda.synchronize()
    _check(f"quick_gelu {C}x{rows}{' strided' if strided else ''}", "quick_gelu", full[:, :C], ref, bound)
    assert torch.isnan(full[:, C:]).all()
    assert torch.equal(xs1[:, :C].cpu().float(), x), "the input changed"
    assert torch.equal(xs[:, :C], got) and (xs[:, C:] == 0).all()
    return {"out": got}


@pytest.mark.parametrize("C,rows,strided", T.QG_CASES)
def test_quick_gelu(C, rows, strided):
    run_quick_gelu((C, rows, strided))
    edge = torch.tensor([[-float("inf"), float("inf"), -3.0e38, 3.0e38, float("nan"), -200.0, 0.0, 1.0]], device=DEV, dtype=BF)
    got = torch.empty_like(edge)
    ops.quick_gelu(edge, got)
    g = got[0].float().cpu()
    assert g[0] == 0 and g[1] == float("inf") and g[2] == 0 and g[3] == edge[0, 3].float().cpu() and torch.isnan(g[4])
    assert g[5] == 0 and g[6] == 0 and torch.isfinite(g[[0, 2, 3, 5, 6, 7]]).all()


def test_quick_gelu_grid_wrap():
    """43692 x 3072: 512 threads more than the 65536 x 256 of the capped grid.  The whole output against the fp64
    function and quick_gelu_reference's bound, both evaluated on the device."""
    c = T.WRAP_CASES["quick_gelu"][3]
    C, rows, pad = c["C"], c["rows"], 64
    g = torch.Generator(device=DEV)
    g.manual_seed(21)
    xs = (torch.randn((rows, C + pad), device=DEV, generator=g) * 2).to(BF)
    xs[0, :C] = torch.linspace(-40, 40, C, device=DEV).to(BF)
    full = _nan((rows, C + 2 * pad), BF)
    ops.quick_gelu(xs[:, :C], full[:, :C])
    torch.cuda.synchronize()
    ref, bound = T.quick_gelu_reference(xs[:, :C])
    got = full[:, :C].double()
    assert torch.isfinite(got).all(), "unwritten elements"
    r = float(((got - ref).abs() / bound).max())
    print(f"quick_gelu grid wrap {C}x{rows}: max err / bound {r:.3f}")
    assert r <= 1.0, r
    assert torch.isnan(full[:, C:]).all()


def run_clip_embed(H, alloc=None, vocab=512):
    al = _al(alloc)
    tok, pos, ids = T.embed_inputs(H, vocab)
    ref, bound = T.embed_reference(tok, pos, ids)
    rows = ids.shape[0]
    assert rows == 3 * 77
    ts = al.to(_widened(tok, H + 64).to(BF), {"tok": None})
    ps = al.to(_widened(pos, H + 8).to(BF), {"pos": None})
    di = al.to(ids, {"ids": None})
    full = al.full((rows, H + 128), NAN, torch.float32, {"out": None})
    ops.clip_embed(ts[:, :H], ps[:, :H], di, full[:, :H], T.EMBED_L)
    torch.cuda.synchronize()
    _check(f"clip_embed {H}", "clip_embed", full[:, :H], ref, bound)
    assert torch.equal(full[:, :H].cpu(), T.embed_emulated(tok, pos, ids))       # one fp32 addition: the same bits
    assert torch.isnan(full[:, H:]).all()
    assert torch.equal(ts[:, :H].cpu().float(), tok) and torch.equal(ps[:, :H].cpu().float(), pos), "an input changed"
    return {"out": full[:, :H].clone()}, ts, ps, full


@pytest.mark.parametrize("H", T.EMBED_H)
def test_clip_embed(H):
    _, ts, ps, full = run_clip_embed(H)
    tok, pos, ids = T.embed_inputs(H)
    for bad in (-1, tok.shape[0]):
        wrong = ids.clone()
        wrong[ids.shape[0] // 2] = bad
        with pytest.raises(ValueError):
            ops.clip_embed(ts[:, :H], ps[:, :H], wrong, full[:, :H], T.EMBED_L)


def test_clip_embed_grid_wrap():
    """2270 sequences of 77 at H = 768: 2624 threads more than the capped grid holds.  One fp32 addition: bit for bit
    against the same expression on the device."""
    c = T.WRAP_CASES["clip_embed"][3]
    H, rows, vocab = c["H"], c["rows"], 512
    g = torch.Generator(device=DEV)
    g.manual_seed(22)
    ts = torch.randn((vocab, H + 64), device=DEV, generator=g).to(BF)
    ps = (torch.randn((T.EMBED_L, H + 8), device=DEV, generator=g) * 0.5).to(BF)
    ids = torch.randint(0, vocab, (rows,), device=DEV, generator=g, dtype=torch.int32)
    ids[0], ids[-1] = vocab - 1, 0
    full = _nan((rows, H + 128), torch.float32)
    ops.clip_embed(ts[:, :H], ps[:, :H], ids, full[:, :H], T.EMBED_L)
    torch.cuda.synchronize()
    r = torch.arange(rows, device=DEV)
    assert torch.equal(full[:, :H], ts[:, :H].float()[ids.long()] + ps[:, :H].float()[r % T.EMBED_L])
    assert torch.isnan(full[:, H:]).all()


def test_zz_report():
    """(runs last) the largest max err / bound per kernel of this module's runs."""
    for key in sorted(RATIOS):
        print(f"  max err / bound {key}: {RATIOS[key]:.3f}")
