"""ca_mseg_score on the GPU against its numpy restatement (tests/mseg_cases.py): the counts, the class map and the index map
bit for bit, the same bits on a second launch, guard rows of a poison value behind every operand and output untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mseg_cases as T  # noqa: E402
import placement  # noqa: E402
import stream_gate  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
GUARD = 256                                   # elements behind every buffer
POISON = {torch.float32: 3.0e38, torch.uint8: 0x5A, torch.int32: -1234567}     # (a poison map value would win every argmax)


def _guarded(al, shape, dtype, role, src=None, fill=None):
    """A contiguous tensor of ``shape`` whose buffer goes on for GUARD poisoned elements: (tensor, guard).  A placing
    allocator that lets this role straddle puts its boundary on the middle element of the tensor, not of the padded buffer."""
    n = int(np.prod(shape))
    flat = al.full((n + GUARD,), POISON[dtype] if fill is None else fill, dtype, {role: n // 2})
    t = flat[:n].view(*shape)
    if src is not None:
        t.copy_(src)
    flat[n:].fill_(POISON[dtype])
    return t, flat[n:]


def _launch(case, maps, labels, tables, scale, alloc=None, outputs=None):
    """One ops.mseg_score call on a case's inputs: (counts int32 [n, 2 + 2 nclass], class maps or None, index maps or
    None) as numpy arrays.  ``alloc``: an allocator of tests/placement.py for the five operand roles."""
    n, (K, h, w), (Hl, Wl) = len(maps), maps[0].shape, labels[0].shape
    al = alloc or placement.Plain(DEV)
    outputs = case.outputs if outputs is None else outputs
    guards = []
    # (uploaded before the first allocation: nothing between the allocations and the launch waits for the device)
    maps_d, labels_d = (torch.from_numpy(np.ascontiguousarray(np.stack(a))).to(DEV) for a in (maps, labels))

    def make(shape, dtype, role, src=None, fill=None):
        t, g = _guarded(al, shape, dtype, role, src, fill)
        guards.append((role, g, dtype))
        return t
    md = make((n, K, h, w), torch.float32, "maps", maps_d)
    ld = make((n, Hl, Wl), torch.uint8, "label", labels_d)
    counts = make((n, 2 + 2 * case.nclass), torch.int32, "counts")
    c_out = make((n, h, w), torch.uint8, "class_out", fill=0xEE) if outputs in ("both", "class") else None
    i_out = make((n, h, w), torch.uint8, "index_out", fill=0xEE) if outputs in ("both", "index") else None
    ops.mseg_score(md, ld, counts, tables, case.nclass, ignore_index=case.ignore, scale=scale,
                   blur_weights=ops.seg_blur_weights() if case.blur else None, class_out=c_out, index_out=i_out)
    torch.cuda.synchronize()
    for role, g, dtype in guards:
        assert bool((g == POISON[dtype]).all()), f"the guard behind {role} was written"
    got_m, want_m = md.cpu().numpy(), np.stack(maps)
    assert np.array_equal(got_m.view(np.uint32), want_m.view(np.uint32)) and np.array_equal(ld.cpu().numpy(), np.stack(labels)), \
        "an input changed"
    return (counts.cpu().numpy(), None if c_out is None else c_out.cpu().numpy(),
            None if i_out is None else i_out.cpu().numpy())


def run_case(case, alloc=None):
    """One case of mseg_cases.CASES, its five buffers from an optional allocator, checked against the restatement item by
    item; returns the outputs."""
    maps, labels, tables, scale = case.inputs()
    counts, c_out, i_out = _launch(case, maps, labels, tables, scale, alloc=alloc)
    for i in range(case.items):
        ref = T.reference(maps[i], labels[i], tables[i], case.nclass, case.ignore, scale, case.blur)
        print(case.name, i, "correct, labelled", counts[i, :2].tolist(), "restatement", ref["counts"][:2].tolist())
        assert counts[i].dtype == np.int32 and np.array_equal(counts[i], ref["counts"]), (case.name, i)
        if c_out is not None:
            assert np.array_equal(c_out[i], ref["class"]), (case.name, i)
        if i_out is not None:
            assert np.array_equal(i_out[i], ref["index"]), (case.name, i)
    if alloc is None:
        again, c2, i2 = _launch(case, maps, labels, tables, scale)
        assert again.tobytes() == counts.tobytes(), "two launches of one input differ"
        assert (c_out is None or np.array_equal(c_out, c2)) and (i_out is None or np.array_equal(i_out, i2))
    return counts, c_out, i_out


@pytest.mark.parametrize("case", T.CASES, ids=repr)
def test_every_case_equals_the_restatement(case):
    run_case(case)


def test_a_launch_of_the_cap_equals_the_single_launches_and_a_side_stream_works():
    case = next(c for c in T.CASES if c.items == L.MSEG_MAX_PROBLEMS == T.MAX_PROBLEMS)
    maps, labels, tables, scale = case.inputs()
    stream = torch.cuda.Stream()
    # (behind a gate, tests/stream_gate.py: a launch on another stream would read poison instead of these inputs)
    warm = stream_gate.Recording(DEV)
    _launch(case, maps, labels, tables, scale, alloc=warm, outputs="both")
    with torch.cuda.stream(stream):
        counts, c_out, i_out = _launch(case, maps, labels, tables, scale, outputs="both",
                                       alloc=stream_gate.Gated(warm, stream_gate.Gate()))
    stream.synchronize()
    for i in (0, 7, 15):
        one, c1, i1 = _launch(case, maps[i:i + 1], labels[i:i + 1], tables[i:i + 1], scale, outputs="both")
        assert np.array_equal(one[0], counts[i]) and np.array_equal(c1[0], c_out[i]) and np.array_equal(i1[0], i_out[i]), i


def test_the_wrapper_rejects_what_the_kernel_cannot_take():
    def z(*shape, dtype=torch.float32):
        return torch.zeros(*shape, device=DEV, dtype=dtype)
    maps, lab, counts, table = [z(3, 8, 8)], [z(8, 8, dtype=torch.uint8)], z(1, 44, dtype=torch.int32), [[0, 1, 2]]
    ops.mseg_score(maps, lab, counts, table, 21)                                   # the control: accepted
    torch.cuda.synchronize()
    assert counts[0, 1].item() == 64
    with pytest.raises(ValueError, match="16384"):
        ops.mseg_score([z(3, 128, 129)], lab, counts, table, 21)
    with pytest.raises(ValueError, match="32"):
        ops.mseg_score([z(33, 8, 8)], lab, counts, [[0] * 33], 21)
    with pytest.raises(ValueError, match="256"):
        ops.mseg_score(maps, lab, z(1, 516, dtype=torch.int32), table, 257)
    with pytest.raises(ValueError, match="maps"):
        ops.mseg_score([z(3, 8, 8, dtype=torch.float64)], lab, counts, table, 21)
    with pytest.raises(ValueError, match="labels"):
        ops.mseg_score(maps, [lab[0].bool()], counts, table, 21)
    with pytest.raises(ValueError, match="counts"):
        ops.mseg_score(maps, lab, z(1, 43, dtype=torch.int32), table, 21)
    with pytest.raises(ValueError, match="counts"):
        ops.mseg_score(maps, lab, z(1, 44, dtype=torch.int64), table, 21)
    with pytest.raises(ValueError, match="maps"):
        ops.mseg_score([z(3, 8, 16)[:, :, ::2]], lab, counts, table, 21)           # not contiguous
    with pytest.raises(ValueError, match="maps"):
        ops.mseg_score([z(3, 16, 8)[:, ::2]], lab, counts, table, 21)              # rows not adjacent
    with pytest.raises(ValueError, match="labels"):
        ops.mseg_score(maps, [lab[0].cpu()], counts, table, 21)                    # not on the device
    with pytest.raises(ValueError, match="mseg_score"):
        ops.mseg_score(maps, lab + lab, counts, table, 21)                         # one label too many
    with pytest.raises(ValueError, match="class_of"):
        ops.mseg_score(maps, lab, counts, [[0, 1]], 21)
    with pytest.raises(ValueError, match="class_of"):
        ops.mseg_score(maps, lab, counts, [[0, 1, 21]], 21)
    with pytest.raises(ValueError, match="ignore_index"):
        ops.mseg_score(maps, lab, counts, table, 21, ignore_index=256)
    with pytest.raises(ValueError, match="scale"):
        ops.mseg_score(maps, lab, counts, table, 21, scale=[1.0, 2.0])
    with pytest.raises(ValueError, match="blur_weights"):
        ops.mseg_score(maps, lab, counts, table, 21, blur_weights=[1.0] * 8)
    with pytest.raises(ValueError, match=">= 2"):
        ops.mseg_score([z(3, 1, 8)], lab, counts, table, 21, blur_weights=ops.seg_blur_weights())
    with pytest.raises(ValueError, match="class_out"):
        ops.mseg_score(maps, lab, counts, table, 21, class_out=z(1, 8, 9, dtype=torch.uint8))
    with pytest.raises(ValueError, match="index_out"):
        ops.mseg_score(maps, lab, counts, table, 21, index_out=z(1, 8, 8, dtype=torch.int32))
