"""ca_heatmap_render on the GPU against its numpy restatement (tests/render_cases.py): every output byte equal, lo / hi equal
as values or both NaN.  The unselected planes of a strided table are NaN, the bytes between two output planes, and the
guard elements behind the maps, the table, the pictures, both range buffers and the output keep what they held, and the
output and the range buffer start as garbage: none of it may show."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import placement  # noqa: E402
import render_cases as R  # noqa: E402
import stream_gate  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
GUARD = 64                         # guard elements behind every buffer
MAP_GUARD, BYTE_GUARD, RANGE_GUARD = 7.25e30, 0xA5, -3.5e33
IMG_PAD = 7                        # image_stride = 3 W + 7
LUT = R.synthetic_lut()


def same_f32(a, b) -> bool:
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a == b


def table_buffer(planes, C) -> np.ndarray:
    """fp32 [G n C h w + GUARD]: plane min(1, C - 1) of every map holds the map, the other planes NaN."""
    G, (n, h, w) = len(planes), planes[0].shape
    full = np.full((G, n, C, h, w), np.nan, dtype=np.float32)
    full[:, :, min(1, C - 1)] = np.stack(planes)
    return np.concatenate([full.reshape(-1), np.full(GUARD, MAP_GUARD, dtype=np.float32)])


def launch(case, inputs=None, lut=LUT, alloc=None, out_fill=BYTE_GUARD, range_in_ptrs=None):
    """One ca_heatmap_render call for a case of at most 16 groups, straight through the binding.  Returns (out uint8
    [G, n, H, W, 3], ranges fp32 [G, 2], the device range buffer); checks the inputs and every guard element."""
    planes, given, pics = inputs or case.inputs()
    G, n, C, h, w, H, W = case.groups, case.n_maps, case.C, case.h, case.w, case.H, case.W
    assert G <= L.RENDER_MAX_PROBLEMS
    al = alloc or placement.Plain(DEV)
    tab = table_buffer(planes, C)
    md = al.to(torch.from_numpy(tab), {"maps": None})
    lut_np = np.concatenate([lut.reshape(-1), np.full(GUARD, BYTE_GUARD, dtype=np.uint8)])
    ld = al.to(torch.from_numpy(lut_np), {"lut": None})
    step = 3 * H * W + case.out_pad
    od = al.full((G * n * step + GUARD,), out_fill, torch.uint8, {"out": None})
    rd = al.full((2 * G + GUARD,), RANGE_GUARD, torch.float32, {"range_out": G})     # (a straddle: inside the 2 G floats)
    gd = pd = None
    if given is not None:
        g_np = np.concatenate([np.asarray(given, dtype=np.float32).reshape(-1), np.full(GUARD, MAP_GUARD, dtype=np.float32)])
        gd = al.to(torch.from_numpy(g_np), {"range_in": G})
    istep = 3 * W + IMG_PAD
    if pics is not None:
        p_np = np.full((G, H, istep), BYTE_GUARD, dtype=np.uint8)
        for g in range(G):
            p_np[g, :, :3 * W] = pics[g].reshape(H, 3 * W)
        p_np = np.concatenate([p_np.reshape(-1), np.full(GUARD, BYTE_GUARD, dtype=np.uint8)])
        pd = al.to(torch.from_numpy(p_np), {"image": None})
    arr = (L.RenderProblem * G)()
    for g in range(G):
        p = arr[g]
        p.maps = md.data_ptr() + 4 * ((g * n * C + min(1, C - 1)) * h * w)
        p.map_stride, p.n_maps = C * h * w, n
        p.range_in = None if gd is None else gd.data_ptr() + 8 * g
        if range_in_ptrs is not None:
            p.range_in = range_in_ptrs[g]
        p.range_out = rd.data_ptr() + 8 * g
        if pd is not None:
            p.image, p.image_stride = pd.data_ptr() + g * H * istep, istep
        p.out, p.out_stride = od.data_ptr() + g * n * step, step
    flags = (L.RENDER_BILINEAR if case.bilinear else 0) | (L.RENDER_BLEND if pics is not None else 0)
    L.check(L.load().ca_heatmap_render(arr, G, h, w, H, W, ld.data_ptr(), case.alpha or 0.0, flags,
                                       torch.cuda.current_stream().cuda_stream), "ca_heatmap_render")
    torch.cuda.synchronize()
    assert np.array_equal(md.cpu().numpy().view(np.uint32), tab.view(np.uint32)), "the map table changed"
    assert np.array_equal(ld.cpu().numpy(), lut_np), "the look-up table changed"
    if pd is not None:
        assert np.array_equal(pd.cpu().numpy(), p_np), "the pictures changed"
    if gd is not None:
        assert np.array_equal(gd.cpu().numpy().view(np.uint32), g_np.view(np.uint32)), "the given ranges changed"
    o = od.cpu().numpy()
    assert (o[G * n * step:] == out_fill).all(), "bytes behind the output were written"
    o = o[:G * n * step].reshape(G, n, step)
    assert (o[:, :, 3 * H * W:] == out_fill).all(), "bytes between two output planes were written"
    r = rd.cpu().numpy()
    assert (r[2 * G:] == np.float32(RANGE_GUARD)).all(), "floats behind range_out were written"
    return np.ascontiguousarray(o[:, :, :3 * H * W]).reshape(G, n, H, W, 3), r[:2 * G].reshape(G, 2), rd


def check(case, out, ranges, refs):
    for g, (ref, (lo, hi)) in enumerate(refs):
        assert same_f32(ranges[g, 0], lo) and same_f32(ranges[g, 1], hi), (case.name, g, ranges[g], lo, hi)
        if not np.array_equal(out[g], ref):
            bad = np.argwhere(out[g] != ref)
            k, y, x, c = bad[0]
            raise AssertionError(f"{case.name} group {g}: {len(bad)} bytes differ, first at plane {k} pixel ({y}, {x}) "
                                 f"channel {c}: {out[g][k, y, x]} against {ref[k, y, x]}")


def run_case(case, alloc=None, **kw):
    inputs = case.inputs()
    out, ranges, _ = launch(case, inputs, alloc=alloc, **kw)
    check(case, out, ranges, case.references(LUT, inputs))
    return out, ranges


@pytest.mark.parametrize("case", [c for c in R.CASES if c.groups <= L.RENDER_MAX_PROBLEMS], ids=repr)
def test_every_case_equals_the_restatement(case):
    run_case(case)


def test_seventeen_groups_and_every_option_through_the_wrapper():
    lut = torch.from_numpy(LUT).to(DEV)
    for name in ("groups17", "groups10", "blend-alpha0.3", "given-narrow", "maps19-C3"):
        case = R.BY_NAME[name]
        planes, given, pics = case.inputs()
        k = min(1, case.C - 1)
        tabs = [torch.from_numpy(table_buffer([p], case.C)[:-GUARD].reshape(case.n_maps, case.C, case.h, case.w)).to(DEV)
                for p in planes]
        out, used = ops.heatmap_render(
            [t[:, k] for t in tabs], lut, size=(case.H, case.W), bilinear=case.bilinear,
            images=None if pics is None else [torch.from_numpy(p).to(DEV) for p in pics], alpha=case.alpha,
            ranges=None if given is None else torch.tensor(np.asarray(given, dtype=np.float32), device=DEV))
        torch.cuda.synchronize()
        assert len(out) == case.groups and tuple(used.shape) == (case.groups, 2)
        check(case, [o.cpu().numpy() for o in out], used.cpu().numpy(), case.references(LUT, (planes, given, pics)))


def test_the_same_bytes_on_a_second_launch_and_over_another_garbage():
    for name in ("geo-37x53-to-100x75-bilinear", "maps257-C3", "blend-alpha0.5", "family-nan-nearest"):
        case = R.BY_NAME[name]
        a, ra = run_case(case)
        b, rb, _ = launch(case)
        c, rc, _ = launch(case, out_fill=0x3C)
        assert a.tobytes() == b.tobytes() == c.tobytes(), name
        assert ra.tobytes() == rb.tobytes() == rc.tobytes(), name


def test_range_in_may_be_the_range_out_of_an_earlier_launch():
    first, second = R.BY_NAME["family-heat-nearest"], R.BY_NAME["given-data"]
    _, r1, rd = launch(first)
    planes, _, _ = second.inputs()
    given = [tuple(r1[0])] * second.groups                      # every group of the second launch reads group 0's range
    out, r2, _ = launch(second, (planes, None, None), range_in_ptrs=[rd.data_ptr()] * second.groups)
    check(second, out, r2, second.references(LUT, (planes, given, None)))
    assert np.array_equal(rd.cpu().numpy()[:2], r1[0]), "the earlier launch's range changed"


def test_the_range_is_the_one_seg_score_finds():
    """ca_seg_score's lo / hi are pinned by tests/test_seg_kernels_gpu.py: the same map gives the same two floats here."""
    case = R.Case("seg-tie", 64, 64, 64, 64, n_maps=1, family="heat", seed=91)
    planes, _, _ = case.inputs()
    _, ranges, _ = launch(case, (planes, None, None))
    md = torch.from_numpy(planes[0][0]).to(DEV)
    res = torch.zeros(1, ops.SEG_RECORD_BYTES, dtype=torch.uint8, device=DEV)
    ops.seg_score([md], [torch.ones(64, 64, dtype=torch.uint8, device=DEV)], res)
    rec = L.SegRecord.from_buffer_copy(res.cpu().numpy().tobytes())
    assert np.float32(rec.lo) == ranges[0, 0] and np.float32(rec.hi) == ranges[0, 1]


def test_a_matplotlib_table_and_a_side_stream():
    case = R.BY_NAME["geo-64x64-to-224x224-bilinear"]
    lut = R.cmap_lut("plasma")
    assert np.array_equal(ops.colormap_lut("plasma", DEV).cpu().numpy(), lut)
    assert ops.colormap_lut("plasma", DEV) is ops.colormap_lut("plasma", DEV)
    inputs = case.inputs()
    stream = torch.cuda.Stream()
    # (behind a gate, tests/stream_gate.py: a launch on another stream would read poison instead of these inputs)
    warm = stream_gate.Recording(DEV)
    launch(case, inputs, lut=lut, alloc=warm)
    with torch.cuda.stream(stream):
        out, ranges, _ = launch(case, inputs, lut=lut, alloc=stream_gate.Gated(warm, stream_gate.Gate()))
    stream.synchronize()
    check(case, out, ranges, case.references(lut, inputs))


def test_the_wrapper_rejects_what_the_kernel_cannot_take():
    lut = torch.from_numpy(LUT).to(DEV)
    ok = torch.zeros(2, 3, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="16384"):
        ops.heatmap_render([torch.zeros(1, 128, 129, device=DEV)], lut)
    with pytest.raises(ValueError, match="4096"):
        ops.heatmap_render([ok[:, 0]], lut, size=4097)
    with pytest.raises(ValueError):
        ops.heatmap_render([ok[:, :, :, :4][:, 0]], lut)                # rows not contiguous
    with pytest.raises(ValueError):
        ops.heatmap_render([ok[:, 0].double()], lut)
    with pytest.raises(ValueError):
        ops.heatmap_render([ok[:, 0]], lut[:258])
    with pytest.raises(ValueError, match="alpha"):
        ops.heatmap_render([ok[:, 0]], lut, images=torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="alpha"):
        ops.heatmap_render([ok[:, 0]], lut, images=torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV), alpha=1.5)
    with pytest.raises(ValueError):
        ops.heatmap_render([ok[:, 0]], lut, images=torch.zeros(8, 9, 3, dtype=torch.uint8, device=DEV), alpha=0.5)
    with pytest.raises(ValueError):
        ops.heatmap_render([ok[:, 0]], lut, ranges=torch.zeros(3, 2, device=DEV))
    with pytest.raises(ValueError):
        ops.heatmap_render([ok[:, 0]], lut, out=[torch.zeros(2, 8, 8, 4, dtype=torch.uint8, device=DEV)[..., :3]])
    out, used = ops.heatmap_render([ok[:, 2]], lut, size=5)             # and the call itself is fine: a constant group is bad
    torch.cuda.synchronize()
    assert tuple(out[0].shape) == (2, 5, 5, 3) and bool((out[0] == lut[R.ROW_BAD]).all()) and bool((used == 0).all())
