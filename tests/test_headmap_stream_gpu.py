"""ca_head_maps' stream contract, with the helpers of tests/stream_gate.py and tests/test_stream_contract_gpu.py as they
stand: ops.head_maps enqueues on the current stream behind a gate kernel and returns without waiting, and one captured
launch gives eager's bits on replay."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import headmap_cases as H  # noqa: E402
import stream_contract_cases as P  # noqa: E402
import stream_gate as SG  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from test_headmap_kernels_gpu import DEV, NORM, inputs_and_reference, outputs, place, problems  # noqa: E402
from test_stream_contract_gpu import BF, _like, _rand, _raw, _replay_check  # noqa: E402


def test_head_maps_runs_on_its_stream_and_returns_before_it_drains():
    """A warm-up on the current stream, then the same launch on a second stream behind a gate kernel: the call returns
    while the gate still runs, and gives the warm-up's bytes."""
    case = H.BY_ID["heads_NH5_L257_C17_none_n16_all"]
    inp, _ = inputs_and_reference(case)

    def run(al):
        dev = place(case, inp, al)
        ops.head_maps(problems(case, dev), case.shape["NH"], NORM[case.shape["norm"]])
        torch.cuda.synchronize()
        return {f"{i}.{k}": v.clone() for i, g in enumerate(outputs(dev)) for k, v in g.items()}
    rec = SG.Recording(DEV)
    with SG.watching() as warm_calls:
        want = run(rec)
    assert warm_calls and rec.t_first is not None
    torch.cuda.synchronize()
    gate = SG.Gate()
    al = SG.Gated(rec, gate)
    s2 = torch.cuda.Stream()
    assert s2.cuda_stream != 0 and s2 != torch.cuda.current_stream()
    try:
        with torch.cuda.stream(s2), SG.watching(gate) as calls:
            got = run(al)
    finally:
        torch.cuda.synchronize()
    al.release()
    seen = [(n, running) for n, running, _ in calls if n not in P.NO_STREAM]
    assert tuple(n for n, _ in seen) == ("ca_head_maps",), seen
    assert all(running for _, running in seen), "ca_head_maps returned only after the gate had finished"
    assert set(got) == set(want)
    for k in want:
        assert _raw(got[k]) == _raw(want[k]), f"{k} behind the gate != the warm-up run"


@pytest.mark.parametrize("norm", ["none", "entmax15"])
def test_replay_head_maps_with_the_accumulators_reset_inside_the_capture(norm):
    Lp, Cc, NH = 300, 12, 5
    sets = [dict(img=_rand((Lp, NH * 128), s, 1.0, BF), con=_rand((Cc, NH * 128), s + 1, 0.2, BF), acc0=_rand((Cc, Lp), s + 2))
            for s in (7, 17)]
    st = _like(sets[0])
    outs = dict(acc=torch.empty(Cc, Lp, device=DEV), heads=torch.empty(NH, Cc, Lp, device=DEV))

    def call():
        outs["acc"].copy_(st["acc0"])            # the accumulators' reset: inside the capture
        outs["heads"].zero_()
        ops.head_maps([ops.HeadMaps(st["img"], st["con"], heads=outs["heads"], weight_h=1.0, acc=outs["acc"], weight=0.5)],
                      NH, NORM[norm])
    _replay_check("head_maps", sets, st, outs, call)
    assert L.NORM_NONE == NORM["none"]
