"""ca_propagate_maps' stream contract, with the helpers of tests/stream_gate.py and tests/test_stream_contract_gpu.py as
they stand: ops.propagate_maps enqueues its two launches on the current stream behind a gate kernel and returns without
waiting, and one captured call gives eager's bits on replay (the workspace is passed in: nothing is allocated under
capture)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import propmap_cases as PM  # noqa: E402
import stream_contract_cases as P  # noqa: E402
import stream_gate as SG  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from test_propmap_kernels_gpu import DEV, place, problem  # noqa: E402
from test_stream_contract_gpu import BF, _like, _rand, _raw, _replay_check  # noqa: E402

STREAM_CASES = [c for c in PM.CASES if (c.heads, c.f16, c.prescaled) == (3, False, False) and c.nq <= 200][:3]


def test_propagate_maps_runs_on_its_stream_and_returns_before_it_drains():
    """A warm-up on the current stream, then the same call on a second stream behind a gate kernel: the call returns while
    the gate still runs, and gives the warm-up's bytes."""
    assert len(STREAM_CASES) == 3

    def go(al):
        dev = [place(c, al, tag=f"[{i}]") for i, c in enumerate(STREAM_CASES)]
        need = sum((c.heads * c.C * c.nq * 4 + 15) // 16 * 16 for c in STREAM_CASES)
        ws = al.full((need,), 0, torch.uint8)
        ops.propagate_maps([problem(c, d) for c, d in zip(STREAM_CASES, dev)], 3, PM.SCALE_LOG2, workspace=ws)
        torch.cuda.synchronize()
        return {f"{i}.{k}": d[k].clone() for i, d in enumerate(dev) for k in ("acc", "acc2")}
    rec = SG.Recording(DEV)
    with SG.watching() as warm_calls:
        want = go(rec)
    assert warm_calls and rec.t_first is not None
    torch.cuda.synchronize()
    gate = SG.Gate()
    al = SG.Gated(rec, gate)
    s2 = torch.cuda.Stream()
    assert s2.cuda_stream != 0 and s2 != torch.cuda.current_stream()
    try:
        with torch.cuda.stream(s2), SG.watching(gate) as calls:
            got = go(al)
    finally:
        torch.cuda.synchronize()
    al.release()
    seen = [(n, running) for n, running, _ in calls if n not in P.NO_STREAM]
    assert tuple(n for n, _ in seen) == ("ca_propagate_maps",), seen
    assert all(running for _, running in seen), "ca_propagate_maps returned only after the gate had finished"
    assert set(got) == set(want)
    for k in want:
        assert _raw(got[k]) == _raw(want[k]), f"{k} behind the gate != the warm-up run"


def test_replay_propagate_maps_with_the_accumulator_reset_inside_the_capture():
    nq, n0, n1, heads, C = 70, 24, 150, 2, 5
    W = heads * 128
    sets = [dict(qkv=_rand((n0 + n1, 3 * W), s, 1.0, BF), v=_rand((C, n1), s + 2), acc0=_rand((C, nq), s + 1)) for s in (5, 15)]
    st = _like(sets[0])
    outs = dict(acc=torch.empty(C, nq, device=DEV))
    ws = torch.empty(heads * C * nq * 4, dtype=torch.uint8, device=DEV)

    def call():
        outs["acc"].copy_(st["acc0"])            # the accumulator's reset: inside the capture
        qkv = st["qkv"]
        ops.propagate_maps([ops.PropagateMaps(qkv[:nq, :W], qkv[:n0, W:2 * W], qkv[n0:, W:2 * W], st["v"], acc=outs["acc"],
                                              weight=0.5)], heads, PM.SCALE_LOG2, workspace=ws)
    _replay_check("propagate_maps", sets, st, outs, call)
