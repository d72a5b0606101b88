"""bench.py's plain run (no --full) on the real HIP path: the headline line and nothing else, and --dump-outputs writing
what the last timed step returned.  --full's extras (batched_equals_single and the rest) are exercised by
tests/test_multirank_gpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out_dir, maps = str(tmp_path / "out"), str(tmp_path / "maps.npy")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "2", "--dump-outputs", out_dir, "--dump-maps", maps],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["metric"].startswith("concept-heatmaps/sec") and line["unit"] == "concept-heatmaps/s"
    assert line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(3 * 4 / (3 * line["ms_per_step"] * 1e-3))
    # what only --full measures did not run
    assert "cpu_baseline" not in line and line["batched_equals_single"] is None
    assert line["concept_attention_block"] is None and line["roofline_attention"] is None
    assert line["roofline"]["kernel"] == "whole path"

    assert sorted(os.listdir(out_dir)) == ["concept_heatmaps.npy", "cross_attention_maps.npy", "image_latent.npy"]
    got = {n: np.load(os.path.join(out_dir, n + ".npy")) for n in ("image_latent", "concept_heatmaps",
                                                                   "cross_attention_maps")}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["image_latent"].shape == (1, 4096, 64) and np.isfinite(got["image_latent"]).all()
    # the last timed step is the last item of the gathered maps ([items, 2, C, side, side])
    all_maps = np.load(maps)
    assert all_maps.shape == (3, 2, 4, 64, 64)
    assert np.array_equal(got["concept_heatmaps"], all_maps[-1:, 0])
    assert np.array_equal(got["cross_attention_maps"], all_maps[-1:, 1])
    for name in ("concept_heatmaps", "cross_attention_maps"):
        assert np.abs(got[name].sum(axis=1) - 1.0).max() < 1e-3, name   # softmax over the concepts
