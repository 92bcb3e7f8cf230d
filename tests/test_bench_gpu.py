"""bench.py's plain run: the headline line only, and --dump-outputs writing what the last timed step
returned (records and inlier lists), checked against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as orc
import pitt_object_table_segmentation_amd as pitt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(tmp_path):
    B, P, W, K = 3, 2, 1, 3
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
                        "--settle-steps", "0", "--pipeline", str(P), "--frames-per-gpu", str(B), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == K and line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and abs(line["value"] - B / (line["ms_per_step"] * 1e-3)) <= 0.01 * line["value"]
    assert line["untimed_steps"] == W
    # nothing beside the headline in a plain run
    for k in ("roofline", "kernels", "value_without_settle", "steady_state", "clutter", "config5", "cpu_baseline"):
        assert k not in line, k

    files = sorted(os.listdir(out))
    assert set(files) == {n + ".npy" for n in pitt.RESULT_DTYPE.names} | {
        "inlier_index_sums.npy", "inlier_sample_frames.npy", "inlier_sample.npy"}
    arr = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arr.values())
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    # the last of W + K pipelined steps ran slot (W + K - 1) % P, whose batch holds frames slot * B + [0, B)
    slot = (W + K - 1) % P
    assert arr["inlier_sample_frames"].tolist() == list(range(B))  # B <= 16: every frame is in the sample
    for f in range(B):
        o = orc.plane_segment(*pitt.synth_frame(pitt.SCENE_TABLE, 1000 + slot * B + f, 640, 480))
        n = len(o.inliers)
        assert np.array_equal(arr["coefficients"][f].view(np.int32), o.coefficients.view(np.int32)), f
        assert arr["n_inliers"][f] == n and arr["hypotheses"][f] == o.hypotheses, f
        assert arr["inlier_index_sums"][f] == float(o.inliers.astype(np.int64).sum()), f
        row = arr["inlier_sample"][f]
        assert np.array_equal(row[:n], o.inliers.astype(np.float32)) and np.all(row[n:] == -1), f
