"""`bench.py` as a command on the GPU: a plain run prints the headline line and nothing that belongs to --full, and
--dump-outputs writes the last step's arrays, the same from run to run (a small step: 6 frames, 2 timed steps)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 6
FULL_ONLY = ("stage_timing", "stage_rooflines", "h2d_upload_ms_per_step", "pcie_inclusive_frames_per_s", "end_to_end",
             "png_end_to_end", "loop_handler", "sequence", "roofline", "cpu_baseline")


def _plain_run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--frames", str(FRAMES), "--dump-outputs", str(out_dir)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_headline_and_dumps_repeatable_outputs(tmp_path):
    res = [_plain_run(tmp_path / d) for d in ("a", "b")]
    d = res[0]
    assert d["full"] is False and d["steps"] == 2 and d["warmup"] == 1
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(FRAMES / (d["ms_per_step"] / 1e3), rel=1e-3)  # the two are one measurement
    assert all(d[k] is None for k in FULL_ONLY) and d["stages_ms_per_launch"] == {} and "pose_check" not in d
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"poses.npy", "keypoint_count.npy", "keypoints.npy", "matches.npy", "filtered.npy", "edges.npy",
            "map_keyframes.npy", "map_landmarks.npy"} <= set(names)
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all()
        np.testing.assert_array_equal(a, b, err_msg=n)
        total += a.nbytes
    assert total <= 64 << 20
    poses = np.load(tmp_path / "a" / "poses.npy")
    assert poses.shape == (FRAMES, 7)
    np.testing.assert_allclose(np.linalg.norm(poses[:, :4], axis=1), 1.0, atol=1e-9)  # unit quaternions: poses written
    kpc = np.load(tmp_path / "a" / "keypoint_count.npy")
    assert kpc.shape == (2 * FRAMES + 1,) and (kpc > 0).all()
    assert d["config"]["mean_keypoints_per_image"] == pytest.approx(kpc.mean(), abs=0.06)
