"""GPU (MI355X): bench.py's plain run - the headline only, exactly --steps timed steps, the result line's keys - and
--dump-outputs, which writes the last timed step's maps: the same bytes from run to run, pair 0's maps the reference's."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu


def _plain_run(dump_dir, steps):
    cmd = [sys.executable, os.path.join(util.ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", "16",
           "--dump-outputs", str(dump_dir)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_exactly_steps_and_dumps_its_outputs(tmp_path):
    a = _plain_run(tmp_path / "a", 3)
    assert a["steps"] == a["steps_requested"] == 3 and a["full"] is False
    assert a["unit"] == "pairs/s" and a["higher_is_better"] is True and a["dtype"] == "u8" and a["metric"].startswith("stereo pairs/sec")
    assert a["value"] > 0 and a["ms_per_step"] > 0 and abs(a["ms_per_step"] * a["steps"] - 1e3 * a["timed_seconds"]) < 1.5
    assert not set(a) & {"parity_gate", "configs", "cpu_baseline", "roofline", "host_to_host", "latency_ms_batch1", "trailer"}, sorted(a)
    d = a["dump_outputs"]
    assert d["pairs"][0] == 0 and len(d["pairs"]) == 8 and d["row_step"] == 1
    left, right = (np.load(str(tmp_path / "a" / f)) for f in ("disparity_left.npy", "disparity_right.npy"))
    assert left.dtype == right.dtype == np.float32 and left.shape == right.shape == (8, 375, 1242)
    assert left.nbytes + right.nbytes <= 64 << 20
    # pair 0 of the batch is kitti_mini pair 0: its maps are the reference's (tests/golden/digests.json)
    ref = util.digests()["kitti0_d128"]["stages"]
    sha = lambda x: hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()
    assert sha(left[0]) == ref["final1"] and sha(right[0]) == ref["final2"]
    # same arguments, same inputs, same outputs - whatever the number of steps
    _plain_run(tmp_path / "b", 2)
    for f in ("disparity_left.npy", "disparity_right.npy"):
        assert np.array_equal(np.load(str(tmp_path / "a" / f)).view(np.uint32), np.load(str(tmp_path / "b" / f)).view(np.uint32)), f
