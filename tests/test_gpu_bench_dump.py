"""bench.py's plain run and --dump-outputs on a small slice of the headline workload: --steps sets the timed steps, the line carries
ms_per_step, and two runs with the same arguments write the same float64 outputs (within 64 MB) of what the last step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu


def _run(out_dir, steps):
    cmd = [sys.executable, os.path.join(H.ROOT, "bench.py"), "--gpus", "1", "--docs", "512", "--steps", str(steps), "--warmup", "1", "--dump-outputs", out_dir]
    p = subprocess.run(cmd, cwd=H.ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    ra, rb = _run(a, 3), _run(b, 2)
    for r, steps in ((ra, 3), (rb, 2)):
        assert r["steps"] == steps and r["ms_per_step"] > 0 and r["value"] > 0 and r["full"] is False
        assert r["sustained"] is None and r["extras"] is None and r["parity"] is None and "cpu_baseline" not in r
        assert r["docs_converged"] == 512
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and "logs.npy" in names and "digests.npy" in names and "sample_values.npy" in names
    total = 0
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype == np.float64 and x.shape == y.shape and np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    logs = np.load(os.path.join(a, "logs.npy"))
    assert logs.shape == (512 * 3, 6) and (logs[:, 0] == 0).all()
    assert np.load(os.path.join(a, "docs_converged.npy"))[0] == 512
