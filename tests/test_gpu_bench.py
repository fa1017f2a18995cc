"""bench.py's command line: a plain run times `--steps` steps and prints the headline line only,
`--dump-outputs` writes what the last timed step computed (equal bit for bit to the same steps
through the Python mirror), `--full` adds the CPU baseline.  Small shapes: the benchmark's own
process is what is under test here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hsddp
from hsddp import synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = ["--batch", "48", "--phases", "2", "--knots", "10"]


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *SHAPE, *args],
                       cwd=ROOT, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_dumps_last_step_outputs(tmp_path):
    out = _bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert out["higher_is_better"] is True and out["dtype"] == "f64" and out["unit"] == "trajectory-iterations/s"
    assert out["value"] == pytest.approx(48 * 1e3 / out["ms_per_step"], rel=1e-9)
    assert "cpu_baseline" not in out
    files = sorted(os.listdir(tmp_path))
    assert files and all(f.endswith(".npy") for f in files)
    arrs = {f[:-4]: np.load(tmp_path / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20

    # the same steps through the mirror: 1 warm-up + 2 timed inner iterations of the same batch
    prob = syn.make_batch(48, 2, 10, "trot")
    s = hsddp.Solver(prob, hsddp.load_settings(no_early_exit=1, max_AL_iter=1, max_DDP_iter=3))
    s.begin()
    s.iterate(1)
    s.iterate(2)
    info, tr, cmds = s.element_info(), s.trajectory(), s.extract_commands()
    s.close()
    idx = arrs["sample_elements"].astype(int)
    assert len(idx) == 48 and np.array_equal(idx, np.arange(48))  # the whole batch when it is small
    assert np.array_equal(arrs["Xbar"], tr["Xbar"][idx]) and np.array_equal(arrs["Ubar"], tr["Ubar"][idx])
    assert np.all(arrs["info_iters"] == 3)
    for f in ("cost", "feas", "merit", "n_ls_trials", "status"):
        assert np.array_equal(arrs["info_" + f], info[f].astype(np.float64)), f
    for f in ("hkd_controls", "des_body_state", "feedback", "mpc_times", "contacts"):
        assert np.array_equal(arrs["cmd_" + f], cmds[f].astype(arrs["cmd_" + f].dtype)), f


def test_full_run_adds_cpu_baseline():
    out = _bench("--steps", "1", "--warmup", "1", "--full", "--cpu-elements", "8", "--cpu-iters", "1")
    assert out["steps"] == 1 and out["ms_per_step"] > 0
    cpu = out["cpu_baseline"]
    assert cpu["unit"] == out["unit"] and cpu["value"] > 0 and cpu["kind"] == "port"
