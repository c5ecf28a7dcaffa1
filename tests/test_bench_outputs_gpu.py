"""A plain `bench.py` run (no --full) measures the headline alone and, with --dump-outputs DIR, writes what its last timed step
computed: the E/P/L correlator values of every channel-epoch, from seeded inputs, so that two runs (or two builds) can be compared
output for output."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--epochs", "16", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_dumps_the_last_step_and_nothing_else_runs(tmp_path):
    j = _plain_run(tmp_path / "a")
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    assert j["unit"] == "Msamples/s" and j["higher_is_better"] is True and j["dtype"] == "f32" and j["metric"]
    # the --full entries did not run
    assert j["roofline"]["segments_ms"] is None and j["cpu_baseline"] is None
    for k in ("shared_stream", "int16_input", "galileo_e1_5tap", "hybrid_gps_galileo_beidou", "closed_loop", "acquisition"):
        assert k not in j, k

    a = np.load(tmp_path / "a" / "correlators.npy")
    assert a.dtype == np.float32 and a.shape == (32, 16, 3, 2) and np.all(np.isfinite(a))
    # the check --full makes: every channel's prompt sees its satellite (amplitude from the stream's seed, as bench.py draws it)
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    amp = []
    for gid in range(32):
        rng = np.random.Generator(np.random.PCG64(1002 + 7 * gid))
        amp.append(np.sqrt(10.0 ** (rng.uniform(38.0, 48.0) / 10.0) / bench.FS))
    pmag = np.hypot(a[:, :, 1, 0], a[:, :, 1, 1]).mean(axis=1)
    assert np.all(pmag > 0.5 * np.array(amp) * bench.N_EPOCH)

    # same arguments, same inputs: a second run computes the same values bit for bit (no atomics in the batched launch)
    _plain_run(tmp_path / "b")
    assert np.load(tmp_path / "b" / "correlators.npy").tobytes() == a.tobytes()
