"""bench.py's plain run and --dump-outputs: a plain run times the LM steps only (the extras'
keys are null until --full asks for them), --steps sets the number of timed trips, and the
dumped arrays are what the timed solve returned -- bitwise the drop-in LevMarq called with the
same arguments in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_writes_whole_float64_arrays(tmp_path):
    d = tmp_path / "out" / "nested"
    a = {"X": np.arange(5, dtype=np.float32), "F0": np.linspace(0.0, 1.0, 7)}
    bench.dump_outputs(str(d), a)
    assert sorted(os.listdir(d)) == ["F0.npy", "X.npy"]
    for k, v in a.items():
        z = np.load(d / f"{k}.npy")
        assert z.dtype == np.float64 and np.array_equal(z, v)


def test_dump_outputs_samples_past_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8 * 100)
    big, small = np.arange(1000, dtype=np.float64), np.arange(10, dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    za, zb = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert np.array_equal(za, zb)                                   # the same entries in every run
    assert za.size == 50 and np.all(np.diff(za) > 0) and np.all(np.isin(za, big))
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 8 * 100 + 2 * 128


def test_options_default_to_a_plain_run(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"])
    a = bench._args()
    assert a.full is False and a.dump_outputs is None and a.steps == 4 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench._args()
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_dumps_what_the_timed_solve_returned(tmp_path):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import Context, DeviceObjective, run_levmarq
    m, n, steps = 600, 130, 3
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--residuals", str(m), "--params", str(n), "--dump-outputs", str(d)],
                       capture_output=True, timeout=240)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["trips_accepted"] + line["trips_rejected"] == steps
    assert line["ms_per_step"] > 0 and abs(line["ms_per_step"] * line["value"] - 1e3) <= 1e-6
    assert line["full"] is False
    for k in ("bfgs_hg", "bfgs_cfg2_solve", "bfgs_bnd_cfg5_solve", "cpu_baseline", "rows_mode_extra"):
        assert line[k] is None, k
    obj = DeviceObjective.synthetic(Context(0), L.OBJ_LINRES, n, m)
    X, F0, FO, _ = run_levmarq(obj, np.zeros(n), [0.001, 10.0, 1e-7, steps, 0.0, -1])
    assert sorted(os.listdir(d)) == ["F0.npy", "FOpt.npy", "X.npy"]
    for name, ref in (("X", X), ("F0", F0), ("FOpt", FO)):
        z = np.load(d / f"{name}.npy")
        assert z.dtype == np.float64 and np.array_equal(z, ref), name
