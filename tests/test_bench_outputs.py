"""bench.py --dump-outputs: what the timed path returned for the last feed of its last step, as float .npy files within 64 MB,
the same from run to run; a plain run (no --full) prints the headline line and nothing that takes runs of its own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers

BENCH = os.path.join(helpers.ROOT, "bench.py")


def test_dump_outputs_stays_within_budget_with_a_seeded_sample(tmp_path):
    import bench
    import readsb_amd
    n = 600000                                                     # more records than the budget holds
    msgs = np.zeros(n, dtype=readsb_amd.MSG_DTYPE)
    msgs["timestamp"] = np.arange(n, dtype=np.int64) * 12345678901
    msgs["msg"] = (np.arange(n * 14) % 251).reshape(n, 14)
    counters = {"demod_preambles": 2 ** 40 + 3, "demod_accepted": [1, 2, 3], "signal_power_sum": 0.125}
    for k in range(2):
        bench.dump_outputs(str(tmp_path / str(k)), msgs, counters)
    files = sorted(os.listdir(tmp_path / "0"))
    assert files == sorted(os.listdir(tmp_path / "1"))
    assert sum(os.path.getsize(tmp_path / "0" / f) for f in files) <= 64_000_000
    idx = np.load(tmp_path / "0" / "msg_index.npy")
    assert idx.dtype == np.float64 and 0 < len(idx) < n and (np.diff(idx) > 0).all()
    assert np.load(tmp_path / "0" / "msg_count.npy")[0] == n
    for f in files:
        a, b = np.load(tmp_path / "0" / f), np.load(tmp_path / "1" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
    ts = np.load(tmp_path / "0" / "msg_timestamp.npy")
    assert np.array_equal(ts, msgs["timestamp"][idx.astype(np.int64)].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "0" / "msg_msg.npy"), msgs["msg"][idx.astype(np.int64)].astype(np.float32))
    assert np.load(tmp_path / "0" / "counter_demod_preambles.npy")[0] == 2 ** 40 + 3
    assert list(np.load(tmp_path / "0" / "counter_demod_accepted.npy")) == [1, 2, 3]


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(built, tmp_path):
    lines = []
    for k in range(2):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--loops", "2", "--samples", str(96 * 131072),
                            "--dump-outputs", str(tmp_path / str(k))], capture_output=True, text=True, timeout=300, cwd=helpers.ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    d = lines[0]
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "Msamples/s"
    assert "cpu_baseline" not in d and "configs" not in d and "pcie_inclusive_msamples_s" not in d
    files = sorted(os.listdir(tmp_path / "0"))
    assert files == sorted(os.listdir(tmp_path / "1")) and "msg_timestamp.npy" in files and "counter_samples_processed.npy" in files
    assert sum(os.path.getsize(tmp_path / "0" / f) for f in files) <= 64_000_000
    assert np.load(tmp_path / "0" / "msg_count.npy")[0] == d["messages_per_feed"] > 0
    assert np.load(tmp_path / "0" / "counter_samples_processed.npy")[0] > 0
    for f in files:
        a, b = np.load(tmp_path / "0" / f), np.load(tmp_path / "1" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b, equal_nan=True), f
