"""Throughput of mgpu_snip_device (kernels/snip.inc: `readsb --snip` on the GPU) on a UC8 block resident in HBM
(python tools/bench_snip.py [--gib G] [--reps N] [--reference PATH]).

The block is a seeded capture of tools/synth_iq.c (16 Mi samples, 900 messages/s) repeated to --gib GiB on the device.  Three levels:
1 (only the byte pair 127, 127 is quiet: everything is kept), 8 (the noise is quiet, the messages and 32 samples behind each are kept:
about a tenth) and 129 (everything is quiet: 32 samples are kept).  Per level one JSON line: microseconds per call — wall clock around
the synchronous C-ABI call, which ends in a stream synchronise and the read-back of two totals — the algorithmic bytes 2n + 2 * kept
over that time and as a share of the 8 TB/s peak, an upper bound of the bytes the three passes move (the count pass reads the input
and writes a keep bit per sample; the write pass reads the bits, reads the 16-byte groups that keep something — at most the whole input
a SECOND time — and writes the kept samples), and the ratio to a plain device-to-device copy of the same 2n bytes (hipMemcpy + device
synchronise) timed in the same process, alternating with the calls.  The kept count is checked against tests/snip_util.py's model
scaled from one repetition of the capture.  Run it under `rocprofv3 --kernel-trace --stats`, in a run of its own, for the kernels'
own durations.  --reference PATH (oracle/_ref/full/readsb_full): the reference's own rate, one core of this host, `--snip 8` over the
first 256 MiB through a file, process start included."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import readsb_amd  # noqa: E402
import beast_util as bu  # noqa: E402
import helpers  # noqa: E402
import snip_util as su  # noqa: E402

PEAK_BYTES_PER_S = 8e12
UNIT = 16 << 20                                     # samples of the capture that is repeated


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reference", default=None)
    a = ap.parse_args()
    unit = helpers.synth(nsamples=UNIT, seed=20, rate=900.0)
    copies = max(int(a.gib * (1 << 30)) // unit.nbytes, 1)
    n = copies * UNIT
    d = readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=131072)
    hip = bu.Hip()
    hip.rt.hipDeviceSynchronize.argtypes = []
    d_iq, d_out = hip.malloc(2 * n), hip.malloc(2 * n)
    for k in range(copies):
        assert hip.rt.hipMemcpy(d_iq + k * unit.nbytes, unit.ctypes.data, unit.nbytes, 1) == 0

    def copy():
        assert hip.rt.hipMemcpy(d_out, d_iq, 2 * n, 3) == 0 and hip.rt.hipDeviceSynchronize() == 0

    for level in (1, 8, 129):
        # the model on one repetition: every further one starts with the counter the one before left
        first, c1 = su.model(unit.tobytes(), level)
        again, c2 = su.model(unit.tobytes(), level, c1)
        want = (len(first) + (copies - 1) * len(again)) // 2
        assert min(c1, 33) == min(c2, 33)                      # ... which decides no differently from the third on
        call = lambda: d.snip_device(d_iq, n, level, d_out, n)
        for _ in range(3):
            kept, run = call()
            copy()
        assert kept == want, (level, kept, want)
        call()                                             # (the copy above went into the same buffer)
        head = hip.download(d_out, min(len(first), 1 << 20)).tobytes()
        assert head == first[: len(head)]
        t_call, t_copy = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            copy()
            t2 = time.perf_counter()
            t_call.append(t1 - t0)
            t_copy.append(t2 - t1)
        us, us_best, cp = np.median(t_call) * 1e6, min(t_call) * 1e6, np.median(t_copy) * 1e6
        alg = 2 * n + 2 * kept
        moved_max = 2 * n + n // 8 + n // 8 + min(2 * n, 16 * kept) + 2 * kept
        print(json.dumps({"call": "mgpu_snip_device", "level": level, "samples": n, "kept": kept, "kept_fraction": round(kept / n, 6),
                          "us_per_call": round(us, 1), "us_per_call_best": round(us_best, 1), "algorithmic_bytes": alg,
                          "algorithmic_bytes_per_s": round(alg / us * 1e6), "share_of_8TBps_peak": round(alg / us * 1e6 / PEAK_BYTES_PER_S, 4),
                          "bytes_moved_at_most": moved_max, "moved_bytes_per_s_at_most": round(moved_max / us * 1e6),
                          "copy_2n_bytes_us": round(cp, 1), "copy_bytes_per_s_read_plus_write": round(4 * n / cp * 1e6),
                          "call_over_copy": round(us / cp, 3), "reps": a.reps,
                          "timing": "median wall clock around the C-ABI call (launches, stream sync, read-back of the totals); the copy: hipMemcpy + hipDeviceSynchronize"}),
              flush=True)
    if a.reference:
        m = min(unit.nbytes * copies, 256 << 20)
        with tempfile.NamedTemporaryFile(dir=os.environ.get("TMPDIR", "/tmp")) as f, tempfile.NamedTemporaryFile(dir=os.environ.get("TMPDIR", "/tmp")) as g:
            for k in range(m // unit.nbytes or 1):
                f.write(unit.tobytes()[: m])
            f.flush()
            size = os.path.getsize(f.name)
            t = []
            for _ in range(3):
                with open(f.name, "rb") as fin, open(g.name, "wb") as fout:
                    t0 = time.perf_counter()
                    subprocess.run([a.reference, "--snip=8"], stdin=fin, stdout=fout, check=True)
                    t.append(time.perf_counter() - t0)
            print(json.dumps({"call": "readsb --snip 8 (the reference, one core of this host, file to file)", "input_bytes": size, "output_bytes": os.path.getsize(g.name),
                              "seconds": round(min(t), 3), "input_bytes_per_s": round(size / min(t))}), flush=True)
    hip.free_all()
    d.close()


if __name__ == "__main__":
    main()
