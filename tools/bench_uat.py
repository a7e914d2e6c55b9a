"""Throughput of UAT input — mgpu_uat_encode_device (kernels/uat.inc: k_uat_index, the scans, k_uat_size, k_uat_write) — on a drawn
feed of about 10^6 downlink lines of dump978's form (tests/uat_util.py: feed) resident in HBM, every optional array asked for.  Beside
it, in the same process: (i) a plain device-to-device copy of the same number of input-plus-output bytes, (ii) with --harness PATH the
reference's uat2esnt_convert_message on one core of this host over the same lines (tests/host_stub/uat_ref_harness.c, the conversion
only: the file is read and cut into lines before the clock starts)
(python tools/bench_uat.py [--lines N] [--harness PATH] | --build-harness DIR).  One JSON line per row.  Two clocks around the
synchronous C-ABI call: HIP events recorded on the null stream before and behind it, and the host's wall clock (launches, the
stream's synchronisation and the read-back of the five totals are inside both); run it under `rocprofv3 --kernel-trace --stats`
for the split into the passes."""
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
from readsb_amd import binding  # noqa: E402
import uat_util as uu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--harness", default=None)
    ap.add_argument("--build-harness", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.build_harness:                                              # where the full reference build is (make -C oracle full): no GPU needed
        os.makedirs(a.build_harness, exist_ok=True)
        print(uu.build_ref_harness(a.build_harness))
        return
    drawn = b"".join(uu.feed(1 << 14, seed=11))                      # 16 384 drawn lines, repeated
    reps_in = max(a.lines // (1 << 14), 1)
    nlines = reps_in << 14
    text = np.frombuffer(drawn * reps_in, dtype=np.uint8)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    def malloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), nbytes) == 0
        return p.value
    d = readsb_amd.Demodulator(max_samples=1 << 20)
    most = 4 * nlines
    d_text, d_out, d_msgs, d_sig, d_line = malloc(text.size), malloc(most * 45), malloc(most * 64), malloc(most), malloc(most * 8)
    assert hip.hipMemcpy(d_text, text.ctypes.data, text.size, 1) == 0
    c = [C.c_uint64(0) for _ in range(6)]
    deferred = np.zeros(4096, dtype=np.uint64)
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0

    def by_events(f):
        """-> (ms by the two events, s by the wall clock) of one synchronous call"""
        assert hip.hipEventRecord(ev[0], None) == 0
        t0 = time.perf_counter()
        f()
        wall = time.perf_counter() - t0
        assert hip.hipEventRecord(ev[1], None) == 0 and hip.hipEventSynchronize(ev[1]) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        return float(ms.value), wall

    def timed(f):
        for _ in range(3):
            f()
        t = [by_events(f) for _ in range(a.reps)]
        return float(np.median([x[0] for x in t])) * 1e-3, float(np.median([x[1] for x in t]))

    def encode(records=True):
        args = binding.UatArgs(C.sizeof(binding.UatArgs), 0, d_text, text.size, d_out, most * 45, d_msgs if records else None, d_sig if records else None,
                               d_line if records else None, most if records else 0, deferred.ctypes.data, deferred.size, 1700000000000, *[C.pointer(x) for x in c], 0)
        assert d.lib.mgpu_uat_encode_device(d.ctx, C.byref(args)) == 0
    encode()
    nbytes, consumed, lines, nframes, nshort, ndef = (int(x.value) for x in c)
    assert consumed == text.size and lines == nlines and ndef == 0
    moved = text.size + nbytes
    d_a, d_b = malloc(moved), malloc(moved)

    def copy():
        assert hip.hipMemcpy(d_b, d_a, moved, 3) == 0 and hip.hipDeviceSynchronize() == 0
    rows = []
    for name, f, b in (("mgpu_uat_encode_device (text, records, signal bytes, source lines)", encode, moved + nframes * 73),
                       ("mgpu_uat_encode_device (text only)", lambda: encode(False), moved),
                       ("(i) hipMemcpy device to device of the input-plus-output bytes", copy, moved)):
        ev_s, wall_s = timed(f)
        rows.append({"job": name, "lines": nlines, "input_bytes": int(text.size), "frames": nframes, "output_bytes": nbytes, "short": nshort, "us_per_call_events": round(ev_s * 1e6, 1),
                     "us_per_call_wall": round(wall_s * 1e6, 1), "lines_per_s": round(nlines / ev_s), "GB_per_s_in_plus_out": round(moved / ev_s / 1e9, 2),
                     "bytes_read_and_written": b, "reps": a.reps})
        print(json.dumps(rows[-1]), flush=True)
    print(json.dumps({"ratio": "encode (text only) time / copy time of the same input-plus-output bytes, by events",
                      "value": round(rows[1]["us_per_call_events"] / rows[2]["us_per_call_events"], 2),
                      "with_records": round(rows[0]["us_per_call_events"] / rows[2]["us_per_call_events"], 2)}), flush=True)
    if a.harness:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "feed.bin")
            text.tofile(path)
            r = subprocess.run([a.harness, path, "/dev/null", "/dev/null", "3"], check=True, capture_output=True, text=True)
        w = r.stdout.split()
        sec = float(w[1])
        print(json.dumps({"job": "(ii) the reference's uat2esnt_convert_message, one CPU core (tests/host_stub/uat_ref_harness.c)", "lines": int(w[3]), "seconds": sec,
                          "lines_per_s": round(int(w[3]) / sec), "encode_speedup_by_events": round(sec / (rows[0]["us_per_call_events"] * 1e-6), 1)}))
    d.close()


if __name__ == "__main__":
    main()
