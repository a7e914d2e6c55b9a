"""Throughput of SBS input — mgpu_sbs_decode_device (kernels/sbs_in.inc: k_sbs_in_index, the scans, k_sbs_in_size, k_sbs_in_write) — on a
drawn feed of about 10^6 BaseStation lines, three as readsb's writer prints them to one of mlat-client's (tests/sbs_in_util.py: feed),
resident in HBM, records and source lines asked for.  Beside it, in the same process: (i) a plain device-to-device copy of the same
number of input-plus-output bytes, (ii) with --harness PATH the reference's readAscii + decodeSbsLine on one core of this host over
the first --ref-lines lines (tests/host_stub/sbs_in_ref_harness.c: the difference between a run of 1 and a run of 1 + --ref-reps
passes over the stream, so that process start, the file and the dump of the records cancel)
(python tools/bench_sbs_in.py [--lines N] [--harness PATH] | --build-harness DIR).  One JSON line per row.  Two clocks around the
synchronous C-ABI call: HIP events recorded on the null stream before and behind it, and the host's wall clock (launches, the
stream's synchronisation and the read-back of the five totals are inside both); run it under `rocprofv3 --kernel-trace --stats`
for the split into the passes.  No threshold: the numbers go to profiles/sbs_in_bench.txt."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import readsb_amd  # noqa: E402
from readsb_amd import binding  # noqa: E402
import sbs_in_util as su  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--harness", default=None)
    ap.add_argument("--ref-lines", type=int, default=1 << 17)
    ap.add_argument("--ref-reps", type=int, default=4)
    ap.add_argument("--build-harness", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.build_harness:                                              # where the full reference build is (make -C oracle full): no GPU needed
        os.makedirs(a.build_harness, exist_ok=True)
        print(su.build_ref_harness(a.build_harness))
        return
    drawn = b"".join(su.feed(1 << 14, seed=11))                      # 16 384 drawn lines, repeated
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
    d_text, d_recs, d_line = malloc(text.size), malloc(nlines * 96), malloc(nlines * 8)
    assert hip.hipMemcpy(d_text, text.ctypes.data, text.size, 1) == 0
    c = [C.c_uint64(0) for _ in range(5)]
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

    def decode(lines=True):
        args = binding.SbsInArgs(C.sizeof(binding.SbsInArgs), su.SOURCES["sbs"], d_text, text.size, su.NOW_MS, d_recs, d_line if lines else None, nlines,
                                 deferred.ctypes.data, deferred.size, *[C.pointer(x) for x in c], 0)
        assert d.lib.mgpu_sbs_decode_device(d.ctx, C.byref(args)) == 0
    decode()
    consumed, lines, nrecs, ninvalid, ndef = (int(x.value) for x in c)
    assert consumed == text.size and lines == nlines == nrecs and ndef == 0 and ninvalid == 0
    moved = text.size + nrecs * 96
    d_a, d_b = malloc(moved), malloc(moved)

    def copy():
        assert hip.hipMemcpy(d_b, d_a, moved, 3) == 0 and hip.hipDeviceSynchronize() == 0
    rows = []
    for name, f, b in (("mgpu_sbs_decode_device (records and source lines)", decode, moved + nrecs * 8),
                       ("mgpu_sbs_decode_device (records only)", lambda: decode(False), moved),
                       ("(i) hipMemcpy device to device of the input-plus-output bytes", copy, moved)):
        ev_s, wall_s = timed(f)
        rows.append({"job": name, "lines": nlines, "input_bytes": int(text.size), "records": nrecs, "output_bytes": nrecs * 96, "us_per_call_events": round(ev_s * 1e6, 1),
                     "us_per_call_wall": round(wall_s * 1e6, 1), "lines_per_s": round(nlines / ev_s), "GB_per_s_in_plus_out": round(moved / ev_s / 1e9, 2),
                     "bytes_read_and_written": b, "reps": a.reps})
        print(json.dumps(rows[-1]), flush=True)
    print(json.dumps({"ratio": "decode (records only) time / copy time of the same input-plus-output bytes, by events",
                      "value": round(rows[1]["us_per_call_events"] / rows[2]["us_per_call_events"], 2),
                      "with_source_lines": round(rows[0]["us_per_call_events"] / rows[2]["us_per_call_events"], 2)}), flush=True)
    if a.harness:
        part = drawn * max(a.ref_lines // (1 << 14), 1)
        ref_lines = max(a.ref_lines // (1 << 14), 1) << 14
        with tempfile.TemporaryDirectory() as tmp:
            t = []
            for reps in (1, 1 + a.ref_reps):
                t0 = time.perf_counter()
                head, _, _ = su.run_ref_harness(a.harness, part, "sbs", tmp, reps=reps)
                t.append(time.perf_counter() - t0)
                assert int(head[1]) == int(head[2]) == ref_lines
        sec = (t[1] - t[0]) / a.ref_reps
        print(json.dumps({"job": "(ii) the reference's readAscii + decodeSbsLine, one CPU core (tests/host_stub/sbs_in_ref_harness.c)", "lines": ref_lines,
                          "seconds_per_pass": round(sec, 4), "lines_per_s": round(ref_lines / sec),
                          "decode_speedup_by_events": round((ref_lines / sec) and rows[0]["lines_per_s"] / (ref_lines / sec), 1)}))
    d.close()


if __name__ == "__main__":
    main()
