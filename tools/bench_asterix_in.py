"""Throughput of ASTERIX input — mgpu_asterix_decode_device (kernels/asterix_in.inc: k_ast_in_map, _compose, _walk, _expand, _mark,
_count, the scans, _decode) — on a drawn feed of about 10^6 well-formed CAT021 records (tests/asterix_in_util.py: feed), resident in
HBM, records and frame indices asked for.  Beside it, in the same process: (i) a plain device-to-device copy of the same number of
input-plus-output bytes, (ii) with --harness PATH the reference's readAsterix + decodeAsterixMessage on one core of this host over the
first --ref-records records (tests/host_stub/asterix_in_ref_harness.c: the difference between a run of 1 and a run of 1 + --ref-reps
passes over the stream, so that process start, the file and the dump of the records cancel)
(python tools/bench_asterix_in.py [--records N] [--harness PATH] | --build-harness DIR).  One JSON line per row.  Two clocks around
the synchronous C-ABI call: HIP events recorded on the null stream before and behind it, and the host's wall clock (launches, the
stream's synchronisation and the read-back of the totals are inside both); run it under `rocprofv3 --kernel-trace --stats` for the
split into the passes.  No threshold: the numbers go to profiles/asterix_in_bench.txt."""
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
import asterix_in_util as au  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--harness", default=None)
    ap.add_argument("--ref-records", type=int, default=1 << 17)
    ap.add_argument("--ref-reps", type=int, default=4)
    ap.add_argument("--build-harness", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.build_harness:                                              # where the full reference build is (make -C oracle full): no GPU needed
        os.makedirs(a.build_harness, exist_ok=True)
        print(au.build_ref_harness(a.build_harness))
        return
    drawn = b"".join(au.feed(1 << 14, seed=11))                      # 16 384 drawn records, repeated
    reps_in = max(a.records // (1 << 14), 1)
    nrecords = reps_in << 14
    data = np.frombuffer(drawn * reps_in, dtype=np.uint8)
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
    d_data, d_recs, d_frame = malloc(data.size), malloc(nrecords * 128), malloc(nrecords * 8)
    assert hip.hipMemcpy(d_data, data.ctypes.data, data.size, 1) == 0
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

    last = {}

    def decode(frames=True):
        args, c = au.args_for(binding, (d_data, data.size), au.SOURCE, au.NOWS[0], d_recs, d_frame if frames else None, nrecords)
        assert d.lib.mgpu_asterix_decode_device(d.ctx, C.byref(args)) == 0
        last.update({k: int(v.value) for k, v in c.items()})
    decode()
    assert last["consumed"] == data.size and last["nframes"] == nrecords == last["nrecs"] and last["stop"] == 0 and last["nundefined"] == 0, last
    moved = data.size + nrecords * 128
    d_a, d_b = malloc(moved), malloc(moved)

    def copy():
        assert hip.hipMemcpy(d_b, d_a, moved, 3) == 0 and hip.hipDeviceSynchronize() == 0
    rows = []
    for name, f, b in (("mgpu_asterix_decode_device (records and frame indices)", decode, moved + nrecords * 8),
                       ("mgpu_asterix_decode_device (records only)", lambda: decode(False), moved),
                       ("(i) hipMemcpy device to device of the input-plus-output bytes", copy, moved)):
        ev_s, wall_s = timed(f)
        rows.append({"job": name, "records": nrecords, "input_bytes": int(data.size), "tiles": int(data.size) // au.TILE + 1, "output_bytes": nrecords * 128,
                     "us_per_call_events": round(ev_s * 1e6, 1), "us_per_call_wall": round(wall_s * 1e6, 1), "records_per_s": round(nrecords / ev_s),
                     "GB_per_s_in_plus_out": round(moved / ev_s / 1e9, 2), "bytes_read_and_written": b, "reps": a.reps})
        print(json.dumps(rows[-1]), flush=True)
    print(json.dumps({"ratio": "decode (records only) time / copy time of the same input-plus-output bytes, by events",
                      "value": round(rows[1]["us_per_call_events"] / rows[2]["us_per_call_events"], 2),
                      "with_frame_indices": round(rows[0]["us_per_call_events"] / rows[2]["us_per_call_events"], 2)}), flush=True)
    if a.harness:
        part = drawn * max(a.ref_records // (1 << 14), 1)
        ref_records = max(a.ref_records // (1 << 14), 1) << 14
        with tempfile.TemporaryDirectory() as tmp:
            t = []
            for reps in (1, 1 + a.ref_reps):
                t0 = time.perf_counter()
                head, _, _ = au.run_ref_harness(a.harness, part, tmp, reps=reps)
                t.append(time.perf_counter() - t0)
                assert int(head[1]) == int(head[2]) == ref_records
        sec = (t[1] - t[0]) / a.ref_reps
        print(json.dumps({"job": "(ii) the reference's readAsterix + decodeAsterixMessage, one CPU core (tests/host_stub/asterix_in_ref_harness.c)",
                          "records": ref_records, "seconds_per_pass": round(sec, 4), "records_per_s": round(ref_records / sec),
                          "decode_speedup_by_events": round((ref_records / sec) and rows[0]["records_per_s"] / (ref_records / sec), 1)}))
    d.close()


if __name__ == "__main__":
    main()
