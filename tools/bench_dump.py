"""Throughput of the decoded-message dump — mgpu_dump_encode_ex_device (kernels/dump.inc: k_dump_size, the scans, k_dump_write) —
on about 10^6 records resident in HBM, run through the field decode and the position decode first.  --mix aircraft (the default):
the message list of a synthetic 60 s capture of 200 aircraft (tools/synth_iq.c, the capture of the gate's golden
uc8_fix_200ac_60s), demodulated here and repeated; --mix fuzz: the record set of tools/bench_text.py, uniformly fuzzed frames of every
format — longer dumps, every lane of a wave in another format.  Beside it, in the same process: (i) a plain device-to-device copy of the same
number of output bytes, (ii) the SBS encoder on the same list, (iii) with --harness PATH the reference's displayModesMessage on one
core of this host over the first 262 144 records, its stdout to /dev/null, process start and the case file's read included
(python tools/bench_dump.py [--mix aircraft|fuzz] [--messages N] [--harness PATH] | --build-harness DIR).  One JSON line per row.  Wall clock around the
C-ABI `_device` call (launches + stream sync + the read-back of the totals included); run it under `rocprofv3 --kernel-trace --stats`
for the split into the size pass, the scans and the write pass."""
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
import dump_util as du  # noqa: E402
import fields_util as fu  # noqa: E402
import sbs_util as su  # noqa: E402
from bench_text import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=1 << 20)
    ap.add_argument("--mix", choices=("aircraft", "fuzz"), default="aircraft")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--harness", default=None)
    ap.add_argument("--build-harness", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.build_harness:                                              # where the full reference build is (make -C oracle full): no GPU needed
        os.makedirs(a.build_harness, exist_ok=True)
        print(du.build_ref_harness(a.build_harness))
        return
    if a.mix == "aircraft":
        import helpers
        iq = helpers.synth(seconds=60.0, seed=4242, rate=2000.0)
        dm = readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=256 * 131072)
        m = np.ascontiguousarray(dm.demodulate_capture(iq)[0])
        dm.close()
        del iq
    else:
        frames, bits = fu.fuzz_frames(1 << 18, 7)
        m = np.zeros(len(frames), dtype=readsb_amd.MSG_DTYPE)
        m["msg"], m["raw"], m["msgbits"], m["msgtype"] = frames, frames, bits, frames[:, 0] >> 3
        m["timestamp"] = np.arange(len(m)) * 977 + 0x1A00
        m["sysTimestamp"] = su.NOW_MS - 5000 + np.arange(len(m)) // 64
        m["sig_sumsq"], m["sig_len"] = np.random.default_rng(1).integers(1 << 20, 1 << 36, size=len(m)), 268
        m["score"] = 1800
        m["addr"] = (frames[:, 1].astype(np.uint32) << 16) | (frames[:, 2].astype(np.uint32) << 8) | frames[:, 3]
    reps_in = max(a.messages // len(m), 1)
    n = reps_in * len(m)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def malloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), nbytes) == 0
        return p.value
    fb, pb = readsb_amd.FIELDS_DTYPE.itemsize, readsb_amd.POSITION_DTYPE.itemsize
    d = readsb_amd.Demodulator(max_samples=1 << 20)
    d_in, d_f, d_p, d_def = malloc(n * 64), malloc(n * fb), malloc(n * pb), malloc(4096 * 16)
    for k in range(reps_in):
        assert hip.hipMemcpy(d_in + k * m.nbytes, m.ctypes.data, m.nbytes, 1) == 0
    d.decode_fields_device(d_in, n, d_f)
    for _ in range(2):
        d.cpr_track_device(d_in, d_f, n, d_p, ref=(52.0, 4.5))
    cap = n * 1024                                                   # far above the mix's few hundred bytes a message
    d_out = malloc(cap)
    d_sbs = malloc(n * su.SBS_LINE_MAX)
    rows = []

    def dump(flags=0):
        return d.dump_encode_device(d_in, d_f, n, d_out, cap, flags=flags, d_positions_ptr=d_p, d_deferred_ptr=d_def, deferred_cap=4096)
    nbytes = dump()[0]
    d_copy = malloc(nbytes)

    def copy():
        assert hip.hipMemcpy(d_copy, d_out, nbytes, 3) == 0 and hip.hipDeviceSynchronize() == 0
        return (nbytes,)
    jobs = (
        ("mgpu_dump_encode_ex_device (every message, positions)", dump),
        ("mgpu_dump_encode_ex_device (MGPU_DUMP_RAW | MGPU_DUMP_MLAT)", lambda: dump(du.RAW | du.MLAT)),
        ("(i) hipMemcpy device to device of the dump's bytes", copy),
        ("(ii) mgpu_sbs_encode_ex_device (every message, positions)",
         lambda: d.sbs_encode_device(d_in, d_f, n, su.NOW_MS, d_sbs, n * su.SBS_LINE_MAX, d_positions_ptr=d_p)),
    )
    for name, f in jobs:
        med, best, out = timed(f, a.reps)
        nb = int(out[0])
        rows.append({"output": name, "mix": a.mix, "messages": n, "bytes": nb, "deferred": int(out[1]) if len(out) > 1 else 0, "skipped": int(out[2]) if len(out) > 2 else 0,
                     "us_per_call": round(med * 1e6, 1), "us_per_call_best": round(best * 1e6, 1), "messages_per_s": round(n / med),
                     "GB_per_s": round(nb / med / 1e9, 3), "ns_per_output_byte": round(med * 1e9 / max(nb, 1), 4), "reps": a.reps,
                     "timing": "median wall clock around the call, launch + sync included"})
        print(json.dumps(rows[-1]), flush=True)
    print(json.dumps({"ratio": "dump encode time / copy time of the same bytes", "value": round(rows[0]["us_per_call"] / rows[2]["us_per_call"], 2),
                      "sbs_for_scale": "sbs encode time / copy-rate time of ITS bytes",
                      "sbs_value": round(rows[3]["us_per_call"] / (rows[3]["bytes"] / (rows[2]["bytes"] / rows[2]["us_per_call"])), 2)}), flush=True)
    if a.harness:
        k = min(len(m), 1 << 18)
        m = m[:k]
        c = du.empty_cases(k)
        c["msgs"] = m
        c["fields"] = np.empty(k, dtype=readsb_amd.FIELDS_DTYPE)
        c["positions"] = np.empty(k, dtype=readsb_amd.POSITION_DTYPE)
        assert hip.hipMemcpy(c["fields"].ctypes.data, d_f, c["fields"].nbytes, 2) == 0 and hip.hipMemcpy(c["positions"].ctypes.data, d_p, c["positions"].nbytes, 2) == 0
        rec = du.case_records(c, 0)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "cases.bin")
            rec.tofile(path)
            t0 = time.perf_counter()
            subprocess.run([a.harness, path, "/dev/null", os.path.join(tmp, "lens.bin"), "0", "0", "0"], check=True)
            t = time.perf_counter() - t0
        dumps = int(rec["run"].sum())
        print(json.dumps({"output": "(iii) the reference's displayModesMessage, one CPU core, stdout to /dev/null (tests/host_stub/dump_ref_harness.c)",
                          "records": k, "dumps": dumps, "seconds": round(t, 4), "messages_per_s": round(dumps / t)}))
    d.close()


if __name__ == "__main__":
    main()
