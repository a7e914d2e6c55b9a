"""Throughput of the outputs behind the list — mgpu_sbs_encode_ex_device and mgpu_raw_encode_ex_device (kernels/text.inc) and
mgpu_asterix_encode_ex_device (kernels/asterix.inc, the ASTERIX CAT021 target reports: same inputs, same run) — on records
resident in HBM, the record set of tools/bench_behind.py run through the field decode, the gate and the position decode first, with
the beast encoder (k_beast_size + k_beast_write) on the same records in the same process for scale
(python tools/bench_text.py [--messages N] [--harness PATH] | --build-harness DIR).  Prints one JSON line per output: microseconds per call, milliseconds per 1 M messages, lines and
bytes written per second, nanoseconds per output byte.  Wall clock around the C-ABI `_device` calls (launch + stream sync + the read-back
of the totals included); run it under `rocprofv3 --kernel-trace --stats` for the kernels' own durations.
--build-harness DIR builds the reference's own writers (tests/sbs_util.py: build_ref_harness; needs the full reference build of
`make -C oracle full`, no GPU) as DIR/text_ref_harness and exits — oracle/_ref is the place that travels with the tree;
--harness PATH then adds the lines per second of modesSendSBSOutput on
one core of this host over the first 262 144 records, process start and the case file's read included."""
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
import fields_util as fu  # noqa: E402
import sbs_util as su  # noqa: E402


def timed(f, reps, warmup=3):
    for _ in range(warmup):
        out = f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(min(t)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=8 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--harness", default=None)
    ap.add_argument("--build-harness", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.build_harness:                                              # where the full reference build is (make -C oracle full): no GPU needed
        os.makedirs(a.build_harness, exist_ok=True)
        print(su.build_ref_harness(a.build_harness))
        return
    frames, bits = fu.fuzz_frames(1 << 18, 7)
    m = np.zeros(len(frames), dtype=readsb_amd.MSG_DTYPE)
    m["msg"], m["msgbits"], m["msgtype"] = frames, bits, frames[:, 0] >> 3
    m["timestamp"] = np.arange(len(m)) * 977 + 0x1A00
    m["sysTimestamp"] = su.NOW_MS - 5000 + np.arange(len(m)) // 64
    m["sig_sumsq"], m["sig_len"] = np.random.default_rng(1).integers(1 << 20, 1 << 36, size=len(m)), 268
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
    d_in, d_f, d_v, d_p = malloc(n * 64), malloc(n * fb), malloc(n), malloc(n * pb)
    d_sbs, d_raw, d_beast = malloc(n * su.SBS_LINE_MAX), malloc(n * su.RAW_LINE_MAX), malloc(n * 44)
    asx_max = readsb_amd.binding.ASTERIX_RECORD_MAX
    d_asx = malloc(n * asx_max)
    d_def = malloc(n * 16)
    for k in range(reps_in):
        assert hip.hipMemcpy(d_in + k * m.nbytes, m.ctypes.data, m.nbytes, 1) == 0
    d.decode_fields_device(d_in, n, d_f)
    for _ in range(2):                                               # the same list twice: its aircraft are known from the second call on
        d.track_gate_device(d_in, d_f, n, d_v)
        d.cpr_track_device(d_in, d_f, n, d_p, ref=(52.0, 4.5))
    jobs = (
        ("mgpu_sbs_encode_ex_device (gate verdicts, positions)",
         lambda: d.sbs_encode_device(d_in, d_f, n, su.NOW_MS, d_sbs, n * su.SBS_LINE_MAX, d_positions_ptr=d_p, d_verdict_ptr=d_v, d_deferred_ptr=d_def,
                                     deferred_cap=n)),
        ("mgpu_sbs_encode_ex_device (every message, positions)",
         lambda: d.sbs_encode_device(d_in, d_f, n, su.NOW_MS, d_sbs, n * su.SBS_LINE_MAX, d_positions_ptr=d_p)),
        ("mgpu_asterix_encode_ex_device (gate verdicts, positions)",
         lambda: d.asterix_encode_device(d_in, d_f, n, su.NOW_MS, d_asx, n * asx_max, d_positions_ptr=d_p, d_verdict_ptr=d_v, d_deferred_ptr=d_def,
                                         deferred_cap=n)),
        ("mgpu_asterix_encode_ex_device (every message, positions)",
         lambda: d.asterix_encode_device(d_in, d_f, n, su.NOW_MS, d_asx, n * asx_max, d_positions_ptr=d_p)),
        ("mgpu_raw_encode_ex_device (mlat, every message)", lambda: d.raw_encode_device(d_in, n, d_raw, n * su.RAW_LINE_MAX, mlat=True)),
        ("mgpu_beast_encode_device (k_beast_size + k_beast_write)", lambda: (d.beast_encode_device(d_in, n, d_beast, n * 44),)),
    )
    for name, f in jobs:
        med, best, out = timed(f, a.reps)
        nbytes = int(out[0])
        print(json.dumps({"output": name, "messages": n, "bytes": nbytes, "deferred": int(out[1]) if len(out) > 1 else 0,
                          "skipped": int(out[2]) if len(out) > 2 else 0, "us_per_call": round(med * 1e6, 1), "us_per_call_best": round(best * 1e6, 1),
                          "ms_per_1M_messages": round(med * 1e3 * 1e6 / n, 4),
                          "messages_per_s": round(n / med), "bytes_per_s": round(nbytes / med), "ns_per_output_byte": round(med * 1e9 / max(nbytes, 1), 4),
                          "reps": a.reps, "timing": "median wall clock around the C-ABI call, launch + sync included"}), flush=True)
    if a.harness:
        k = len(m)
        c = su.empty_cases(k)
        c["msgs"] = m
        c["fields"] = np.empty(k, dtype=readsb_amd.FIELDS_DTYPE)
        c["positions"] = np.empty(k, dtype=readsb_amd.POSITION_DTYPE)
        assert hip.hipMemcpy(c["fields"].ctypes.data, d_f, c["fields"].nbytes, 2) == 0 and hip.hipMemcpy(c["positions"].ctypes.data, d_p, c["positions"].nbytes, 2) == 0
        c = su.in_domain(c)
        with tempfile.TemporaryDirectory() as tmp:
            t0 = time.perf_counter()
            stream, lens = su.run_ref_harness(a.harness, "sbs", c, workdir=tmp)
            t = time.perf_counter() - t0
        lines = int((lens > 0).sum())
        print(json.dumps({"output": "the reference's modesSendSBSOutput, one CPU core (tests/host_stub/text_ref_harness.c)", "records": len(lens), "lines": lines,
                          "bytes": len(stream), "seconds": round(t, 4), "lines_per_s": round(lines / t), "bytes_per_s": round(len(stream) / t)}))
    d.close()


if __name__ == "__main__":
    main()
