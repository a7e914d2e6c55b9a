"""Throughput of the stages behind the message list — k_decode_fields, k_beast_size/k_beast_write, the tracking gate
(mgpu_track_gate_device), the position decode (mgpu_cpr_track_device), the aggregator's time merge (mgpu_merge_by_time_device, the
list as 4 segments, with the digit passes it took) and the encoder with receiver ids that change on every message
(mgpu_beast_encode_ex_device) — on records resident in HBM
(python tools/bench_behind.py [--messages N]).  Prints one JSON line per stage: messages/s, algorithmic
GB/s (64 + 176 B per message for the field decode; 64 B in + the frame bytes out for the encoder; for the gate and the
position decode the records read and written once, 64 + 176 + 1 and 64 + 176 + 32 B, their sort's traffic not counted) against the
8 TB/s HBM peak.  Wall clock around the C-ABI `_device` calls (launch + stream sync included), so run it under
`rocprofv3 --kernel-trace --stats` for the kernels' own durations (profiles/r01_behind_*)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import readsb_amd  # noqa: E402
import fields_util as fu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=8 << 20)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    frames, bits = fu.fuzz_frames(1 << 18, 7)
    m = np.zeros(len(frames), dtype=readsb_amd.MSG_DTYPE)
    m["msg"], m["msgbits"], m["msgtype"] = frames, bits, frames[:, 0] >> 3
    m["timestamp"] = np.arange(len(m)) * 977 + 0x1A00
    m["sig_sumsq"], m["sig_len"] = np.random.default_rng(1).integers(1 << 20, 1 << 36, size=len(m)), 268
    aa = (frames[:, 1].astype(np.uint32) << 16) | (frames[:, 2].astype(np.uint32) << 8) | frames[:, 3]
    m["addr"] = aa
    reps_in = a.messages // len(m)
    n = reps_in * len(m)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    d = readsb_amd.Demodulator(max_samples=1 << 20)
    d_in, d_f, d_b, d_v, d_p = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_v), n) == 0 and hip.hipMalloc(C.byref(d_p), n * readsb_amd.binding.POSITION_DTYPE.itemsize) == 0
    assert hip.hipMalloc(C.byref(d_in), n * 64) == 0 and hip.hipMalloc(C.byref(d_f), n * readsb_amd.FIELDS_DTYPE.itemsize) == 0 and hip.hipMalloc(C.byref(d_b), n * 44) == 0
    for k in range(reps_in):
        assert hip.hipMemcpy(C.c_void_p(d_in.value + k * m.nbytes), m.ctypes.data, m.nbytes, 1) == 0
    for _ in range(3):
        d.decode_fields_device(d_in.value, n, d_f.value)
        nbytes = d.beast_encode_device(d_in.value, n, d_b.value, n * 44)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        d.decode_fields_device(d_in.value, n, d_f.value)
    t_f = (time.perf_counter() - t0) / a.reps
    t0 = time.perf_counter()
    for _ in range(a.reps):
        d.beast_encode_device(d_in.value, n, d_b.value, n * 44)
    t_b = (time.perf_counter() - t0) / a.reps
    # the stages with a table: the same list every time (its aircraft are known from the second call on), the receiver's location set
    ref = (52.0, 4.5)
    for _ in range(2):
        d.track_gate_device(d_in.value, d_f.value, n, d_v.value)
        d.cpr_track_device(d_in.value, d_f.value, n, d_p.value, ref=ref)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        d.track_gate_device(d_in.value, d_f.value, n, d_v.value)
    t_g = (time.perf_counter() - t0) / a.reps
    t0 = time.perf_counter()
    for _ in range(a.reps):
        d.cpr_track_device(d_in.value, d_f.value, n, d_p.value, ref=ref)
    t_c = (time.perf_counter() - t0) / a.reps
    # the aggregator's output: the list as 4 receivers' segments merged by time, then encoded with ids that change on every message
    d_m, d_ids, d_bx = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_m), n * 64) == 0 and hip.hipMalloc(C.byref(d_ids), n * 8) == 0 and hip.hipMalloc(C.byref(d_bx), n * 62 + 64) == 0
    quarter = n // 4
    segs, counts = [d_in.value + k * quarter * 64 for k in range(4)], [quarter, quarter, quarter, n - 3 * quarter]
    for _ in range(2):
        d.merge_by_time_device(segs, counts, d_m.value, ids=[1, 2, 3, 4], d_ids_ptr=d_ids.value)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        d.merge_by_time_device(segs, counts, d_m.value, ids=[1, 2, 3, 4], d_ids_ptr=d_ids.value)
    t_m = (time.perf_counter() - t0) / a.reps
    passes = d.merge_last_passes()
    alt = (np.arange(1 << 20, dtype=np.uint64) & np.uint64(1)) + np.uint64(0x1A00000000000021)
    for k in range(0, n, len(alt)):
        assert hip.hipMemcpy(C.c_void_p(d_ids.value + k * 8), alt.ctypes.data, min(len(alt), n - k) * 8, 1) == 0
    for _ in range(2):
        nbytes_x = d.beast_encode_ex_device(d_in.value, n, d_bx.value, n * 62 + 64, d_ids_ptr=d_ids.value)[0]
    t0 = time.perf_counter()
    for _ in range(a.reps):
        d.beast_encode_ex_device(d_in.value, n, d_bx.value, n * 62 + 64, d_ids_ptr=d_ids.value)
    t_x = (time.perf_counter() - t0) / a.reps
    # the plain encoder once more, behind everything else: run to run spread of the figure above
    t0 = time.perf_counter()
    for _ in range(a.reps):
        d.beast_encode_device(d_in.value, n, d_b.value, n * 44)
    t_b2 = (time.perf_counter() - t0) / a.reps
    pos = np.empty(len(m), dtype=readsb_amd.binding.POSITION_DTYPE)
    assert hip.hipMemcpy(pos.ctypes.data, d_p, pos.nbytes, 2) == 0
    print(json.dumps({"list": "fuzzed frames", "position_messages_share": round(float(((pos["global_result"] != 0) | (pos["method"] != 0)).mean()), 4),
                      "methods_in_first_block": {str(k): int((pos["method"] == k).sum()) for k in range(5)}}))
    fb = readsb_amd.FIELDS_DTYPE.itemsize
    for name, t, algo in (("k_decode_fields", t_f, n * (64 + fb)), ("k_beast_size+k_beast_write", t_b, n * 64 + nbytes),
                          ("mgpu_track_gate_device", t_g, n * (64 + fb + 1)), ("mgpu_cpr_track_device", t_c, n * (64 + fb + 32)),
                          (f"mgpu_merge_by_time_device (4 segments, {passes} digit passes)", t_m, n * (64 + 64 + 8)),
                          ("mgpu_beast_encode_ex_device (ids change every message)", t_x, n * (64 + 8) + nbytes_x),
                          ("k_beast_size+k_beast_write (again, last)", t_b2, n * 64 + nbytes)):
        print(json.dumps({"kernel": name, "messages": n, "ms": round(t * 1e3, 4), "messages_per_s": round(n / t),
                          "algorithmic_GBps": round(algo / t / 1e9, 1), "frac_of_hbm_peak": round(algo / t / 8e12, 4),
                          "timing": "wall clock around the C-ABI call, launch + sync included"}))
    d.close()


if __name__ == "__main__":
    main()
