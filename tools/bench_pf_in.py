"""Throughput of Planefinder input — mgpu_pf_decode_device (kernels/pf_in.inc: k_pf_in_events, _states, _count, the scans,
k_pf_in_classify, then over the candidates raw_in.inc's k_raw_in_first, _new, _mark, _verdict, _write) — on the record list
tools/bench_beast_in.py draws (the message list of the synthetic 200-aircraft minute, tools/synth_iq.c, demodulated on this context) as
Planefinder frames (tests/pf_in_util.py's builder: stuffed, seconds and nanoseconds from the record's timestamp), one frame in twenty
carrying another packet id, repeated to about 10^6 frames, resident in HBM; messages, handler calls, signal doubles, class and offset
per handler call asked for.
Two states of the filter: EMPTY before the call (mgpu_reset before each, outside the clocks) and WARM (every address known).  Beside
it, in the same process: (i) a plain device-to-device copy of the same number of input-plus-output bytes, (ii) with --harness PATH the
reference's readPlanefinder + decodePfMessage + decodeModesMessage on one core of this host over the first --ref-frames frames
(tests/host_stub/pf_in_ref_harness.c: the difference between a run of 1 and a run of 1 + --ref-reps passes, so that process start, the
tables and the dump cancel)
(python tools/bench_pf_in.py [--frames N] [--seconds S] [--harness PATH] | --build-harness DIR).  One JSON line per row.  Two clocks
around the synchronous C-ABI call: HIP events recorded on the null stream before and behind it, and the host's wall clock (launches,
the two synchronisations, the members' upload and scatter and the read-back of the totals are inside both); run it under
`rocprofv3 --kernel-trace --stats` for the split into the passes.  No threshold: the numbers go to profiles/pf_in_bench.txt."""
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
import pf_in_util as pu  # noqa: E402
import helpers  # noqa: E402


def frames_of(msgs):
    """The records as Planefinder frames; every twentieth under packet id 0x41."""
    out = []
    for k, m in enumerate(msgs):
        nb = 2 if m["msgtype"] == 77 else 14 if m["msgbits"] == 112 else 7
        ts = int(m["timestamp"]) & 0xFFFFFFFFFFFF
        sig = min(255, int(round((float(m["sig_sumsq"]) / max(int(m["sig_len"]), 1)) ** 0.5 / 257.0)))
        out.append(pu.frame(bytes(m["msg"][:nb]), secs=0x65000000 + ts // 12000000, nanos=(ts % 12000000) * 83, sig=sig, pid=0x41 if k % 20 == 19 else pu.PID))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--harness", default=None)
    ap.add_argument("--ref-frames", type=int, default=1 << 17)
    ap.add_argument("--ref-reps", type=int, default=4)
    ap.add_argument("--build-harness", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.build_harness:                                              # where the full reference build is (make -C oracle full): no GPU needed
        os.makedirs(a.build_harness, exist_ok=True)
        print(pu.build_ref_harness(a.build_harness))
        return
    d = readsb_amd.Demodulator(max_samples=1 << 22, filter_clock=binding.FILTER_CLOCK_EXTERNAL)
    iq = helpers.synth(seconds=a.seconds, seed=4242, rate=2000.0)
    msgs = np.ascontiguousarray(d.demodulate_capture(iq)[0])
    del iq
    unit = b"".join(frames_of(msgs))
    reps_in = max(a.frames // len(msgs), 1)
    room = reps_in * len(msgs)
    data = np.frombuffer(unit * reps_in, dtype=np.uint8)
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
    d_data, d_msgs, d_sig, d_of, d_cls, d_off = malloc(data.size), malloc(room * 64), malloc(room * 8), malloc(room * 8), malloc(room), malloc(room * 8)
    assert hip.hipMemcpy(d_data, data.ctypes.data, data.size, 1) == 0
    outs, cn = pu.new_outs(), binding.PfInCounters()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0

    def by_events(f, before=None):
        """-> (ms by the two events, s by the wall clock) of one synchronous call"""
        if before:
            before()
        assert hip.hipEventRecord(ev[0], None) == 0
        t0 = time.perf_counter()
        f()
        wall = time.perf_counter() - t0
        assert hip.hipEventRecord(ev[1], None) == 0 and hip.hipEventSynchronize(ev[1]) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        return float(ms.value), wall

    def timed(f, before=None):
        for _ in range(3):
            if before:
                before()
            f()
        t = [by_events(f, before) for _ in range(a.reps)]
        return float(np.median([x[0] for x in t])) * 1e-3, float(np.median([x[1] for x in t]))

    def decode(extras=True):
        p = dict(msgs=d_msgs, signal=d_sig if extras else None, frame_of=d_of if extras else None, cls=d_cls if extras else None, off=d_off if extras else None)
        args = pu.pf_args(binding, d_data, data.size, None, outs, cn, now_ms=pu.NOW_MS, msgs_cap=room, frames_cap=room if extras else 0, pointers=p)
        assert d.lib.mgpu_pf_decode_device(d.ctx, C.byref(args)) == 0
    d.reset()
    decode()
    cold = binding.pf_in_counters_dict(cn)
    nframes, cold_msgs = int(outs[1].value), int(outs[2].value)
    # (a message with DLE ETX in it ends its frame early, as in the reference: the frames framed can differ from the frames built by a few)
    assert int(outs[0].value) == data.size and cold["past_end"] == 0 and 0 < nframes <= room, (int(outs[0].value), data.size, cold, nframes, room)
    decode()
    warm, warm_msgs = binding.pf_in_counters_dict(cn), int(outs[2].value)
    print(json.dumps({"feed": "the synthetic minute's messages as Planefinder frames, one in twenty of another packet id", "unit_messages": len(msgs), "unit_bytes": len(unit),
                      "filter_empty": cold, "filter_warm": warm, "messages_empty": cold_msgs, "messages_warm": warm_msgs}), flush=True)
    # the bytes a call reads and writes: the stream and a record per message; with every output also the signal and the handler call
    # per message and a class and an offset per handler call
    moved = {False: data.size + warm_msgs * 64, True: data.size + warm_msgs * (64 + 8 + 8) + nframes * (1 + 8)}
    d_a, d_b = malloc(moved[True]), malloc(moved[True])

    def copy(extras=True):
        assert hip.hipMemcpy(d_b, d_a, moved[extras], 3) == 0 and hip.hipDeviceSynchronize() == 0

    def copy_in():
        assert hip.hipMemcpy(d_b, d_a, data.size, 3) == 0 and hip.hipDeviceSynchronize() == 0
    rows = []
    for name, f, before, nbytes in (("mgpu_pf_decode_device, filter warm (messages, handler calls, signal, class and offset per call)", decode, None, moved[True]),
                                    ("mgpu_pf_decode_device, filter warm (messages only)", lambda: decode(False), None, moved[False]),
                                    ("mgpu_pf_decode_device, filter empty before the call (everything)", decode, d.reset, moved[True]),
                                    ("(i) hipMemcpy device to device of the input-plus-output bytes, every output", copy, None, moved[True]),
                                    ("(i) hipMemcpy device to device of the input-plus-output bytes, messages only", lambda: copy(False), None, moved[False]),
                                    ("(i) hipMemcpy device to device of the input bytes alone", copy_in, None, int(data.size))):
        ev_s, wall_s = timed(f, before)
        rows.append({"job": name, "frames": nframes + cold["nskipped"], "handler_calls": nframes, "input_bytes": int(data.size), "messages_warm": warm_msgs,
                     "output_bytes": nbytes - int(data.size), "us_per_call_events": round(ev_s * 1e6, 1), "us_per_call_wall": round(wall_s * 1e6, 1),
                     "frames_per_s": round((nframes + cold["nskipped"]) / ev_s), "input_GB_per_s": round(data.size / ev_s / 1e9, 2), "GB_per_s_in_plus_out": round(nbytes / ev_s / 1e9, 2),
                     "reps": a.reps})
        print(json.dumps(rows[-1]), flush=True)
    print(json.dumps({"ratio": "decode time / copy time of the same input-plus-output bytes, by events",
                      "with_everything": round(rows[0]["us_per_call_events"] / rows[3]["us_per_call_events"], 2),
                      "messages_only": round(rows[1]["us_per_call_events"] / rows[4]["us_per_call_events"], 2),
                      "filter_empty": round(rows[2]["us_per_call_events"] / rows[3]["us_per_call_events"], 2),
                      "ns_per_input_byte_warm": round(rows[0]["us_per_call_events"] * 1e3 / data.size, 4)}), flush=True)
    if a.harness:
        k = max(a.ref_frames // len(msgs), 1)
        part, ref_frames = unit * k, k * len(msgs)
        with tempfile.TemporaryDirectory() as tmp:
            t = []
            for reps in (1, 1 + a.ref_reps):
                t0 = time.perf_counter()
                res = pu.run_ref_harness(a.harness, [part], (1, 1, 0), tmp, reps=reps)[0]
                t.append(time.perf_counter() - t0)
                assert int(res["head"][1]) <= ref_frames
        sec = (t[1] - t[0]) / a.ref_reps
        print(json.dumps({"job": "(ii) the reference's readPlanefinder + decodePfMessage + decodeModesMessage, filter empty before the pass, one CPU core "
                                 "(tests/host_stub/pf_in_ref_harness.c)", "frames": ref_frames, "seconds_per_pass": round(sec, 4), "frames_per_s": round(ref_frames / sec),
                          "decode_speedup_by_events": round(rows[2]["frames_per_s"] / (ref_frames / sec), 1)}))
    d.close()


if __name__ == "__main__":
    main()
