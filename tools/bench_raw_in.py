"""Throughput of raw input — mgpu_raw_decode_device (kernels/raw_in.inc: k_sbs_in_index, the scans, k_raw_in_size, k_raw_in_classify,
then over the candidates k_raw_in_first, _new, _mark, _verdict, _write) — on a drawn feed of about 10^6 AVR lines over a pool of 4 096
aircraft, resident in HBM, messages, source lines, signal doubles and the class per line asked for.  The mix, per 100 lines: 40 DF17
(2 of them with one damaged bit), 15 DF11 (1 with IID != 0), 15 DF4/5, 15 DF20/21, 10 DF0/16, 5 of aircraft nobody announced (rejected
unknown); half as '*' lines, a quarter each as '@' and '<' lines; 16 384 drawn lines repeated.
Two states of the filter: EMPTY before the call (mgpu_reset before each, outside the clocks: every aircraft's first clean DF17 / DF11
is a new add and the table grows from 256 buckets) and WARM (the pool known: no new adds).  Beside it, in the same process: (i) a plain
device-to-device copy of the same number of input-plus-output bytes, (ii) with --harness PATH the reference's readAscii +
decodeHexMessage + decodeModesMessage on one core of this host over the first --ref-lines lines (tests/host_stub/raw_in_ref_harness.c:
the difference between a run of 1 and a run of 1 + --ref-reps passes, so that process start, the tables and the dump cancel)
(python tools/bench_raw_in.py [--lines N] [--harness PATH] | --build-harness DIR).  One JSON line per row.  Two clocks around the
synchronous C-ABI call: HIP events recorded on the null stream before and behind it, and the host's wall clock (launches, the two
synchronisations, the members' upload and scatter and the read-back of the totals are inside both); run it under
`rocprofv3 --kernel-trace --stats` for the split into the passes.  No threshold: the numbers go to profiles/raw_in_bench.txt."""
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
import frames_util as fr  # noqa: E402
import raw_in_util as ru  # noqa: E402

DRAWN = 1 << 14


def feed(n=DRAWN, seed=11, aircraft=4096):
    """n drawn lines -> [bytes]"""
    rng = np.random.default_rng(seed)
    pool = (0x400000 + rng.choice(0x3FFFFF, aircraft, replace=False)).astype(np.uint32)
    addr = pool[rng.integers(0, aircraft, n)]
    kind = rng.integers(0, 100, n)
    frames = np.zeros((n, 14), dtype=np.uint8)
    es = kind < 40
    frames[es] = fr._es_frames(int(es.sum()), 0, addr[es], np.zeros(int(es.sum()), dtype=bool))
    damaged = np.nonzero(kind < 2)[0]
    frames[damaged] = fr.flip(frames[damaged], rng.integers(40, 112, len(damaged)))
    s11 = (kind >= 40) & (kind < 55)
    frames[s11] = fr.df11_frames(addr[s11], np.where(kind[s11] == 40, 5, 0))
    for lo, hi, dfs in ((55, 70, (4, 5)), (70, 85, (20, 21)), (85, 95, (0, 16))):
        sel = (kind >= lo) & (kind < hi)
        frames[sel] = fr.ap_frames(np.array(dfs)[rng.integers(0, 2, int(sel.sum()))], addr[sel], payload_seed=lo)
    stray = kind >= 95
    frames[stray] = fr.ap_frames(4, (0x100000 + rng.integers(0, 0xFFFF, int(stray.sum()))).astype(np.uint32), payload_seed=95)
    ts, sig, lead = rng.integers(0, 1 << 48, n), rng.integers(0, 256, n), rng.integers(0, 4, n)
    return [ru.avr(frames[k], (b"*", b"*", b"@", b"<")[lead[k]], ts=b"%012X" % int(ts[k]), sig=b"%02X" % int(sig[k])) for k in range(n)]


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
        print(ru.build_ref_harness(a.build_harness))
        return
    drawn = b"".join(feed())
    reps_in = max(a.lines // DRAWN, 1)
    nlines = reps_in * DRAWN
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
    d = readsb_amd.Demodulator(max_samples=1 << 20, filter_clock=binding.FILTER_CLOCK_EXTERNAL)
    d_text, d_msgs, d_line, d_sig, d_cls = malloc(text.size), malloc(nlines * 64), malloc(nlines * 8), malloc(nlines * 8), malloc(nlines)
    assert hip.hipMemcpy(d_text, text.ctypes.data, text.size, 1) == 0
    c = [C.c_uint64(0) for _ in range(3)]
    cn = binding.RawInCounters()
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
        args = binding.RawInArgs(C.sizeof(binding.RawInArgs), 0, d_text, text.size, ru.NOW_MS, d_msgs, d_line if extras else None, d_sig if extras else None, nlines,
                                 d_cls if extras else None, nlines if extras else 0, *[C.pointer(x) for x in c], C.pointer(cn), 0)
        assert d.lib.mgpu_raw_decode_device(d.ctx, C.byref(args)) == 0
    d.reset()
    decode()
    consumed, lines, nmsgs = (int(x.value) for x in c)
    cold = [int(cn.remote_received_modes), int(cn.remote_rejected_unknown_icao), int(cn.remote_rejected_bad), *[int(x) for x in cn.remote_accepted]]
    assert consumed == text.size and lines == nlines == cold[0]
    decode()
    warm = [int(cn.remote_received_modes), int(cn.remote_rejected_unknown_icao), int(cn.remote_rejected_bad), *[int(x) for x in cn.remote_accepted]]
    warm_msgs = int(c[2].value)
    print(json.dumps({"feed": "received, rejected unknown, rejected bad, accepted[0..2]", "filter_empty": cold, "filter_warm": warm, "messages_empty": nmsgs,
                      "messages_warm": warm_msgs}), flush=True)
    moved = text.size + warm_msgs * 64
    d_a, d_b = malloc(moved), malloc(moved)

    def copy():
        assert hip.hipMemcpy(d_b, d_a, moved, 3) == 0 and hip.hipDeviceSynchronize() == 0
    rows = []
    for name, f, before in (("mgpu_raw_decode_device, filter warm (messages, source lines, signal, class per line)", decode, None),
                            ("mgpu_raw_decode_device, filter warm (messages only)", lambda: decode(False), None),
                            ("mgpu_raw_decode_device, filter empty before the call (messages, source lines, signal, class per line)", decode, d.reset),
                            ("(i) hipMemcpy device to device of the input-plus-output bytes", copy, None)):
        ev_s, wall_s = timed(f, before)
        rows.append({"job": name, "lines": nlines, "input_bytes": int(text.size), "messages_warm": warm_msgs, "output_bytes": warm_msgs * 64,
                     "us_per_call_events": round(ev_s * 1e6, 1), "us_per_call_wall": round(wall_s * 1e6, 1), "lines_per_s": round(nlines / ev_s),
                     "GB_per_s_in_plus_out": round(moved / ev_s / 1e9, 2), "reps": a.reps})
        print(json.dumps(rows[-1]), flush=True)
    print(json.dumps({"ratio": "decode (messages only, filter warm) time / copy time of the same input-plus-output bytes, by events",
                      "value": round(rows[1]["us_per_call_events"] / rows[3]["us_per_call_events"], 2),
                      "with_everything": round(rows[0]["us_per_call_events"] / rows[3]["us_per_call_events"], 2),
                      "filter_empty": round(rows[2]["us_per_call_events"] / rows[3]["us_per_call_events"], 2)}), flush=True)
    if a.harness:
        k = max(a.ref_lines // DRAWN, 1)
        part, ref_lines = drawn * k, k * DRAWN
        with tempfile.TemporaryDirectory() as tmp:
            t = []
            for reps in (1, 1 + a.ref_reps):
                t0 = time.perf_counter()
                res = ru.run_ref_harness(a.harness, [part], (1, 1, 0), tmp, reps=reps)[0]
                t.append(time.perf_counter() - t0)
                assert int(res["head"][1]) == ref_lines
        sec = (t[1] - t[0]) / a.ref_reps
        print(json.dumps({"job": "(ii) the reference's readAscii + decodeHexMessage + decodeModesMessage, filter empty before the pass, one CPU core "
                                 "(tests/host_stub/raw_in_ref_harness.c)", "lines": ref_lines, "seconds_per_pass": round(sec, 4), "lines_per_s": round(ref_lines / sec),
                          "decode_speedup_by_events": round(rows[2]["lines_per_s"] / (ref_lines / sec), 1)}))
    d.close()


if __name__ == "__main__":
    main()
