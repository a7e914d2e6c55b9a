"""Test infrastructure: builds, the synthetic IQ generator, and the two CPU checkers under
oracle/ (our plain-C restatement, and oracle/_ref = the reference's own C files)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
TOOLS_DIR = os.path.join(ROOT, "tools")
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
REF_BIN = os.path.join(ORACLE_DIR, "_ref", "ref_demod")
STARTUP_MS = 1000000  # ORACLE_STARTUP_MS

FMT_NAMES = {0: "UC8", 1: "SC16", 2: "SC16Q11"}
FMT_BYTES = {0: 2, 1: 4, 2: 4}

# struct oracle_msg (72 bytes), struct oracle_stats
ORACLE_MSG = np.dtype([
    ("timestamp", "<i8"), ("sys_rel_ms", "<i8"), ("score", "<i4"), ("correctedbits", "<i4"), ("msgbits", "<i4"),
    ("msgtype", "<i4"), ("addr", "<u4"), ("msg", "u1", 14), ("raw", "u1", 14), ("signalLevel", "<f8"),
])
assert ORACLE_MSG.itemsize == 72
ORACLE_STATS = np.dtype([
    ("demod_preambles", "<u8"), ("demod_rejected_bad", "<u8"), ("demod_rejected_unknown_icao", "<u8"),
    ("demod_accepted", "<u8", 3), ("demod_preamblePhase", "<u8", 5), ("demod_bestPhase", "<u8", 5),
    ("strong_signal_count", "<u8"), ("signal_power_count", "<u8"), ("noise_power_count", "<u8"),
    ("samples_processed", "<u8"), ("samples_lost", "<u8"), ("nbuffers", "<u8"), ("nflips", "<u8"),
    ("signal_power_sum", "<f8"), ("noise_power_sum", "<f8"), ("peak_signal_power", "<f8"),
    ("t_convert_s", "<f8"), ("t_demod_s", "<f8"), ("demod_modeac", "<u8"),
])
COUNTER_FIELDS = ["demod_preambles", "demod_rejected_bad", "demod_rejected_unknown_icao", "demod_accepted",
                  "demod_preamblePhase", "demod_bestPhase", "strong_signal_count", "signal_power_count",
                  "noise_power_count", "samples_processed", "samples_lost", "nbuffers", "nflips"]


def ensure_built():
    """Build whatever is missing (everything is normally built by __graft_entry__.build())."""
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build(quiet=True)


_synth = None


def synth(seconds=None, nsamples=None, fmt=0, seed=88172645463325252, rate=2000.0, naircraft=200, dense=0,
          noise=3.0, first=0, threads=8):
    """Seeded synthetic capture (tools/synth_iq.c) as a uint8 array of raw IQ bytes."""
    global _synth
    if _synth is None:
        _synth = C.CDLL(os.path.join(TOOLS_DIR, "libsynth_iq.so"))
        _synth.synth_iq_generate.argtypes = [C.c_uint64, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double,
                                             C.c_uint64, C.c_uint64, C.c_void_p, C.c_int]
    n = int(nsamples if nsamples is not None else round(seconds * 2400000))
    out = np.empty(n * FMT_BYTES[fmt], dtype=np.uint8)
    _synth.synth_iq_generate(seed, fmt, rate, naircraft, dense, noise, first, n, out.ctypes.data, threads)
    return out


_oracle = None


class OracleCfg(C.Structure):
    _fields_ = [("format", C.c_int), ("nfix_crc", C.c_int), ("fixDF", C.c_int), ("preamble_threshold", C.c_int)]


def oracle_lib():
    global _oracle
    if _oracle is None:
        lib = C.CDLL(os.path.join(ORACLE_DIR, "libmodes_oracle.so"))
        lib.modes_oracle_run.argtypes = [C.POINTER(OracleCfg), C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]
        lib.modes_oracle_free.argtypes = [C.c_void_p]
        lib.modes_oracle_convert.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_double),
                                             C.POINTER(C.c_double)]
        lib.modes_oracle_uc8_lut.restype = C.POINTER(C.c_uint16)
        lib.modes_oracle_checksum.argtypes = [C.c_void_p, C.c_int]
        lib.modes_oracle_checksum.restype = C.c_uint32
        lib.modes_oracle_crc_init.argtypes = [C.c_int]
        lib.modes_oracle_diagnose.argtypes = [C.c_uint32, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.modes_oracle_table_size.argtypes = [C.c_int]
        lib.modes_oracle_stream_begin.argtypes = [C.POINTER(OracleCfg), C.c_int64]
        lib.modes_oracle_stream_mag_buf.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_int64, C.c_double, C.c_double]
        lib.modes_oracle_stream_take.argtypes = [C.POINTER(C.c_void_p), C.c_void_p]
        lib.modes_oracle_stream_take.restype = C.c_uint64
        lib.modes_oracle_stream_filter_add.argtypes = [C.c_uint32]
        _oracle = lib
    return _oracle


def oracle_run(iq, fmt=0, nfix=1, fixdf=1, thr=58, want_mag=False, mode_ac=0, filter_clock=0):
    """Our CPU restatement (oracle/modes_oracle.c) on an in-memory capture.  filter_clock 1 = the reference program's other
    start-up order (first ICAO filter flip before buffer 0)."""
    lib = oracle_lib()
    lib.modes_oracle_set_mode_ac(int(mode_ac))
    lib.modes_oracle_set_filter_clock(int(filter_clock))
    iq = np.ascontiguousarray(iq).view(np.uint8).reshape(-1)
    n = iq.size // FMT_BYTES[fmt]
    cfg = OracleCfg(fmt, nfix, fixdf, thr)
    out, nout = C.c_void_p(), C.c_uint64()
    st = np.zeros(1, dtype=ORACLE_STATS)
    mag = np.zeros(n + 326, dtype=np.uint16) if want_mag else None
    lib.modes_oracle_run(C.byref(cfg), iq.ctypes.data, n, C.byref(out), C.byref(nout), st.ctypes.data,
                         mag.ctypes.data if want_mag else None)
    msgs = np.zeros(nout.value, dtype=ORACLE_MSG)
    if nout.value:
        C.memmove(msgs.ctypes.data, out.value, nout.value * ORACLE_MSG.itemsize)
    lib.modes_oracle_free(out)
    return (msgs, st[0], mag) if want_mag else (msgs, st[0])


BUF_SAMPLES, TRAILING = 131072, 326
SHOW_ONLY = 0xff123456       # modesInit's icaoFilterAdd(Modes.show_only) (readsb.c:310): the filter's first entry


def _script_grid(ops, fmt):
    """-> [(first buffer, buffers)] per feed, [(buffers so far, op)] for the other operations, the concatenated IQ bytes."""
    grid, others, nbuf, parts, short = [], [], 0, [], False
    for op in ops:
        if op[0] == "feed":
            iq = np.ascontiguousarray(op[1]).view(np.uint8).reshape(-1)
            n = iq.size // FMT_BYTES[fmt]
            assert n > 0 and not short, "only the last feed of a script may end short"
            short = n % BUF_SAMPLES != 0
            nb = -(-n // BUF_SAMPLES)
            grid.append((nbuf, nb))
            nbuf += nb
            parts.append(iq)
        else:
            assert op[0] in ("expire", "add")
            others.append((nbuf, op))
    assert short, "a script's last feed ends short (an exact multiple has the reader push one more, empty, buffer)"
    return grid, others, np.concatenate(parts)


def oracle_stream(ops, fmt=0, nfix=1, fixdf=1, thr=58, mode_ac=0, filter_clock=0):
    """Our CPU restatement driven by a filter script (what a host that keeps its own ICAO filter forwards between feeds):
    ops = [("feed", iq) | ("expire",) | ("add", addr)] in stream order, filter_clock = mgpu_config.filter_clock.  The buffer grid is
    ifileRun's, walked as tests/host_stub/modes_gpu_standin.c walks it.  With filter_clock 2 the library starts empty and the script
    itself starts with ("add", SHOW_ONLY), as modesInit does; modes_oracle_stream_begin has made that add already.
    -> [(messages, counters)] per feed, the counters as they stand right after the feed."""
    lib = oracle_lib()
    _script_grid(ops, fmt)
    ops = list(ops)
    if filter_clock == 2:
        assert ops and tuple(ops[0]) == ("add", SHOW_ONLY), "a filter_clock 2 script starts with modesInit's add of show_only"
        ops = ops[1:]
    lib.modes_oracle_set_mode_ac(int(mode_ac))
    lib.modes_oracle_set_filter_clock(int(filter_clock))
    cfg = OracleCfg(fmt, nfix, fixdf, thr)
    lib.modes_oracle_stream_begin(C.byref(cfg), STARTUP_MS)
    bufs = [np.zeros(BUF_SAMPLES + TRAILING, dtype=np.uint16) for _ in range(2)]
    lens, k, counter, out = [0, 0], 0, 0, []
    try:
        for op in ops:
            if op[0] == "expire":
                lib.modes_oracle_stream_filter_expire()
            elif op[0] == "add":
                lib.modes_oracle_stream_filter_add(int(op[1]))
            else:
                iq = np.ascontiguousarray(op[1]).view(np.uint8).reshape(-1)
                n = iq.size // FMT_BYTES[fmt]
                for off in range(0, n, BUF_SAMPLES):
                    slen = min(BUF_SAMPLES, n - off)
                    cur, last, lastlen = bufs[k & 1], bufs[(k + 1) & 1], lens[(k + 1) & 1]
                    cur[:TRAILING] = last[lastlen:lastlen + TRAILING] if k > 0 and lastlen >= TRAILING else 0
                    piece = iq[off * FMT_BYTES[fmt]:(off + slen) * FMT_BYTES[fmt]]
                    ml, mp = C.c_double(), C.c_double()
                    lib.modes_oracle_convert(fmt, piece.ctypes.data, cur[TRAILING:].ctypes.data, slen, C.byref(ml), C.byref(mp))
                    lens[k & 1] = slen
                    st = counter * 5
                    lib.modes_oracle_stream_mag_buf(cur.ctypes.data, slen, st, st // 12000 + STARTUP_MS, ml.value, mp.value)
                    counter += slen
                    k += 1
                ptr, stats = C.c_void_p(), np.zeros(1, dtype=ORACLE_STATS)
                nout = lib.modes_oracle_stream_take(C.byref(ptr), stats.ctypes.data)
                msgs = np.zeros(nout, dtype=ORACLE_MSG)
                if nout:
                    C.memmove(msgs.ctypes.data, ptr.value, nout * ORACLE_MSG.itemsize)
                lib.modes_oracle_free(ptr)
                out.append((msgs, stats[0]))
    finally:
        lib.modes_oracle_set_mode_ac(0)
        lib.modes_oracle_set_filter_clock(0)
    return out


def reference_run(iq, fmt=0, nfix=1, fixdf=1, thr=58, want_mag=False, mode_ac=0, flip_before=False, ops=None, filter_clock=None):
    """The checker of the -m gpu parity tests: the reference's OWN objects (oracle/_ref, compiled from the reference's C files in
    place; the prebuilt files travel to the GPU box) where they are there, the restatement otherwise, so that a developer without
    them can still run the suite (tests/test_oracle.py pins the restatement to _ref either way).  That the objects ARE there on a
    GPU run is a test of its own (test_gpu_parity.py::test_reference_objects_are_present), so the fallback cannot pass unnoticed.
    flip_before = the reference program's other start-up order (oracle_run's filter_clock=1; pinned in tests/test_oracle.py).
    ops = a filter script (oracle_stream) in place of iq, with filter_clock 0 / 1 / 2: -> [(messages, counters)] per feed
    (the reference's objects where they take scripts, ref_takes_scripts(); tests/test_oracle_filter_script.py pins the restatement
    to them there)."""
    if ops is not None:
        clock = (1 if flip_before else 0) if filter_clock is None else filter_clock
        if ref_takes_scripts():
            return ref_run(None, fmt, nfix, fixdf, thr, mode_ac=mode_ac, ops=ops, filter_clock=clock)
        return oracle_stream(ops, fmt, nfix, fixdf, thr, mode_ac=mode_ac, filter_clock=clock)
    if have_ref():
        return ref_run(iq, fmt, nfix, fixdf, thr, want_mag=want_mag, mode_ac=mode_ac, flip_before=flip_before)
    return oracle_run(iq, fmt, nfix, fixdf, thr, want_mag=want_mag, mode_ac=mode_ac, filter_clock=1 if flip_before else 0)


def oracle_convert(iq, fmt):
    lib = oracle_lib()
    iq = np.ascontiguousarray(iq).view(np.uint8).reshape(-1)
    n = iq.size // FMT_BYTES[fmt]
    mag = np.empty(n, dtype=np.uint16)
    ml, mp = C.c_double(), C.c_double()
    lib.modes_oracle_convert(fmt, iq.ctypes.data, mag.ctypes.data, n, C.byref(ml), C.byref(mp))
    return mag, ml.value, mp.value


def have_ref():
    return os.path.exists(REF_BIN)


_ref_scripts = None


def ref_takes_scripts():
    """Is there a ref_demod, and was it built from a harness that takes filter scripts?  A build from an earlier oracle/ref_harness.c
    (oracle/_ref is built where the reference tree is, and carried from there) ignores ORACLE_FILTER_SCRIPT without a word, so the
    program is asked (`ref_demod --capabilities`).  Without one, scripts go to the restatement, exactly as every run does where
    oracle/_ref is missing; the per-feed counts of tests/filter_util.py's RECORDED, taken from _ref, hold either way."""
    global _ref_scripts
    if _ref_scripts is None:
        _ref_scripts = False
        if have_ref():
            r = subprocess.run([REF_BIN, "--capabilities"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
            _ref_scripts = r.returncode == 0 and "filter-script" in r.stdout.split()
    return _ref_scripts


REF_TRACE = np.dtype([("nout", "<u8"), ("stats", ORACLE_STATS)])      # ref_harness.c's trace: one record after every buffer


def ref_run(iq, fmt=0, nfix=1, fixdf=1, thr=58, want_mag=False, mode_ac=0, flip_before=False, ops=None, filter_clock=None):
    """The reference's own objects (oracle/_ref/ref_demod), one process per run.  ops = a filter script (oracle_stream) in place
    of iq, filter_clock 0 / 1 / 2 with it: -> [(messages, counters)] per feed."""
    grid = None
    if ops is not None:
        assert iq is None and not want_mag
        assert ref_takes_scripts(), f"{REF_BIN} is missing or was built from a harness without filter scripts: `make -C oracle ref`"
        grid, others, iq = _script_grid(ops, fmt)
        flip_before = filter_clock == 1
    iq = np.ascontiguousarray(iq).view(np.uint8).reshape(-1)
    with tempfile.TemporaryDirectory() as d:
        fin, fm, fs, fg, fscript = (os.path.join(d, x) for x in ("in.iq", "out.msgs", "out.stats", "out.mag", "script.txt"))
        iq.tofile(fin)
        cmd = [REF_BIN, FMT_NAMES[fmt], str(nfix), str(fixdf), str(thr), fin, fm, fs] + ([fg] if want_mag else [])
        env = dict(os.environ)
        if mode_ac:
            env["ORACLE_MODE_AC"] = "1"
        else:
            env.pop("ORACLE_MODE_AC", None)
        for name in ("ORACLE_FLIP_BEFORE", "ORACLE_FILTER_SCRIPT", "ORACLE_FILTER_EXTERNAL"):
            env.pop(name, None)
        if flip_before:
            env["ORACLE_FLIP_BEFORE"] = "1"
        if grid is not None:
            with open(fscript, "w") as f:
                for nbuf, op in others:
                    f.write(f"{nbuf} E\n" if op[0] == "expire" else f"{nbuf} A {int(op[1]):x}\n")
            env["ORACLE_FILTER_SCRIPT"] = fscript
            if filter_clock == 2:
                env["ORACLE_FILTER_EXTERNAL"] = "1"
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL, env=env)
        msgs = np.fromfile(fm, dtype=ORACLE_MSG)
        st = np.fromfile(fs, dtype=ORACLE_STATS)[0]
        if grid is not None:
            trace = np.fromfile(fscript + ".trace", dtype=REF_TRACE)
            assert len(trace) == grid[-1][0] + grid[-1][1] and (len(trace) == 0 or trace["nout"][-1] == len(msgs))
            out = []
            for first, nb in grid:
                lo = int(trace["nout"][first - 1]) if first else 0
                out.append((msgs[lo:int(trace["nout"][first + nb - 1])], trace["stats"][first + nb - 1]))
            return out
        if want_mag:
            return msgs, st, np.fromfile(fg, dtype=np.uint16)
    return msgs, st


def assert_same_messages(gpu_msgs, oracle_msgs, startup_ms=STARTUP_MS):
    """Bit-exact comparison of the product's mgpu_msg list with the checker's oracle_msg list."""
    assert len(gpu_msgs) == len(oracle_msgs), f"message count {len(gpu_msgs)} != oracle {len(oracle_msgs)}"
    if len(gpu_msgs) == 0:
        return
    g, o = gpu_msgs, oracle_msgs
    for name, a, b in [
        ("timestamp", g["timestamp"], o["timestamp"]),
        ("sysTimestamp", g["sysTimestamp"] - startup_ms, o["sys_rel_ms"]),
        ("score", g["score"].astype(np.int64), o["score"].astype(np.int64)),
        ("correctedbits", g["correctedbits"].astype(np.int64), o["correctedbits"].astype(np.int64)),
        ("msgbits", g["msgbits"].astype(np.int64), o["msgbits"].astype(np.int64)),
        ("msgtype", g["msgtype"].astype(np.int64), o["msgtype"].astype(np.int64)),
        ("addr", g["addr"].astype(np.int64), o["addr"].astype(np.int64)),
    ]:
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, f"{name}: {bad.size} mismatches, first at message {bad[0]}: {a[bad[0]]} vs {b[bad[0]]}"
    for name in ("msg", "raw"):
        bad = np.nonzero((g[name] != o[name]).any(axis=1))[0]
        assert bad.size == 0, f"{name}: {bad.size} mismatches, first at {bad[0]}: {g[name][bad[0]]} vs {o[name][bad[0]]}"
    sig = g["sig_sumsq"].astype(np.float64) / 65535.0 / 65535.0 / g["sig_len"].astype(np.float64)
    bad = np.nonzero(sig != o["signalLevel"])[0]
    assert bad.size == 0, f"signalLevel: {bad.size} mismatches, first at {bad[0]}: {sig[bad[0]]} vs {o['signalLevel'][bad[0]]}"


def assert_same_counters(gpu_counters, oracle_stats, float_tol=0.0):
    for f in COUNTER_FIELDS:
        a = np.asarray(gpu_counters[f], dtype=np.uint64)
        b = np.asarray(oracle_stats[f], dtype=np.uint64)
        assert (a == b).all(), f"counter {f}: gpu {a} != oracle {b}"
    for f in ("signal_power_sum", "peak_signal_power", "noise_power_sum"):
        a, b = float(gpu_counters[f]), float(oracle_stats[f])
        if np.isnan(a) and np.isnan(b):
            continue
        if float_tol == 0.0:
            assert a == b, f"{f}: gpu {a!r} != oracle {b!r}"
        else:
            assert abs(a - b) <= float_tol * max(1.0, abs(b)), f"{f}: gpu {a!r} vs oracle {b!r}"


def beast_frames(stream):
    """Split a beast byte stream into raw frames and their unescaped fields (type, 48-bit timestamp, sig, message)."""
    out, i, n = [], 0, len(stream)
    while i < n:
        assert stream[i] == 0x1A
        j = i + 2
        while j < n and not (stream[j] == 0x1A and (j + 1 >= n or stream[j + 1] != 0x1A)):
            j += 2 if stream[j] == 0x1A else 1
        raw = bytes(stream[i:j])
        body = raw[2:].replace(b"\x1a\x1a", b"\x1a")
        out.append((raw, raw[1], int.from_bytes(body[:6], "big"), body[6], body[7:]))
        i = j
    return out


GOLDEN_BEAST = [("uc8_fix_2s", dict(seconds=2.0, seed=99, rate=1500.0), dict(nfix=1, mode_ac=0)),
                ("uc8_aggressive_modeac_3s", dict(seconds=3.0, seed=98, rate=700.0, dense=2), dict(nfix=2, mode_ac=1))]
