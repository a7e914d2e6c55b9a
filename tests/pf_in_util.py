"""Planefinder input (readPlanefinder + decodePfMessage over a DLE-framed stream): the frame builder and case groups behind
tests/golden/pf_in_cases.npz, the golden's loader, the reference harness (tests/host_stub/pf_in_ref_harness.c, which includes the
reference's net_io.c and links oracle/_ref/full's other objects) and the library's host side (mgpu_pf_decode_host, mgpu_pf_parse_host).
Groups b, c, d and d2 are the raw input's (tests/raw_in_util.py: the CRC matrix, the order cases, the growth of the filter's table) with
every AVR line turned into the Planefinder frame of the same message; group a is the framing's own, group p reads past the end."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np

import helpers
import raw_in_util as ru
import sbs_util

GOLDEN = os.path.join(helpers.GOLDEN_DIR, "pf_in_cases.npz")
HARNESS_SRC = os.path.join(helpers.ROOT, "tests", "host_stub", "pf_in_ref_harness.c")
NOW_MS = ru.NOW_MS
TILE = 8192                                     # kUatTile of kernels.h: bytes per tile of kernels/pf_in.inc
CHUNK = 32                                      # bytes of a tile one lane takes
REACH = 53                                      # kPfInReach: what a handler call reads from its start DLE at the most
DLE, ETX, PID = 0x10, 0x03, 0xC1
MGPU_OK, MGPU_E_INVAL, MGPU_E_OVERFLOW = 0, -1, -5
MODEAC, BAD, ACCEPT, COND, UNKNOWN, MODEAC_OFF, TYPE = range(1, 8)                          # MGPU_PF_IN_*
STEP_END, STEP_SKIP, STEP_OTHER, STEP_FRAME, STEP_INCOMPLETE = range(5)                      # MGPU_PF_STEP_*
MSG = ru.MSG
HEAD = ("consumed", "nframes", "nmsgs", "remote_received_modes", "remote_received_modeac", "remote_rejected_unknown_icao", "remote_rejected_bad", "remote_accepted0",
        "remote_accepted1", "remote_accepted2")
# (nfix_crc, fixDF, mode_ac) per group; groups d and d2 also prepare the filter
CONFIGS = {"a": ((1, 1, 0), (1, 1, 1)), "b": ((0, 1, 0), (2, 1, 0), (1, 0, 0)), "bb": ((0, 1, 0), (2, 1, 0), (1, 0, 0)), "c": ((1, 1, 0),), "d": ((1, 1, 0),),
           "d2": ((1, 1, 0),), "p": ((1, 1, 1),)}
GROUPS = ("a", "b", "bb", "c", "d", "p")
ALL_CONFIGS = [(n, f, m) for n in (0, 1, 2) for f in (0, 1) for m in (0, 1)]
FIELDS = ("pad", "type", "sig", "secs", "nanos", "msg")


def key(group, cfg):
    return "%s_n%df%dm%d" % (group, *cfg)


# ---- frames ----

def stuffed(data):
    return bytes(data).replace(b"\x10", b"\x10\x10")


def frame(msg, secs=0x01234567, nanos=0x0089ABCD, sig=0x80, type_=None, pid=PID, pad=0, stuff=FIELDS, end=b"\x10\x03"):
    """One Planefinder frame of a message given by its bytes (2, 7 or 14: type nibble 0, 1, 2 unless type_ says otherwise).  stuff:
    the fields whose DLE bytes are doubled."""
    msg = bytes(np.asarray(msg, dtype=np.uint8).reshape(-1).tobytes()) if not isinstance(msg, (bytes, bytearray)) else bytes(msg)
    t = type_ if type_ is not None else {2: 0, 7: 1, 14: 2}[len(msg)]
    parts = dict(pad=bytes([pad]), type=bytes([t]), sig=bytes([sig]), secs=int(secs).to_bytes(4, "big"), nanos=int(nanos).to_bytes(4, "big"), msg=msg)
    body = b"".join(stuffed(parts[f]) if f in stuff else parts[f] for f in FIELDS)
    return bytes([DLE, pid]) + body + end


def frame_of_df(f, **kw):
    """A frame array of frames_util (14 bytes, short ones padded) at the length its DF gives."""
    f = np.asarray(f, dtype=np.uint8).reshape(-1)
    return frame(f[: 14 if f[0] & 0x80 else 7].tobytes(), **kw)


TINY = bytes([DLE, PID, DLE, ETX])              # the 4-byte frame: its decode runs through its own end into what lies behind it


def _pf_avr(fr_, lead=b"*", ts=b"0123456789AB", sig=b"80", semi=b";", end=b"\n", nbytes=None, suffix=b""):
    """raw_in_util.avr's signature: the Planefinder frame of the same message (time and signal from the line where they are hex)."""
    h = fr_ if isinstance(fr_, (bytes, bytearray)) else ru.hexs(fr_, nbytes)
    try:
        t = int(ts, 16)
    except ValueError:
        t = 0
    try:
        s = int(sig, 16) & 0xFF
    except ValueError:
        s = 0
    return frame(bytes.fromhex(h.decode()), secs=(t >> 20) & 0xFFFFFFFF if lead in (b"@", b"<", b"%") else 0x10000000 + len(h), nanos=(t & 0xFFFFF) * 953,
                 sig=s if lead == b"<" else 0x10 if len(h) % 3 == 0 else 0x55)


@contextlib.contextmanager
def _as_pf():
    """raw_in_util's groups built with Planefinder frames for AVR lines (its whitespace filler lines lie between frames here)."""
    old = ru.avr
    ru.avr = _pf_avr
    try:
        yield
    finally:
        ru.avr = old


def filler(rng, n, pool=ru.POOL, first=0):
    """Ordinary traffic of a pool of aircraft (times that count up; one frame in eleven of another packet id)."""
    out = []
    for k in range(first, first + n):
        a = int(pool[rng.integers(0, len(pool))])
        kind = int(rng.integers(0, 8))
        f = ru.es(a, k) if kind < 3 else ru.df11(a) if kind == 3 else ru.ap((0, 4, 5, 16, 20, 21)[int(rng.integers(0, 6))], a, seed=k)
        secs, nanos, sig = 0x65101000 + k // 7, (k * 16777259) % 1000000000, (k * 13) & 0xFF
        x = frame_of_df(f, secs=secs, nanos=nanos, sig=sig)
        if kind == 7:
            x = frame(bytes([0x10 if k % 3 == 0 else k & 0xFF, (k >> 3) & 0xFF]), secs=secs, nanos=nanos, sig=sig)
        if k % 11 == 0:
            x = frame(bytes(range(k & 15, (k & 15) + 7)), pid=(0x41, 0xC0, 0x00, 0xFF)[k // 11 % 4])
        out.append(x)
    return out


def pad_to(parts, total, rng, period=1 << 30):
    """Filler traffic behind the cases until the stream has `total` bytes at least (period: the traffic repeats, which a golden file
    compresses well)."""
    have = sum(len(x) for x in parts)
    k = 0
    while have < total:
        x = filler(np.random.default_rng(k % period), 1, first=k % period)[0] if k % 9 else (b"\x00between\xff", b"\x10\x10", b"\x10\x03", b"\x03\x03", b"\x10")[k // 9 % 5]
        parts.append(x)
        have += len(x)
        k += 1
    return parts


A = ru.A


def group_a():
    """The framing matrix."""
    rng = np.random.default_rng(31)
    long_, short, ac = ru.es(A, 3)[:14].tobytes(), ru.df11(A)[:7].tobytes(), b"\x77\x00"
    good = frame(long_)
    g = [frame(long_), frame(short), frame(ac), TINY, good, good]
    # a DLE in every field position of every type: stuffed, and bare (the decode shifts, the frame may end early)
    for msg in (ac, short, long_):
        for at in range(1 + 1 + 1 + 8 + len(msg)):
            body = bytearray(b"\x00" + bytes([{2: 0, 7: 1, 14: 2}[len(msg)]]) + b"\x80" + bytes.fromhex("0123456700 89abcd".replace(" ", "")) + msg)
            body[at] = DLE
            g += [bytes([DLE, PID]) + stuffed(body) + b"\x10\x03", bytes([DLE, PID]) + bytes(body) + b"\x10\x03", good]
            body[at] = ETX
            g += [bytes([DLE, PID]) + bytes(body) + b"\x10\x03"]
    # DLE DLE ETX in a body: the frame ends at its second DLE
    g += [frame(long_[:8] + b"\x10\x03" + long_[10:]), good, frame(b"\x10\x03", sig=0x10), good, frame(short, secs=0x00001003), good]
    # the 4-byte frame in front of each kind of frame, and in a row
    g += [TINY, frame(short), TINY, frame(ac), TINY, TINY, TINY, good, TINY, frame(long_, pid=0x41), good]
    # runs of DLE, DLE ETX while searching, a lone ETX
    for n in range(1, 8):
        g += [bytes([DLE]) * n + good, bytes([DLE]) * n + good[1:], bytes([DLE]) * n + b"\x03" + good]
    g += [b"\x10\x03", good, b"\x10\x03\x10\x03", good, b"\x03\x10", good]
    # packet ids: anything but 0xc1 is skipped; 0x10 and 0x03 start no frame
    for pid in (0x41, 0x00, 0xC0, 0xC2, 0xFF, 0x10, 0x03, 0x01):
        g += [frame(long_, pid=pid), good]
    # a frame of another id holding what looks like frames: the first DLE ETX ends it
    g += [bytes([DLE, 0x41]) + good + good, good]
    # every type byte's low nibble, and bits 4 to 7 on the types that decode
    for t in range(3, 16):
        g += [frame(short, type_=t), frame(long_, type_=t | 0xA0)]
    for hi in range(1, 16):
        g += [frame(ac, type_=hi << 4), frame(short, type_=hi << 4 | 1), frame(long_, type_=hi << 4 | 2)]
    g += [frame(long_, secs=0xFFFFFFFF, nanos=0xFFFFFFFF, sig=0xFF), frame(short, secs=0, nanos=0, sig=0), frame(long_, secs=0x10101010, nanos=0x10101010, sig=0x10, pad=0x10),
          frame(b"\x10" * 14, secs=0x10101010, nanos=0x10101010, sig=0x10, pad=0x10, type_=0x12)]
    # a long frame of another id without an event in it, then traffic
    g += [bytes([DLE, 0x41]) + bytes(300) + b"\x10\x03", good]
    pad_to(g, 3 * TILE + 500, rng, period=60)
    g.append(good[:20])                                                                       # a frame without an end
    return g


def group_p():
    """Reads past the end: the 4-byte frame as the stream's last bytes, Mode A/C on."""
    rng = np.random.default_rng(35)
    g = pad_to([], 3 * TILE + 100, rng, period=45)
    g += [frame(ru.es(A, 9)[:14].tobytes()), TINY]
    return g


def group_d():
    """Growth, as raw_in_util.group_d with seven probes per new address (the stream stays below five tiles).
    -> (frames, the handler call of the first growth L*, that of the second, the probes: [(handler call, address, passes)])"""
    rng = np.random.default_rng(14)
    f = ru.FilterModel()
    for op in ru.D_OPS:
        f.expire() if op < 0 else f.add(op)
    g, probes, growths, seen_new = [], [], [], []

    def probe(a, seed):
        probes.append((len(g), int(a), f.test(int(a))))
        g.append(frame_of_df(ru.ap((0, 4, 5, 16, 20, 21)[seed % 6], int(a), seed), secs=0x65101000 + seed, sig=seed & 0xFF))

    def adder(a, k):
        if f.add(int(a)):
            growths.append(len(g))
        g.append(frame_of_df(ru.es(int(a), k) if k % 3 else ru.df11(int(a)), nanos=k))

    readd, onstar = int(ru.D_INACTIVE[7]), int(ru.D_INACTIVE[11])       # re-added in front of L*; the adder on L* itself is of the inactive generation
    k = 0
    for i, a in enumerate(ru.D_NEW):
        if i == 20:
            adder(readd, 1)
        if i == 30:
            adder(int(ru.D_ACTIVE[3]), 1)                                # already active: no new add
        if f.occupied == (1 << 8) // 3 and f.bits == 8:
            probe(ru.D_INACTIVE[5], k)                                   # in front of L*: still known
            probe(onstar, k + 1)
            adder(onstar, 1)                                             # L*
            assert growths and growths[-1] == len(g) - 1
            probe(ru.D_INACTIVE[5], k + 2)                               # behind L*: gone
            probe(onstar, k + 3)
            probe(readd, k + 4)
        adder(a, 1 + (i % 5))
        seen_new.append(int(a))
        for j in range(7):
            pick = int(rng.integers(0, 5))
            src = (ru.D_INACTIVE, ru.D_ACTIVE, np.array(seen_new), ru.D_NEW[i + 1:] if i + 1 < len(ru.D_NEW) else ru.D_NEW, ru.D_INACTIVE)[pick]
            probe(src[int(rng.integers(0, len(src)))], k + j)
        k += 13
    assert len(growths) == 2 and f.bits == 10, growths
    return g, growths[0], growths[1], probes


def _keep(parts, total):
    have, keep = 0, 0
    while have < total and keep < len(parts):
        have += len(parts[keep])
        keep += 1
    return parts[:keep]


def build_groups():
    with _as_pf():
        b, c, d2 = ru.group_b(), ru.group_c(), ru.group_d2()
    # the CRC matrix is longer than five tiles: two halves, each behind the three frames that make the matrix's addresses known
    head, rest = b[:3], b[3:]
    half = len(rest) // 2
    rng = np.random.default_rng(32)
    # group c's cases end in its third tile: three tiles and a little of its filler are kept
    return {"a": group_a(), "b": pad_to(head + rest[:half], 3 * TILE + 300, rng, period=50), "bb": pad_to(head + rest[half:], 3 * TILE + 300, rng, period=50),
            "c": _keep(c, 3 * TILE + 300), "d": group_d()[0], "d2": d2, "p": group_p()}


def group_d_info():
    """-> (frames, L*, the second growth, probes) of group d: the indices are handler calls."""
    return group_d()


def order_cases(addr0):
    with _as_pf():
        return ru.order_cases(addr0)


def stream_of(parts):
    return b"".join(parts)


def ops_of(group):
    return ru.D_OPS if group in ("d", "d2") else []


def draw_stream(rng, nframes, hostile=0.15):
    """Traffic with damage: bytes overwritten (often with DLE or ETX), inserted, dropped; a cut at the end."""
    s = bytearray(stream_of(filler(rng, nframes, first=int(rng.integers(0, 1000)))))
    for _ in range(int(hostile * nframes)):
        at = int(rng.integers(0, max(1, len(s))))
        kind = int(rng.integers(0, 6))
        if kind == 0:
            s[at: at + 1] = bytes([(DLE, ETX)[int(rng.integers(0, 2))]])
        elif kind == 1:
            s[at: at + 1] = bytes(rng.integers(0, 256, 1, dtype=np.uint8))
        elif kind == 2:
            s[at:at] = bytes(rng.choice(np.array([DLE, DLE, ETX, PID, 0x41, 0x00], dtype=np.uint8), int(rng.integers(1, 5))))
        elif kind == 3:
            del s[at: at + int(rng.integers(1, 5))]
        elif kind == 4:
            s[at:at] = bytes(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8))
        else:
            s[at:at] = (TINY, b"\x10\x03", b"\x10\x10", b"\x10", bytes([DLE, PID]), bytes([DLE, 0x41]))[int(rng.integers(0, 6))]
    cut = int(rng.integers(0, 70))
    if cut and int(rng.integers(0, 2)):
        del s[len(s) - min(cut, len(s)):]
    return bytes(s)


def draw_automaton_stream(rng, n):
    """n bytes over {DLE, ETX, 0xc1, 0x41, 0}: every state of the framer within a few bytes."""
    return bytes(rng.choice(np.array([DLE, ETX, PID, 0x41, 0], dtype=np.uint8), n))


# ---- the reference ----

def have_ref_full():
    return sbs_util.have_ref_full()


def build_ref_harness(workdir):
    """tests/host_stub/pf_in_ref_harness.c compiled with the flags of `make -C oracle full` and linked against that build's other
    objects, readsb.o with its main renamed in a copy (as tests/raw_in_util.py builds its harness)."""
    return ru.build_ref_harness(workdir, "pf_in", HARNESS_SRC)


def parse_results(blob, n):
    """n results as the harness writes them -> [dict(head, cls, off, frame_of, signal, msgs)]"""
    return ru.read_results(blob, n, 10, (("cls", np.uint8), ("off", np.uint64)), (("frame_of", np.uint64), ("signal", np.float64), ("msgs", MSG)))


def run_ref_harness(exe, streams, cfg, workdir, ops=(), now_ms=NOW_MS, reps=1):
    """The reference over the streams, one after the other against one filter prepared by ops -> a result per stream"""
    paths = []
    for k, s in enumerate(streams):
        paths.append(os.path.join(workdir, "pf_in_stream%d.bin" % k))
        open(paths[-1], "wb").write(s)
    fpath = os.path.join(workdir, "pf_in_filter.bin")
    np.asarray(list(ops), dtype=np.int32).tofile(fpath)
    r = subprocess.run([exe, str(int(now_ms)), *[str(x) for x in cfg], fpath, str(int(reps)), *paths], check=True, capture_output=True, timeout=600)
    return parse_results(r.stdout, len(streams))


def load_golden():
    """-> {key(group, cfg): dict(stream, head, cls, off, frame_of, signal, msgs)}"""
    z = np.load(GOLDEN)
    out = {}
    for g, cfgs in CONFIGS.items():
        for cfg in cfgs:
            k = key(g, cfg)
            out[k] = dict(stream=z[g + "_stream"].tobytes(), head=z[k + "_head"], cls=z[k + "_class"], off=np.cumsum(z[k + "_off"].astype(np.uint64), dtype=np.uint64),
                          frame_of=np.cumsum(z[k + "_frame_of"].astype(np.uint64), dtype=np.uint64), signal=z[k + "_signal"], msgs=z[k + "_msgs"].view(MSG).reshape(-1))
    return out


# ---- the library's host side ----

def pf_args(binding, buf, nbytes, arrays, outs, cn, now_ms=NOW_MS, msgs_cap=None, frames_cap=None, pass_bytes=0, pointers=None):
    """struct mgpu_pf_in_args over numpy arrays (or raw pointers): arrays = dict(msgs, signal, frame_of, cls, off), any of the optional
    ones None; outs = (consumed, nframes, nmsgs) ctypes values."""
    p = pointers or {k: (v.ctypes.data if v is not None else None) for k, v in arrays.items()}
    return binding.PfInArgs(C.sizeof(binding.PfInArgs), 0, buf, nbytes, int(now_ms), p["msgs"], p["signal"], p["frame_of"],
                            msgs_cap if msgs_cap is not None else len(arrays["msgs"]), p["cls"], p["off"], frames_cap if frames_cap is not None else len(arrays["cls"]),
                            C.pointer(outs[0]), C.pointer(outs[1]), C.pointer(outs[2]), C.pointer(cn), int(pass_bytes))


def new_outs():
    return (C.c_uint64(0), C.c_uint64(0), C.c_uint64(0))


def result_of(binding, rc, arrays, outs, cn):
    n, nf = int(outs[2].value), int(outs[1].value)
    m, f = min(n, len(arrays["msgs"])), min(nf, len(arrays["cls"]))
    return dict(rc=rc, consumed=int(outs[0].value), nframes=nf, nmsgs=n, counters=binding.pf_in_counters_dict(cn), msgs=arrays["msgs"][:m], signal=arrays["signal"][:m],
                frame_of=arrays["frame_of"][:m], cls=arrays["cls"][:f], off=arrays["off"][:f])


def new_arrays(nbytes):
    cap = nbytes // 4 + 1
    return dict(msgs=np.zeros(cap, dtype=MSG), signal=np.zeros(cap, dtype=np.float64), frame_of=np.zeros(cap, dtype=np.uint64), cls=np.zeros(cap, dtype=np.uint8),
                off=np.zeros(cap, dtype=np.uint64))


def host_decode(lib, stream, cfg, filt=None, now_ms=NOW_MS, pass_bytes=0):
    """mgpu_pf_decode_host: the sequential walk.  cfg = (nfix_crc, fixDF, mode_ac); filt: a raw_in_util.FilterModel, moved on by the call."""
    from readsb_amd import binding
    buf = np.frombuffer(bytes(stream) + b"\x10", dtype=np.uint8)                             # (a byte behind the stream that nothing may read as the stream's)
    arrays, outs, cn = new_arrays(len(stream)), new_outs(), binding.PfInCounters()
    a = pf_args(binding, buf.ctypes.data, len(stream), arrays, outs, cn, now_ms, pass_bytes=pass_bytes)
    kcfg = binding.RawInConfig(C.sizeof(binding.RawInConfig), *cfg[:3])
    rc = ru.through_filter(filt, len(stream) // 4 + 2, lambda f: lib.mgpu_pf_decode_host(C.byref(a), C.byref(kcfg), f))
    return result_of(binding, rc, arrays, outs, cn)


def parse_host(lib, stream, offset, cfg, now_ms=NOW_MS):
    """mgpu_pf_parse_host -> (rc, binding.PfInFrame)"""
    from readsb_amd import binding
    buf = stream if isinstance(stream, np.ndarray) else np.frombuffer(bytes(stream), dtype=np.uint8)
    kcfg = binding.RawInConfig(C.sizeof(binding.RawInConfig), *cfg[:3])
    out = binding.PfInFrame()
    rc = int(lib.mgpu_pf_parse_host(buf.ctypes.data, len(stream), int(offset), int(now_ms), C.byref(kcfg), C.byref(out)))
    return rc, out


def compare(res, ref, what=""):
    """A library result (result_of) against a reference result (parse_results / load_golden), bytewise."""
    head = [res["consumed"], res["nframes"], res["nmsgs"], res["counters"]["remote_received_modes"], res["counters"]["remote_received_modeac"],
            res["counters"]["remote_rejected_unknown_icao"], res["counters"]["remote_rejected_bad"], *res["counters"]["remote_accepted"]]
    assert head == [int(x) for x in ref["head"]], (what, dict(zip(HEAD, head)), dict(zip(HEAD, [int(x) for x in ref["head"]])))
    assert res["cls"].tobytes() == ref["cls"].tobytes(), (what, "class", np.flatnonzero(res["cls"] != ref["cls"])[:10])
    assert res["off"].tobytes() == ref["off"].astype(np.uint64).tobytes(), (what, "frame_off")
    assert res["frame_of"].tobytes() == ref["frame_of"].astype(np.uint64).tobytes(), (what, "frame_of")
    assert res["signal"].tobytes() == ref["signal"].tobytes(), (what, "signal")
    assert res["msgs"].tobytes() == ref["msgs"].tobytes(), (what, "msgs", np.flatnonzero(res["msgs"] != ref["msgs"])[:10])


def same(res, other, what=""):
    """Two library results, everything."""
    for k in ("rc", "consumed", "nframes", "nmsgs", "counters"):
        assert res[k] == other[k], (what, k, res[k], other[k])
    for k in ("msgs", "signal", "frame_of", "cls", "off"):
        assert res[k].tobytes() == other[k].tobytes(), (what, k)
