"""Beast input (readBeast + decodeBinMessage over a binary stream): the stream builders and case groups behind
tests/golden/beast_in_cases.npz, the golden's loader, the reference harness (tests/host_stub/beast_in_ref_harness.c, which includes the
reference's net_io.c and links oracle/_ref/full's other objects) and the library's host side (mgpu_beast_decode_host,
mgpu_beast_parse_host).  Groups b, c, d and d2 are the raw input's (tests/raw_in_util.py: the CRC matrix, the order cases, the growth
of the filter's table) with every AVR line turned into the beast frame of the same message; groups a and e are the framing's own."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np

import helpers
import raw_in_util as ru
import sbs_util

GOLDEN = os.path.join(helpers.GOLDEN_DIR, "beast_in_cases.npz")
HARNESS_SRC = os.path.join(helpers.ROOT, "tests", "host_stub", "beast_in_ref_harness.c")
NOW_MS = ru.NOW_MS
TILE = 8192                                     # kUatTile of kernels.h: bytes per tile of kernels/beast_in.inc
HALO = 64                                       # kBeastInHalo: entry offsets of a tile
GROUP = 64                                      # kBeastInGroup: tiles whose exit maps are composed into one
CHUNK = 32                                      # bytes of a tile one lane takes
MAX_FRAME = 62                                  # kBeastInMaxFrame
TAIL = 256                                      # kBeastInTail
MGPU_OK, MGPU_E_INVAL, MGPU_E_OVERFLOW = 0, -1, -5
MODEAC, BAD, ACCEPT, COND, UNKNOWN, MODEAC_OFF, POSITION, PONG = range(1, 9)                  # MGPU_BEAST_IN_*
STOP_END, STOP_SYNTH, STOP_UUID = range(3)                                                   # MGPU_BEAST_STOP_*
STEP_GARBAGE, STEP_SKIP, STEP_FRAME, STEP_INCOMPLETE, STEP_SYNTH, STEP_UUID = range(6)       # MGPU_BEAST_STEP_*
MSG = ru.MSG
HEAD = ("consumed", "nframes", "nmsgs", "remote_received_modes", "remote_received_modeac", "remote_rejected_unknown_icao", "remote_rejected_bad", "remote_accepted0",
        "remote_accepted1", "remote_accepted2", "remote_malformed_beast", "receiver_id_out")
# (nfix_crc, fixDF, mode_ac, net_ingest) per group; groups d and d2 also prepare the filter
CONFIGS = {"a": ((1, 1, 0, 0), (1, 1, 1, 0)), "b": ((0, 1, 0, 0), (2, 1, 0, 0), (1, 0, 0, 0)), "c": ((1, 1, 0, 0),), "d": ((1, 1, 0, 0),),
           "d2": ((1, 1, 0, 0),), "e": ((1, 1, 1, 0), (1, 1, 1, 1))}
GROUPS = ("a", "b", "c", "d", "e")
ID_IN = 0x0102030405060708                      # c->receiverId in front of every golden stream
ALL_CONFIGS = [(n, f, m, i) for n in (0, 1, 2) for f in (0, 1) for m in (0, 1) for i in (0, 1)]


def key(group, cfg):
    return "%s_n%df%dm%di%d" % (group, *cfg)


# ---- frames ----

def esc(data):
    return bytes(data).replace(b"\x1a", b"\x1a\x1a")


def frame(msg, ts=0x0123456789AB, sig=0x80, type_=None, escape=True):
    """One beast frame of a message given by its bytes (2, 7 or 14: '1', '2', '3' unless type_ says otherwise)."""
    msg = bytes(np.asarray(msg, dtype=np.uint8).reshape(-1).tobytes()) if not isinstance(msg, (bytes, bytearray)) else bytes(msg)
    t = type_ if type_ is not None else {2: b"1", 7: b"2", 14: b"3"}[len(msg)]
    body = int(ts).to_bytes(6, "big") + bytes([sig]) + msg
    return b"\x1a" + t + (esc(body) if escape else body)


def frame_of_df(f, **kw):
    """A frame array of frames_util (14 bytes, short ones padded) at the length its DF gives."""
    f = np.asarray(f, dtype=np.uint8).reshape(-1)
    return frame(f[: 14 if f[0] & 0x80 else 7].tobytes(), **kw)


def prefix(rid, escape=True):
    b = int(rid).to_bytes(8, "big")
    return b"\x1a\xe3" + (esc(b) if escape else b)


def position(payload=None):
    return b"\x1a5" + esc(payload if payload is not None else bytes(range(0x40, 0x40 + 21)))


def pong(payload=b"\x01\x02\x03"):
    return b"\x1aP" + esc(payload)


MAXIMAL = prefix(0x1A1A1A1A1A1A1A1A) + frame(b"\x1a" * 14, ts=0x1A1A1A1A1A1A, sig=0x1A)       # 62 bytes: every escapable byte 0x1a
assert len(MAXIMAL) == MAX_FRAME


def _beast_avr(fr_, lead=b"*", ts=b"0123456789AB", sig=b"80", semi=b";", end=b"\n", nbytes=None, suffix=b""):
    """raw_in_util.avr's signature: the beast frame of the same message (timestamp and signal where they are hex, else 0)."""
    h = fr_ if isinstance(fr_, (bytes, bytearray)) else ru.hexs(fr_, nbytes)
    try:
        t = int(ts, 16)
    except ValueError:
        t = 0
    try:
        s = int(sig, 16) & 0xFF
    except ValueError:
        s = 0
    return frame(bytes.fromhex(h.decode()), ts=t if lead in (b"@", b"<", b"%") else int(len(h)) * 0x010203, sig=s if lead == b"<" else 0x1A if len(h) % 3 == 0 else 0x55)


@contextlib.contextmanager
def _as_beast():
    """raw_in_util's groups built with beast frames for AVR lines (its whitespace filler lines are garbage between frames here)."""
    old = ru.avr
    ru.avr = _beast_avr
    try:
        yield
    finally:
        ru.avr = old


ID_POOL = [0x1A00 + 0x0101010101 * k for k in range(12)] + [0x1A1A1A1A1A1A1A1A, 0, 0xFFFFFFFFFFFFFFFF, 0x001A001A001A001A]


def filler(rng, n, pool=ru.POOL, ids=True, first=0):
    """Ordinary traffic of a pool of aircraft (timestamps that count up, a receiver id from a small pool in front of every fifth)."""
    out = []
    for k in range(first, first + n):
        a = int(pool[rng.integers(0, len(pool))])
        kind = int(rng.integers(0, 8))
        f = ru.es(a, k) if kind < 3 else ru.df11(a) if kind == 3 else ru.ap((0, 4, 5, 16, 20, 21)[int(rng.integers(0, 6))], a, seed=k)
        ts, sig = 0x00191A000000 + 26 * 257 * k, (k * 13) & 0xFF
        x = frame_of_df(f, ts=ts, sig=sig)
        if kind == 7:
            x = frame(bytes([0x1A if k % 3 == 0 else k & 0xFF, (k >> 3) & 0xFF]), ts=ts, sig=sig)
        if ids and k % 5 == 0:
            x = prefix(ID_POOL[int(rng.integers(0, len(ID_POOL)))]) + x
        out.append(x)
    return out


def pad_to(parts, total, rng, ids=True, period=1 << 30):
    """Filler traffic behind the cases until the stream has `total` bytes at least (period: the traffic repeats, which a golden file
    compresses well)."""
    have = sum(len(x) for x in parts)
    k = 0
    while have < total:
        x = filler(np.random.default_rng(k % period), 1, ids=ids, first=k % period)[0] if k % 9 else (b"\x00garbage\xff", b"\x1aW", b"\x1a\x1a", pong(), position())[k // 9 % 5]
        parts.append(x)
        have += len(x)
        k += 1
    return parts


A = ru.A


def group_a():
    """The framing matrix."""
    rng = np.random.default_rng(21)
    long_, short, ac = ru.es(A, 3)[:14].tobytes(), ru.df11(A)[:7].tobytes(), b"\x77\x00"
    good = frame(long_)
    g = [frame(long_), frame(short), frame(ac), position(), pong(), b"\x1aWO", b"\x1aWx", b"\x1aW"]
    for t in (b"4", b"H", b"0", b"\x00", b"\xff", b"6", b"p", b"w"):               # unknown types: two bytes of garbage
        g += [b"\x1a" + t + long_, good]
    # 0x1a in every field position of every type, escaped
    for msg in (ac, short, long_):
        for at in range(6 + 1 + len(msg)):
            body = bytearray(int(0x0123456789AB).to_bytes(6, "big") + b"\x80" + msg)
            body[at] = 0x1A
            t = {2: b"1", 7: b"2", 14: b"3"}[len(msg)]
            g.append(b"\x1a" + t + esc(body))
            # ... and unescaped: the frame is abandoned at it; the 0x1a starts a valid frame where the next byte is a type
            g.append(b"\x1a" + t + bytes(body[: at + 1]) + good[1:])
            g.append(b"\x1a" + t + bytes(body))
    for at in range(21):
        p = bytearray(range(0x40, 0x40 + 21))
        p[at] = 0x1A
        g += [position(bytes(p)), b"\x1a5" + bytes(p), good]
    for at in range(3):
        p = bytearray(b"\x01\x02\x03")
        p[at] = 0x1A
        g += [pong(bytes(p)), b"\x1aP" + bytes(p), good]
    g += [frame(b"\x1a" * 14, ts=0x1A1A1A1A1A1A, sig=0x1A), frame(b"\x1a" * 7, ts=0x1A1A1A1A1A1A, sig=0x1A), frame(b"\x1a\x1a", ts=0x1A1A1A1A1A1A, sig=0x1A), MAXIMAL]
    # runs of 0x1a in front of a valid frame
    for n in range(1, 8):
        g += [b"\x1a" * n + good, b"\x1a" * n + good[1:]]
    # 0x1a and every second byte (0xe4 and 0xe8 stop: not here)
    for b in range(256):
        if b not in (0xE4, 0xE8):
            g += [bytes([0x1A, b]), frame(short, ts=b)]
    # receiver ids: every byte 0x1a, escaped and not; in front of every type; not followed by 0x1a; followed by another prefix, 0xe8
    for at in range(8):
        rid = bytearray(int(0x1122334455667788).to_bytes(8, "big"))
        rid[at] = 0x1A
        g += [b"\x1a\xe3" + esc(rid) + good, b"\x1a\xe3" + bytes(rid) + good, good]
    for behind in (frame(long_), frame(short), frame(ac), position(), pong(), b"\x1aWO", b"\x1a4", b"xyz", b"", prefix(0x99) + good, b"\x1a\xe8" + bytes(8) + good,
                   b"\x1a\xe3", b"\x1a\x1a"):
        g += [prefix(0x0A0B0C0D0E0F1011 + len(g)) + behind, good]
    # garbage runs
    for n in (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300):
        g += [bytes(rng.integers(0x20, 0x7F, n, dtype=np.uint8)), good]
    pad_to(g, 3 * TILE + 500, rng, period=60)
    g.append(MAXIMAL[:40])                                                                    # an incomplete frame at the end
    return g


def group_e():
    """Receiver ids: prefixes at the ends of tiles, in a row, abandoned; the same stream with and without net_ingest."""
    rng = np.random.default_rng(25)
    g = [prefix(0xA1)]
    for tile in (1, 2, 3):
        pad_to(g, tile * TILE - 140, rng, ids=False, period=25)
        for k in range(8):                                                                   # prefixes across the tile's edge
            g += [prefix(0x1A1A000000000000 + 256 * tile + k), frame(ru.es(A, k)[:14].tobytes(), sig=k)]
    g += [prefix(1), prefix(2), prefix(3) + b"zz", prefix(0x1A, escape=False) + frame(b"\x12\x34"), frame(b"\x12\x35")]
    pad_to(g, 3 * TILE + 2000, rng, ids=True, period=35)
    return g


def build_groups():
    with _as_beast():
        b, c, d, d2 = ru.group_b(), ru.group_c(), ru.group_d()[0], ru.group_d2()
    # group c's cases end in its third tile: three tiles and a little of its filler are kept
    have, keep = 0, 0
    while have < 3 * TILE + 300:
        have += len(c[keep])
        keep += 1
    c = c[:keep]
    return {"a": group_a(), "b": b, "c": c, "d": d, "d2": d2, "e": group_e()}


def group_d_info():
    """-> (frames, L*, the second growth, probes) of group d: the indices are handler calls."""
    with _as_beast():
        return ru.group_d()


def stream_of(parts):
    return b"".join(parts)


def ops_of(group):
    return ru.D_OPS if group in ("d", "d2") else []


def draw_stream(rng, nframes, hostile=0.15):
    """Traffic with damage: bytes overwritten (often with 0x1a), inserted, dropped; garbage; a cut at the end."""
    s = bytearray(stream_of(filler(rng, nframes, first=int(rng.integers(0, 1000)))))
    for _ in range(int(hostile * nframes)):
        at = int(rng.integers(0, max(1, len(s))))
        kind = int(rng.integers(0, 6))
        if kind == 0:
            s[at: at + 1] = b"\x1a"
        elif kind == 1:
            s[at: at + 1] = bytes(rng.integers(0, 256, 1, dtype=np.uint8))
        elif kind == 2:
            s[at:at] = bytes(rng.choice(np.array([0x1A, 0x1A, 0xE3, 0x31, 0x32, 0x33, 0x35, 0x50, 0x57, 0x00], dtype=np.uint8), int(rng.integers(1, 4))))
        elif kind == 3:
            del s[at: at + int(rng.integers(1, 5))]
        elif kind == 4:
            s[at:at] = bytes(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8)).replace(b"\x1a", b"\x19")
        else:
            s[at:at] = (b"\x1aW", b"\x1a\x1a", b"\x1a", pong(), position(), prefix(int(rng.integers(0, 1 << 62))))[int(rng.integers(0, 6))]
    cut = int(rng.integers(0, 70))
    if cut and int(rng.integers(0, 2)):
        del s[len(s) - min(cut, len(s)):]
    if int(rng.integers(0, 8)) == 0:
        s += bytes(int(rng.integers(200, 320)))                                              # a trailing run without 0x1a around the tail rule's 256
    return bytes(s)


# ---- the reference ----

def have_ref_full():
    return sbs_util.have_ref_full()


def build_ref_harness(workdir):
    """tests/host_stub/beast_in_ref_harness.c compiled with the flags of `make -C oracle full` and linked against that build's other
    objects, readsb.o with its main renamed in a copy (as tests/raw_in_util.py builds its harness)."""
    return ru.build_ref_harness(workdir, "beast_in", HARNESS_SRC)


def parse_results(blob, n):
    """n results as the harness writes them -> [dict(head, cls, off, frame_of, ids, signal, msgs)]"""
    return ru.read_results(blob, n, 12, (("cls", np.uint8), ("off", np.uint64)),
                           (("frame_of", np.uint64), ("ids", np.uint64), ("signal", np.float64), ("msgs", MSG)))


def run_ref_harness(exe, streams, cfg, workdir, ops=(), now_ms=NOW_MS, reps=1, id_in=ID_IN):
    """The reference over the streams, one after the other against one filter prepared by ops -> a result per stream"""
    paths = []
    for k, s in enumerate(streams):
        paths.append(os.path.join(workdir, "beast_in_stream%d.bin" % k))
        open(paths[-1], "wb").write(s)
    fpath = os.path.join(workdir, "beast_in_filter.bin")
    np.asarray(list(ops), dtype=np.int32).tofile(fpath)
    r = subprocess.run([exe, str(int(now_ms)), *[str(x) for x in cfg], str(int(id_in)), fpath, str(int(reps)), *paths], check=True, capture_output=True, timeout=600)
    return parse_results(r.stdout, len(streams))


def load_golden():
    """-> {key(group, cfg): dict(stream, head, cls, off, frame_of, ids, signal, msgs)}"""
    z = np.load(GOLDEN)
    out = {}
    for g, cfgs in CONFIGS.items():
        for cfg in cfgs:
            k = key(g, cfg)
            out[k] = dict(stream=z[g + "_stream"].tobytes(), head=z[k + "_head"], cls=z[k + "_class"], off=np.cumsum(z[k + "_off"].astype(np.uint64), dtype=np.uint64),
                          frame_of=np.cumsum(z[k + "_frame_of"].astype(np.uint64), dtype=np.uint64), ids=z[k + "_ids"], signal=z[k + "_signal"], msgs=z[k + "_msgs"].view(MSG).reshape(-1))
    return out


# ---- the library's host side ----

def beast_args(binding, buf, nbytes, arrays, outs, cn, now_ms=NOW_MS, id_in=ID_IN, net_ingest=0, msgs_cap=None, frames_cap=None, pass_bytes=0, pointers=None):
    """struct mgpu_beast_in_args over numpy arrays (or raw pointers): arrays = dict(msgs, ids, signal, frame_of, cls, off), any of the
    optional ones None; outs = (consumed, nframes, nmsgs, stop, stop_off, id_out) ctypes values."""
    p = pointers or {k: (v.ctypes.data if v is not None else None) for k, v in arrays.items()}
    return binding.BeastInArgs(C.sizeof(binding.BeastInArgs), 0, buf, nbytes, int(now_ms), int(id_in), int(net_ingest), 0, p["msgs"], p["ids"], p["signal"], p["frame_of"],
                               msgs_cap if msgs_cap is not None else len(arrays["msgs"]), p["cls"], p["off"], frames_cap if frames_cap is not None else len(arrays["cls"]),
                               C.pointer(outs[0]), C.pointer(outs[1]), C.pointer(outs[2]), C.pointer(outs[3]), C.pointer(outs[4]), C.pointer(outs[5]), C.pointer(cn),
                               int(pass_bytes))


def new_outs():
    return (C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0))


def result_of(binding, rc, arrays, outs, cn):
    n, nf = int(outs[2].value), int(outs[1].value)
    m, f = min(n, len(arrays["msgs"])), min(nf, len(arrays["cls"]))
    return dict(rc=rc, consumed=int(outs[0].value), nframes=nf, nmsgs=n, stop=int(outs[3].value), stop_off=int(outs[4].value), id_out=int(outs[5].value),
                counters=binding.beast_in_counters_dict(cn), msgs=arrays["msgs"][:m], ids=arrays["ids"][:m], signal=arrays["signal"][:m], frame_of=arrays["frame_of"][:m],
                cls=arrays["cls"][:f], off=arrays["off"][:f])


def new_arrays(nbytes):
    cap, fcap = nbytes // 11 + 1, nbytes // 5 + 1
    return dict(msgs=np.zeros(cap, dtype=MSG), ids=np.zeros(cap, dtype=np.uint64), signal=np.zeros(cap, dtype=np.float64), frame_of=np.zeros(cap, dtype=np.uint64),
                cls=np.zeros(fcap, dtype=np.uint8), off=np.zeros(fcap, dtype=np.uint64))


def host_decode(lib, stream, cfg, filt=None, now_ms=NOW_MS, id_in=ID_IN):
    """mgpu_beast_decode_host: the sequential walk.  cfg = (nfix_crc, fixDF, mode_ac, net_ingest); filt: a raw_in_util.FilterModel,
    moved on by the call."""
    from readsb_amd import binding
    buf = np.frombuffer(bytes(stream) + b"\xee", dtype=np.uint8)                             # (a byte behind the stream that nothing may read as the stream's)
    arrays, outs, cn = new_arrays(len(stream)), new_outs(), binding.BeastInCounters()
    a = beast_args(binding, buf.ctypes.data, len(stream), arrays, outs, cn, now_ms, id_in, cfg[3])
    kcfg = binding.RawInConfig(C.sizeof(binding.RawInConfig), *cfg[:3])
    rc = ru.through_filter(filt, len(stream) // 11 + 2, lambda f: lib.mgpu_beast_decode_host(C.byref(a), C.byref(kcfg), f))
    return result_of(binding, rc, arrays, outs, cn)


def parse_host(lib, stream, offset, cfg, now_ms=NOW_MS):
    """mgpu_beast_parse_host -> (rc, binding.BeastInFrame)"""
    from readsb_amd import binding
    buf = stream if isinstance(stream, np.ndarray) else np.frombuffer(bytes(stream), dtype=np.uint8)
    kcfg = binding.BeastInConfig(C.sizeof(binding.BeastInConfig), cfg[0], cfg[1], cfg[2], cfg[3], 0)
    out = binding.BeastInFrame()
    rc = int(lib.mgpu_beast_parse_host(buf.ctypes.data, len(stream), int(offset), int(now_ms), C.byref(kcfg), C.byref(out)))
    return rc, out


def walk_host(lib, stream, cfg, now_ms=NOW_MS):
    """readBeast's loop restated over mgpu_beast_parse_host alone (no filter): -> dict(consumed, stop, garbage, nframes, frames:
    [(offset, class)], id_sets, commands) — the plain walk the sequential resolver must agree with."""
    stream = np.frombuffer(bytes(stream), dtype=np.uint8)
    n, som, pending, garbage, frames, ids, cmds, stop, left = len(stream), 0, 0, 0, [], 0, 0, STOP_END, False
    while som < n:
        rc, f = parse_host(lib, stream, som, cfg, now_ms)
        assert rc in (0, 1)
        if f.step == STEP_GARBAGE:
            pending += 1
            som = f.next
            continue
        garbage += pending + f.garbage
        pending = 0
        ids += f.id_set
        cmds += f.command
        som = f.next
        if f.step == STEP_INCOMPLETE:
            left = True
            break
        if f.step in (STEP_SYNTH, STEP_UUID):
            left, stop = True, STOP_SYNTH if f.step == STEP_SYNTH else STOP_UUID
            break
        if f.step == STEP_FRAME:
            frames.append((int(f.frame_off), int(f.cls)))
    if not left:
        som = n - pending
    if stop == STOP_END and n - som > TAIL:
        garbage += n - som
        som = n
    return dict(consumed=som, stop=stop, garbage=garbage, nframes=len(frames), frames=frames, id_sets=ids, commands=cmds)


def cut_at_stop(lib, stream, cfg):
    """The stream cut in front of its first stop (the reference closes the client or reads a UUID there)."""
    w = walk_host(lib, stream, cfg)
    return stream if w["stop"] == STOP_END else stream[: w["consumed"]]


def compare(res, ref, what=""):
    """A library result (result_of) against a reference result (parse_results / load_golden), bytewise."""
    head = [res["consumed"], res["nframes"], res["nmsgs"], res["counters"]["remote_received_modes"], res["counters"]["remote_received_modeac"],
            res["counters"]["remote_rejected_unknown_icao"], res["counters"]["remote_rejected_bad"], *res["counters"]["remote_accepted"],
            res["counters"]["remote_malformed_beast"], res["id_out"]]
    assert head == [int(x) for x in ref["head"]], (what, dict(zip(HEAD, head)), dict(zip(HEAD, [int(x) for x in ref["head"]])))
    assert res["cls"].tobytes() == ref["cls"].tobytes(), (what, "class", np.flatnonzero(res["cls"] != ref["cls"])[:10])
    assert res["off"].tobytes() == ref["off"].astype(np.uint64).tobytes(), (what, "frame_off")
    assert res["frame_of"].tobytes() == ref["frame_of"].astype(np.uint64).tobytes(), (what, "frame_of")
    assert res["ids"].tobytes() == ref["ids"].astype(np.uint64).tobytes(), (what, "receiver ids", np.flatnonzero(res["ids"] != ref["ids"])[:10])
    assert res["signal"].tobytes() == ref["signal"].tobytes(), (what, "signal")
    assert res["msgs"].tobytes() == ref["msgs"].tobytes(), (what, "msgs", np.flatnonzero(res["msgs"] != ref["msgs"])[:10])
