"""ASTERIX input (readAsterix + decodeAsterixMessage over a length-chained stream): the record builder and the case generators behind
tests/golden/asterix_in_cases.npz, the golden's loader, the reference harness (tests/host_stub/asterix_in_ref_harness.c, which includes
the reference's net_io.c and links oracle/_ref/full's other objects), the framing rule restated in Python and what the tests expect of
a stream.  A case is one or more records; a group is one stream."""
import ctypes as C
import os
import subprocess

import numpy as np

import helpers
import sbs_util

GOLDEN = os.path.join(helpers.GOLDEN_DIR, "asterix_in_cases.npz")
HARNESS_SRC = os.path.join(helpers.ROOT, "tests", "host_stub", "asterix_in_ref_harness.c")
GROUPS = ("a", "b", "c1", "c2")
# 2023-11-14 22:15:23.456 and 2026-10-20 00:00:00.999: one second into a day, so a stamp of the evening belongs to the day before
# (readAsterixTime's rule at 12 hours)
NOWS = (1700000123456, 1792454400999)
SOURCE = 1                                      # SOURCE_INDIRECT: remote < 64
TILE = 65536                                    # kAstTile of kernels.h
GROUP_TILES = 32                                # kAstGroup
MGPU_OK, MGPU_E_INVAL, MGPU_E_OVERFLOW = 0, -1, -5
STOP_END, STOP_ZERO_LEN, STOP_CLOSED = 0, 1, 2
REC = np.dtype([("sysTimestamp", "<i8"), ("decoded_lat", "<f8"), ("decoded_lon", "<f8"), ("mach", "<f8"), ("addr", "<u4"), ("flags", "<u4"), ("ast_flags", "<u4"),
                ("baro_alt", "<i4"), ("geom_alt", "<i4"), ("baro_rate", "<i4"), ("geom_rate", "<i4"), ("ias", "<u4"), ("tas", "<u4"), ("squawkHex", "<u4"),
                ("squawkDec", "<u4"), ("category", "<u4"), ("mcp_altitude", "<u4"), ("fms_altitude", "<u4"), ("gs_v0", "<f4"), ("heading", "<f4"), ("roll", "<f4"),
                ("callsign", "S8"), ("source", "u1"), ("addrtype", "u1"), ("airground", "u1"), ("emergency", "u1"), ("nav_modes", "u1"), ("nac_v", "u1"),
                ("nac_p", "u1"), ("sil", "u1"), ("sil_type", "u1"), ("gva", "u1"), ("sda", "u1"), ("nic_baro", "u1"), ("op_version", "u1"), ("heading_type", "u1"),
                ("baro_alt_unit", "u1"), ("geom_alt_unit", "u1"), ("reserved", "u1", 4)])
assert REC.itemsize == 128

# the items in the order decodeAsterixMessage reads them (net_io.c:1950-2396): name, FSPEC byte, bit
ITEMS = (("010", 0, 0x80), ("040", 0, 0x40), ("161", 0, 0x20), ("015", 0, 0x10), ("071", 0, 0x08), ("130", 0, 0x04), ("131", 0, 0x02),
         ("072", 1, 0x80), ("150", 1, 0x40), ("151", 1, 0x20), ("080", 1, 0x10), ("073", 1, 0x08), ("074", 1, 0x04), ("075", 1, 0x02),
         ("076", 2, 0x80), ("140", 2, 0x40), ("090", 2, 0x20), ("210", 2, 0x10), ("070", 2, 0x08), ("230", 2, 0x04), ("145", 2, 0x02),
         ("152", 3, 0x80), ("200", 3, 0x40), ("155", 3, 0x20), ("157", 3, 0x10), ("160", 3, 0x08), ("165", 3, 0x04), ("077", 3, 0x02),
         ("170", 4, 0x80), ("020", 4, 0x40), ("220", 4, 0x20), ("146", 4, 0x10))
SIZES = {"010": 2, "161": 2, "015": 1, "071": 3, "130": 6, "131": 8, "072": 3, "150": 2, "151": 2, "080": 3, "073": 3, "074": 4, "075": 3, "076": 4, "140": 2,
         "210": 1, "070": 2, "230": 2, "145": 2, "152": 2, "200": 1, "155": 2, "157": 2, "160": 4, "165": 2, "077": 3, "170": 6, "020": 1, "146": 2}
EMITTERS = (0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 13, 14, 15, 16, 20, 21, 22, 23, 24)


def len_bytes(length):
    """The two bytes readAsterix's sign-extending expression (:4647) turns into `length`."""
    lo = length & 0xff
    hi = ((length - (lo - 256 if lo >= 128 else lo)) >> 8) & 0xff
    return bytes([hi, lo])


def read_len(hi, lo):
    return ((hi - 256 if hi >= 128 else hi) * 256 + (lo - 256 if lo >= 128 else lo)) & 0xffff


def frame(items, cat=21, length=None, pad=0, fspec_bytes=None):
    """One record: items {name: bytes} in the reader's order behind an FSPEC of their bits; length: what the header says (default: what
    it is, with `pad` bytes of zeros behind the items)."""
    f = [0] * 5
    body = b""
    for name, byte, bit in ITEMS:
        if name in items:
            f[byte] |= bit
            body += items[name]
    n = fspec_bytes or max([i for i in range(5) if f[i]] + [1]) + 1
    fspec = bytes((f[i] | (1 if i < n - 1 else 0)) for i in range(n))
    payload = fspec + body + b"\0" * pad
    return bytes([cat]) + len_bytes(3 + len(payload) if length is None else length) + payload


def chain(nbytes, rng=None):
    """An extension chain of nbytes bytes (nbytes - 1 extension bytes): every byte but the last has its low bit set."""
    vals = rng.integers(0, 128, nbytes) * 2 if rng is not None else np.zeros(nbytes, dtype=np.int64)
    vals[:-1] |= 1
    return bytes(int(v) for v in vals)


def be(value, n):
    return int(value).to_bytes(n, "big", signed=False)


def tod(now_ms, delta_ms=0):
    """I021/07x: 1/128 s since midnight of the moment now_ms + delta_ms."""
    return be(((now_ms + delta_ms) % 86400000) * 128 // 1000 % (1 << 24), 3)


def ordinary(rng, now_ms, k):
    """A well-formed target report: drawn items with drawn, sensible values."""
    r = lambda n: int(rng.integers(0, n))                                                          # noqa: E731
    it = {"080": be(0x400000 + r(0x3fffff), 3)}
    if r(4):
        it["010"] = bytes([r(256), r(256)])
    if r(5):
        it["040"] = (bytes([(r(4) << 5) | (r(4) << 3) | 1, (r(2) << 6) | (r(2) << 5)]) if r(2) else bytes([(r(8) << 5) | (r(4) << 3)]))
    if r(3) == 0:
        it["161"] = be(r(4096), 2)
    if r(3) == 0:
        it["015"] = bytes([r(256)])
    if r(3) == 0:
        it["071"] = tod(now_ms, r(4000) - 2000)
    if r(4):
        it["130"] = be((r(170 << 15) - (85 << 15)) % (1 << 24), 3) + be((r(350 << 15) - (175 << 15)) % (1 << 24), 3)
    elif r(2):
        it["131"] = be((r(170 << 22) - (85 << 22)) % (1 << 32), 4) + be((r(350 << 22) - (175 << 22)) % (1 << 32), 4)
    if r(4) == 0:
        it["072"] = tod(now_ms, r(4000) - 2000)
    if r(3) == 0:
        it["150"] = be((r(2) << 15) | r(2000), 2)
    if r(3) == 0:
        it["151"] = be((r(8) == 0) << 15 | r(600), 2)
    if r(2):
        it["073"] = tod(now_ms, -r(1500))
        if r(2):
            it["074"] = be((r(3) << 30) | r(1 << 30), 4)
    if r(2):
        it["075"] = tod(now_ms, -r(1500))
        if r(2):
            it["076"] = be((r(3) << 30) | r(1 << 30), 4)
    if r(2):
        it["140"] = be((r(8000) - 200) % 65536, 2)
    if r(3):
        it["090"] = (bytes([r(256) & ~1]), bytes([r(256) | 1, r(256) & ~1]), bytes([r(256) | 1, r(256) | 1, r(256) & ~1]), bytes([r(256) | 1, r(256) | 1, r(256) | 1, r(128) * 2]))[r(4)]
    if r(3):
        it["210"] = bytes([(r(2) << 6) | ((0, 1, 2, 2, 2, 3)[r(6)] << 3) | (0, 1, 2, 2, 2, 5)[r(6)]])
    if r(3) == 0:
        it["070"] = be(r(4096), 2)
    if r(4) == 0:
        it["230"] = be((r(6000) - 3000) % 65536, 2)
    if r(3):
        it["145"] = be((r(1800) - 40) % 65536, 2)
    if r(5) == 0:
        it["152"] = be(r(65536), 2)
    if r(3) == 0:
        it["200"] = bytes([r(256)])
    if r(3) == 0:
        it["155"] = be((r(8) == 0) << 15 | r(1 << 15), 2)
    if r(3) == 0:
        it["157"] = be((r(8) == 0) << 15 | r(1 << 15), 2)
    if r(2):
        it["160"] = be((r(8) == 0) << 15 | r(2500), 2) + be(r(65536), 2)
    if r(5) == 0:
        it["165"] = be(r(1024), 2)
    if r(2):
        it["077"] = tod(now_ms, -r(500))
    if r(3) == 0:
        cs = 0
        for ch in ("DLH%d" % r(9999)).ljust(8)[:8]:
            cs = cs << 6 | (ord(ch) & 0x3f)
        it["170"] = be(cs, 6)
    if r(3) == 0:
        it["020"] = bytes([EMITTERS[r(len(EMITTERS))]])
    if r(8) == 0:
        it["220"] = chain(1 + r(3), rng)
    if r(4) == 0:
        it["146"] = be((r(2) << 15) | (r(4) << 13) | r(1 << 13), 2)
    return frame(it)


def every_item(rng):
    """Every item with drawn bytes (chains: two bytes)."""
    it = {name: bytes(int(x) for x in rng.integers(0, 256, n)) for name, n in SIZES.items()}
    for name in ("040", "090", "220"):
        it[name] = chain(2, rng)
    return it


def build_groups():
    """-> {group: [record bytes, ...]}: seeded, so the golden's maker and the live check build the same streams."""
    rng = np.random.default_rng(21021)
    r = lambda n: int(rng.integers(0, n))                                                          # noqa: E731
    g = {k: [] for k in GROUPS}
    a, b = g["a"], g["b"]
    addr = {"080": b"\x4a\xc8\xb3"}
    now = NOWS[0]
    # (a) well-formed records
    full = every_item(rng)
    for name, _, _ in ITEMS:                                                                       # every FSPEC bit alone (beside the address) and all but it
        a.append(frame({**addr, name: full[name]}))
        a.append(frame({k: v for k, v in full.items() if k != name or k == "080"}))
    for k in range(400):
        a.append(ordinary(rng, NOWS[k % 2], k))
    a.append(frame({**addr, "130": be(0x400000, 3) + be(0x800000, 3)}))                            # 90, -180
    a.append(frame({**addr, "130": be(0x400001, 3) + be(0, 3)}))                                   # beyond 90: no position
    a.append(frame({**addr, "130": be(0xc00000, 3) + be(0x7fffff, 3)}))
    a.append(frame({**addr, "131": be(0x20000000, 4) + be(0xc0000000, 4)}))                        # 90, -180
    a.append(frame({**addr, "131": be(0x20000001, 4) + be(0x40000000, 4)}))
    a.append(frame({**addr, "131": be(0xe0000000, 4) + be(0x80000000, 4), "130": be(0x123456, 3) + be(0xfedcba, 3)}))
    for raw in (0, 1, 999, 1000, 0x7fff, 0x8000, 0x8001, 0x8355, 0xffff, 0x4000, 0x0123):          # Mach and IAS
        a.append(frame({**addr, "150": be(raw, 2), "075": tod(now)}))
        a.append(frame({**addr, "151": be(raw, 2)}))
    for q in (b"\x00", b"\xfe", b"\x21\x00", b"\xe1\xfe", b"\x01\x01\x00", b"\xff\xff\x3e", b"\x01\xff\x00", b"\x01\x81\x20\x00", b"\x01\x01\x19\xf0", b"\xff\xff\xff\xff\xfe"):
        a.append(frame({**addr, "090": q}))                                                        # every I021/090 shape, alone and in front of every I021/210
        for v in range(64):
            if v % 8 in (0, 1, 2, 3, 7) or q == b"\xff\xff\x3e":
                a.append(frame({**addr, "090": q, "210": bytes([v]), "040": bytes([(v % 5) << 5])}))
    for v in (0x00, 0x0a, 0x11, 0x52, 0x93, 0xff):
        a.append(frame({**addr, "210": bytes([v])}))
    for e in list(EMITTERS) + [7, 8, 9, 17, 19, 25, 100, 255]:
        a.append(frame({**addr, "020": bytes([e])}))
    for src in range(4):                                                                           # I021/146: SAS, the source, the altitude's sign
        for sas in (0, 1):
            for alt in (0, 1, 0x0fff, 0x1000, 0x1fff, 1400):
                a.append(frame({**addr, "146": be(sas << 15 | src << 13 | alt, 2)}))
    for name in ("155", "157"):
        for raw in (0, 1, 0x3fff, 0x4000, 0x7fff, 0x8000, 0xffff, 0x0140, 0x7ec0):
            a.append(frame({**addr, name: be(raw, 2)}))
    for raw in (0, 0x7fff, 0x8000, 0xffff, 0x1234):
        a.append(frame({**addr, "160": be(raw, 2) + be(0xc000, 2)}))
        a.append(frame({**addr, "152": be(raw, 2), "160": be(raw, 2) + be(0x4000, 2)}))
        a.append(frame({**addr, "140": be(raw, 2), "230": be(raw, 2), "145": be(raw, 2)}))
    for raw in (0xff10, 0xff0f, 4000, 24000, 24001):                         # I021/140's range: -1500 .. 150000 ft
        a.append(frame({**addr, "140": be(raw, 2)}))
    for v in range(0, 256, 3):
        a.append(frame({**addr, "200": bytes([v]), "070": be(v * 257 & 0xffff, 2)}))
    for cs in (0, (1 << 48) - 1, 0x041041041041, 0x820820820820, 0xb2cb2cb2cb2c, 0x6db6db6db6db, 0xc30c30c30c30, 0xe79e79e79e79, 0x0c2d35c71c60, 0x820820820fe0):
        a.append(frame({**addr, "170": be(cs, 6)}))
    pos = {"130": be(0x2468ac, 3) + be(0x013579, 3)}
    for nw in NOWS:                                                                                # the three times, high precision, every FSI, across midnight
        for delta in (0, -1000, 1000, -43199000, 43199000, -43201000, 43201000, -86399000, -(nw % 86400000), -(nw % 86400000) - 8, 86400000 - nw % 86400000 - 8):
            t = tod(nw, delta)
            a += [frame({**addr, "071": t}), frame({**addr, "072": t}), frame({**addr, "077": t}), frame({**addr, "071": tod(nw), "072": t, "077": t}),
                  frame({**addr, "073": t}), frame({**addr, **pos, "073": t}), frame({**addr, "075": t}), frame({**addr, "150": b"\x01\x00", "075": t}),
                  frame({**addr, "150": b"\x81\x00", "075": t, "077": tod(nw)}), frame({**addr, **pos, "073": t, "075": tod(nw), "150": b"\x01\x00"})]
            for fsi in range(4):
                hp = be(fsi << 30 | r(1 << 30), 4)
                a += [frame({**addr, **pos, "073": t, "074": hp}), frame({**addr, "073": t, "074": hp}), frame({**addr, "150": b"\x00\x50", "075": t, "076": hp}),
                      frame({**addr, "075": t, "076": hp}), frame({**addr, **pos, "071": tod(nw), "073": t, "074": hp}), frame({**addr, "074": hp, "076": hp})]
        for raw in (0, 1, 15, 16, 17, 0x7fffff, 0x800000, 0xa8c000 - 1, 0xa8c000, 0xa8c001, 0xffffff):   # 0xa8c000 / 128 = 86400 s
            a.append(frame({**addr, "071": be(raw, 3)}))
            a.append(frame({**addr, **pos, "073": be(raw, 3), "074": be(0x3fffffff, 4)}))
    # (b) hostile but defined
    for k in range(300):                                                                           # drawn item bytes behind a consistent header
        it = every_item(rng)
        keep = {name: v for name, v in it.items() if name == "080" or r(2)}
        b.append(frame(keep))
    for k in range(100):                                                                           # a drawn FSPEC and drawn bytes, the length consistent
        fs = bytes([r(256) | 1, r(256) | 0x11, r(256) | 1, r(256) | 1, r(256) & ~1]) if r(2) else bytes([r(256) | 1, (r(256) | 0x10) & ~1])
        body = bytes(int(x) for x in rng.integers(0, 256, 20 + r(80)))
        if fs[0] & 0x40:                                                                           # (no drawn chain longer than the allocation)
            body = chain(1 + r(3), rng) + body
        payload = fs + (b"\0\0" if fs[0] & 0x80 else b"") + body
        b.append(bytes([21]) + len_bytes(3 + len(payload)) + payload + b"\0" * 0)
    for total in (0x80, 0xff, 0x100, 0x17f, 0x180, 0x7f80, 0x8000, 0x807f, 0x8080):                # low and high length bytes of 0x80 or more
        b.append(frame({**addr, "145": be(400, 2)}, pad=total - 11))
        assert len(b[-1]) == total
    # records that end behind their FSPEC: the items are the bytes of the records that follow, which are framed as themselves
    b += [bytes([21]) + len_bytes(5) + b"\x0d\x10", frame({**addr, "145": be(40, 2)}), ordinary(rng, now, 0)]
    b += [bytes([21]) + len_bytes(8) + b"\xff\xff\xff\xff\xd0", ordinary(rng, now, 1), ordinary(rng, now, 2), ordinary(rng, now, 3), ordinary(rng, now, 4)]
    # len 3: the FSPEC is the next frame's header, 05 10 20: category 5, 0x1020 bytes
    b += [b"\x15\x00\x03", b"\x05\x10\x20" + bytes(int(x) for x in rng.integers(0, 256, 0x1020 - 3))]
    # len 1: the next frame starts at the length's high byte: 00 01 01, category 0, 0x0101 bytes, its third byte this record's FSPEC
    b += [b"\x15\x00\x01", b"\x01\x10\xaa\xbb\xcc" + b"\0" * (0x101 - 2 - 5)]
    # len 2: the next frame starts at the length's low byte: 02 01 10, category 2, 0x0110 bytes
    b += [b"\x15\x00\x02", b"\x01\x10\xaa\xbb\xcd" + b"\0" * (0x110 - 1 - 5)]
    for cat in (0, 1, 20, 22, 23, 34, 48, 62, 255, 128):                                           # other categories
        b.append(frame(every_item(rng), cat=cat))
        b.append(bytes([cat]) + len_bytes(3 + 40) + bytes(int(x) for x in rng.integers(0, 256, 40)))
    for name in ("040", "090", "220"):                                                             # chains of exactly 191 extension bytes: still defined
        b.append(frame({**addr, name: chain(192, rng), "145": be(123, 2)}))
        b.append(frame({**addr, name: chain(192), "070": be(0x0e55, 2)}))
    tail = bytes(int(x) | 1 for x in rng.integers(0, 256, 191 - 5))
    fs = bytes([0x05, 0x11, 0x03, 0x01, 0x11]) + tail + b"\x00"                                    # the main FSPEC: 191 extension bytes
    b.append(bytes([21]) + len_bytes(3 + len(fs) + 6 + 3 + 2 + 2) + fs + be(0x111111, 3) + be(0x222222, 3) + b"\xab\xcd\xef" + be(100, 2) + be(0xc064, 2))
    b.append(bytes([21]) + len_bytes(5) + b"\x0f\xfe")                                             # the last record's items lie past the end of the stream
    # (c1) the record without an address in the middle of a stream; (c2) a truncated tail
    g["c1"] = [ordinary(rng, now, k) for k in range(20)] + [frame({"145": be(77, 2), "170": be(1, 6)})] + [ordinary(rng, now, k) for k in range(5)]
    last = ordinary(rng, now, 0)
    g["c2"] = [ordinary(rng, now, k) for k in range(20)] + [last[: len(last) - 2]]
    return g


def stream_of(records):
    return b"".join(records)


def frames_of(stream):
    """The framing rule restated: -> (the starts of the consumed frames in order, ignoring MGPU_AST_STOP_CLOSED; where the chain ends;
    STOP_END or STOP_ZERO_LEN)."""
    n, at, starts = len(stream), 0, []
    while True:
        if n - at < 3:
            return starts, at, STOP_END
        length = read_len(stream[at + 1], stream[at + 2])
        if length == 0:
            return starts, at, STOP_ZERO_LEN
        if at + length > n:
            return starts, at, STOP_END
        starts.append(at)
        at += length


def closes(stream, at):
    """Is the frame at `at` the one MGPU_AST_STOP_CLOSED stops at: category 21, an FSPEC the allocation holds, no I021/080 bit."""
    if stream[at] != 21:
        return False
    get = lambda p: stream[p] if p < len(stream) else 0                                            # noqa: E731
    p, k = at + 3, 0
    while get(p + k) & 1:
        k += 1
        if k > 191:
            return False
    return not (get(p + 1) & 0x10 if k >= 1 else 0)


def expect(lib, stream, source=SOURCE, now_ms=NOWS[0]):
    """What a call makes of a stream, by the rule above and the library's host parser (mgpu_asterix_parse_record_host; no GPU)."""
    buf = np.frombuffer(bytes(stream) + b"\0", dtype=np.uint8)[: len(stream)]
    starts, end, stop = frames_of(stream)
    one = np.zeros(1, dtype=REC)
    recs, frame_of, nother, nundefined, consumed, nframes = [], [], 0, 0, end, len(starts)
    for k, at in enumerate(starts):
        if stream[at] != 21:
            nother += 1
            continue
        if closes(stream, at):
            consumed, stop, nframes = at + read_len(stream[at + 1], stream[at + 2]), STOP_CLOSED, k + 1
            break
        rc = int(lib.mgpu_asterix_parse_record_host(buf.ctypes.data, len(stream), at, source, now_ms, one.ctypes.data))
        assert rc in (0, 1), rc
        if rc:
            recs.append(one.copy())
            frame_of.append(k)
        else:
            nundefined += 1
    return dict(recs=np.concatenate(recs) if recs else np.zeros(0, dtype=REC), frame_of=np.array(frame_of, dtype=np.uint64), consumed=consumed, nframes=nframes,
                nother=nother, nundefined=nundefined, stop=stop)


def have_ref_full():
    return sbs_util.have_ref_full()


def build_ref_harness(workdir):
    """tests/host_stub/asterix_in_ref_harness.c compiled with the flags of `make -C oracle full` and linked against that build's other
    objects, readsb.o with its main renamed in a copy (as tests/sbs_util.py builds the writers' harness)."""
    exe = os.path.join(workdir, "asterix_in_ref_harness")
    main_o = os.path.join(workdir, "readsb_nomain_asterix_in.o")
    subprocess.run(["objcopy", "--redefine-sym", "main=readsb_main", os.path.join(sbs_util.REF_FULL, "readsb.o"), main_o], check=True)
    objs, flags = sbs_util._full_build()
    subprocess.run(["gcc", *flags, "-I" + os.path.join(helpers.ORACLE_DIR, "stub_full"), "-I/root/reference", "-I" + os.path.join(helpers.ROOT, "include"), HARNESS_SRC,
                    main_o, *[os.path.join(sbs_util.REF_FULL, o + ".o") for o in objs], "-o", exe, "-pthread", "-lpthread", "-lm", "-lrt", "-l:libzstd.so.1", "-lz"],
                   check=True)
    return exe


def run_ref_harness(exe, stream, workdir, source=SOURCE, now_ms=NOWS[0], reps=1):
    """-> (head = consumed, frames, records, other, stop; frame_of; records) as the reference leaves them"""
    path = os.path.join(workdir, "asterix_in_stream.bin")
    open(path, "wb").write(stream)
    r = subprocess.run([exe, path, str(int(source)), str(int(now_ms)), str(int(reps))], check=True, capture_output=True, timeout=600)
    head = np.frombuffer(r.stdout[:40], dtype=np.uint64)
    n = int(head[2])
    frame_of = np.frombuffer(r.stdout[40: 40 + 8 * n], dtype=np.uint64)
    recs = np.frombuffer(r.stdout[40 + 8 * n:], dtype=REC)
    assert len(recs) == n
    return head.copy(), frame_of.copy(), recs.copy()


def load_golden():
    """-> {group: (stream bytes, {now_ms: (head, frame_of, records)})}"""
    z = np.load(GOLDEN)
    return {g: (z[g + "_stream"].tobytes(), {nw: (z[f"{g}_{k}_head"], z[f"{g}_{k}_frame_of"].astype(np.uint64), z[f"{g}_{k}_recs"].view(REC)) for k, nw in enumerate(NOWS)})
            for g in GROUPS}


def feed(nrecords, seed=1, now_ms=NOWS[0]):
    """A drawn feed of well-formed records."""
    rng = np.random.default_rng(seed)
    return [ordinary(rng, now_ms, k) for k in range(nrecords)]


def load_host_lib():
    import readsb_amd.binding as rb
    return rb.load_library()


def args_for(rb, buf, source, now_ms, recs=None, frame_of=None, cap=0, pass_bytes=0):
    """An AsterixInArgs over numpy arrays / device addresses, with fresh counters: -> (args, counters dict of ctypes values)"""
    c = dict(consumed=C.c_uint64(0), nframes=C.c_uint64(0), nrecs=C.c_uint64(0), stop=C.c_uint32(99), nother=C.c_uint64(0), nundefined=C.c_uint64(0))
    a = rb.AsterixInArgs(C.sizeof(rb.AsterixInArgs), int(source), buf[0], buf[1], int(now_ms), recs, frame_of, cap, int(pass_bytes), C.pointer(c["consumed"]),
                         C.pointer(c["nframes"]), C.pointer(c["nrecs"]), C.pointer(c["stop"]), C.pointer(c["nother"]), C.pointer(c["nundefined"]))
    return a, c
