"""Raw input (decodeHexMessage + the front of decodeModesMessage over AVR lines): the case generators behind
tests/golden/raw_in_cases.npz, the golden's loader, the reference harness (tests/host_stub/raw_in_ref_harness.c, which includes the
reference's net_io.c and links oracle/_ref/full's other objects), a model of icao_filter.c's add / expire / growth for placing the
growth cases, and the library's host side (mgpu_raw_decode_host) for built streams.  A group is one stream of 40 to 60 KB (5 to 7
tiles of 8192 bytes) and the configurations it is run under."""
import ctypes as C
import os
import subprocess

import numpy as np

import frames_util as fr
import helpers
import sbs_util

GOLDEN = os.path.join(helpers.GOLDEN_DIR, "raw_in_cases.npz")
HARNESS_SRC = os.path.join(helpers.ROOT, "tests", "host_stub", "raw_in_ref_harness.c")
NOW_MS = 1700000123456
TILE = 8192                                     # kUatTile of kernels.h
CHUNK = 32                                      # bytes of a tile whose line starts one lane takes
MGPU_OK, MGPU_E_INVAL, MGPU_E_OVERFLOW = 0, -1, -5
NONE, MODEAC, BAD, ACCEPT, COND, UNKNOWN = range(6)                                          # MGPU_RAW_*
MSG = np.dtype([("timestamp", "<i8"), ("sysTimestamp", "<i8"), ("sig_sumsq", "<u8"), ("sig_len", "<u2"), ("score", "<i2"), ("phase", "u1"), ("correctedbits", "u1"),
                ("msgtype", "u1"), ("msgbits", "u1"), ("addr", "<u4"), ("msg", "u1", 14), ("raw", "u1", 14)])
assert MSG.itemsize == 64
COUNTERS = ("remote_received_modes", "remote_received_modeac", "remote_rejected_unknown_icao", "remote_rejected_bad", "remote_accepted0", "remote_accepted1",
            "remote_accepted2")
# (nfix_crc, fixDF, mode_ac) per group; group d also prepares the filter
CONFIGS = {"a": ((1, 1, 0), (1, 1, 1)), "b": ((0, 1, 0), (1, 1, 0), (2, 1, 0), (1, 0, 0)), "c": ((1, 1, 0),), "d": ((1, 1, 0),), "d2": ((1, 1, 0),)}
GROUPS = ("a", "b", "c", "d")


def key(group, cfg):
    return "%s_n%df%dm%d" % (group, *cfg)


# ---- lines ----

def hexs(frame, nbytes=None):
    frame = np.asarray(frame, dtype=np.uint8).reshape(-1)
    if nbytes is None:
        nbytes = 14 if frame[0] & 0x80 else 7
    return bytes(frame[:nbytes]).hex().upper().encode()


def avr(frame, lead=b"*", ts=b"0123456789AB", sig=b"80", semi=b";", end=b"\n", nbytes=None, suffix=b""):
    """One AVR line: frame = a uint8 array (its length by its DF unless nbytes) or its hex digits as bytes."""
    h = frame if isinstance(frame, (bytes, bytearray)) else hexs(frame, nbytes)
    head = {b"*": b"*", b":": b":", b"@": b"@" + ts, b"%": b"%" + ts, b"<": b"<" + ts + sig}[lead]
    return head + h + semi + suffix + end


def es(addr, k=0, df18=False):
    """One clean DF17 (DF18) frame of an address."""
    return fr._es_frames(1, k, np.uint32(addr), np.array([df18]))[0]


def ap(df, addr, seed=0):
    return fr.ap_frames(df, addr, payload_seed=seed)[0]


def df11(addr, iid=0):
    return fr.df11_frames(addr, iid)[0]


def flipped(frame, *bits):
    return fr.flip(frame[None, :], *[np.array([b]) for b in bits])[0]


def filler(rng, n, pool):
    """Ordinary traffic of a pool of aircraft: clean DF17 and DF11, and Address/Parity replies, in the writers' forms."""
    out = []
    for k in range(n):
        a = int(pool[rng.integers(0, len(pool))])
        kind = int(rng.integers(0, 6))
        frame = es(a, k) if kind < 2 else df11(a) if kind == 2 else ap((0, 4, 5, 16, 20, 21)[int(rng.integers(0, 6))], a, seed=k)
        lead = (b"*", b"@", b"<", b"*")[k % 4]
        out.append(avr(frame, lead, ts=b"%012X" % int(rng.integers(0, 1 << 48)), sig=b"%02X" % int(rng.integers(0, 256)), end=(b"\n", b"\r\n", b"\n")[k % 3]))
    return out


def pad_to(lines, total, rng, pool):
    """Filler traffic behind the cases until the stream has `total` bytes at least."""
    have = sum(len(x) for x in lines)
    k = 0
    while have < total:
        x = filler(rng, 1, pool)[0] if k % 7 else b"  \n"
        lines.append(x)
        have += len(x)
        k += 1
    return lines


POOL = (0x480000 + 0x1357 * np.arange(24)).astype(np.uint32)
A, B_, Cc = 0x4B172A, 0x3C66E1, 0xA1B2C3       # addresses of the format and CRC matrices


def group_a():
    """The format matrix."""
    long_, short, ac = es(A, 3), df11(A), b"7700"
    apf = ap(4, A, 1)
    g = [avr(long_), avr(short), avr(apf)]
    frames = {28: hexs(long_), 14: hexs(short), 4: ac}
    for lead in (b"<", b"@", b"%", b"*", b":"):
        for semi in (b";", b""):
            for n, h in frames.items():
                g.append(avr(h, lead, semi=semi))
            for n in (3, 5, 13, 15, 27, 29, 26, 30, 0, 1, 2, 12, 16):                       # off the three legal lengths
                g.append(avr((hexs(long_) + b"AB")[:n], lead, semi=semi))
        # whole lines of 4, 5, 13, 14 and 18 bytes
        for total in (4, 5, 13, 14, 18):
            body = (b"0123456789AB" + hexs(short) + hexs(long_))[: total - 2]
            g.append(lead + body + b";\n")
            g.append(lead + (hexs(short) + hexs(long_))[: total - 2] + b";\n")
    g += [b"%" + b"0123456789AB" + b"7700;\n", b"%" + b"0123456789A" + b"7700;\n", b"%;\n", b"%1234;\n", b"%123456789012;\n"]
    for lead in (b"#", b"x", b";", b"(", b" ", b"-"):                                         # unknown lead characters
        g.append(lead + hexs(long_) + b";\n")
    # lower case and non-hex digits in the timestamp, the signal and the frame
    g += [avr(long_, b"@", ts=b"abcdef012345"), avr(long_, b"<", ts=b"abcdef012345", sig=b"fe"), avr(hexs(long_).lower()), avr(hexs(short).lower(), b"<", sig=b"0a")]
    for ts in (b"0123456789AG", b"G123456789AB", b"01234 6789AB", b"zzzzzzzzzzzz", b"00000000000x", b"x00000000000", b"0000x0000000", b"FFFFFFFFFFFF", b"800000000000"):
        g += [avr(long_, b"@", ts=ts), avr(short, b"<", ts=ts), avr(long_, b"%", ts=ts)]
    for sig in (b"00", b"01", b"1A", b"FF", b"ff", b"G0", b"0G", b"GG", b"-1", b" 5", b"9g", b"xF"):
        g.append(avr(long_, b"<", sig=sig))
    for at in (0, 1, 13, 27):
        h = bytearray(hexs(long_))
        h[at] = ord("G")
        g += [avr(bytes(h)), avr(bytes(h), b"<")]
        h[at] = ord(" ")
        g.append(avr(bytes(h), b"@"))
    # whitespace on both sides, '\r', NUL as a terminator, empty lines
    g += [b"  \t" + avr(long_, end=b"  \t\r\n"), b"\v\f" + avr(short, b"@", end=b" \n"), avr(long_, end=b"\r\r\n"), avr(long_, end=b"\r\0"), avr(long_, end=b"\0"),
          b"\n", b"\r\n", b"\0", b"\r\0", b"\n\n\n", b" \n", b"\t \r\n", b"\r\r\n", avr(short, end=b"\0\0\n"), avr(long_)[:20] + b"\0" + avr(long_)[20:],
          b"*" + hexs(long_) + b" ;\n", b"* " + hexs(long_) + b";\n", avr(long_, end=b";\n"), b"\x80\xff" + avr(long_), avr(long_, end=b"\xa0\n"), b";\n", b"*;\n", b"*;;;;\n"]
    # the Aerobits suffix
    sufs = [b"(123,45,1A2B)", b"(123,45)", b"(123)", b"()", b"(,)", b"(,,123,,45,,7F)", b"(123,,45)", b"(,123,45,)", b"(-500,+3,-1F)", b"(+250,-3,+1f)",
            b"(0x10,5,0x1F)", b"(5,5,0X1f)", b"(5,5,0xZ)", b"(5,5,0x)", b"(5,5,-0x1F)", b"(5,5,x1)", b"(5,5,0)", b"(99999999999999999999,1,FFFFFFFFFFFFFFFFFFFF)",
            b"(-99999999999999999999,1,-FFFFFFFFFFFFFFFFFFFF)", b"(9223372036854775807,1,7FFFFFFFFFFFFFFF)", b"(9223372036854775808,1,8000000000000000)",
            b"(-9223372036854775808,1,-8000000000000000)", b"(5,5,FFFFFFFFF)", b"(5,5,80000000)", b"(5,5,7FFFFFFF)", b"(5,5,FFFFFFFF)", b"( 250, 3, 1f)", b"(\t250,3,\t1f )",
            b"(250 ,3,1f)", b"(2 50,3,1 f)", b"(abc,def,ghi)", b"(12abc,3,1fz)", b"(1.5,3,1.5)", b"(5,5,EA600)", b"(5,5,E9A18)", b"(5,5,E9A17)", b"(5,5,F4240)", b"(5,5,6F540)",
            b"(5,5,-EA600)", b"(0,0,0)", b"(1,1,1)", b"(2,1,1)", b"(100,1,1)", b"(300,1,1)", b"(500,1,1)", b"(700,1,1)", b"(900,1,1)", b"(999,1,1)", b"(1000,1,1)", b"(1001,1,1)",
            b"(1100,1,1)", b"(-100,1,1)", b"(-1000,1,1)", b"(3,1,1)", b"(4,1,1)", b"(1,2,3,4)", b"(1,2,3,4,5)", b"((1,2,3)", b"(1,(2,3)", b"(1,2,3))", b")", b"(1,2,3)x"]
    for s in sufs:
        g += [avr(long_, suffix=s), avr(short, b"@", suffix=s, end=b"\r\n"), avr(long_, b"<", suffix=s)]
    g += [b"*" + hexs(long_) + b";123,45)\n", b"(1,2,3)\n", b" (1,2,3)\n", avr(long_, suffix=b" (1,2,3)"), avr(long_, suffix=b"(1,2,3) "), b"*" + hexs(long_) + b"(1,2,3)\n",
          b"*" + hexs(long_) + b";(1,2,3);\n", b"*(1,2,3)\n", b"*1234(1,2,3)\n", avr(ac, suffix=b"(400,2,10)"), avr(ac, b"<", suffix=b"(400,2)")]
    # Mode A/C lines (with mode_ac on and off by the configuration)
    for h in (b"7700", b"0000", b"FFFF", b"ffff", b"12g4", b"1234", b"00FF", b"0080"):
        g += [avr(h), avr(h, b"@"), avr(h, b"<"), avr(h, b":", end=b"\r\n")]
    # lines of the longest length the library takes: 255 and 256 bytes in front of the terminator (LONG_LINES: the departure beyond)
    for body in (255, 256):
        g.append(b" " * (body - 30) + avr(long_))
    rng = np.random.default_rng(11)
    return pad_to(g, 41000, rng, POOL)


# Longer than 256 bytes: frames to the reference (whitespace is trimmed, net_io.c:4116-4123), "not a frame" to the library
LONG_LINES = [b" " * (body - 30) + avr(es(A, 3)) for body in (257, 300, 1000)]


def group_b():
    """The CRC matrix."""
    rng = np.random.default_rng(12)
    g = [avr(es(A, 0)), avr(es(B_, 1)), avr(df11(Cc))]                                        # the addresses the matrix's frames carry are known
    for df in range(32):
        for addr in (A, 0x123456):                                                           # a known address and one nobody added
            if df in (17, 18):
                base = es(addr, df, df18=df == 18)
            elif df == 11:
                base = df11(addr)
            else:
                base = ap(df, addr, seed=df)
            nb = 112 if df & 16 else 56
            g.append(avr(base))
            for b in (0, 2, 4, 8, 20, 31, nb - 1, nb - 13, nb - 24, 40):
                g.append(avr(flipped(base, b), (b"*", b"@")[b & 1]))
            for b0, b1 in ((8, 9), (20, 45), (nb - 1, nb - 2), (3, 30), (33, 50), (5, 6)):
                g.append(avr(flipped(base, b0, b1)))
            # the other length: the DF decides how many bits count (the rest of a short line is zero, mode_s.c:465)
            g.append(avr(base, nbytes=7 if nb == 112 else 14))
    for iid in (1, 5, 64, 127):
        g += [avr(df11(A, iid)), avr(df11(0x123457, iid)), avr(flipped(df11(A, iid), 40))]
    for df18 in (False, True):                                                               # every single bit of DF17 / DF18
        for b in range(112):
            g.append(avr(flipped(es(A, 100 + b, df18), b)))
    for b in range(56):
        g += [avr(flipped(df11(A), b)), avr(flipped(df11(0x223344), b))]
    for k in range(60):                                                                      # drawn pairs of bits
        b0, b1 = sorted(rng.choice(112, 2, replace=False).tolist())
        g += [avr(flipped(es(B_, 300 + k), b0, b1)), avr(flipped(es(0x334455, 300 + k, True), b0, b1))]
        s0, s1 = sorted(rng.choice(56, 2, replace=False).tolist())
        g.append(avr(flipped(df11(Cc), s0, s1)))
    # frames fixDF17msgtype touches: a clean DF17 with one bit of the DF flipped (DF 1, 25, 21, 19, 16), with a second error too
    for j in range(5):
        g += [avr(flipped(es(A, 400 + j), j)), avr(flipped(es(0x556677, 400 + j), j)), avr(flipped(es(A, 410 + j), j, 50))]
    z = np.zeros(14, dtype=np.uint8)
    tail = z.copy()
    tail[7:] = 0xFF
    g += [avr(z, nbytes=14), avr(z, nbytes=7), avr(tail, nbytes=14), avr(flipped(z, 55), nbytes=7), avr(flipped(z, 4), nbytes=7)]
    return pad_to(g, 41000, rng, POOL)


def align_chunk(lines, offset=0):
    """Whitespace lines until the stream position is `offset` modulo 32: the next line starts at a chosen byte of a lane's chunk."""
    have = sum(len(x) for x in lines)
    need = (offset - have) % CHUNK
    if need:
        lines.append(b" " * (need - 1) + b"\n")
    return lines


def order_cases(addr0):
    """-> [(name, [the lines in front of the adder], adder line(s), [the lines behind])]: conditional frames of an address around the one
    line that adds it (or does not)."""
    cases = []
    k = 0

    def cond(a, seed):
        return [avr(ap(4, a, seed)), avr(ap(20, a, seed + 1)), avr(flipped(df11(a), 40)), avr(flipped(es(a, seed), 15))]

    for name, adder in (("df17", lambda a: [avr(es(a, 5))]), ("df11", lambda a: [avr(df11(a))]), ("twice", lambda a: [avr(es(a, 6)), avr(df11(a)), avr(es(a, 7))]),
                        ("df18", lambda a: [avr(es(a, 8, True))]), ("df11_iid", lambda a: [avr(df11(a, 5))]), ("dffix", lambda a: [avr(flipped(es(a, 9), 1))]),
                        ("df17_repaired", lambda a: [avr(flipped(es(a, 10), 60))]), ("df11_repaired", lambda a: [avr(flipped(df11(a), 45))])):
        a = addr0 + 0x010101 * k
        cases.append((name, a, cond(a, 10 * k), adder(a), cond(a, 10 * k + 5)))
        k += 1
    return cases


def group_c():
    """Order: conditional frames in front of their adder, directly behind it in the same lane's 32 bytes, and in the next tile."""
    rng = np.random.default_rng(13)
    g = filler(rng, 40, POOL)
    far = []                                                                                 # what goes into the next tile
    for name, a, before, adders, behind in order_cases(0x500000):
        g += before
        align_chunk(g)                                                                       # the adder starts a chunk: a 17-byte line behind a short adder starts in the same one
        g += adders
        g += behind
        far.append((a, name))
        g += filler(rng, 6, POOL)
        # a short adder and its conditional frame in one chunk
        b = a ^ 0x800000
        g += [avr(ap(5, b, 3))]
        align_chunk(g, 0)
        g += [avr(df11(b) if name != "df11_iid" else df11(b, 9)), avr(ap(5, b, 4))]
    pad_to(g, 2 * TILE + 100, rng, POOL)
    for a, name in far:                                                                      # the next tiles: the same questions again
        g += [avr(ap(0, a, 77)), avr(flipped(df11(a), 41)), avr(ap(21, a ^ 0x800000, 78))]
    return pad_to(g, 41000, rng, POOL)


class FilterModel:
    """icao_filter.c: two generations, occupied, the table's log2 size (resolve.h's IcaoFilter restated for the generators)."""

    def __init__(self):
        self.active, self.inactive, self.occupied, self.bits = [], set(), 0, 8

    def add(self, a):
        if a not in self.active:
            self.active.append(a)
            self.occupied += 1
        grew = False
        if self.occupied > (1 << self.bits) // 3 and self.bits < 20:
            self.bits += 1
            self.inactive = set()
            self.occupied = len(self.active)
            grew = True
        return grew

    def expire(self):
        if self.occupied < (1 << self.bits) // 9 and self.bits > 8:
            self.bits -= 1
        self.occupied = 0
        self.inactive = set(self.active)
        self.active = []

    def test(self, a):
        return a in self.active or a in self.inactive


D_INACTIVE = (0x600000 + 0x0203 * np.arange(40)).astype(np.uint32)
D_ACTIVE = (0x610000 + 0x0305 * np.arange(40)).astype(np.uint32)
D_NEW = (0x620000 + 0x0407 * np.arange(150)).astype(np.uint32)
D_OPS = [int(a) for a in D_INACTIVE] + [-1] + [int(a) for a in D_ACTIVE]                      # the filter's preparation: adds, an expiry, adds


def group_d():
    """Growth.  -> (lines, the line of the first growth L*, the line of the second, the probes: [(line, address, passes)])"""
    rng = np.random.default_rng(14)
    f = FilterModel()
    for op in D_OPS:
        f.expire() if op < 0 else f.add(op)
    assert (f.occupied, f.bits, len(f.inactive)) == (40, 8, 40)
    g, probes, growths = [], [], []
    seen_new = []

    def probe(a, seed):
        probes.append((len(g), int(a), f.test(int(a))))
        g.append(avr(ap((0, 4, 5, 16, 20, 21)[seed % 6], int(a), seed)))

    def adder(a, k):
        if f.add(int(a)):
            growths.append(len(g))
        g.append(avr(es(int(a), k) if k % 3 else df11(int(a))))

    readd = int(D_INACTIVE[7])                                                               # re-added in front of L*: it stays known behind it
    onstar = int(D_INACTIVE[11])                                                             # the adder on L* itself is an inactive-generation address
    k = 0
    for i, a in enumerate(D_NEW):
        if i == 20:
            adder(readd, 1)
        if i == 30:
            adder(int(D_ACTIVE[3]), 1)                                                       # already active: no new add, moves nothing
        # (occupied is 40 + i + 1 here, one more behind the re-add: the 46th new add makes the table grow)
        if f.occupied == (1 << 8) // 3 and f.bits == 8:
            probe(D_INACTIVE[5], k)                                                          # on the line in front of L*: still known
            probe(onstar, k + 1)
            adder(onstar, 1)                                                                 # L*
            assert growths and growths[-1] == len(g) - 1
            probe(D_INACTIVE[5], k + 2)                                                      # on the line behind L*: gone
            probe(onstar, k + 3)                                                             # learnt on L*: known
            probe(readd, k + 4)
        adder(a, 1 + (i % 5))
        seen_new.append(int(a))
        for j in range(11):
            pick = int(rng.integers(0, 5))
            src = (D_INACTIVE, D_ACTIVE, np.array(seen_new), D_NEW[i + 1:] if i + 1 < len(D_NEW) else D_NEW, D_INACTIVE)[pick]
            probe(src[int(rng.integers(0, len(src)))], k + j)
        k += 13
    assert len(growths) == 2 and f.bits == 10, growths
    return g, growths[0], growths[1], probes


def group_d2():
    """The second call: one Address/Parity frame per prepared address and per address of the stream."""
    g = []
    for k, a in enumerate(np.concatenate([D_INACTIVE, D_ACTIVE, D_NEW, np.array([0x123456], dtype=np.uint32)])):
        g.append(avr(ap((0, 4, 5, 16, 20, 21)[k % 6], int(a), k)))
    return g


def build_groups():
    return {"a": group_a(), "b": group_b(), "c": group_c(), "d": group_d()[0], "d2": group_d2()}


def stream_of(lines):
    return b"".join(lines)


def split_lines(stream):
    """The terminated lines of a stream as readAscii frames them, without their terminators (a trailing '\\r' still on them)."""
    return stream.replace(b"\0", b"\n").split(b"\n")[:-1]


# ---- the reference ----

def have_ref_full():
    return sbs_util.have_ref_full()


def build_ref_harness(workdir, name="raw_in", src=HARNESS_SRC):
    """A message input's harness (tests/host_stub/<name>_ref_harness.c; beast_in_util and pf_in_util build theirs here) compiled with
    the flags of `make -C oracle full` and linked against that build's other objects, readsb.o with its main renamed in a copy (as
    tests/sbs_in_util.py builds its harness)."""
    exe = os.path.join(workdir, name + "_ref_harness")
    main_o = os.path.join(workdir, "readsb_nomain_%s.o" % name)
    subprocess.run(["objcopy", "--redefine-sym", "main=readsb_main", os.path.join(sbs_util.REF_FULL, "readsb.o"), main_o], check=True)
    objs, flags = sbs_util._full_build()
    subprocess.run(["gcc", *flags, "-I" + os.path.join(helpers.ORACLE_DIR, "stub_full"), "-I/root/reference", "-I" + os.path.join(helpers.ROOT, "include"), src,
                    main_o, *[os.path.join(sbs_util.REF_FULL, o + ".o") for o in objs], "-o", exe, "-pthread", "-lpthread", "-lm", "-lrt", "-l:libzstd.so.1", "-lz"],
                   check=True)
    return exe


def read_results(blob, n, nhead, unit_fields, msg_fields):
    """n results as a message input's harness writes them: nhead 64-bit words (the second counts the units — lines, handler calls —,
    the third the messages), the per-unit arrays, the per-message arrays; the fields as ((name, dtype), ...) -> [dict(head, names...)]"""
    out, at = [], 0

    def take(count, dtype):
        nonlocal at
        size = count * np.dtype(dtype).itemsize
        v = np.frombuffer(blob[at: at + size], dtype=dtype).copy()
        at += size
        return v

    for _ in range(n):
        r = dict(head=take(nhead, np.uint64))
        for count, fields in ((int(r["head"][1]), unit_fields), (int(r["head"][2]), msg_fields)):
            for name, dtype in fields:
                r[name] = take(count, dtype)
        out.append(r)
    assert at == len(blob)
    return out


def parse_results(blob, n):
    """n results as the harness writes them -> [dict(head, cls, line_of, signal, msgs)]"""
    return read_results(blob, n, 10, (("cls", np.uint8),), (("line_of", np.uint64), ("signal", np.float64), ("msgs", MSG)))


def run_ref_harness(exe, streams, cfg, workdir, ops=(), now_ms=NOW_MS, reps=1):
    """The reference over the streams, one after the other against one filter prepared by ops -> a result per stream"""
    paths = []
    for k, s in enumerate(streams):
        paths.append(os.path.join(workdir, "raw_in_stream%d.bin" % k))
        open(paths[-1], "wb").write(s)
    fpath = os.path.join(workdir, "raw_in_filter.bin")
    np.asarray(list(ops), dtype=np.int32).tofile(fpath)
    r = subprocess.run([exe, str(int(now_ms)), str(cfg[0]), str(cfg[1]), str(cfg[2]), fpath, str(int(reps)), *paths], check=True, capture_output=True, timeout=600)
    return parse_results(r.stdout, len(streams))


def load_golden():
    """-> {key(group, cfg): dict(stream, head, line_of, signal, msgs)}"""
    z = np.load(GOLDEN)
    out = {}
    for g, cfgs in CONFIGS.items():
        for cfg in cfgs:
            k = key(g, cfg)
            out[k] = dict(stream=z[g + "_stream"].tobytes(), head=z[k + "_head"], line_of=z[k + "_line_of"].astype(np.uint64), signal=z[k + "_signal"],
                          msgs=z[k + "_msgs"].view(MSG).reshape(-1), cls=z[k + "_class"])
    return out


def ops_of(group):
    return D_OPS if group in ("d", "d2") else []


# ---- the library's host side ----

def through_filter(filt, room, call):
    """A sequential walk of the library's (mgpu_raw_decode_host and its like) against a FilterModel: call(a reference to the
    binding.RawInFilter that holds filt, with room for `room` new adds) -> its rc; filt is moved on unless the walk failed."""
    from readsb_amd import binding
    filt = filt if filt is not None else FilterModel()
    ga = np.zeros(len(filt.active) + room, dtype=np.uint32)
    ga[: len(filt.active)] = filt.active
    gi = np.concatenate([np.array(sorted(filt.inactive), dtype=np.uint32), np.zeros(1, dtype=np.uint32)])
    f = binding.RawInFilter(ga.ctypes.data, gi.ctypes.data, len(filt.active), len(filt.inactive), filt.occupied, filt.bits)
    rc = int(call(C.byref(f)))
    if rc == MGPU_OK:
        filt.active, filt.inactive, filt.occupied, filt.bits = [int(x) for x in ga[: f.n_active]], set(int(x) for x in gi[: f.n_inactive]), int(f.occupied), int(f.table_bits)
    return rc


def host_decode(lib, stream, cfg, filt=None, now_ms=NOW_MS):
    """mgpu_raw_decode_host: the sequential resolver.  filt: a FilterModel, moved on by the call.
    -> dict(rc, consumed, nlines, nmsgs, counters, msgs, line_of, signal, cls)"""
    from readsb_amd import binding
    buf = np.frombuffer(bytes(stream) + b"\n", dtype=np.uint8)
    nl = len(stream) + 1
    cap = len(stream) // 6 + 1
    msgs, line_of, signal, cls = np.zeros(cap, dtype=MSG), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.float64), np.zeros(nl, dtype=np.uint8)
    c = [C.c_uint64(0) for _ in range(3)]
    cn = binding.RawInCounters()
    a = binding.RawInArgs(C.sizeof(binding.RawInArgs), 0, buf.ctypes.data, len(stream), now_ms, msgs.ctypes.data, line_of.ctypes.data, signal.ctypes.data, cap, cls.ctypes.data, nl,
                          *[C.pointer(x) for x in c], C.pointer(cn), 0)
    kcfg = binding.RawInConfig(C.sizeof(binding.RawInConfig), *cfg)
    rc = through_filter(filt, nl, lambda f: lib.mgpu_raw_decode_host(C.byref(a), C.byref(kcfg), f))
    n = int(c[2].value)
    return dict(rc=rc, consumed=int(c[0].value), nlines=int(c[1].value), nmsgs=n, counters=[int(cn.remote_received_modes), int(cn.remote_received_modeac),
                int(cn.remote_rejected_unknown_icao), int(cn.remote_rejected_bad), *[int(x) for x in cn.remote_accepted]],
                msgs=msgs[:n], line_of=line_of[:n], signal=signal[:n], cls=cls[: int(c[1].value)])
