"""SBS input (decodeSbsLine over BaseStation lines): the case generators behind tests/golden/sbs_in_cases.npz, the golden's loader, the
reference harness (tests/host_stub/sbs_in_ref_harness.c, which includes the reference's net_io.c and links oracle/_ref/full's other
objects) and what the tests expect of a stream.  A case is one or more lines; a group is one stream."""
import os
import subprocess

import numpy as np

import helpers
import sbs_util

GOLDEN = os.path.join(helpers.GOLDEN_DIR, "sbs_in_cases.npz")
HARNESS_SRC = os.path.join(helpers.ROOT, "tests", "host_stub", "sbs_in_ref_harness.c")
GROUPS = ("a", "b", "c")
SOURCES = {"sbs": 3, "mlat": 4, "jaero": 6, "prio": 11}                   # datasource_t, readsb.h:159-173
GROUP_SOURCES = {"a": ("sbs", "mlat", "jaero", "prio"), "b": ("sbs", "mlat", "jaero", "prio"), "c": ("sbs", "mlat")}
NOW_MS = 1700000123456
TILE = 8192                                     # kUatTile of kernels.h
MGPU_OK, MGPU_E_INVAL, MGPU_E_OVERFLOW = 0, -1, -5
REC = np.dtype([("sysTimestamp", "<i8"), ("decoded_lat", "<f8"), ("decoded_lon", "<f8"), ("addr", "<u4"), ("flags", "<u4"), ("sbs_flags", "<u4"), ("baro_alt", "<i4"),
                ("baro_rate", "<i4"), ("gs_v0", "<f4"), ("heading", "<f4"), ("squawkDec", "<u4"), ("squawkHex", "<u4"), ("receiverCountMlat", "<i4"), ("mlatEPU", "<i4"),
                ("callsign", "S8"), ("sbsMsgType", "u1"), ("source", "u1"), ("addrtype", "u1"), ("airground", "u1"), ("baro_alt_unit", "u1"), ("heading_type", "u1"),
                ("reserved", "u1", 14)])
assert REC.itemsize == 96
STAMP = "2023/11/14,22:15:23.456,2023/11/14,22:15:23.789"


def sbs(msgtype="3", addr="4AC8B3", callsign="", alt="", gs="", trk="", lat="", lon="", vr="", sq="", f19="", f20="", f21="", f22="", end=b"\r\n", f1="MSG",
        stamp=STAMP, tail=None):
    """One BaseStation line from its 22 fields (as text); tail: what follows a 22nd comma."""
    fields = [f1, msgtype, "1", "1", addr, "1", stamp, callsign, alt, gs, trk, lat, lon, vr, sq, f19, f20, f21, f22]
    text = ",".join(fields)
    if tail is not None:
        text += "," + tail
    return text.encode("latin-1") + end


def padded(total, end=b"\n", **kw):
    """A valid line whose length before `end` is `total`: filler behind the 22nd comma, which the reference ignores."""
    base = sbs(end=b"", tail="", **kw)
    assert len(base) <= total
    return base + b"x" * (total - len(base)) + end


def writer_line(rng, k, mlat=False):
    """A line as modesSendSBSOutput prints it (net_io.c:3249-3401) or, mlat, as mlat-client does."""
    r = lambda n: int(rng.integers(0, n))                                                          # noqa: E731
    addr = "%06X" % (0x400000 + r(0x3FFFFF))
    stamp = "2023/11/14,22:%02d:%02d.%03d,2023/11/14,22:%02d:%02d.%03d" % (r(60), r(60), r(1000), r(60), r(60), r(1000))
    if mlat:
        ext = k % 3 == 0
        return sbs("3", addr, alt=str(r(45000) - 500) if k % 5 else "", lat="%.4f" % (r(1700000) / 10000.0 - 85), lon="%.4f" % (r(3500000) / 10000.0 - 175),
                   gs=str(r(600)) if k % 4 == 0 else "", trk=str(r(360)) if k % 4 == 0 else "", vr=str(r(6000) - 3000) if k % 7 == 0 else "",
                   f19=str(3 + r(20)) if ext else "", f20=str(r(90000)) if ext else "", stamp=stamp, end=b"\n")
    t = (1, 2, 3, 3, 3, 4, 4, 5, 6, 7, 8)[k % 11]
    flag = lambda: ("", "0", "-1")[r(3)]                                                           # noqa: E731
    kw = dict(stamp=stamp)
    if t == 1:
        kw.update(callsign=("DLH%d" % r(9999)).ljust(8)[:8])
    if t in (2, 3, 5, 6, 7):
        kw.update(alt=str(r(47000) - 1200))
    if t in (2, 4):
        kw.update(gs="%.0f" % (r(6000) / 10.0), trk="%.0f" % (r(3600) / 10.0))
    if t in (2, 3):
        kw.update(lat="%1.6f" % (r(170000000) / 1e6 - 85), lon="%1.6f" % (r(350000000) / 1e6 - 175))
    if t == 4:
        kw.update(vr=str(64 * (r(200) - 100)))
    if t == 6:
        sq = (7500, 7600, 7700, r(8) * 1000 + r(8) * 100 + r(8) * 10 + r(8))[r(4)]
        kw.update(sq="%04d" % sq, f19=flag(), f20=("0", "-1")[sq in (7500, 7600, 7700)], f21=flag())
    if t in (2, 3, 5, 6, 7, 8):
        kw.update(f22=flag())
    return sbs(str(t), addr, **kw)


INT_FIELDS = ("alt", "vr", "sq", "f19", "f20")
REAL_FIELDS = ("gs", "trk", "lat", "lon")
# not of the plain forms (include/modes_gpu.h); what atoi / strtol / strtod make of them is the host's to say
HOSTILE_BOTH = ["1e3", "1E-2", "-2e+1", " 5", "5 ", "\t5", "inf", "-inf", "INF", "nan", "infinity", "0x10", "0x1p3", "12abc", "abc", "+", "-", "--5", "+-5", "35000H",
                "12345678901234567890", "1 2", "5;", "1_000"]
HOSTILE_INT = HOSTILE_BOTH + ["1.5", "5.", ".5", ".", "1234567890", "-1234567890", "0000000001", "99999999999", "-0.0"]
HOSTILE_REAL = HOSTILE_BOTH + [".", "+.", "-.", "1..2", "1.2.3", "1.2345678901234567", "1234567890123456", "0.12345678901234567", "0.00000000000000000000001",
                               "1.00000000000000000000000", "9007199254740993", "1.5.", "1.5e", "0x.8", "1.7976931348623157e308", "1e400", "-1e400", "4.9e-324", "1e-400"]


def build_groups():
    """-> {group: [line bytes, ...]}: seeded, so the golden's maker and the live check build the same streams."""
    rng = np.random.default_rng(30003)
    g = {k: [] for k in GROUPS}
    # (a) ordinary lines: readsb's writer and mlat-client
    for k in range(330):
        g["a"].append(writer_line(rng, k))
    for k in range(110):
        g["a"].append(writer_line(rng, k, mlat=True))
    g["a"].append(b"\r\n")                                                                        # the writer's heartbeat is an empty line
    # (b) every branch and the boundaries of every rule
    b = g["b"]
    full = dict(callsign="BAW123  ", alt="35000", gs="451", trk="271", lat="51.477500", lon="-0.461389", vr="-64", sq="4721", f19="0", f20="0", f21="0", f22="0")
    b += [sbs(**full), sbs(**full, end=b"\n"), sbs()]
    for name in full:                                                                              # each field alone, each field missing
        b.append(sbs(**{name: full[name]}))
        b.append(sbs(**{k: v for k, v in full.items() if k != name}))
    b += [b"\n", b"\r\n", b"X\n", b"X\r\n", b"\r\r\n", b"XY\n", b"XY\r\n", b"XYZ\r\n"]           # lengths 0, 1, 2 (a heartbeat below 2)
    for total in (19, 20, 21):
        b += [b"M" * total + b"\n", b"M" * total + b"\r\n", sbs(end=b"")[:total] + b"\n"]
    b += [b"MSG,3,,,ABCDEF,,,,,,,,,,,,,,,,,\n", b"MSG,3,,,ABCDEF,,,,,,,,,,,,,,,,\n", b",,,,,,,,,,,,,,,,,,,,,,,,\n"]            # the shortest valid line (31), 20 commas
    for total in (198, 199, 200, 201, 202, 255, 256, 257, 258, 300, 1000):
        b += [padded(total, **full), padded(total, end=b"\r\n", **full)]
    b += [padded(199, end=b"\r\r\n", **full), padded(198, end=b"\r\r\n", **full)]                  # one '\r' is removed, the other is content
    base = sbs(end=b"", **full)
    for commas in (20, 21, 22, 23, 30):                                                            # 21 in `base`
        have = base.count(b",")
        b.append((b",".join(base.split(b",")[: commas + 1]) if commas <= have else base + b"," * (commas - have)) + b"\r\n")
    b += [sbs(tail="", **full), sbs(tail="anything,else,,,", **full), sbs(tail="-1", **{**full, "f22": ""})]
    for f1 in ("MSH", "msg", "MSG ", " MSG", "MS", "MSGS", "", "STA", "SEL", "AIR", "ID", "CLK"):
        b.append(sbs(f1=f1, **full))
    for t2 in list("0123456789") + ["", "12", "A", "+", "-", " ", "a", "\x80"]:
        b.append(sbs(msgtype=t2, **full))
    for pos in range(6):
        for bad in ("G", "g", " ", "-", "\xc4"):
            b.append(sbs(addr="4AC8B3"[:pos] + bad + "4AC8B3"[pos + 1:], **full))
    for addr in ("4ac8b3", "aBcDeF", "000000", "FFFFFF", "4AC8B", "4AC8B3F", "", "~4AC8B", "0x4AC8"):
        b.append(sbs(addr=addr, alt="100"))
    for pos in range(10):                                                                          # a bad character at each place, then beyond the eight
        for bad in ("a", "-", ".", "\xe9", "\t"):
            b.append(sbs(callsign="ABCDEFGHIJ"[:pos] + bad + "ABCDEFGHIJ"[pos + 1:]))
    for cs in ("A", "AB", "ABC1234", "ABC12345", "ABC123456", "ABC1234567890", " ", "        ", "A B", "A  B  C ", "a", "Ab", "ABCa", "ABCDEFGa", "ABCDEFGHa", "0", "9Z 0A"):
        b.append(sbs(callsign=cs, alt="1"))
    for alt in ("-5001", "-5000", "-4999", "0", "-0", "+0", "99999", "100000", "100001", "+100", "-1", "123456789", "-123456789", "999999999", "007", "+007", "-007"):
        b.append(sbs(alt=alt))
    for gs in ("0", "-1", "0.0", "-0", "-0.0", "0.4", "0.5", "450", "450.5", ".5", "5.", "+5", "-.5", "1", "000", "00.1", "0.000000000000000000001", "123456789012345",
               "0.0000000000000000000001", "16777217", "0.1"):
        b += [sbs(gs=gs), sbs(trk=gs)]
    for lat, lon in (("0", "0"), ("0", "1.5"), ("1.5", "0"), ("1.5", ""), ("", "1.5"), ("-0.0", "10"), ("10", "-0"), ("51.477500", "-0.461389"), ("-33.946111", "151.177222"),
                     ("12.3456789012345", "-123.456789012345"), ("0.000000000000001", "0.0000000000000000000001"), ("000000000000000000001.5", "+2."), (".5", "-.25"),
                     ("90", "180"), ("-90.000000", "-180.000000"), ("89.999999", "179.999999"), ("0.1", "0.2"), ("0.3", "0.7"), ("123456.789012345", "999999999999999"),
                     ("0.000000", "0.000000"), ("1e", ""), ("", "inf")):
        b.append(sbs(lat=lat, lon=lon))
    for vr in ("0", "-0", "64", "-64", "+64", "32768", "-999999999", "999999999"):
        b.append(sbs(vr=vr))
    for sq in ("0", "0000", "7500", "7600", "7700", "07500", "1200", "-1", "-7700", "1", "9999", "12345", "999999999", "+7700"):
        b.append(sbs(sq=sq))
    for f19 in ("0", "-1", "1", "5", "00", "-01", "+0", "-0", "-2", "65536", "999999999"):
        b.append(sbs(f19=f19))
    for f20 in ("", "0", "-1", "1", "5", "65535", "65536", "999999999", "-5", "00"):                # the flag's value is read from field 21
        for f21 in ("", "0", "-1", "1", "00", "2"):
            b.append(sbs(f20=f20, f21=f21))
    for f22 in ("0", "-1", "1", "-", "-1x", "-10", "0abc", "00", "01", " 0", "-2", "+0"):
        b += [sbs(f22=f22), sbs(f22=f22, tail="0")]
    one = sbs(end=b"", **full)
    b += [one + b"\0", one + b"\r\0", one + b"\0\0\n", b"\0", b"\0\r\n", one[:60] + b"\0" + one[60:] + b"\n", one[:5] + b"\0" + one[5:] + b"\r\n",
          one + b"\0" + one + b"\n", sbs(end=b"", alt="1") + b"\n\0\n"]                            # NUL bytes end lines, wherever they are
    # (c) hostile numbers: every line is valid and holds a number outside the plain forms
    c = g["c"]
    for name in INT_FIELDS:
        for v in HOSTILE_INT:
            c.append(sbs(**{**full, name: v}))
    for name in REAL_FIELDS:
        for v in HOSTILE_REAL:
            c.append(sbs(**{**full, name: v}))
    c += [sbs(alt="1e3"), sbs(gs="1e3", end=b"\n"), sbs(lat="1e1", lon="2e1"), sbs(lat="1", lon="2e1"), sbs(f20=" 0", f21="0"), sbs(f19="0x1")]
    return g


def stream_of(lines):
    return b"".join(lines)


def split_lines(stream):
    """The terminated lines of a stream as readAscii frames them, without their terminators (a trailing '\\r' still on them)."""
    parts = stream.replace(b"\0", b"\n").split(b"\n")
    return parts[:-1]


def have_ref_full():
    return sbs_util.have_ref_full()


def build_ref_harness(workdir):
    """tests/host_stub/sbs_in_ref_harness.c compiled with the flags of `make -C oracle full` and linked against that build's other
    objects, readsb.o with its main renamed in a copy (as tests/sbs_util.py builds the writers' harness)."""
    exe = os.path.join(workdir, "sbs_in_ref_harness")
    main_o = os.path.join(workdir, "readsb_nomain_sbs_in.o")
    subprocess.run(["objcopy", "--redefine-sym", "main=readsb_main", os.path.join(sbs_util.REF_FULL, "readsb.o"), main_o], check=True)
    objs, flags = sbs_util._full_build()
    subprocess.run(["gcc", *flags, "-I" + os.path.join(helpers.ORACLE_DIR, "stub_full"), "-I/root/reference", "-I" + os.path.join(helpers.ROOT, "include"), HARNESS_SRC,
                    main_o, *[os.path.join(sbs_util.REF_FULL, o + ".o") for o in objs], "-o", exe, "-pthread", "-lpthread", "-lm", "-lrt", "-l:libzstd.so.1", "-lz"],
                   check=True)
    return exe


def run_ref_harness(exe, stream, source, workdir, now_ms=NOW_MS, reps=1):
    """-> (head = consumed, lines, records, invalid, valid; line_of; records) as the reference leaves them"""
    path = os.path.join(workdir, "sbs_in_stream.bin")
    open(path, "wb").write(stream)
    r = subprocess.run([exe, path, str(SOURCES[source]), str(int(now_ms)), str(int(reps))], check=True, capture_output=True, timeout=600)
    head = np.frombuffer(r.stdout[:40], dtype=np.uint64)
    n = int(head[2])
    line_of = np.frombuffer(r.stdout[40: 40 + 8 * n], dtype=np.uint64)
    recs = np.frombuffer(r.stdout[40 + 8 * n:], dtype=REC)
    assert len(recs) == n
    return head.copy(), line_of.copy(), recs.copy()


def load_golden():
    """-> {group: (stream bytes, {source: (head, line_of, records)})}"""
    z = np.load(GOLDEN)
    return {g: (z[g + "_stream"].tobytes(), {s: (z[f"{g}_{s}_head"], z[f"{g}_{s}_line_of"].astype(np.uint64), z[f"{g}_{s}_recs"].view(REC)) for s in GROUP_SOURCES[g]}) for g in GROUPS}


def without(line_of, recs, deferred):
    """The reference's records with those of the deferred lines cut out: what the device gives."""
    keep = ~np.isin(line_of, np.asarray(deferred, dtype=np.uint64))
    return line_of[keep], recs[keep]


def feed(nlines, seed=1):
    """A drawn feed: three lines of readsb's writer to one of mlat-client."""
    rng = np.random.default_rng(seed)
    return [writer_line(rng, k, mlat=k % 4 == 3) for k in range(nlines)]
