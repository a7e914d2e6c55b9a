"""UAT input (uat2esnt over dump978 downlink lines): the case generators behind tests/golden/uat_cases.npz, the golden's loader, the
reference harness (tests/host_stub/uat_ref_harness.c against oracle/_ref/full's two uat2esnt objects) and what the tests expect of a
stream.  A case is one line; a group is one stream."""
import math
import os
import subprocess

import numpy as np

import helpers

GOLDEN = os.path.join(helpers.GOLDEN_DIR, "uat_cases.npz")
HARNESS_SRC = os.path.join(helpers.ROOT, "tests", "host_stub", "uat_ref_harness.c")
REF_OBJS = [os.path.join(helpers.ORACLE_DIR, "_ref", "full", n) for n in ("uat2esnt_uat2esnt.o", "uat2esnt_uat_decode.o")]
GROUPS = ("a", "b", "c", "d", "e", "f")
FRAME_TEXT = 45
TILE = 8192                                    # kUatTile of kernels.h
DEV_LINE_MAX = 256
MGPU_OK, MGPU_E_INVAL, MGPU_E_OVERFLOW = 0, -1, -5
UAT_TIMESTAMP = 0xFF004D4C4155
NEEDED = {**{t: 17 for t in (0, 4, 7, 8, 9, 10)}, 3: 27, **{t: 31 for t in (1, 2, 5, 6)}, **{t: 4 for t in range(11, 32)}}
BASE40 = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ  .."
CPR_NL = [10.47047130, 14.82817437, 18.18626357, 21.02939493, 23.54504487, 25.82924707, 27.93898710, 29.91135686, 31.77209708,
          33.53993436, 35.22899598, 36.85025108, 38.41241892, 39.92256684, 41.38651832, 42.80914012, 44.19454951, 45.54626723,
          46.86733252, 48.16039128, 49.42776439, 50.67150166, 51.89342469, 53.09516153, 54.27817472, 55.44378444, 56.59318756,
          57.72747354, 58.84763776, 59.95459277, 61.04917774, 62.13216659, 63.20427479, 64.26616523, 65.31845310, 66.36171008,
          67.39646774, 68.42322022, 69.44242631, 70.45451075, 71.45986473, 72.45884545, 73.45177442, 74.43893416, 75.42056257,
          76.39684391, 77.36789461, 78.33374083, 79.29428225, 80.24923213, 81.19801349, 82.13956981, 83.07199445, 83.99173563,
          84.89166191, 85.75541621, 86.53536998, 87.00000000]


def payload(mdb_type=1, aq=0, addr=0xA12345, raw_lat=0x155555, raw_lon=0x955555, alt_bit=0, raw_alt=0x123, nic=8, ag=0, raw_a=0x0C8,
            raw_b=0x4C8, raw_vvel=0x405, low16=0, ms=(1, 2, 3), b23_26=(0x24, 0x10, 0xA5, 0x02), raw_sec=0x140, nbytes=None):
    """A downlink payload from the raw fields uat_decode.c reads (18 bytes for type 0, 34 otherwise, or nbytes)."""
    b = bytearray(34)
    b[0] = (mdb_type & 31) << 3 | (aq & 7)
    b[1:4] = (addr & 0xFFFFFF).to_bytes(3, "big")
    word = (raw_lat & 0x7FFFFF) << 25 | (raw_lon & 0xFFFFFF) << 1 | (alt_bit & 1)                     # bytes 4-9
    b[4:10] = word.to_bytes(6, "big")
    b[10] = (raw_alt >> 4) & 0xFF
    b[11] = (raw_alt & 15) << 4 | (nic & 15)
    b[12] = (ag & 3) << 6 | (raw_a >> 6) & 0x1F
    b[13] = (raw_a & 0x3F) << 2 | (raw_b >> 9) & 3
    b[14] = (raw_b >> 1) & 0xFF
    b[15] = (raw_b & 1) << 7 | (raw_vvel >> 4) & 0x7F
    b[16] = (raw_vvel & 15) << 4 | (low16 & 15)
    for k, v in enumerate(ms):
        b[17 + 2 * k: 19 + 2 * k] = (v & 0xFFFF).to_bytes(2, "big")
    b[23:27] = bytes(b23_26)
    b[29] = (raw_sec >> 4) & 0xFF
    b[30] = (raw_sec & 15) << 4
    return bytes(b[: nbytes if nbytes is not None else (18 if mdb_type == 0 else 34)])


def ms_words(emitter, text):
    """The three base-40 words of an emitter category (0-39) and eight characters given as indices into BASE40."""
    c = list(text)
    return (emitter * 1600 + c[0] * 40 + c[1], c[2] * 1600 + c[3] * 40 + c[4], c[5] * 1600 + c[6] * 40 + c[7])


def idx(text, alt=False):
    """Indices into BASE40 of a string of up to eight characters, padded with spaces; alt: the second ' ' and '.' of the alphabet."""
    out = []
    for ch in text.ljust(8):
        i = BASE40.index(ch)
        out.append(i + 1 if alt and ch in " ." else i)
    return out


def line(pl, extra="rs=2;rssi=-12.3;t=1234.567;", sign="-", upper=True):
    h = pl.hex()
    return (sign + (h.upper() if upper else h) + ";" + extra + "\n").encode("latin-1")


def raw_of_lat(lat):
    return int(round((lat if lat >= 0 else lat + 180.0) * 16777216.0 / 360.0)) & 0x7FFFFF


def raw_of_lon(lon):
    return int(round((lon if lon >= 0 else lon + 360.0) * 16777216.0 / 360.0)) & 0xFFFFFF


def sig_model(k10):
    """The signal byte of the simple-form value k10 / 10 by this interpreter's float and libm: only for choosing cases near the steps."""
    ss = float(np.float32(k10 / 10.0))
    w = math.pow(10.0, ss / 10.0)
    s = int(round(math.sqrt(w) * 255.0))
    return min(255, max(s, 1 if w > 0 else 0))


def cpr_model(lat, lon, odd, surface):
    """encode_cpr_lat / encode_cpr_lon before the mask, for placing cases at the zone edges."""
    nb = float(1 << 19 if surface else 1 << 17)
    dlat = 360.0 / (59 if odd else 60)

    def mod(a, b):
        r = math.fmod(a, b)
        return r + b if r < 0 else r
    yz = math.floor(nb * mod(lat, dlat) / dlat + 0.5)
    rlat = dlat * (1.0 * yz / nb + math.floor(lat / dlat))
    nl = 59 - sum(1 for t in CPR_NL if not abs(rlat) < t) - (1 if odd else 0)
    dlon = 360.0 / max(nl, 1)
    return int(yz), int(math.floor(nb * mod(lon, dlon) / dlon + 0.5))


def lat_of_raw(raw):
    lat = raw * 360.0 / 16777216.0
    return lat - 180 if lat > 90 else lat


def lon_of_raw(raw):
    lon = raw * 360.0 / 16777216.0
    return lon - 360 if lon > 180 else lon


def build_groups():
    """-> {group: [line bytes, ...]}: seeded, so the golden's maker and the live check build the same streams."""
    rng = np.random.default_rng(978)
    r = lambda n: int(rng.integers(0, n))                                                          # noqa: E731
    g = {k: [] for k in GROUPS}

    # (a) drawn frames: every MDB type and address qualifier, either altitude type, the secondary altitude on either side, every air/ground state
    for t in range(32):
        for aq in range(8):
            for k in range(4):
                raw_alt = r(4096) if k else 0
                g["a"].append(line(payload(t, aq, addr=1 + r(0xFFFFFF), raw_lat=r(1 << 23), raw_lon=r(1 << 24), alt_bit=r(2), raw_alt=raw_alt, nic=r(16),
                                           ag=(k + t) % 4 if k < 3 else 2, raw_a=r(2048), raw_b=r(2048), raw_vvel=r(2048), low16=r(16),
                                           ms=ms_words(r(40), [r(40) for _ in range(8)]), b23_26=(r(256), r(256), r(256), r(256)),
                                           raw_sec=max(0, min(4095, raw_alt + r(41) - 20)) if k != 2 else r(4096)),
                                   extra="rs=%d;rssi=%.1f;t=%d.%03d;" % (r(20), -r(400) / 10.0, r(100000), r(1000))))
    g["a"].append(line(payload(1, 0, addr=0)))                                                     # address 0: nothing
    # (b) CPR edges
    for i, t in enumerate(CPR_NL):
        for sgn in (1, -1):
            for d in (-2, -1, 0, 1, 2):
                g["b"].append(line(payload(1 if d else 0, 0, raw_lat=(raw_of_lat(sgn * t) + d) & 0x7FFFFF, raw_lon=r(1 << 24), ag=2 if (i + d) % 3 == 0 else 0, raw_b=0x2AA)))
    for raw_lat in (0, 1, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, (1 << 23) - 1):                   # 0, +90, -90 (just past), just below 0
        for raw_lon in (0, 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 24) - 1):               # 0, +180, -180 (just past), just below 0
            for nic in (0, 7):
                for ag in (0, 1, 2):
                    g["b"].append(line(payload(2, 0, raw_lat=raw_lat, raw_lon=raw_lon, nic=nic, ag=ag, raw_b=0x2AA)))
    for surface in (False, True):                                                                  # zone edges: YZ or XZ rounds up to NbPow
        found = {"yz": 0, "xz": 0}
        for odd in (0, 1):
            dlat = 360.0 / (59 if odd else 60)
            for zone in list(range(1, 15)) + list(range(-14, 0)):
                base = raw_of_lat(zone * dlat)
                for d in range(-3, 4):
                    raw = (base + d) & 0x7FFFFF
                    yz, _ = cpr_model(lat_of_raw(raw), 10.0, odd, surface)
                    found["yz"] += yz == (1 << 19 if surface else 1 << 17)
                    g["b"].append(line(payload(0, 0, raw_lat=raw, raw_lon=raw_of_lon(10.0), ag=2 if surface else 0, raw_b=0x2AA)))
            for lat in (0.5, -33.0, 52.25, -71.0):
                yz, _ = cpr_model(lat, 0.0, odd, surface)
                rlat = dlat * (1.0 * yz / (1 << 19 if surface else 1 << 17) + math.floor(lat / dlat))
                nl = max(1, 59 - sum(1 for t in CPR_NL if not abs(rlat) < t) - odd)
                for zone in (1, 2, nl // 2, nl - 1, -1, -2):
                    base = raw_of_lon(zone * 360.0 / nl)
                    for d in range(-3, 4):
                        raw = (base + d) & 0xFFFFFF
                        _, xz = cpr_model(lat_of_raw(raw_of_lat(lat)), lon_of_raw(raw), odd, surface)
                        found["xz"] += xz == (1 << 19 if surface else 1 << 17)
                        g["b"].append(line(payload(0, 2, raw_lat=raw_of_lat(lat), raw_lon=raw, ag=2 if surface else 1, raw_b=0x2AA)))
        assert found["yz"] >= 5 and found["xz"] >= 5, found
    for lat in (-80.0, -45.5, -0.01, 0.01, 37.7, 89.9):                                            # negative latitudes, the surface in every quadrant
        for lon in (-179.0, -90.25, -0.01, 0.01, 120.5, 179.9):
            for ag in (0, 2):
                g["b"].append(line(payload(1, 0, raw_lat=raw_of_lat(lat), raw_lon=raw_of_lon(lon), ag=ag, raw_b=0x2AA + r(256))))
    # (c) callsigns and squawks
    for em in range(40):
        for flag in (0x02, 0x00):
            for aq in (0, 2, 1, 3):
                text = idx("N%dAB" % (100 + em)) if flag else idx("%04d" % (1000 + 37 * em))
                g["c"].append(line(payload(1 if em % 2 else 3, aq, ms=ms_words(em, text), b23_26=(0, 0, 0, flag))))
    names = ["AB CD", "AB.CD", " LEAD", "TRAIL  ", "", " ", ".", "A       "[:8], "A B C D ", "....", "X", "0X12", "ABCDEFGH", "A.B C.D "]
    squawks = ["7500", "7600", "7700", "7500 ", " 7500", "  7700", "75000", "750", "0X12", "0X", "0XG", "0X7500", "ABCD", "FFFF", "12G4", "1.23", "1 23", "7777", "0000",
               "", " ", ".", "0X0X", "X7500", "00007500", "FFFFFFFF", "7600.", "7700 1"]
    for alt in (False, True):
        for aq in (0, 2, 4):
            for text in names:
                g["c"].append(line(payload(1, aq, ms=ms_words(3, idx(text, alt)), b23_26=(0, 0, 0, 0x02))))
            for text in squawks:
                g["c"].append(line(payload(3, aq, ms=ms_words(9, idx(text, alt)), b23_26=(0, 0, 0, 0x00))))
    # (d) encoder boundaries and saturations
    for raw_gs in (0, 1, 2, 3, 4, 5, 16, 17, 18, 71, 72, 73, 101, 102, 103, 106, 107, 176, 177, 178, 1022, 1023, 0x400, 0x401, 0x403, 0x7FF):
        for tt in (0, 1, 2, 3):
            g["d"].append(line(payload(0, 0, ag=2, raw_a=raw_gs, raw_b=tt << 9 | r(512))))
    for raw_trk in (0, 1, 2, 3, 4, 255, 256, 509, 510, 511):
        g["d"].append(line(payload(0, 0, ag=2, raw_a=10, raw_b=1 << 9 | raw_trk)))
    for raw_alt in (0, 1, 2, 3, 40, 41, 0x7FE, 0x7FF, 0x800, 0x801, 0x802, 4094, 4095):
        for alt_bit in (0, 1):
            for raw_sec in (0, 1, raw_alt, max(0, raw_alt - 1), min(4095, raw_alt + 1), min(4095, raw_alt + 125), min(4095, raw_alt + 126), min(4095, raw_alt + 127),
                            max(0, raw_alt - 125), max(0, raw_alt - 126), max(0, raw_alt - 127), 4095):
                for nic in (0, 5):
                    g["d"].append(line(payload(2, 0, raw_lat=0 if not nic else 0x155555, raw_lon=0 if not nic else 0x955555, alt_bit=alt_bit, raw_alt=raw_alt, nic=nic, raw_sec=raw_sec)))
    for raw_v in (0, 1, 2, 3, 4, 5, 6, 1021, 1022, 1023, 0x400, 0x401, 0x402, 0x405, 0x7FE, 0x7FF):
        for ag in (0, 1):
            g["d"].append(line(payload(0, 0, ag=ag, raw_a=raw_v, raw_b=0x010, raw_vvel=0)))
            g["d"].append(line(payload(0, 0, ag=ag, raw_a=0, raw_b=raw_v, raw_vvel=0x403)))
    for raw_vv in (0, 1, 2, 3, 510, 511, 0x200, 0x201, 0x202, 0x3FF, 0x400, 0x401, 0x5FF, 0x600, 0x601, 0x7FF):
        for ag in (0, 1):
            g["d"].append(line(payload(0, 0, ag=ag, raw_a=0, raw_b=0, raw_vvel=raw_vv)))
            g["d"].append(line(payload(0, 0, ag=ag, raw_a=3, raw_b=0, raw_vvel=raw_vv)))
    # (e) line syntax
    pl = payload(1, 0)
    g["e"] += [line(pl, upper=False), line(pl, upper=True), ("-" + pl.hex()[:10].upper() + pl.hex()[10:] + ";ss=-3.0;\n").encode()]
    for bad in ("g0", "0g", "G1", " 1", "1 ", "0x", "-1", "1;", "z9"):
        h = pl.hex()
        g["e"].append(("-" + h[:20] + bad + h[22:] + ";rssi=-5.0;\n").encode())
    g["e"].append(("-" + pl.hex()[:67] + ";rssi=-5.0;\n").encode())                                # an odd digit before the ';'
    g["e"] += [("-" + pl.hex() + "\n").encode(), ("-" + pl.hex()[:40] + "\n").encode(), b"-\n", b"-0\n"]       # no ';'
    g["e"] += [line(pl, sign="+"), ("+" + "00" * 432 + ";rs=1;ss=-2.0;\n").encode(), b"+\n", b"+;ss=-2.0;\n"]             # uplink
    g["e"] += [b"\n", b"\n", b"\r\n", b" \n", b"#comment\n", line(pl, sign="*"), line(pl, sign="<"), b";\n"]              # empty lines, other first bytes
    g["e"] += [line(pl, extra="rssi=-7.5;\r"), line(pl, extra="rs=1;\r"), ("-" + pl.hex() + ";\r\n").encode()]
    g["e"] += [b"-" + pl.hex().encode() + b";rs=1;\0ss=-9.0;\n", b"-" + pl.hex()[:30].encode() + b"\0" + pl.hex()[30:].encode() + b";ss=-9.0;\n",
               b"-" + pl.hex().encode() + b";ss=-9.0\0;rssi=-3.0;\n", b"\0-" + pl.hex().encode() + b";ss=-9.0;\n", b"-" + pl.hex().encode() + b"\0\n"]
    g["e"] += [line(pl, extra="ss=-10.0;rssi=-20.0;"), line(pl, extra="rssi=-20.0;ss=-10.0;"), line(pl, extra="ss=0.0;rssi=-20.0;"), line(pl, extra="ss=-0.0;rssi=-6.5;"),
               line(pl, extra="rssi=0;ss=0;rssi=-1.5;ss=-30.0;"), line(pl, extra="ss=0;rssi=-0;"), line(pl, extra="rs=3;t=5.5;"), line(pl, extra=""),
               line(pl, extra="xss=-10.0;rssi=-4.0;"), line(pl, extra="SS=-10.0;"), line(pl, extra=";ss=-10.0;"), line(pl, extra=";;;rssi=-11.0"),
               line(pl, extra="ss=+5.5;"), line(pl, extra="ss=+0;ss=-0;rssi=+000;ss=007;"), line(pl, extra="ss=999.9;"), line(pl, extra="ss=-999.9;"),
               line(pl, extra="ss=-99;"), line(pl, extra="ss=-100"), line(pl, extra="rssi=-48.2"), line(pl, extra="t=1.0;ss=-3.3;rssi=-9.9;")]
    base = line(pl, extra="rssi=-12.3;t=")
    g["e"].append(base[:-1] + b"1" * (DEV_LINE_MAX + 1 - len(base)) + b"\n")                        # 256 bytes: the longest line the device takes
    for nb in (34, 35, 100, 122):                                                                  # longer payloads: decoded from their first bytes
        g["e"].append(("-" + (pl + bytes(range(nb - 34))).hex() + ";ss=-4.0;\n").encode())
    steps = [k for k in range(-9998, 10000) if sig_model(k) != sig_model(k - 1)]
    assert len(steps) >= 100
    for k in sorted(set(steps + [s - 1 for s in steps] + [-9999, 9999, -1, 0, 1])):
        a = abs(k)
        g["e"].append(line(payload(0, 0), extra="rssi=%s%d.%d;" % ("-" if k < 0 else "", a // 10, a % 10)))
    # (f) the deferral group: values outside the simple form, lines longer than the device takes
    for v in ("1e1", "-1.5e+1", "-2E0", "12.34", "-12.30", "0012.3", "1234", " 5.0", "\t-5.0", "inf", "-inf", "INF", "nan", "infinity", "0x1p3", "-0x1.8p1", "5.", ".5", "-.5",
              "+-5", "-", "", "abc", "5.0x", "5 ", "1,5", "--5.0"):
        g["f"].append(line(pl, extra="rssi=%s;" % v))
        g["f"].append(line(payload(0, 2), extra="rs=1;ss=%s" % v))
    g["f"] += [line(pl, extra="ss=0;rssi=1e0;"), line(pl, extra="rssi=-0.00;ss=-3.0;"), line(pl, extra="rssi=-7.5\r")]       # ('\r' is content)
    for total in (258, 259, 300, 1000):
        base = line(pl, extra="rssi=-12.3;t=")
        g["f"].append(base[:-1] + b"1" * (total - len(base)) + b"\n")
    g["f"].append(("-" + (pl + bytes(398)).hex() + ";ss=-4.0;\n").encode())                        # 432 payload bytes: the most the reference takes
    g["f"].append(("-" + (pl + bytes(399)).hex() + ";ss=-4.0;\n").encode())                        # 433: nothing
    g["f"].append(b"-" + pl.hex().encode() + b";ss=-9.0;\0" + b"x" * 300 + b"\n")                  # long by its bytes, short by its content
    return g


def stream_of(lines):
    return b"".join(lines)


def have_ref_objs():
    return all(os.path.exists(p) for p in REF_OBJS)


def build_ref_harness(tmp):
    exe = os.path.join(tmp, "uat_ref_harness")
    subprocess.run(["gcc", "-std=gnu11", "-O2", "-Wall", "-o", exe, HARNESS_SRC, *REF_OBJS, "-lm"], check=True)
    return exe


def run_ref_harness(exe, stream, tmp):
    """-> (the reference's bytes, a length per line)"""
    paths = [os.path.join(tmp, n) for n in ("uat_stream.bin", "uat_out.bin", "uat_lens.bin")]
    open(paths[0], "wb").write(stream)
    subprocess.run([exe, *paths], check=True, timeout=300)
    return open(paths[1], "rb").read(), np.fromfile(paths[2], dtype=np.int32)


def load_golden():
    """-> {group: (stream bytes, the reference's bytes, a length per line)}"""
    z = np.load(GOLDEN)
    return {g: (z[g + "_stream"].tobytes(), z[g + "_out"].tobytes(), z[g + "_lens"].astype(np.int32)) for g in GROUPS}


def split_lines(stream):
    """The complete lines of a stream, without their '\\n'."""
    parts = stream.split(b"\n")
    return parts[:-1]


def frames_of(out):
    """The AVR lines of an output -> (signal bytes, frames as an [n, 14] array)."""
    assert len(out) % FRAME_TEXT == 0
    n = len(out) // FRAME_TEXT
    sig = np.zeros(n, dtype=np.uint8)
    frames = np.zeros((n, 14), dtype=np.uint8)
    for k in range(n):
        t = out[k * FRAME_TEXT: (k + 1) * FRAME_TEXT]
        assert t[:13] == b"<FF004D4C4155" and t[43:] == b";\n", t
        sig[k] = int(t[13:15], 16)
        frames[k] = np.frombuffer(bytes.fromhex(t[15:43].decode()), dtype=np.uint8)
    return sig, frames


def expected(out, lens, deferred=()):
    """What a call over a golden stream must give, from the reference's bytes: (text, line_of, ndeferred-free lens).  The deferred
    lines' bytes are cut out."""
    lens = np.asarray(lens, dtype=np.int64).copy()
    starts = np.concatenate([[0], np.cumsum(lens)])
    keep = np.ones(len(lens), dtype=bool)
    keep[list(deferred)] = False
    text = b"".join(out[starts[k]: starts[k + 1]] for k in range(len(lens)) if keep[k])
    line_of = np.repeat(np.arange(len(lens))[keep], (lens[keep] // FRAME_TEXT))
    return text, line_of.astype(np.uint64)


def merge_deferred(text, line_of, settled):
    """The device's text with the host-settled lines {index: bytes} put where they belong."""
    out, at = [], 0
    pending = sorted(settled.items())
    for k in range(len(line_of)):
        while pending and pending[0][0] < line_of[k]:
            out.append(pending.pop(0)[1])
        out.append(text[at: at + FRAME_TEXT])
        at += FRAME_TEXT
    out += [t for _, t in pending]
    return b"".join(out)


def feed(nlines, seed=1):
    """A drawn feed of dump978's form: mostly type 1 and 0 airborne targets, some on the ground, a few uplink and noise lines."""
    rng = np.random.default_rng(seed)
    r = lambda n: int(rng.integers(0, n))                                                          # noqa: E731
    lines = []
    for k in range(nlines):
        u = r(100)
        if u < 2:
            lines.append(("+" + bytes(rng.integers(0, 256, 40, dtype=np.uint8)).hex() + ";rs=%d;rssi=-%d.%d;\n" % (r(20), r(40), r(10))).encode())
            continue
        t = 1 if u < 60 else 0 if u < 90 else (2, 3, 5, 6)[u % 4]
        pl = payload(t, (0, 0, 0, 2, 3)[u % 5], addr=0xA00000 + r(4000), raw_lat=raw_of_lat(25 + r(2400) / 100.0) + r(64), raw_lon=raw_of_lon(-125 + r(5800) / 100.0) + r(64),
                     alt_bit=0, raw_alt=41 + r(1600), nic=8, ag=2 if u % 17 == 0 else 0, raw_a=r(600) | (r(2) << 10), raw_b=r(600) | (r(2) << 10), raw_vvel=r(64) | (r(4) << 9),
                     ms=ms_words(1 + r(6), idx("N%d" % (1000 + r(9000)))), b23_26=(0x24, 0x10, 0xA5, 0x02 if u % 3 else 0), raw_sec=41 + r(1600))
        lines.append(line(pl, extra="rs=%d;rssi=-%d.%d;t=%d.%03d;" % (r(20), r(40), r(10), 1700000000 + k // 500, r(1000))))
    return lines
