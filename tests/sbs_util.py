"""The text outputs' checker and its inputs: plain Python references of modesSendSBSOutput (net_io.c:3184-3404) and modesSendRawOutput
(net_io.c:1837-1863) with the line rules of mgpu_sbs_encode_ex* / mgpu_raw_encode_ex* (include/modes_gpu.h) on top, the case generators
of tests/golden/make_text_golden.py, and the driver of tests/host_stub/text_ref_harness.c (the reference's own two writers).
tests/test_text_reference.py pins the references (CPU); tests/test_gpu_text.py compares the kernels with them, byte for byte.

'%.6f' % x and '%.0f' % x are correctly rounded conversions of the exact binary value (round half to even), as glibc's printf."""
import os
import re
import shlex
import subprocess
import time

import numpy as np

import helpers
from readsb_amd.binding import DEFERRED_DTYPE as DEFERRED, FIELDS_DTYPE as FIELDS, MSG_DTYPE as MSG, POSITION_DTYPE as POSITION

BLOCK = 256                                    # messages per workgroup of k_text_size / k_text_write
SBS_LINE_MAX, RAW_LINE_MAX = 176, 43
MS_END = 253402300800000                       # 10000-01-01: sysTimestamp and now_ms lie in [0, MS_END)
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
MGPU_E_INVAL, MGPU_E_OVERFLOW = -1, -5
NOW_MS = 1700000000123                         # 2023/11/14 22:13:20.123

# flags of struct mgpu_fields the SBS line reads
F_BARO_ALT, F_GEOM_ALT, F_HEADING, F_GS = 1 << 0, 1 << 1, 1 << 2, 1 << 3
F_BARO_RATE, F_GEOM_RATE, F_SQUAWK, F_CALLSIGN = 1 << 6, 1 << 7, 1 << 8, 1 << 9
F_SPI_VALID, F_SPI, F_ALERT_VALID, F_ALERT = 1 << 14, 1 << 15, 1 << 16, 1 << 17
NON_ICAO = 1 << 24
HEADING_GROUND_TRACK = 1
GATE_DROP, GATE_FORWARD, GATE_DEFER, GATE_RELIABLE, GATE_POSSIBLE, GATE_CERTAIN = 0, 1, 2, 4, 8, 16
POS_METHODS = (1, 2, 3)                        # MGPU_CPR_GLOBAL / _LOCAL_RECEIVER / _LOCAL_AIRCRAFT

NONE, LINE, DEFER, SKIP = 0, 1, 2, 3


def sbs_msg_type(df, me):
    if df in (4, 20):
        return 5
    if df in (5, 21):
        return 6
    if df in (0, 16):
        return 7
    if df == 11:
        return 8
    if df in (17, 18):
        return 1 if 1 <= me <= 4 else 2 if 5 <= me <= 8 else 3 if 9 <= me <= 18 else 4 if me == 19 else 0
    return 0


def _date_time(ms):
    t = time.gmtime(ms // 1000)
    return "%04d/%02d/%02d,%02d:%02d:%02d.%03d" % (t.tm_year, t.tm_mon, t.tm_mday, t.tm_hour, t.tm_min, t.tm_sec, ms % 1000)


def _wrap32(v):
    return (v + (1 << 31)) % (1 << 32) - (1 << 31)


def sbs_classes(fields, sys_ts, positions=None, verdict=None):
    """Per message NONE / LINE / DEFER / SKIP, in the order the header gives: verdict, format, domain."""
    n = len(fields)
    cls = np.full(n, LINE, dtype=np.uint8)
    if verdict is not None:
        v = np.asarray(verdict).astype(np.uint8)
        w = v & 3
        due = (w == GATE_FORWARD) & ((v & GATE_CERTAIN) != 0)
        dfr = ~due & ((w == GATE_DEFER) | (w == GATE_FORWARD)) & ((v & GATE_POSSIBLE) != 0)
        cls = np.where(due, LINE, np.where(dfr, DEFER, NONE)).astype(np.uint8)
    df, me = fields["msgtype"], fields["metype"]
    typ = np.array([sbs_msg_type(int(a), int(b)) for a, b in zip(df.tolist(), me.tolist())], dtype=np.uint8) if n else np.zeros(0, dtype=np.uint8)
    cls[((fields["addr"] & NON_ICAO) != 0) | (typ == 0)] = NONE
    t = np.asarray(sys_ts).astype(np.int64)
    ok = (t >= 0) & (t < MS_END)
    with np.errstate(invalid="ignore"):
        gs, hd = fields["gs_selected"].astype(np.float64), fields["heading"].astype(np.float64)
        ok &= ~((fields["flags"] & F_GS) != 0) | (np.abs(gs) < 2147483648.0)
        has_hd = ((fields["flags"] & F_HEADING) != 0) & (fields["heading_type"] == HEADING_GROUND_TRACK)
        ok &= ~has_hd | (np.abs(hd) < 2147483648.0)
        if positions is not None:
            has_pos = np.isin(positions["method"], POS_METHODS)
            ok &= ~has_pos | ((np.abs(positions["lat"]) <= 90.0) & (np.abs(positions["lon"]) <= 360.0))
    cls[(cls != NONE) & ~ok] = SKIP
    return cls, typ


def sbs_line(typ, f, sys_ts, now_text, pos, delta, use_gnss, override_squawk):
    """One line, fields 1-22 (net_io.c:3249-3401).  f: a FIELDS record as a dict of Python values; pos: (lat, lon) or None."""
    p = ["MSG,%d,1,1,%06X,1," % (typ, f["addr"]), _date_time(sys_ts), ",", now_text]
    flags = f["flags"]
    p.append(",")
    if flags & F_CALLSIGN:
        p.append(f["callsign"].split(b"\0")[0].decode("latin-1"))
    baro, geom, dv = flags & F_BARO_ALT, flags & F_GEOM_ALT, delta != INT32_MIN
    if use_gnss:
        if geom:
            p.append(",%dH" % f["geom_alt"])
        elif baro and dv:
            p.append(",%dH" % _wrap32(f["baro_alt"] + delta))
        elif baro:
            p.append(",%d" % f["baro_alt"])
        else:
            p.append(",")
    else:
        if baro:
            p.append(",%d" % f["baro_alt"])
        elif geom and dv:
            p.append(",%d" % _wrap32(f["geom_alt"] - delta))
        else:
            p.append(",")
    p.append(",%.0f" % f["gs_selected"] if flags & F_GS else ",")
    p.append(",%.0f" % f["heading"] if (flags & F_HEADING) and f["heading_type"] == HEADING_GROUND_TRACK else ",")
    p.append(",%1.6f,%1.6f" % pos if pos is not None else ",,")
    br, gr = flags & F_BARO_RATE, flags & F_GEOM_RATE
    if use_gnss:
        p.append(",%dH" % f["geom_rate"] if gr else ",%d" % f["baro_rate"] if br else ",")
    else:
        p.append(",%d" % f["baro_rate"] if br else ",%d" % f["geom_rate"] if gr else ",")
    sq = flags & F_SQUAWK
    p.append(",%04d" % override_squawk if override_squawk != -1 else ",%04d" % f["squawkDec"] if sq else ",")
    p.append((",-1" if flags & F_ALERT else ",0") if flags & F_ALERT_VALID else ",")
    p.append((",-1" if f["squawkHex"] in (0x7500, 0x7600, 0x7700) else ",0") if sq else ",")
    p.append((",-1" if flags & F_SPI else ",0") if flags & F_SPI_VALID else ",")
    p.append(",-1" if f["airground"] == 1 else ",0" if f["airground"] == 2 else ",")
    p.append("\r\n")
    return "".join(p).encode("latin-1")


_SBS_NAMES = ("addr", "flags", "callsign", "baro_alt", "geom_alt", "gs_selected", "heading", "heading_type", "baro_rate", "geom_rate", "squawkDec",
              "squawkHex", "airground")


def sbs_reference(msgs, fields, now_ms, positions=None, verdict=None, geom_delta=None, use_gnss=False, override_squawk=-1):
    """-> (stream bytes, line length per message (0: none), deferred[] {index, offset}, the number of skipped messages)"""
    n = len(msgs)
    assert len(fields) == n and 0 <= now_ms < MS_END
    cls, typ = sbs_classes(fields, msgs["sysTimestamp"], positions, verdict)
    now_text = _date_time(int(now_ms))
    cols = {k: fields[k].tolist() for k in _SBS_NAMES}
    ts = msgs["sysTimestamp"].tolist()
    has_pos = np.isin(positions["method"], POS_METHODS).tolist() if positions is not None else None
    lat, lon = (positions["lat"].tolist(), positions["lon"].tolist()) if positions is not None else (None, None)
    delta = np.asarray(geom_delta).astype(np.int64).tolist() if geom_delta is not None else None
    lines, length = [], np.zeros(n, dtype=np.int64)
    for i in np.nonzero(cls == LINE)[0].tolist():
        f = {k: cols[k][i] for k in _SBS_NAMES}
        line = sbs_line(int(typ[i]), f, ts[i], now_text, (lat[i], lon[i]) if has_pos is not None and has_pos[i] else None,
                        delta[i] if delta is not None else INT32_MIN, use_gnss, override_squawk)
        assert len(line) <= SBS_LINE_MAX
        lines.append(line)
        length[i] = len(line)
    start = np.cumsum(length) - length
    dsel = cls == DEFER
    out = np.zeros(int(dsel.sum()), dtype=DEFERRED)
    out["index"], out["offset"] = np.nonzero(dsel)[0], start[dsel]
    return b"".join(lines), length, out, int((cls == SKIP).sum())


def raw_reference(msgs, mlat=False, verdict=None, net_rule=False, verbatim=False):
    """-> (stream bytes, line length per message, deferred[] {index, offset})"""
    n = len(msgs)
    bits = msgs["msgbits"]
    carried = np.isin(bits, (16, 56, 112))
    emit, deferred = carried.copy(), np.zeros(n, dtype=bool)
    if not verbatim:
        wire_ok = (msgs["correctedbits"] < 2) if net_rule else np.ones(n, dtype=bool)
        emit &= wire_ok
        if verdict is not None:
            v = np.asarray(verdict).astype(np.uint8) & 3
            deferred = emit & (v == GATE_DEFER)
            emit = emit & (v == GATE_FORWARD)
    payload = msgs["raw"] if verbatim else msgs["msg"]
    ts = msgs["timestamp"].astype(np.int64).tolist()
    lines, length = [], np.zeros(n, dtype=np.int64)
    for i in np.nonzero(emit)[0].tolist():
        if mlat and ts[i] != 0:
            head = ("@%012X" % (ts[i] & 0xFFFFFFFFFFFFFFFF))[:13]          # sprintf, then p += 13: the first twelve digits stay
        else:
            head = "*"
        line = (head + payload[i, :bits[i] // 8].tobytes().hex().upper() + ";\n").encode()
        lines.append(line)
        length[i] = len(line)
    start = np.cumsum(length) - length
    out = np.zeros(int(deferred.sum()), dtype=DEFERRED)
    out["index"], out["offset"] = np.nonzero(deferred)[0], start[deferred]
    return b"".join(lines), length, out


# ---- case generators ---------------------------------------------------------------------------------------------------------------

VERDICTS = np.array([GATE_DROP, GATE_DROP | GATE_POSSIBLE, GATE_FORWARD, GATE_FORWARD | GATE_POSSIBLE, GATE_FORWARD | GATE_RELIABLE | GATE_POSSIBLE | GATE_CERTAIN,
                     GATE_FORWARD | GATE_POSSIBLE | GATE_CERTAIN, GATE_DEFER, GATE_DEFER | GATE_POSSIBLE, GATE_DEFER | GATE_RELIABLE | GATE_POSSIBLE, 3,
                     GATE_FORWARD | GATE_CERTAIN], dtype=np.uint8)


def gate_like_verdicts(n, seed, p_due=0.7):
    """Verdict bytes as the gate writes them and a few it never writes: p_due of them a line for certain."""
    rng = np.random.default_rng(seed)
    v = VERDICTS[rng.integers(0, len(VERDICTS), size=n)]
    due = rng.random(n) < p_due
    v[due] = np.where(rng.random(int(due.sum())) < 0.5, VERDICTS[4], VERDICTS[5])
    return v


def empty_cases(n):
    return {"msgs": np.zeros(n, dtype=MSG), "fields": np.zeros(n, dtype=FIELDS), "positions": np.zeros(n, dtype=POSITION),
            "verdict": np.full(n, VERDICTS[4], dtype=np.uint8), "geom_delta": np.full(n, INT32_MIN, dtype=np.int32)}


def concat_cases(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def slice_cases(c, lo, hi):
    return {k: v[lo:hi] for k, v in c.items()}


def fuzz_cases(per_type, seed):
    """(a) field records of fuzzed frames of every DF / ME type through the oracle's field decode, balanced so that every msgType 1-8
    and every no-line path has per_type records; gate-like verdicts, candidate positions on the records that carry a CPR word."""
    import fields_util as fu
    rng = np.random.default_rng(seed)
    es_frames, es_bits = fu.fuzz_frames(60 * per_type, seed + 1, dfs=(17, 18))
    ot_frames, ot_bits = fu.fuzz_frames(24 * per_type, seed + 2, dfs=(0, 4, 5, 11, 16, 20, 21, 24, 27, 31))
    frames, bits = np.concatenate([es_frames, ot_frames]), np.concatenate([es_bits, ot_bits])
    fields = fu.oracle_fields(frames, bits).view(FIELDS)
    typ = np.array([sbs_msg_type(int(a), int(b)) for a, b in zip(fields["msgtype"].tolist(), fields["metype"].tolist())])
    icao = (fields["addr"] & NON_ICAO) == 0
    es = np.isin(fields["msgtype"], (17, 18))
    groups = [np.nonzero((typ == t) & icao)[0] for t in range(1, 9)]
    groups += [np.nonzero(~icao & (typ != 0))[0], np.nonzero(~es & (typ == 0))[0], np.nonzero(es & (typ == 0) & icao)[0]]
    pick = []
    for g in groups:
        assert len(g) >= per_type, [len(x) for x in groups]
        pick.append(g[:per_type])
    pick = rng.permutation(np.concatenate(pick))
    n = len(pick)
    c = empty_cases(n)
    c["fields"] = fields[pick].copy()
    c["msgs"]["msg"], c["msgs"]["raw"], c["msgs"]["msgbits"] = frames[pick], frames[pick], bits[pick]
    c["msgs"]["msgtype"], c["msgs"]["addr"] = c["fields"]["msgtype"], c["fields"]["addr"]
    c["msgs"]["sysTimestamp"] = 1690000000000 + np.cumsum(rng.integers(0, 5000, size=n))
    c["msgs"]["timestamp"] = 12000 * (c["msgs"]["sysTimestamp"] - 1690000000000)
    c["verdict"] = gate_like_verdicts(n, seed + 3)
    has_cpr = (c["fields"]["flags"] & (1 << 10)) != 0
    c["positions"]["method"] = np.where(has_cpr, rng.integers(0, 5, size=n), 0)
    placed = np.isin(c["positions"]["method"], POS_METHODS)
    c["positions"]["lat"] = np.where(placed, rng.uniform(-90, 90, size=n), 0.0)
    c["positions"]["lon"] = np.where(placed, rng.uniform(-180, 180, size=n), 0.0)
    c["geom_delta"] = np.where(rng.random(n) < 0.5, INT32_MIN, rng.integers(-2000, 2000, size=n)).astype(np.int32)
    return c


def _base(n, df=17, me=11):
    c = empty_cases(n)
    c["fields"]["msgtype"], c["fields"]["metype"], c["fields"]["addr"] = df, me, 0x4840D6
    c["msgs"]["sysTimestamp"] = NOW_MS + 876
    return c


def edge_cases(seed):
    """(b) records at the edges of the domain, every optional field present and absent in every combination a decoder could not give
    (geometric altitude on a record that has a line), and records outside the domain."""
    rng = np.random.default_rng(seed)
    parts = []
    stamps = [0, 999, 951782399999, 951782400000, 4102444799999, MS_END - 1, 68169599999, 68169600000, 1709164800000, 1709251199999,
              -1, MS_END, INT32_MIN, (1 << 63) - 1, -(1 << 63)]
    c = _base(len(stamps))
    c["msgs"]["sysTimestamp"] = stamps
    parts.append(c)
    # altitudes and rates at the ends of int32, with and without a geom_delta, every valid-flag combination
    vals = [INT32_MIN, INT32_MAX, 0, -1, 38000, -1000]
    combos = [(fl, a, g, d) for fl in range(4) for a in vals for g in (INT32_MAX, INT32_MIN, 360) for d in (INT32_MIN, 0, 1, -1, INT32_MAX, 25)]
    c = _base(len(combos))
    for k, (fl, a, g, d) in enumerate(combos):
        c["fields"]["flags"][k] = (F_BARO_ALT if fl & 1 else 0) | (F_GEOM_ALT if fl & 2 else 0) | (F_BARO_RATE if fl & 2 else 0) | (F_GEOM_RATE if fl & 1 else 0)
        c["fields"]["baro_alt"][k], c["fields"]["geom_alt"][k], c["geom_delta"][k] = a, g, d
        c["fields"]["baro_rate"][k], c["fields"]["geom_rate"][k] = g, a
    parts.append(c)
    # callsigns: full without NUL, inner NUL, leading NUL, empty, bytes above 127
    names = [b"ABCDEFGH", b"AB\0DEFGH", b"\0BCDEFGH", b"", b"A", b"KLM 1023", b"\xff\x80, \r\n\x01\x7f"]
    c = _base(2 * len(names), me=4)
    c["fields"]["callsign"] = names + names
    c["fields"]["flags"][:len(names)] = F_CALLSIGN
    parts.append(c)
    # squawks and the four flags
    sq = [(0, 0), (0x7500, 7500), (0x7600, 7600), (0x7700, 7700), (0x1200, 1200), (0x7777, 7777), (0x0001, 1), (0xFFFF, 65535)]
    c = _base(len(sq) * 8, df=5, me=0)
    for k in range(len(c["verdict"])):
        h, d = sq[k % len(sq)]
        m = k // len(sq)
        c["fields"]["squawkHex"][k], c["fields"]["squawkDec"][k] = h, d
        c["fields"]["flags"][k] = (F_SQUAWK if m & 1 else 0) | (F_ALERT_VALID if m & 2 else 0) | (F_ALERT if m & 4 else 0) | (F_SPI_VALID if m & 4 else 0) \
            | (F_SPI if m & 2 else 0)
        c["fields"]["airground"][k] = k % 5
    parts.append(c)
    # addresses: leading zeros, non-ICAO, bits above 24 (8 digits)
    addrs = [0, 1, 0xABCDEF, 0xFFFFFF, NON_ICAO, NON_ICAO | 0x123456, 0xFE000000, 0xFEFFFFFF, 0x02000000, 0xFFFFFFFF]
    c = _base(len(addrs))
    c["fields"]["addr"] = addrs
    parts.append(c)
    # every DF and ME type
    c = _base(32 + 32 + 2, df=17)
    c["fields"]["metype"][:32] = np.arange(32)
    c["fields"]["msgtype"][32:64], c["fields"]["metype"][32:64] = np.arange(32), 19
    c["fields"]["msgtype"][64:], c["fields"]["metype"][64:] = (77, 18), (1, 31)
    parts.append(c)
    # every verdict byte
    c = _base(256, df=4)
    c["verdict"] = np.arange(256, dtype=np.uint8)
    parts.append(c)
    # the longest line of the domain
    c = _base(2)
    f = c["fields"]
    f["flags"] = F_CALLSIGN | F_GEOM_ALT | F_GS | F_HEADING | F_GEOM_RATE | F_SQUAWK | F_ALERT_VALID | F_ALERT | F_SPI_VALID | F_SPI
    f["callsign"], f["geom_alt"], f["geom_rate"], f["gs_selected"], f["heading"], f["heading_type"] = b"WWWWWWWW", INT32_MIN, INT32_MIN, -2147483520.0, -2147483520.0, 1
    f["squawkHex"], f["squawkDec"], f["airground"] = 0x7700, 65535, 1
    f["addr"] = (0xFFFFFF, 0xFEFFFFFF)
    c["positions"]["method"], c["positions"]["lat"], c["positions"]["lon"] = 1, -89.9999995, -359.9999995
    parts.append(c)
    # flag combinations at random over plausible values: both use_gnss branches of fields 12 and 17 and each H form get their share
    n = 1200
    c = _base(n)
    f = c["fields"]
    f["msgtype"] = rng.choice([0, 4, 5, 11, 16, 17, 18, 20, 21], size=n)
    f["metype"] = rng.integers(1, 20, size=n)
    keep = F_BARO_ALT | F_GEOM_ALT | F_HEADING | F_GS | F_BARO_RATE | F_GEOM_RATE | F_SQUAWK | F_CALLSIGN | F_SPI_VALID | F_SPI | F_ALERT_VALID | F_ALERT
    f["flags"] = rng.integers(0, 1 << 18, size=n) & rng.integers(0, 1 << 18, size=n) & keep
    f["baro_alt"], f["geom_alt"] = rng.integers(-1000, 50000, size=n), rng.integers(-1000, 50000, size=n)
    f["baro_rate"], f["geom_rate"] = rng.integers(-6000, 6000, size=n), rng.integers(-6000, 6000, size=n)
    f["gs_selected"], f["heading"] = rng.uniform(0, 600, size=n), rng.uniform(0, 360, size=n)
    f["heading_type"] = rng.integers(0, 3, size=n)
    f["squawkDec"] = rng.integers(0, 7778, size=n)
    f["airground"] = rng.integers(0, 4, size=n)
    f["callsign"] = [bytes(rng.choice(list(b"ABCXYZ019 "), size=8).tolist()) for _ in range(n)]
    c["geom_delta"] = np.where(rng.random(n) < 0.5, INT32_MIN, rng.integers(-500, 500, size=n)).astype(np.int32)
    c["positions"]["method"] = rng.integers(0, 5, size=n)
    c["positions"]["lat"], c["positions"]["lon"] = rng.uniform(-90, 90, size=n), rng.uniform(-180, 180, size=n)
    c["msgs"]["sysTimestamp"] = rng.integers(0, MS_END, size=n)
    c["verdict"] = gate_like_verdicts(n, seed + 1)
    parts.append(c)
    # outside the domain: floats and positions
    bad_f = [np.inf, -np.inf, np.nan, 2147483648.0, -2147483648.0, 3.0e38, 2147483520.0]
    bad_p = [(np.nan, 0), (0, np.nan), (np.inf, 0), (0, -np.inf), (90.00000000000001, 0), (-90.00000000000001, 0), (0, 360.00000000000006),
             (0, -360.00000000000006), (90.0, 360.0), (-90.0, -360.0), (1e300, 1e300)]
    c = _base(3 * len(bad_f) + 2 * len(bad_p))
    f = c["fields"]
    for k, x in enumerate(bad_f):
        f["gs_selected"][k], f["flags"][k] = x, F_GS
        f["heading"][len(bad_f) + k], f["flags"][len(bad_f) + k], f["heading_type"][len(bad_f) + k] = x, F_HEADING, 1
        f["heading"][2 * len(bad_f) + k], f["gs_selected"][2 * len(bad_f) + k] = x, x          # not valid, or not the ground track: not printed
        f["flags"][2 * len(bad_f) + k], f["heading_type"][2 * len(bad_f) + k] = F_HEADING, 2
    for k, (la, lo) in enumerate(bad_p):
        for m, method in enumerate((1, 4)):
            j = 3 * len(bad_f) + 2 * k + m
            c["positions"]["lat"][j], c["positions"]["lon"][j], c["positions"]["method"][j] = la, lo, method
    parts.append(c)
    return concat_cases(parts)


def tie_doubles(seed, nrandom=2000):
    """(c) every q / 128 for odd q, |q| <= 23040 — the exact ties of six decimals — each with both neighbours; the three doubles
    nearest (k + 0.5) * 1e-6 for random k; zeros, the smallest subnormals, tiny values, the ends of the domain."""
    q = np.arange(1, 23041, 2, dtype=np.float64)
    ties = np.concatenate([q, -q]) / 128.0
    ties = np.concatenate([ties, np.nextafter(ties, np.inf), np.nextafter(ties, -np.inf)])
    rng = np.random.default_rng(seed)
    k = rng.integers(-180000000, 180000000, size=nrandom).astype(np.float64)
    near = (k + 0.5) * 1e-6
    near = np.concatenate([near, np.nextafter(near, np.inf), np.nextafter(near, -np.inf)])
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 90.0, -90.0, 180.0, -180.0, 360.0, -360.0, 4.9999999e-7, 5e-7, 5.0000001e-7,
                        -5e-7, -4.9e-7, 0.9999995, 9.9999995, 99.9999995, 359.9999995, 89.9999995])
    return np.concatenate([ties, near, special])


def double_cases(seed):
    """(c) as SBS records: the values within +-90 go to the latitude, the others to the longitude, two per line."""
    x = tie_doubles(seed)
    lat, lon = x[np.abs(x) <= 90.0], x[np.abs(x) > 90.0]
    n = max(len(lat), len(lon))
    c = _base(n)
    c["positions"]["method"] = 1 + np.arange(n) % 3
    c["positions"]["lat"] = np.resize(lat, n)
    c["positions"]["lon"] = np.resize(np.concatenate([lon, lat]), n)
    return c


def float_cases():
    """(d) k + 0.5 for k = 0 .. 400 with both float neighbours, their negatives, +-0.0f, the largest values of the domain: one on
    the ground speed and another on the heading of every record."""
    k = np.arange(401, dtype=np.float32) + np.float32(0.5)
    x = np.concatenate([k, np.nextafter(k, np.float32(np.inf)), np.nextafter(k, np.float32(-np.inf))])
    x = np.concatenate([x, -x, np.array([0.0, -0.0, 1e-45, -1e-45, 2147483520.0, -2147483520.0, 8388607.5, 8388608.0, 16777216.0, 0.49999997, -0.49999997],
                                        dtype=np.float32)])
    c = _base(len(x), me=19)
    c["fields"]["flags"], c["fields"]["heading_type"] = F_GS | F_HEADING, 1
    c["fields"]["gs_selected"], c["fields"]["heading"] = x, x[::-1]
    return c


def raw_cases(seed):
    """(e) timestamps around the twelve-digit limit, all three lengths and a few the format does not carry, every correctedbits."""
    rng = np.random.default_rng(seed)
    stamps = [0, 1, (1 << 48) - 1, 1 << 48, (1 << 52) + 0xABC, -1, 0x1234567890AB5D, (1 << 56) - 1, 1 << 60, (1 << 63) - 1, -(1 << 63), 0xABCDEF]
    rows = [(t, b, cb) for t in stamps for b in (16, 56, 112, 0, 8, 120, 255) for cb in (0, 1, 2)]
    m = np.zeros(len(rows), dtype=MSG)
    m["timestamp"], m["msgbits"], m["correctedbits"] = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    m["msg"] = rng.integers(0, 256, size=(len(rows), 14))
    m["raw"] = rng.integers(0, 256, size=(len(rows), 14))
    v = np.arange(len(rows), dtype=np.uint8) * 7 % 32
    return m, v


def hostile_cases(n, seed):
    """Random bytes as field and position records, with enough of them steered into the printable domain that lines of every kind appear."""
    rng = np.random.default_rng(seed)
    c = empty_cases(n)
    c["fields"] = rng.integers(0, 256, size=n * FIELDS.itemsize, dtype=np.uint8).view(FIELDS).copy()
    c["positions"] = rng.integers(0, 256, size=n * POSITION.itemsize, dtype=np.uint8).view(POSITION).copy()
    f = c["fields"]
    tame = rng.random(n) < 0.7
    f["msgtype"][tame] = rng.choice([0, 4, 5, 11, 16, 17, 18, 20, 21], size=int(tame.sum()))
    f["metype"][tame] = rng.integers(0, 24, size=int(tame.sum()))
    f["addr"][tame] &= 0xFEFFFFFF
    okf = rng.random(n) < 0.6
    f["gs_selected"][okf], f["heading"][okf] = rng.uniform(-700, 700, size=int(okf.sum())), rng.uniform(-400, 400, size=int(okf.sum()))
    c["positions"]["method"] = rng.integers(0, 6, size=n)
    okp = rng.random(n) < 0.6
    c["positions"]["lat"][okp], c["positions"]["lon"][okp] = rng.uniform(-90, 90, size=int(okp.sum())), rng.uniform(-360, 360, size=int(okp.sum()))
    c["msgs"]["sysTimestamp"] = np.where(rng.random(n) < 0.9, rng.integers(0, MS_END, size=n), rng.integers(-(1 << 63), (1 << 63) - 1, size=n))
    c["verdict"] = rng.integers(0, 256, size=n, dtype=np.uint8)
    c["verdict"][rng.random(n) < 0.5] = VERDICTS[4]
    c["geom_delta"] = rng.integers(INT32_MIN, INT32_MAX, size=n).astype(np.int32)
    c["geom_delta"][rng.random(n) < 0.3] = INT32_MIN
    return c


def sbs_of(c, now_ms=NOW_MS, **kw):
    """sbs_reference on a case set."""
    return sbs_reference(c["msgs"], c["fields"], now_ms, positions=c["positions"], verdict=c["verdict"], geom_delta=c["geom_delta"], **kw)


# ---- the golden file ------------------------------------------------------------------------------------------------------------------

GOLDEN = os.path.join(helpers.GOLDEN_DIR, "text_cases.npz")
GROUPS = ("a", "b", "c", "d")
OVERRIDES = (0, 7700, 2147483647)
RAW_VARIANTS = [(mlat, net_rule, verbatim) for mlat in (False, True) for net_rule in (False, True) for verbatim in (False, True)]


def override_cases(b):
    """The records of group (b) the override squawks are run on: every fourth."""
    return {k: v[::4] for k, v in b.items()}


def in_domain(c):
    """The records the reference's writer can be given: all but those the skip rule takes out."""
    keep = sbs_classes(c["fields"], c["msgs"]["sysTimestamp"], c["positions"], None)[0] != SKIP
    return {k: v[keep] for k, v in c.items()}


def load_golden():
    """-> (the SBS case sets by group, the raw records and their verdicts, the stored streams by name: ref_* the reference's own bytes,
    want_raw_* the raw streams with the library's rules on top, the class of every SBS record by group)"""
    z = np.load(GOLDEN)
    sets = {g: {k: z[f"{g}_{k}"] for k in ("msgs", "fields", "positions", "verdict", "geom_delta")} for g in GROUPS}
    streams = {k: z[k].tobytes() for k in z.files if k.startswith(("want_", "ref_"))}
    for alias in z["aliases"].tolist():
        name, same_as = alias.split("=")
        streams[name] = streams[same_as]
    return sets, (z["e_msgs"], z["e_verdict"]), streams, {g: z[f"cls_{g}"] for g in GROUPS}


def raw_expectations(m, v):
    """Every raw stream the golden pins beyond the reference's own: name -> bytes."""
    out = {}
    for mlat, net_rule, verbatim in RAW_VARIANTS:
        for gated in (0, 1):
            out[f"raw_m{int(mlat)}n{int(net_rule)}v{int(verbatim)}g{gated}"] = raw_reference(m, mlat, v if gated else None, net_rule, verbatim)[0]
    return out


# ---- the reference's own writers (tests/host_stub/text_ref_harness.c) -----------------------------------------------------------------

REF_FULL = os.path.join(helpers.ORACLE_DIR, "_ref", "full")
HARNESS_SRC = os.path.join(helpers.ROOT, "tests", "host_stub", "text_ref_harness.c")
HARNESS_CASE = np.dtype([("sysTimestamp", "<i8"), ("timestamp", "<i8"), ("lat", "<f8"), ("lon", "<f8"), ("geom_delta", "<i4"), ("msgbits", "<i4"),
                         ("has_pos", "u1"), ("delta_valid", "u1"), ("kind", "u1"), ("pad", "u1", 5), ("msg", "u1", 14), ("raw", "u1", 14), ("pad2", "u1", 4),
                         ("fields", FIELDS)])


def have_ref_full():
    return os.path.isdir("/root/reference") and os.path.exists(os.path.join(REF_FULL, "readsb.o"))


def _oracle_make_var(name):
    """A variable of oracle/Makefile (continuation lines joined): the harness is built from what `make -C oracle full` builds, with its flags."""
    text = open(os.path.join(helpers.ORACLE_DIR, "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^%s\s*=\s*(.*)$" % name, text, flags=re.M)
    assert m, name
    return shlex.split(m.group(1))


def _full_build():
    """-> (the object files of the full reference build but net_io.o and readsb.o, its compiler flags without the include paths)"""
    objs = [s.replace("/", "_") for s in _oracle_make_var("FULL_SRCS") if s not in ("net_io", "readsb")]
    flags = [f for f in _oracle_make_var("FULL_CFLAGS") if not f.startswith("-I")]
    return objs, flags


def build_ref_harness(workdir):
    """tests/host_stub/text_ref_harness.c — which includes the reference's net_io.c — compiled with the flags of `make -C oracle full`
    and linked against that build's other objects, readsb.o with its main renamed in a copy."""
    exe = os.path.join(workdir, "text_ref_harness")
    main_o = os.path.join(workdir, "readsb_nomain.o")
    subprocess.run(["objcopy", "--redefine-sym", "main=readsb_main", os.path.join(REF_FULL, "readsb.o"), main_o], check=True)
    objs, flags = _full_build()
    subprocess.run(["gcc", *flags, "-I" + os.path.join(helpers.ORACLE_DIR, "stub_full"), "-I/root/reference", HARNESS_SRC, main_o,
                    *[os.path.join(REF_FULL, o + ".o") for o in objs], "-o", exe, "-pthread", "-lpthread", "-lm", "-lrt", "-l:libzstd.so.1", "-lz"], check=True)
    return exe


def run_ref_harness(exe, kind, c, now_ms=NOW_MS, use_gnss=False, override_squawk=-1, mlat=False, verbatim=False, workdir=None):
    """kind 'sbs': every record of the case set through modesSendSBSOutput; 'raw': c = message records through modesSendRawOutput.
    -> (the bytes written, the length written per record)"""
    if kind == "sbs":
        n = len(c["msgs"])
        rec = np.zeros(n, dtype=HARNESS_CASE)
        rec["sysTimestamp"], rec["fields"] = c["msgs"]["sysTimestamp"], c["fields"]
        rec["has_pos"] = np.isin(c["positions"]["method"], POS_METHODS)
        rec["lat"], rec["lon"] = c["positions"]["lat"], c["positions"]["lon"]
        rec["delta_valid"] = c["geom_delta"] != INT32_MIN
        rec["geom_delta"] = np.where(c["geom_delta"] != INT32_MIN, c["geom_delta"], 0)
    else:
        n = len(c)
        rec = np.zeros(n, dtype=HARNESS_CASE)
        rec["kind"] = 1
        rec["timestamp"], rec["msgbits"], rec["msg"], rec["raw"] = c["timestamp"], c["msgbits"], c["msg"], c["raw"]
    path = os.path.join(workdir, "cases.bin")
    rec.tofile(path)
    r = subprocess.run([exe, path, str(int(now_ms)), str(int(use_gnss)), str(int(override_squawk)), str(int(mlat)), str(int(verbatim))], check=True,
                       capture_output=True)
    lens = np.frombuffer(r.stdout[: 4 * n], dtype=np.int32)
    return r.stdout[4 * n:], lens
