"""The message dump's checker and its inputs: the case generators of tests/golden/make_dump_golden.py, a plain-Python model of
displayModesMessage's text (model_dump) and of the rules of mgpu_dump_encode_ex* (include/modes_gpu.h) about who gets a dump — the mode's
domain, MGPU_DUMP_QUIET, the deferral of the one transcendental —, the driver of tests/host_stub/dump_ref_harness.c (the reference's own displayModesMessage)
and the golden file's loader.  The expected bytes of every test are the REFERENCE's, cut per case by the lengths the harness recorded:
tests/test_dump_reference.py runs readsb_amd/csrc/dump_format.h against them on the CPU, tests/test_gpu_dump.py the kernels."""
import math
import os
import subprocess
import time

import numpy as np

import helpers
import sbs_util
from readsb_amd.binding import DEFERRED_DTYPE as DEFERRED, FIELDS_DTYPE as FIELDS, MSG_DTYPE as MSG, POSITION_DTYPE as POSITION

BLOCK = 256                                    # messages per workgroup of k_dump_size / k_dump_write
SCAN_THREADS = 1024                            # k_beast_scan: more than BLOCK * SCAN_THREADS messages make it take two rounds
DUMP_MAX = 2599                                # kDumpMax, readsb_amd/csrc/dump_format.h
MS_END = 253402300800000
ONLYADDR, RAW, MLAT, QUIET = 1, 2, 4, 8        # MGPU_DUMP_*
MODES = {"full": 0, "mlat": MLAT, "raw": RAW, "rawmlat": RAW | MLAT, "onlyaddr": ONLYADDR}
NONE, LINE, DEFER, SKIP = 0, 1, 2, 3
HEX_UNKNOWN, NON_ICAO = 0xDEADBEEF, 1 << 24
MAGIC = (0xFF004D4C4154, 0xFF004D4C4155, 0xFF004D4C4160)
POS_METHODS = (1, 2, 3)
MGPU_E_INVAL, MGPU_E_OVERFLOW = -1, -5

F = {name: 1 << bit for bit, name in enumerate(
    ("BARO_ALT", "GEOM_ALT", "HEADING", "GS", "IAS", "TAS", "BARO_RATE", "GEOM_RATE", "SQUAWK", "CALLSIGN", "CPR", "CPR_ODD", "CATEGORY", "GEOM_DELTA", "SPI_VALID",
     "SPI", "ALERT_VALID", "ALERT", "EMERGENCY", "ALT_Q", "ACAS_RA", "ROLL", "TRACK_RATE", "MACH"))}
NAV_HEADING, NAV_FMS, NAV_MCP, NAV_QNH, NAV_MODES = 1, 2, 4, 8, 16
OPTIONAL = ("reduce_forward", "receiver_ids", "positions", "decoded_nic", "decoded_rc")

# struct dump_case of tests/host_stub/dump_ref_harness.c and dump_format_check.cpp
CASE = np.dtype([("msg", MSG), ("fields", FIELDS), ("lat", "<f8"), ("lon", "<f8"), ("receiver_id", "<u8"), ("decoded_rc", "<u4"), ("method", "u1"),
                 ("has_positions", "u1"), ("decoded_nic", "u1"), ("run", "u1"), ("reduce_forward", "u1"), ("pad", "u1", 7)])
assert CASE.itemsize == 280


def empty_cases(n):
    c = {"msgs": np.zeros(n, dtype=MSG), "fields": np.zeros(n, dtype=FIELDS), "positions": np.zeros(n, dtype=POSITION),
         "reduce_forward": np.zeros(n, dtype=np.uint8), "receiver_ids": np.zeros(n, dtype=np.uint64), "decoded_nic": np.zeros(n, dtype=np.uint8),
         "decoded_rc": np.zeros(n, dtype=np.uint32)}
    m = c["msgs"]
    m["msgbits"], m["sig_len"], m["sig_sumsq"], m["sysTimestamp"], m["timestamp"] = 112, 268, 0, 1700000000123, 12000000
    return c


def concat_cases(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def take_cases(c, idx):
    return {k: v[idx] for k, v in c.items()}


# ---- who gets a dump (include/modes_gpu.h) ---------------------------------------------------------------------------------------------

def signal_level(m):
    """mgpu_msg_signal_level, operation by operation in double."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return m["sig_sumsq"].astype(np.float64) / 65535.0 / 65535.0 / m["sig_len"].astype(np.float64)


def rssi_margin(level):
    """|frac(|10 log10 level| * 10) - 0.5|: below 2^-20 the device defers.  level > 0, != 1."""
    t = abs(10.0 * math.log10(level)) * 10.0
    return abs(t - math.floor(t) - 0.5)


def classes(c, flags, show_only=0):
    """Per message NONE / LINE / DEFER / SKIP as dump_classify (readsb_amd/csrc/dump_format.h) decides on the device."""
    m, f = c["msgs"], c["fields"]
    n = len(m)
    cls = np.full(n, LINE, dtype=np.uint8)
    quiet = (f["addr"] != show_only) if flags & QUIET else np.zeros(n, dtype=bool)
    if not flags & ONLYADDR:
        bits = m["msgbits"]
        cls[~((bits == 56) | (bits == 112) | ((bits == 16) & (f["msgtype"] >= 32)))] = SKIP
        if not flags & RAW:
            ok = (m["sysTimestamp"] >= 0) & (m["sysTimestamp"] < MS_END) & (m["timestamp"] >= 0) & (m["sig_len"] != 0)
            with np.errstate(invalid="ignore"):
                def fin(name):
                    return np.abs(f[name].astype(np.float64)) < 2147483648.0
                fl, nav = f["flags"], f["nav_flags"]
                ok &= ~((fl & F["HEADING"]) != 0) | fin("heading")
                ok &= ~((fl & F["TRACK_RATE"]) != 0) | fin("track_rate")
                ok &= ~((fl & F["ROLL"]) != 0) | fin("roll")
                gs = (fl & F["GS"]) != 0
                ok &= ~gs | (fin("gs_selected") & (fin("gs_v0") | (f["gs_v0"] == f["gs_selected"])) & (fin("gs_v2") | (f["gs_v2"] == f["gs_selected"])))
                ok &= ~((fl & F["MACH"]) != 0) | fin("mach")
                ok &= ~((nav & NAV_HEADING) != 0) | fin("nav_heading")
                ok &= ~((nav & NAV_QNH) != 0) | fin("nav_qnh")
                if c.get("positions") is not None:
                    p = c["positions"]
                    placed = np.isin(p["method"], POS_METHODS) & ((fl & F["CPR"]) != 0)
                    ok &= ~placed | ((np.abs(p["lat"]) <= 90.0) & (np.abs(p["lon"]) <= 360.0))
            cls[~ok] = SKIP
            level = signal_level(m)
            for i in np.nonzero((cls == LINE) & (m["sig_sumsq"] != 0) & (level != 1.0))[0].tolist():
                if rssi_margin(float(level[i])) < 2.0 ** -20:
                    cls[i] = DEFER
    cls[quiet] = NONE
    return cls


def expected(c, flags, ref_chunks, show_only=0):
    """What mgpu_dump_encode_ex* owes for a case set whose reference dumps (one bytes object per case, b"" where the reference was
    not run) are ref_chunks: -> (the stream: deferred dropped, deferred[] {index, offset}, skipped, the length per message that is
    in the stream)."""
    cls = classes(c, flags, show_only)
    length = np.array([len(ref_chunks[i]) if cls[i] == LINE else 0 for i in range(len(cls))], dtype=np.int64)
    start = np.cumsum(length) - length
    d = np.zeros(int((cls == DEFER).sum()), dtype=DEFERRED)
    d["index"], d["offset"] = np.nonzero(cls == DEFER)[0], start[cls == DEFER]
    return b"".join(ref_chunks[i] for i in np.nonzero(cls == LINE)[0].tolist()), d, int((cls == SKIP).sum()), length


def splice(stream, deferred, texts):
    """The stream with the host's text of every deferred message put in at its offset."""
    out, at = [], 0
    for e, t in zip(deferred, texts):
        out += [stream[at:int(e["offset"])], t]
        at = int(e["offset"])
    return b"".join(out + [stream[at:]])


# ---- the dump itself: a plain-Python model of displayModesMessage (mode_s.c:1809-2239) ---------------------------------------------------
# Written from the reference's format strings with Python's own % conversions ('%.1f' % x rounds the exact binary value half to even, as
# glibc's printf does) and math.log10 (the host's libm, as the reference's): nothing of readsb_amd/csrc/dump_format.h is used.

_DF_NAMES = {0: "Short Air-Air Surveillance", 4: "Survelliance, Altitude Reply", 5: "Survelliance, Identity Reply", 11: "All Call Reply",
             16: "Long Air-Air ACAS", 17: "Extended Squitter", 18: "Extended Squitter (Non-Transponder)", 19: "Extended Squitter (Military)",
             20: "Comm-B, Altitude Reply", 21: "Comm-B, Identity Reply", 22: "Military Use", 32: "Mode A/C Reply",
             **{k: "Comm-D Extended Length Message" for k in range(24, 32)}}
_COMMB = ["unknown format", "ambiguous format", "empty response", "BDS1,0 Datalink capabilities", "BDS1,7 Common usage GICB capabilities",
          "BDS2,0 Aircraft identification", "BDS3,0 ACAS resolution advisory", "BDS4,0 Selected vertical intention", "BDS5,0 Track and turn report",
          "BDS6,0 Heading and speed report", "BDS4,4 Meteorological routine air report"]
_ADDRTYPE = ["adsb_icao", "adsb_icao_nt", "adsr_icao", "tisb_icao", "adsc", "mlat", "other", "mode_s", "adsb_other", "adsr_other", "tisb_trackfile",
             "tisb_other", "mode_ac"]
_AIRGROUND = ["invalid", "ground", "airborne", "airborne?"]
_HEADING = ["unknown heading type", "Ground track", "True heading", "Mag heading", "Heading", "Track/Heading"]
_CPR = ["unknown CPR type", "Surface", "Airborne", "TIS-B Coarse"]
_SIL_TYPE = ["invalid type", "unknown type", "per sample", "per flight hour"]
_SIL = {1: "p <= 0.1%", 2: "p <= 0.001%", 3: "p <= 0.00001%"}
_EMERGENCY = ["no emergency", "general emergency (7700)", "lifeguard / medical emergency", "minimum fuel", "no communications (7600)",
              "unlawful interference (7500)", "downed aircraft"]
_NAV_MODES = ["autopilot", "vnav", "althold", "approach", "lnav", "tcas"]
_NAV_SOURCE = {2: "aircraft altitude", 3: "MCP selected altitude", 4: "FMS selected altitude"}
_ES_SUB = {19: {1: "Airborne velocity over ground, subsonic", 2: "Airborne velocity over ground, supersonic", 3: "Airspeed and heading, subsonic",
                4: "Airspeed and heading, supersonic"},
           23: {0: "Test message", 7: "National use / 1090-WP-15-20 Mode A squawk"}, 28: {1: "Emergency/priority status", 2: "ACAS RA broadcast"},
           29: {0: "Target state and status (V1)", 1: "Target state and status (V2)"},
           31: {0: "Aircraft operational status (airborne)", 1: "Aircraft operational status (surface)"}}


def _pick(names, v, default):
    return names[v] if v < len(names) else default


def _es_name(me, sub):
    if me == 0:
        return "No position information (airborne or surface)"
    if me <= 4:
        return "Aircraft identification and category"
    if me <= 8:
        return "Surface position"
    if me <= 18:
        return "Airborne position (barometric altitude)"
    if 20 <= me <= 22:
        return "Airborne position (geometric altitude)"
    if me in _ES_SUB:
        return _ES_SUB[me].get(sub, "Unknown")
    return {24: "Reserved for surface system status", 27: "Reserved for trajectory change", 30: "Aircraft Operational Coordination"}.get(me, "Unknown")


def model_crc(raw, msgtype, nbits):
    """mm->crc as mode_s.c:466 leaves it: modesChecksum (crc.c:67-82) of the sliced frame, its DF set to 17 where fixDF17msgtype did."""
    b = list(raw[:nbits // 8])
    if msgtype == 17 and b[0] >> 3 != 17:
        b[0] = (b[0] & 7) | (17 << 3)
    rem = 0
    for x in b[:-3]:
        rem ^= x << 16
        for _ in range(8):
            rem = ((rem << 1) ^ 0xFFF409) & 0xFFFFFF if rem & 0x800000 else (rem << 1) & 0xFFFFFF
    return rem ^ (b[-3] << 16) ^ (b[-2] << 8) ^ b[-1]


def _acas_line(mv, addr, df, ms):
    """sprintACASInfoShort (json_out.c:443-629) with a == NULL, and printACASInfoShort's newline.  mv: MV as a 56-bit integer."""
    def bit(k):
        return (mv >> (56 - k)) & 1
    t = time.gmtime(ms // 1000)
    p = ["%04d-%02d-%02d,%02d:%02d:%02d.%d, %06x,DF:,%2u,bytes:,%014X," % (t.tm_year, t.tm_mon, t.tm_mday, t.tm_hour, t.tm_min, t.tm_sec, ms % 1000 // 100,
                                                                         addr, df, mv),
         "           ,           ,     ,ft,     ,fpm,ARA:,", "".join(str(bit(k)) for k in range(9, 16)), ",RAT:,%u,MTE:,%u,RAC:," % (bit(27), bit(28)),
         "".join(str(bit(k)) for k in range(23, 27)), ", "]
    racs = ["not below", "not above", "not left ", "not right"]
    p.append("".join(racs[k - 23] for k in range(23, 27) if bit(k)) if any(bit(k) for k in range(23, 27)) else "         ")
    p.append(", ")
    ara, rat, mte = bit(9), bit(27), bit(28)
    if rat:
        p.append("Clear of Conflict")
    elif ara:
        p.append("RA:")
        corr, down, increase, reversal, crossing, positive = (bit(k) for k in range(10, 16))
        sense = " Descend" if down else " Climb"
        if corr and positive:
            if reversal and increase:
                p.append(" Increase")
            p.append(sense)
            if reversal:
                p.append(";" + sense + " NOW")
            if crossing:
                p.append("; Crossing" + sense)
        if corr and not positive:
            p.append(" Level Off")
        if not corr and positive:
            p.append(" Maintain vertical Speed" + ("; Crossing Maintain" if crossing else ""))
        if not corr and not positive:
            p.append(" Monitor vertical Speed")
    elif mte:
        p.append("RA multithreat:")
        for k, text in ((10, " correct upwards;"), (11, " climb required;"), (12, " correct downwards;"), (13, " descent required;"), (14, " crossing;")):
            if bit(k):
                p.append(text)
        p.append(" increase/maintain vertical rate" if bit(15) else "      reduce/limit vertical rate")
    if (mv >> 26) & 3 == 1:
        p.append("; TIDh: %06x" % ((mv >> 2) & 0xFFFFFF))
    p.append(",\n")
    return "".join(p)


def model_dump(m, f, flags, pos=None, reduce_forward=0, receiver_id=0, decoded_nic=0, decoded_rc=0):
    """The bytes displayModesMessage prints for one message inside the mode's domain.  m, f: a MSG and a FIELDS record (numpy scalars);
    pos: a POSITION record or None."""
    addr, df = int(f["addr"]), int(f["msgtype"])
    if flags & ONLYADDR:
        return b"%06x\n" % addr
    ts, ms = int(m["timestamp"]), int(m["sysTimestamp"])
    msg = bytes(m["msg"])
    p = [("@%012X" % (ts & 0xFFFFFFFFFFFFFFFF) if flags & MLAT and ts else "*") + msg[:int(m["msgbits"]) // 8].hex() + ";\n"]
    if flags & RAW:
        return p[0].encode()
    addr9 = ""
    if df < 32:
        a = addr if addr != HEX_UNKNOWN else 0                          # maybe_addr of a memset-0 message
        addr9 = "%s%06x %s" % ("~" if a & NON_ICAO else " ", a & 0xFFFFFF, " " if addr != HEX_UNKNOWN else "?")
        p.append("hex: %s CRC: %06x fixed bits: %d decode: ok\n" % (addr9, model_crc(bytes(m["raw"]), df, int(m["msgbits"])), int(m["correctedbits"])))
    if int(m["sig_sumsq"]) > 0:
        level = float(int(m["sig_sumsq"])) / 65535.0 / 65535.0 / float(int(m["sig_len"]))
        p.append("RSSI: %8.1f dBFS   " % (10 * math.log10(level)))
    rf = int(reduce_forward)
    p.append("reduce_forward: %d\n" % (rf - 256 if rf > 127 else rf))
    if int(m["score"]):
        p.append("Score: %d\n" % int(m["score"]))
    if int(receiver_id):
        h = "%016x" % int(receiver_id)
        p.append("receiverId: %s-%s-%s\n" % (h[:8], h[8:12], h[12:]))
    if ts in MAGIC:
        p.append(("This is a synthetic MLAT message.\n", "This is a synthetic UAT message.\n", "This is a no_forward message.\n")[MAGIC.index(ts)])
    else:
        p.append("receiverTime: %27.2fus\n" % (ts / 12.0))
    t = time.gmtime(ms // 1000)
    p.append("utcTime: %02d:%02d:%02d.%03d epoch: %.3f\n" % (t.tm_hour, t.tm_min, t.tm_sec, ms % 1000, ms / 1000.0))
    g = {k: int(f[k]) for k in ("VS", "CC", "SL", "RI", "AC", "FS", "DR", "UM", "ID", "AA", "IID", "CA", "CF", "KE", "ND")}
    if df == 0:
        p.append("DF:  0 addr:%s VS:%u CC:%u SL:%u RI:%u AC:%u\n" % (addr9, g["VS"], g["CC"], g["SL"], g["RI"], g["AC"]))
    elif df in (4, 20):
        p.append("DF: %2d addr:%s FS:%u DR:%u UM:%u AC:%u" % (df, addr9, g["FS"], g["DR"], g["UM"], g["AC"]))
    elif df in (5, 21):
        p.append("DF: %2d addr:%s FS:%u DR:%u UM:%u ID:%u" % (df, addr9, g["FS"], g["DR"], g["UM"], g["ID"]))
    elif df == 11:
        p.append("DF: 11 AA:%06X IID:%u CA:%u\n" % (g["AA"], g["IID"], g["CA"]))
    elif df == 16:
        p.append("DF: 16 addr:%s VS:%u SL:%u RI:%u AC:%u MV:%s\n" % (addr9, g["VS"], g["SL"], g["RI"], g["AC"], msg[4:11].hex().upper()))
        if int(f["flags"]) & F["ACAS_RA"]:
            p.append(_acas_line(int.from_bytes(msg[4:11], "big"), addr, df, ms))
    elif df == 17:
        p.append("DF: 17 AA:%06X CA:%u ME:%s\n" % (g["AA"], g["CA"], msg[4:11].hex().upper()))
    elif df == 18:
        p.append("DF: 18 AA:%06X CF:%u ME:%s\n" % (g["AA"], g["CF"], msg[4:11].hex().upper()))
    elif 24 <= df <= 31:
        p.append("DF: 24 addr:%s KE:%u ND:%u MD:%s\n" % (addr9, g["KE"], g["ND"], msg[1:11].hex().upper()))
    if df in (4, 5):
        p.append("\n")
    if df in (20, 21):
        p.append(" MB:%s\n" % msg[4:11].hex().upper())
    p.append(" " + ("modeac" if df == 77 else "out of range" if df > 32 else _DF_NAMES.get(df, "reserved")))
    me, sub = int(f["metype"]), int(f["mesub"])
    if df in (17, 18):
        p.append(" %s (%u/%u)" % (_es_name(me, sub), me, sub) if me > 18 and not 20 <= me <= 22 else " %s (%u)" % (_es_name(me, sub), me))
    p.append("\n")
    if df in (20, 21):
        p.append("  Comm-B format: %s\n" % _pick(_COMMB, int(f["commb_format"]), "unknown format"))
    if addr != HEX_UNKNOWN:
        kind = _pick(_ADDRTYPE, int(f["addrtype"]), "unknown")
        p.append("  Other Address: %06X (%s)\n" % (addr & 0xFFFFFF, kind) if addr & NON_ICAO else "  ICAO Address:  %06X (%s)\n" % (addr, kind))
    fl, acc, nav, op = int(f["flags"]), int(f["acc_flags"]), int(f["nav_flags"]), int(f["op_flags"])
    if int(f["airground"]):
        p.append("  Air/Ground:    %s\n" % _pick(_AIRGROUND, int(f["airground"]), "(unknown airground state)"))
    unit = lambda v: "ft" if v == 0 else "m" if v == 1 else "(unknown altitude unit)"                # noqa: E731
    if fl & F["BARO_ALT"]:
        p.append("  Baro altitude:           %8d %s\n" % (int(f["baro_alt"]), unit(int(f["baro_alt_unit"]))))
    if fl & F["GEOM_ALT"]:
        p.append("  Geom altitude:           %8d %s\n" % (int(f["geom_alt"]), unit(int(f["geom_alt_unit"]))))
    if fl & F["GEOM_DELTA"]:
        p.append("  Geom - baro:   %8d ft\n" % int(f["geom_delta"]))
    if fl & F["HEADING"]:
        p.append("  %-13s     %5.1f\n" % (_pick(_HEADING, int(f["heading_type"]), _HEADING[0]), float(f["heading"])))
    if fl & F["TRACK_RATE"]:
        x = float(f["track_rate"])
        p.append("  Track rate:    %6.2f deg/sec %s\n" % (x, "left" if x < 0 else "right" if x > 0 else ""))
    if fl & F["ROLL"]:
        x = float(f["roll"])
        p.append("  Roll:          %5.1f degrees %s\n" % (x, "left" if x < -0.05 else "right" if x > 0.05 else ""))
    if fl & F["GS"]:
        sel, v0, v2 = float(f["gs_selected"]), float(f["gs_v0"]), float(f["gs_v2"])
        p.append("  Groundspeed:   %5.1f kt" % sel + (" (v0: %.1f kt)" % v0 if v0 != sel else "") + (" (v2: %.1f kt)" % v2 if v2 != sel else "") + "\n")
    if fl & F["IAS"]:
        p.append("  IAS:           %3u kt\n" % int(f["ias"]))
    if fl & F["TAS"]:
        p.append("  TAS:           %3u kt\n" % int(f["tas"]))
    if fl & F["MACH"]:
        p.append("  Mach number:   %.3f\n" % float(f["mach"]))
    if fl & F["BARO_RATE"]:
        p.append("  Baro rate:     %6d ft/min\n" % int(f["baro_rate"]))
    if fl & F["GEOM_RATE"]:
        p.append("  Geom rate:     %6d ft/min\n" % int(f["geom_rate"]))
    if fl & F["SQUAWK"]:
        p.append("  Squawk:        %04d\n" % int(f["squawkDec"]))
    out = "".join(p).encode("latin-1")
    p = []
    if fl & F["CALLSIGN"]:
        out += b"  Ident:         " + bytes(f["callsign"]).split(b"\0")[0] + b"\n"
    if fl & F["CATEGORY"]:
        p.append("  Category:      %02X\n" % int(f["category"]))
    if fl & F["CPR"]:
        p.append("  CPR type:      %s\n  CPR odd flag:  %s\n" % (_pick(_CPR, int(f["cpr_type"]), _CPR[0]), "odd" if fl & F["CPR_ODD"] else "even"))
        if pos is not None and int(pos["method"]) in POS_METHODS:
            p.append("  CPR latitude:  %11.6f (%5u)\n  CPR longitude: %11.6f (%5u)\n  CPR decoding:  %s\n  NIC:           %u\n  Rc:            %.3f km / %.1f NM\n"
                     % (float(pos["lat"]), int(f["cpr_lat"]), float(pos["lon"]), int(f["cpr_lon"]), "global" if int(pos["method"]) == 1 else "local",
                        int(decoded_nic), int(decoded_rc) / 1000.0, int(decoded_rc) / 1852.0))
        else:
            p.append("  CPR latitude:  (%u)\n  CPR longitude: (%u)\n  CPR decoding:  none\n" % (int(f["cpr_lat"]), int(f["cpr_lon"])))
    for k, (label, name) in enumerate((("NIC-A:   ", None), ("NIC-B:   ", None), ("NIC-C:   ", None), ("NIC-baro:", None), ("NACp:    ", "nac_p"),
                                       ("NACv:    ", "nac_v"), ("GVA:     ", "gva"))):
        if acc & (1 << k):
            p.append("  %s      %d\n" % (label, int(f[name]) if name else (acc >> (8 + k)) & 1))
    if int(f["sil_type"]):
        p.append("  SIL:           %d (%s, %s)\n" % (int(f["sil"]), _SIL.get(int(f["sil"]), "p > 0.1%"), _pick(_SIL_TYPE, int(f["sil_type"]), _SIL_TYPE[0])))
    if acc & (1 << 7):
        p.append("  SDA:           %d\n" % int(f["sda"]))
    if op & 1:
        p.append("  Aircraft Operational Status:\n    Version:            %d\n    Capability classes: " % (int(f["op_version"]) & 7))
        tc = int(f["op_cc_tc"]) & 3
        for on, text in ((op & 32, "ACAS "), (op & 64, "CDTI "), (op & 128, "1090IN "), (op & 256, "ARV "), (op & 512, "TS "), (tc, "TC=%d " % tc),
                         (op & 1024, "UATIN "), (op & 2048, "POA "), (op & 4096, "B2-LOW "), (op & 8192, "L/W=%d " % int(f["op_cc_lw"])),
                         (int(f["op_cc_antenna_offset"]), "GPS-OFFSET=%d " % int(f["op_cc_antenna_offset"]))):
            if on:
                p.append(text)
        p.append("\n    Operational modes:  ")
        for on, text in ((op & 2, "ACASRA "), (op & 4, "IDENT "), (op & 8, "ATC "), (op & 16, "SAF ")):
            if on:
                p.append(text)
        p.append("\n")
        if sub == 1:
            p.append("    Track/heading:      %s\n" % _pick(_HEADING, int(f["op_tah"]), _HEADING[0]))
        p.append("    Heading ref dir:    %s\n" % _pick(_HEADING, int(f["op_hrd"]), _HEADING[0]))
    if nav & NAV_HEADING:
        p.append("  Selected heading: %5.1f\n" % float(f["nav_heading"]))
    if nav & NAV_FMS:
        p.append("  FMS selected altitude:      %5u ft\n" % int(f["nav_fms_altitude"]))
    if nav & NAV_MCP:
        p.append("  MCP selected altitude:      %5u ft\n" % int(f["nav_mcp_altitude"]))
    if nav & NAV_QNH:
        p.append("  QNH:                     %.1f millibars\n" % float(f["nav_qnh"]))
    if int(f["nav_altitude_source"]):
        p.append("  Target altitude source:  %s\n" % _NAV_SOURCE.get(int(f["nav_altitude_source"]), "unknown"))
    if nav & NAV_MODES:
        p.append("  Nav modes:               %s\n" % " ".join(name for k, name in enumerate(_NAV_MODES) if int(f["nav_modes"]) & (1 << k)))
    if fl & F["EMERGENCY"]:
        p.append("  Emergency/priority:      %s\n" % _pick(_EMERGENCY, int(f["emergency"]), "reserved"))
    p.append("\n")
    return out + "".join(p).encode("latin-1")


def model_chunks(c, flags, optional=True):
    """The model's dump per case, b"" for the cases outside the mode's domain."""
    cls = classes(c, flags)
    out = []
    for i in range(len(cls)):
        if cls[i] == SKIP:
            out.append(b"")
        elif optional:
            out.append(model_dump(c["msgs"][i], c["fields"][i], flags, c["positions"][i], c["reduce_forward"][i], c["receiver_ids"][i], c["decoded_nic"][i],
                                  c["decoded_rc"][i]))
        else:
            out.append(model_dump(c["msgs"][i], c["fields"][i], flags))
    return out


# ---- case generators ------------------------------------------------------------------------------------------------------------------

def _safe_sumsq(rng, n):
    """Signal sums of plausible levels, none within 2^-16 of an RSSI rounding boundary: groups (a)-(d) must defer nothing."""
    out = np.zeros(n, dtype=np.uint64)
    for i in range(n):
        while True:
            s = int(10.0 ** rng.uniform(6.0, 12.3))
            if rssi_margin(s / 65535.0 / 65535.0 / 268.0) > 2.0 ** -16 and rssi_margin(s / 65535.0 / 65535.0 / 134.0) > 2.0 ** -16:
                break
        out[i] = s
    return out


def _dress(c, rng):
    """Message-level members and the caller's arrays at random over what a receiver sees."""
    n = len(c["msgs"])
    m = c["msgs"]
    m["sig_sumsq"] = np.where(rng.random(n) < 0.1, 0, _safe_sumsq(rng, n))
    m["sig_len"] = np.where(m["msgbits"] == 112, 268, 134)
    m["score"] = np.where(rng.random(n) < 0.3, 0, rng.integers(-5, 1801, size=n))
    m["phase"] = rng.integers(4, 9, size=n)
    m["sysTimestamp"] = 1690000000000 + np.cumsum(rng.integers(0, 5000, size=n))
    m["timestamp"] = 12000 * (m["sysTimestamp"] - 1690000000000) + rng.integers(0, 12000, size=n)
    m["msgtype"], m["addr"] = c["fields"]["msgtype"], c["fields"]["addr"]
    c["reduce_forward"] = (rng.random(n) < 0.4).astype(np.uint8)
    c["receiver_ids"] = np.where(rng.random(n) < 0.5, 0, rng.integers(1, 1 << 63, size=n)).astype(np.uint64)
    has_cpr = (c["fields"]["flags"] & F["CPR"]) != 0
    c["positions"]["method"] = np.where(has_cpr | (rng.random(n) < 0.1), rng.integers(0, 5, size=n), 0)
    c["positions"]["lat"], c["positions"]["lon"] = rng.uniform(-90, 90, size=n), rng.uniform(-180, 180, size=n)
    c["decoded_nic"] = rng.integers(0, 12, size=n).astype(np.uint8)
    c["decoded_rc"] = rng.choice(np.array([0, 7, 25, 75, 186, 371, 926, 1852, 3704, 7408, 14816, 37040, 4294967295], dtype=np.uint32), size=n)
    return c


def fuzz_cases(n_es, n_other, n_commb, n_ac, seed):
    """(a) fuzzed frames of every DF, ME type and Comm-B register through the oracle's field decode; a third of them as repaired
    frames: raw[] differs from msg[] in one or two bits, or in one bit of the DF (a DF17 whose DF was repaired)."""
    import fields_util as fu
    rng = np.random.default_rng(seed)
    parts = [fu.fuzz_frames(n_es, seed + 1, dfs=(17, 18)), fu.fuzz_frames(n_other, seed + 2), fu.commb_frames(n_commb, seed + 3)]
    ac = np.zeros((n_ac, 14), dtype=np.uint8)
    ac[:, :2] = rng.integers(0, 256, size=(n_ac, 2))
    parts.append((ac, np.full(n_ac, 16, dtype=np.int32)))
    frames, bits = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    order = rng.permutation(len(frames))
    frames, bits = frames[order], bits[order]
    c = empty_cases(len(frames))
    c["fields"] = fu.oracle_fields(frames, bits).view(FIELDS).copy()
    m = c["msgs"]
    m["msg"], m["msgbits"] = frames, bits
    raw = frames.copy()
    kind = rng.integers(0, 6, size=len(frames))
    for i in np.nonzero(bits != 16)[0].tolist():
        if kind[i] in (1, 2) and c["fields"]["msgtype"][i] not in (20, 21):        # (decodeCommB runs on unrepaired frames only: those stay clean)
            for b in rng.choice(int(bits[i]) - 5, size=int(kind[i]), replace=False) + 5:
                raw[i, b // 8] ^= 0x80 >> (b % 8)
            m["correctedbits"][i] = kind[i]
        elif kind[i] == 3 and c["fields"]["msgtype"][i] == 17:
            raw[i, 0] ^= 0x80 >> int(rng.integers(0, 5))
            m["correctedbits"][i] = 1
    m["raw"] = raw
    return _dress(c, rng)


def edge_cases(n, seed):
    """(b) field records no decoder gives: every flag and enum at random, in and out of range, over tame floats — so that every line
    of the dump appears with every neighbour — then records at and outside the domain's edges."""
    rng = np.random.default_rng(seed)
    c = empty_cases(n)
    f = rng.integers(0, 256, size=n * FIELDS.itemsize, dtype=np.uint8).view(FIELDS).copy()
    f["msgtype"] = rng.choice(np.array([0, 4, 5, 11, 16, 17, 18, 20, 21, 24, 31, 1, 19, 22, 23, 32, 33, 77, 200], dtype=np.uint8), size=n)
    f["flags"] &= rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    tame = rng.random(n) < 0.7
    for name, hi in (("addrtype", 14), ("airground", 5), ("cpr_type", 5), ("heading_type", 7), ("sil_type", 5), ("baro_alt_unit", 3), ("geom_alt_unit", 3),
                     ("commb_format", 12), ("emergency", 8), ("nav_altitude_source", 6), ("op_hrd", 7), ("op_tah", 7), ("sil", 5), ("metype", 32), ("mesub", 8)):
        f[name][tame] = rng.integers(0, hi, size=int(tame.sum()))
    f["addr"][tame] &= 0x1FFFFFF
    f["addr"][-13:-1] = (HEX_UNKNOWN, 0, 1, 0xFFFFFF, NON_ICAO, NON_ICAO | 0x123456, 0xFE000000, 0xFFFFFFFF, HEX_UNKNOWN, HEX_UNKNOWN, HEX_UNKNOWN, HEX_UNKNOWN)
    f["msgtype"][-5:-1] = (0, 4, 17, 20)
    f["msgtype"][-13] = 5
    for name, lo, hi in (("heading", 0, 360), ("gs_selected", 0, 700), ("roll", -90, 90), ("track_rate", -16, 16), ("mach", 0, 4), ("nav_qnh", 800, 1100),
                         ("nav_heading", 0, 360)):
        f[name] = rng.uniform(lo, hi, size=n)
    f["gs_v0"] = np.where(rng.random(n) < 0.5, f["gs_selected"], rng.uniform(0, 700, size=n))
    f["gs_v2"] = np.where(rng.random(n) < 0.5, f["gs_selected"], rng.uniform(0, 700, size=n))
    for name in ("baro_alt", "geom_alt", "geom_delta", "baro_rate", "geom_rate"):
        f[name][tame] = rng.integers(-2000, 60000, size=int(tame.sum()))
    c["fields"] = f
    m = c["msgs"]
    m["msg"], m["raw"] = rng.integers(0, 256, size=(n, 14)), rng.integers(0, 256, size=(n, 14))
    m["msgbits"] = np.where(f["msgtype"] == 77, 16, rng.choice([56, 112], size=n))
    m["correctedbits"] = rng.choice([0, 0, 1, 2, 255], size=n)
    c = _dress(c, rng)
    c["reduce_forward"] = rng.choice(np.array([0, 1, 127, 128, 255], dtype=np.uint8), size=n)
    c["decoded_nic"] = rng.choice(np.array([0, 7, 255], dtype=np.uint8), size=n)
    c["fields"]["flags"][n // 2:] |= F["CPR"]                     # the CPR block in both forms, with every method
    c["positions"]["method"][n // 2:] = rng.integers(0, 6, size=n - n // 2)
    # DF16 with an ACAS advisory: every bit of MV at random
    k = 128
    c["fields"]["msgtype"][:k], c["msgs"]["msgtype"][:k] = 16, 16
    c["fields"]["flags"][:k] |= F["ACAS_RA"]
    i = np.arange(k)
    c["msgs"]["msg"][:k, 5] = i * 2 + (i & 1)                      # ARA, bits 9-15: every combination
    rat, mte = i % 8 == 6, ((i < 64) & (i % 2 == 0)) | (i % 16 == 5)
    c["msgs"]["msg"][:k, 7] = (c["msgs"]["msg"][:k, 7] & 0xCF) | (rat << 5) | (mte << 4)
    # the longest values of the domain
    j = n - 1
    g = c["fields"]
    g["flags"][j], g["acc_flags"][j], g["nav_flags"][j], g["op_flags"][j] = 0xFFFFFFFF, 0xFFFF, 0xFF, 0xFFFF
    for name in ("heading", "gs_selected", "roll", "track_rate", "mach", "nav_qnh", "nav_heading"):
        g[name][j] = -2147483520.0
    g["gs_v0"][j], g["gs_v2"][j] = 2147483520.0, -1.0
    for name in ("baro_alt", "geom_alt", "geom_delta", "baro_rate", "geom_rate"):
        g[name][j] = -(1 << 31)
    g["msgtype"][j], c["msgs"]["msgtype"][j], c["msgs"]["msgbits"][j], g["heading_type"][j], g["nav_modes"][j] = 16, 16, 112, 0, 63
    g["addr"][j], g["mesub"][j], c["msgs"]["score"][j], c["msgs"]["timestamp"][j] = 0xFEFFFFFF, 1, -32768, (1 << 63) - 1
    c["positions"]["method"][j], c["positions"]["lat"][j], c["positions"]["lon"][j] = 2, -89.9999995, -359.9999995
    c["decoded_rc"][j], c["decoded_nic"][j], c["receiver_ids"][j], c["reduce_forward"][j] = 4294967295, 255, (1 << 64) - 1, 128
    # outside the domain, one reason per record
    bad = []
    for name, flag, where in (("heading", F["HEADING"], "flags"), ("track_rate", F["TRACK_RATE"], "flags"), ("roll", F["ROLL"], "flags"), ("gs_selected", F["GS"], "flags"),
                              ("gs_v0", F["GS"], "flags"), ("gs_v2", F["GS"], "flags"), ("mach", F["MACH"], "flags"), ("nav_qnh", NAV_QNH, "nav_flags"),
                              ("nav_heading", NAV_HEADING, "nav_flags")):
        for x in (np.inf, -np.inf, np.nan, 2147483648.0, -2147483648.0, 2147483520.0):
            for valid in (True, False):
                b = _plain(1)
                b["fields"][name] = x
                b["fields"][where] = flag if valid else 0
                bad.append(b)
    for la, lo in ((np.nan, 0), (0, np.nan), (np.inf, 0), (90.00000000000001, 0), (0, -360.00000000000006), (90.0, 360.0), (-90.0, -360.0), (1e300, 1e300)):
        for method in (1, 3, 4):
            for flags in (F["CPR"], 0):
                b = _plain(1)
                b["fields"]["flags"], b["positions"]["method"], b["positions"]["lat"], b["positions"]["lon"] = flags, method, la, lo
                bad.append(b)
    for name, vals in (("sysTimestamp", (-1, MS_END, MS_END - 1, 0, -(1 << 63), (1 << 63) - 1)), ("timestamp", (-1, -(1 << 63))), ("sig_len", (0, 1)),
                       ("msgbits", (0, 8, 16, 48, 64, 120, 255))):
        for v in vals:
            b = _plain(1)
            b["msgs"][name] = v
            bad.append(b)
    return concat_cases([c] + bad)


def _plain(n, df=17, me=11):
    c = empty_cases(n)
    c["fields"]["msgtype"], c["fields"]["metype"], c["fields"]["addr"], c["fields"]["AA"] = df, me, 0x4840D6, 0x4840D6
    c["msgs"]["msgtype"], c["msgs"]["addr"] = df, 0x4840D6
    c["msgs"]["msg"][:, 0], c["msgs"]["raw"][:, 0] = df << 3, df << 3
    c["msgs"]["sig_sumsq"] = 123456789012
    return c


def float_cases():
    """(c) the floats nearest (k + 0.5) * 10^-N for N = 1, 2, 3 with both neighbours, their negatives, +-0.0 and the smallest
    values: each on every printed float of a record, so every format (%5.1f, %6.2f, %.3f, %.1f) meets every value."""
    vals = []
    for nd in (1, 2, 3):
        k = np.concatenate([np.arange(0, 12), np.array([99, 127, 128, 255, 999, 1000, 4095, 9999, 65535, 99999, 999999])]).astype(np.float64)
        x = ((k + 0.5) / 10.0 ** nd).astype(np.float32)
        vals += [x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))]
    x = np.concatenate(vals)
    x = np.concatenate([x, -x, np.array([0.0, -0.0, 1e-45, -1e-45, 0.05, -0.05, 0.049999997, -0.050000004, 2147483520.0, 8388607.5, 16777216.0],
                                        dtype=np.float32)])
    c = _plain(len(x), df=20, me=0)
    f = c["fields"]
    f["flags"] = F["HEADING"] | F["TRACK_RATE"] | F["ROLL"] | F["GS"] | F["MACH"]
    f["nav_flags"] = NAV_HEADING | NAV_QNH
    f["heading_type"] = np.arange(len(x)) % 6
    for shift, name in enumerate(("heading", "track_rate", "roll", "gs_selected", "gs_v0", "gs_v2", "mach", "nav_qnh", "nav_heading")):
        f[name] = np.roll(x, 7 * shift)
    return c


def time_cases():
    """(d) timestamps at 0 and 1, around 2^48 and 2^53 * 12, the three magic values and the ends of int64; sysTimestamp at day and year
    boundaries and the ends of the domain."""
    ts = [0, 1, 5, 6, 7, 11, 12, 13, (1 << 48) - 1, 1 << 48, (1 << 48) + 1, 12 * (1 << 53) - 1, 12 * (1 << 53), 12 * (1 << 53) + 6, 12 * (1 << 53) + 7,
          12 * (1 << 53) + 18, 12 * ((1 << 52) + 1) + 6, 3 * (1 << 53) + 1, (1 << 63) - 1, (1 << 62) + 12345, 0x123456789ABCDEF, *(5 * MAGIC), MAGIC[0] - 1, MAGIC[2] + 1,
          123456789, 12000000 * 86400 + 5]
    st = [0, 999, 1000, 86399999, 86400000, 951782399999, 951782400000, 1709164800000, 1709251199999, 1735689599999, 1735689600000, 4102444799999,
          4102444800000, MS_END - 1]
    n = len(ts) + len(st)
    c = _plain(n, df=4, me=0)
    c["msgs"]["msgbits"] = 56
    c["msgs"]["timestamp"][:len(ts)] = ts
    c["msgs"]["sysTimestamp"][len(ts):] = st
    # the ACAS line prints the date and the tenth of a second: a DF16 advisory on every system time
    a = _plain(len(st), df=16, me=0)
    a["msgs"]["sysTimestamp"] = st
    a["fields"]["flags"] = F["ACAS_RA"]
    a["msgs"]["msg"][:, 4:11] = (0x30, 0xC0, 0x00, 0x12, 0x34, 0x56, 0x78)
    return concat_cases([c, a])


RSSI_NEAR = (-107, -100, -96, -90, -111, -120, -104)              # m: 10 log10(level) = (m + 0.5) / 10, S ~ 1e11


def rssi_cases():
    """(e) signal sums S = round(10^((m + 0.5) / 100) * 65535^2 * 268): |10 log10(level)| * 10 lands within 1e-9 of a rounding
    boundary; their neighbours S +- 20000, which are 8e-6 from it; level exactly 1.0, just below and above it, and 0.
    -> (cases, the indices of the near ones)"""
    sums, near = [], []
    for m in RSSI_NEAR:
        s = round(10.0 ** ((m + 0.5) / 100.0) * 65535.0 ** 2 * 268.0)
        near.append(len(sums) + 1)
        sums += [s - 20000, s, s + 20000]
    one = 65535 * 65535 * 268
    sums += [one, one - 1, one + 1, 0, 1, (1 << 64) - 1, one * 10, one // 10]
    c = _plain(len(sums))
    c["msgs"]["sig_sumsq"] = np.array(sums, dtype=np.uint64)
    return c, np.array(near)


def build_groups():
    e, near = rssi_cases()
    return {"a": fuzz_cases(420, 360, 200, 20, seed=4100), "b": edge_cases(480, seed=4200), "c": float_cases(), "d": time_cases(), "e": e}, near


# ---- the reference's own printer (tests/host_stub/dump_ref_harness.c) -----------------------------------------------------------------

HARNESS_SRC = os.path.join(helpers.ROOT, "tests", "host_stub", "dump_ref_harness.c")
have_ref_full = sbs_util.have_ref_full


def build_ref_harness(workdir):
    """tests/host_stub/dump_ref_harness.c compiled with the flags of `make -C oracle full` and linked against that build's objects,
    readsb.o with its main renamed in a copy (as sbs_util.build_ref_harness, but net_io.o stays: nothing of it is included here)."""
    exe = os.path.join(workdir, "dump_ref_harness")
    main_o = os.path.join(workdir, "readsb_nomain.o")
    subprocess.run(["objcopy", "--redefine-sym", "main=readsb_main", os.path.join(sbs_util.REF_FULL, "readsb.o"), main_o], check=True)
    objs, flags = sbs_util._full_build()
    subprocess.run(["gcc", *flags, "-I" + os.path.join(helpers.ORACLE_DIR, "stub_full"), "-I/root/reference", HARNESS_SRC, main_o,
                    *[os.path.join(sbs_util.REF_FULL, o + ".o") for o in objs + ["net_io"]], "-o", exe, "-pthread", "-lpthread", "-lm", "-lrt",
                    "-l:libzstd.so.1", "-lz"], check=True)
    return exe


def case_records(c, flags):
    """The case set as records of the harness and of dump_format_check: `run` marks what the mode's domain admits."""
    n = len(c["msgs"])
    rec = np.zeros(n, dtype=CASE)
    rec["msg"], rec["fields"] = c["msgs"], c["fields"]
    rec["has_positions"] = 1
    rec["lat"], rec["lon"], rec["method"] = c["positions"]["lat"], c["positions"]["lon"], c["positions"]["method"]
    rec["receiver_id"], rec["decoded_rc"], rec["decoded_nic"], rec["reduce_forward"] = c["receiver_ids"], c["decoded_rc"], c["decoded_nic"], c["reduce_forward"]
    rec["run"] = classes(c, flags) != SKIP
    return rec


def run_ref_harness(exe, c, flags, workdir):
    """-> (the bytes displayModesMessage printed for the cases inside the mode's domain, the length per case)"""
    rec = case_records(c, flags)
    paths = [os.path.join(workdir, name) for name in ("cases.bin", "out.bin", "lens.bin")]
    rec.tofile(paths[0])
    subprocess.run([exe, *paths, str(int(bool(flags & ONLYADDR))), str(int(bool(flags & RAW))), str(int(bool(flags & MLAT)))], check=True)
    return open(paths[1], "rb").read(), np.fromfile(paths[2], dtype=np.int32)


# ---- the golden file ------------------------------------------------------------------------------------------------------------------

GOLDEN = os.path.join(helpers.GOLDEN_DIR, "dump_cases.npz")
GROUPS = ("a", "b", "c", "d", "e")


def load_golden():
    """-> (the case sets by group, {(group, mode): (the reference's bytes, its length per case)}, the near cases of group e)"""
    z = np.load(GOLDEN)
    sets = {g: {k: z[f"{g}_{k}"] for k in ("msgs", "fields", "positions", "reduce_forward", "receiver_ids", "decoded_nic", "decoded_rc")} for g in GROUPS}
    ref = {(g, mode): (z[f"ref_{g}_{mode}"].tobytes(), z[f"len_{g}_{mode}"].astype(np.int64)) for g in GROUPS for mode in MODES}
    return sets, ref, z["e_near"]


def chunks(stream, lens):
    """The reference's bytes cut per case."""
    end = np.cumsum(lens)
    return [stream[int(e - k):int(e)] for e, k in zip(end, lens)]
