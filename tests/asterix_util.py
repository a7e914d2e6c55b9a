"""The ASTERIX CAT021 output's checker and its inputs: a plain Python restatement of the record modesSendAsterixOutput writes
(net_io.c:2416-2945) with the rules of mgpu_asterix_encode_ex* (include/modes_gpu.h) on top — who gets a record, the domain and its skip
rule — the case generators of tests/golden/make_asterix_golden.py, and the driver of tests/host_stub/asterix_ref_harness.c (the
reference's own writer).  tests/test_asterix_reference.py pins the checker (CPU); tests/test_gpu_asterix.py compares the kernels with
it, byte for byte.

The reference's arithmetic is restated in the types C gives it: float products in numpy float32, everything else in float64; a
conversion to an integer type truncates towards zero and keeps the low bits (inside the domain, where that is defined)."""
import os
import subprocess

import numpy as np

import helpers
import sbs_util as su
from sbs_util import (DEFER, GATE_DEFER, GATE_FORWARD, INT32_MAX, INT32_MIN, LINE, MS_END, NONE, NOW_MS, POS_METHODS, SKIP,  # noqa: F401
                      concat_cases, gate_like_verdicts, slice_cases)
from readsb_amd.binding import DEFERRED_DTYPE as DEFERRED, FIELDS_DTYPE as FIELDS, MSG_DTYPE as MSG, POSITION_DTYPE as POSITION

BLOCK = 256
RECORD_MAX = 74                                # 3 + 6 FSPEC + 65 of items: I021/152 excludes I021/075 and I021/160
DAY_MS = 86400000

# flags of struct mgpu_fields the record reads (include/modes_gpu.h)
F_BARO_ALT, F_GEOM_ALT, F_HEADING, F_GS, F_IAS, F_TAS, F_BARO_RATE, F_GEOM_RATE = (1 << k for k in range(8))
F_SQUAWK, F_CALLSIGN, F_CPR, F_CPR_ODD, F_CATEGORY, F_GEOM_DELTA, F_SPI_VALID, F_SPI = (1 << k for k in range(8, 16))
F_ALERT_VALID, F_ALERT, F_EMERGENCY, F_ALT_Q_BIT, F_ACAS_RA, F_ROLL, F_TRACK_RATE, F_MACH = (1 << k for k in range(16, 24))
F_WIND, F_OAT, F_STATIC_PRESSURE, F_TURBULENCE, F_HUMIDITY = (1 << k for k in range(24, 29))
ACC_NIC_BARO_VALID, ACC_NAC_P_VALID, ACC_NAC_V_VALID, ACC_GVA_VALID, ACC_SDA_VALID, ACC_NIC_BARO = 1 << 3, 1 << 4, 1 << 5, 1 << 6, 1 << 7, 1 << 11
NAV_FMS_ALT, NAV_MCP_ALT, NAV_MODES = 1 << 1, 1 << 2, 1 << 4
OP_VALID, OP_OM_ACAS_RA, OP_CC_ACAS, OP_CC_CDTI, OP_CC_ARV, OP_CC_TS = 1 << 0, 1 << 1, 1 << 5, 1 << 6, 1 << 8, 1 << 9
NON_ICAO = 1 << 24
HEADING_GROUND_TRACK, HEADING_MAGNETIC = 1, 3
SOURCE_ADSR, SOURCE_ADSB = 9, 10
AIS = "@ABCDEFGHIJKLMNOPQRSTUVWXYZ[\\]^_ !\"#$%&'()*+,-./0123456789:;<=>?"

# name of an item -> (FSPEC byte, bit), as the writer sets them
FSPEC_BITS = {"010": (0, 7), "040": (0, 6), "130": (0, 2), "150": (1, 6), "151": (1, 5), "080": (1, 4), "073": (1, 3), "075": (1, 1),
              "140": (2, 6), "090": (2, 5), "210": (2, 4), "070": (2, 3), "230": (2, 2), "145": (2, 1), "152": (3, 7), "200": (3, 6),
              "155": (3, 5), "157": (3, 4), "160": (3, 3), "077": (3, 1), "170": (4, 7), "020": (4, 6), "220": (4, 5), "146": (4, 4),
              "008": (5, 7), "400": (5, 2)}


def _trunc(x):
    """C's conversion of a double to a (wide enough) integer, where |x| < 2^31; 0 elsewhere (never used there)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(x) < 2147483648.0
    return np.trunc(np.where(ok, x, 0.0)).astype(np.int64)


def _wrap32(v):
    return (np.asarray(v, dtype=np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)


def _wrap16(v):
    return (np.asarray(v, dtype=np.int64) + (1 << 15)) % (1 << 16) - (1 << 15)


def _idiv25(v):
    """C's v / 25 on ints: towards zero."""
    v = np.asarray(v, dtype=np.int64)
    return np.sign(v) * (np.abs(v) // 25)


def scaled_values(fields, positions=None, ac_baro_alt=None):
    """Every value the writer converts, as the double (or the float widened to double) it converts: name -> float64 array."""
    f = fields
    f32, f64 = np.float32, np.float64
    with np.errstate(over="ignore", invalid="ignore"):
        out = {
            "mach": f["mach"].astype(f64) * 1000.0,
            "ias": f["ias"].astype(f64) / 3600.0 * 16384.0,
            "roll": (f["roll"].astype(f32) * f32(100)).astype(f64),
            "oat": (f["oat"].astype(f32) * f32(4)).astype(f64),
            "baro_m": f["baro_alt"].astype(f64) * 3.2808,
            "mag": f["heading"].astype(f64) * 182.0444,
            "gs": f["gs_v0"].astype(f64) * 4.5511,
            "trk": f["heading"].astype(f64) * (65536 / 360.0),
            "wd": f["wind_direction"].astype(f64),
            "galt": np.where(f["geom_alt_unit"] == 0, f["geom_alt"].astype(f64) / 6.25, f["geom_alt"].astype(f64) / 20.5053),
            "brate": f["baro_rate"].astype(f64) / 3.125,
            "grate": f["geom_rate"].astype(f64) / 3.125,
        }
        base = np.zeros(len(f), dtype=np.int64) if ac_baro_alt is None else np.asarray(ac_baro_alt).astype(np.int64)
        out["dalt"] = _wrap32(base + f["geom_delta"].astype(np.int64)).astype(f64) / 6.25
        if positions is not None:
            out["lat"] = positions["lat"].astype(f64) / (180 / 2.0 ** 23)
            out["lon"] = positions["lon"].astype(f64) / (180 / 2.0 ** 23)
    return out


def item_presence(fields, positions=None, ids=None, ac_category=None):
    """name -> bool array: which items (by FSPEC bit) a record has; plus the pieces the length depends on."""
    f = fields
    n = len(f)
    fl, nav, op = f["flags"], f["nav_flags"], f["op_flags"]
    has = lambda a, bit: (a & bit) != 0                                                             # noqa: E731
    pos = np.isin(positions["method"], POS_METHODS) if positions is not None else np.zeros(n, dtype=bool)
    vel = has(fl, F_GS) & has(fl, F_HEADING) & (f["heading_type"] == HEADING_GROUND_TRACK)
    ops = has(op, OP_VALID)
    cc_tc = f["op_cc_tc"] & 3
    cat_valid = has(fl, F_CATEGORY)
    ac_cat = np.zeros(n, dtype=np.uint8) if ac_category is None else np.asarray(ac_category).astype(np.uint8)
    idv = np.zeros(n, dtype=np.uint64) if ids is None else np.asarray(ids).astype(np.uint64)
    true = np.ones(n, dtype=bool)
    return {
        "010": true, "040": true, "130": pos, "150": has(fl, F_IAS) | has(fl, F_MACH), "151": has(fl, F_TAS), "080": true, "073": pos, "075": vel,
        "140": has(fl, F_GEOM_ALT) | has(fl, F_GEOM_DELTA), "090": true, "210": ops, "070": has(fl, F_SQUAWK), "230": has(fl, F_ROLL),
        "145": has(fl, F_BARO_ALT), "152": has(fl, F_HEADING) & (f["heading_type"] == HEADING_MAGNETIC),
        "200": has(fl, F_SPI_VALID) | has(fl, F_ALERT_VALID) | has(fl, F_EMERGENCY) | has(nav, NAV_MODES),
        "155": has(fl, F_BARO_RATE), "157": has(fl, F_GEOM_RATE), "160": vel, "077": true, "170": has(fl, F_CALLSIGN),
        "020": cat_valid | (ac_cat == 0),
        "220": has(fl, F_WIND) | has(fl, F_OAT) | has(fl, F_TURBULENCE) | has(fl, F_STATIC_PRESSURE) | has(fl, F_HUMIDITY),
        "146": has(nav, NAV_FMS_ALT) | has(nav, NAV_MCP_ALT),
        "008": ops & (has(op, OP_OM_ACAS_RA) | (cc_tc != 0) | has(op, OP_CC_TS) | has(op, OP_CC_ARV) | has(op, OP_CC_CDTI) | ~has(op, OP_CC_ACAS)),
        "400": idv != 0,
    }


def asterix_classes(fields, positions=None, verdict=None, ac_baro_alt=None):
    """Per message NONE / LINE / DEFER / SKIP: the verdict as for the raw lines (FORWARD a record, DEFER listed), then the domain over
    the items the record has."""
    f = fields
    n = len(f)
    cls = np.full(n, LINE, dtype=np.uint8)
    if verdict is not None:
        v = np.asarray(verdict).astype(np.uint8) & 3
        cls = np.where(v == GATE_FORWARD, LINE, np.where(v == GATE_DEFER, DEFER, NONE)).astype(np.uint8)
    sv = scaled_values(f, positions, ac_baro_alt)
    p = item_presence(f, positions)
    fl = f["flags"]
    with np.errstate(invalid="ignore"):
        fits = {k: np.abs(x) < 2147483648.0 for k, x in sv.items()}
        ok = np.ones(n, dtype=bool)
        if positions is not None:
            ok &= ~p["130"] | ((np.abs(positions["lat"]) <= 90.0) & (np.abs(positions["lon"]) <= 360.0))
        ok &= ~((fl & F_MACH) != 0) | fits["mach"]
        ok &= ~p["230"] | fits["roll"]
        ok &= ~(p["145"] & (f["baro_alt_unit"] == 1)) | fits["baro_m"]
        ok &= ~p["152"] | fits["mag"]
        ok &= ~p["160"] | (fits["gs"] & fits["trk"])
        ok &= ~((fl & F_WIND) != 0) | fits["wd"]
        ok &= ~((fl & F_OAT) != 0) | fits["oat"]
    cls[(cls != NONE) & ~ok] = SKIP
    return cls


def _tod(t, midnight):
    """int tsm = t - midnight (truncated to 32 bits); + a day if negative; (int)(tsm * 0.128)"""
    tsm = ((int(t) - midnight + (1 << 31)) % (1 << 32)) - (1 << 31)
    if tsm < 0:
        tsm += DAY_MS
    return int(float(tsm) * 0.128)                      # int() truncates towards zero


def _category_byte(cat):
    """I021/020 with category_valid: the byte written for the category, None where the (tc, ca) pair has no case."""
    tc, ca = 0x0e - ((cat & 0xF0) >> 4), cat & 7
    if not ca:
        return 0
    if tc == 2:
        return {1: 20, 3: 21, 4: 22, 5: 22, 6: 22, 7: 22}.get(ca)
    if tc == 3:
        return {1: 11, 2: 12, 3: 16, 4: 15, 6: 13, 7: 14}.get(ca)
    if tc == 4:
        return 10 if ca == 7 else ca
    return None


def _be(v, nbytes):
    return [(v >> (8 * k)) & 0xFF for k in range(nbytes - 1, -1, -1)]


_NAMES = ("addr", "flags", "heading_type", "acc_flags", "nav_flags", "op_flags", "addrtype", "source", "airground", "tas", "nac_v", "nac_p", "sil", "sil_type", "sda", "gva",
          "op_version", "op_cc_tc", "squawkHex", "baro_alt", "baro_alt_unit", "nav_modes", "emergency", "callsign", "category", "wind_speed",
          "nav_fms_altitude", "nav_mcp_altitude")


def asterix_record(f, sv, has_pos, tod_msg, tod_now, rid, ac_cat, remote):
    """One record.  f: the members of a FIELDS record as Python values; sv: its converted values as Python ints (already truncated);
    -> (bytes, the set of item names whose FSPEC bit is set)"""
    fl, acc, nav, op = f["flags"], f["acc_flags"], f["nav_flags"], f["op_flags"]
    b, items = [], {"010", "040", "080", "090", "077"}
    b += [0, 1]
    # I021/040
    trd = 3 << 5 if f["addr"] & NON_ICAO else 2 << 5 if f["addrtype"] in (8, 9, 11) else 0
    if not fl & F_ALT_Q_BIT:
        trd |= 1 << 3
    b += [trd | 1, 1 << 6] if f["airground"] == 1 else [trd]
    if has_pos:                                                                                   # I021/130
        items |= {"130", "073"}
        lat, lon = sv["lat"], sv["lon"]
        b += _be(lat + 0x1000000 if lat < 0 else lat, 3) + _be(lon + 0x1000000 if lon < 0 else lon, 3)
    if fl & (F_IAS | F_MACH):                                                                     # I021/150
        items.add("150")
        v = sv["mach"] if fl & F_MACH else sv["ias"]
        b += [(0x80 if fl & F_MACH else 0) | ((v & 0x7F00) >> 8), v & 0xFF]
    if fl & F_TAS:                                                                                # I021/151
        items.add("151")
        b += [(f["tas"] & 0x7F00) >> 8, f["tas"] & 0xFF]
    b += _be(f["addr"], 3)                                                                        # I021/080
    if has_pos:                                                                                   # I021/073
        b += _be(tod_msg, 3)
    vel = (fl & F_GS) and (fl & F_HEADING) and f["heading_type"] == HEADING_GROUND_TRACK
    if vel:                                                                                       # I021/075
        items |= {"075", "160"}
        b += _be(tod_msg, 3)
    if fl & F_GEOM_ALT:                                                                           # I021/140
        items.add("140")
        b += _be(sv["galt"], 2)
    elif fl & F_GEOM_DELTA:
        items.add("140")
        b += _be(sv["dalt"], 2)
    # I021/090: the second extension's bits go where p + 1 points — the first extension's place if that one stayed empty
    q = [((f["nac_v"] << 5) & 0xFF) if acc & ACC_NAC_V_VALID else 0]
    e1 = (0x80 if (acc & ACC_NIC_BARO_VALID) and (acc & ACC_NIC_BARO) else 0) | (((f["sil"] << 5) & 0xFF) if f["sil_type"] != 0 else 0) \
        | (((f["nac_p"] << 1) & 0xFF) if acc & ACC_NAC_P_VALID else 0)
    e2 = (0x20 if f["sil_type"] == 2 else 0) | (((f["sda"] << 3) & 0xFF) if acc & ACC_SDA_VALID else 0) | (((f["gva"] << 1) & 0xFF) if acc & ACC_GVA_VALID else 0)
    for e in (e1, e2):
        if e:
            q[-1] |= 1
            q.append(e)
    b += q
    if op & OP_VALID:                                                                             # I021/210
        items.add("210")
        if remote:
            v = 2 if f["addrtype"] in (0, 8) else 1 if f["addrtype"] in (2, 9) else 0
        else:
            v = 2 if f["source"] == SOURCE_ADSB else 1 if f["source"] == SOURCE_ADSR else 0
        b.append(v | ((f["op_version"] & 7) << 3))
    if fl & F_SQUAWK:                                                                             # I021/070
        items.add("070")
        s = f["squawkHex"]
        b += [((s & 0x7000) >> 11) | ((s & 0x0400) >> 10), ((s & 0x0300) >> 2) | ((s & 0x0070) >> 1) | (s & 7)]
    if fl & F_ROLL:                                                                               # I021/230
        items.add("230")
        b += _be(sv["roll"], 2)
    if fl & F_BARO_ALT:                                                                           # I021/145
        items.add("145")
        b += _be(sv["baro_m"] if f["baro_alt_unit"] == 1 else sv["baro_ft"], 2)
    if (fl & F_HEADING) and f["heading_type"] == HEADING_MAGNETIC:                                # I021/152
        items.add("152")
        b += _be(sv["mag"], 2)
    if (fl & (F_SPI_VALID | F_ALERT_VALID | F_EMERGENCY)) or (nav & NAV_MODES):                   # I021/200
        items.add("200")
        v = 0x40 if (nav & NAV_MODES) and (f["nav_modes"] & 2) else 0
        if fl & F_EMERGENCY:
            v |= (f["emergency"] << 2) & 0xFF
        if fl & F_ALERT_VALID:
            v |= 1 if fl & F_ALERT else 0
        elif (fl & F_SPI_VALID) and (fl & F_SPI):
            v |= 3
        b.append(v)
    for flag, name, key in ((F_BARO_RATE, "155", "brate"), (F_GEOM_RATE, "157", "grate")):        # I021/155, /157
        if fl & flag:
            items.add(name)
            v = sv[key]                                                                           # already (int16_t)... >> 1
            b += [(v & 0x7F00) >> 8, v & 0xFF]
    if vel:                                                                                       # I021/160
        b += [(sv["gs"] & 0x7F00) >> 8, sv["gs"] & 0xFF] + _be(sv["trk"], 2)
    b += _be(tod_now, 3)                                                                          # I021/077
    if fl & F_CALLSIGN:                                                                           # I021/170
        items.add("170")
        enc = 0
        for ch in f["callsign"].ljust(8, b"\0"):
            k = AIS.find(chr(ch)) if 0 < ch < 128 else -1
            enc = (enc << 6) + (k if k >= 0 else 32)
        b += _be(enc, 6)
    if fl & F_CATEGORY:                                                                           # I021/020
        items.add("020")
        v = _category_byte(f["category"])
        if v is not None:
            b.append(v)
    elif ac_cat == 0:
        items.add("020")
        b.append(0)
    if fl & (F_WIND | F_OAT | F_TURBULENCE | F_STATIC_PRESSURE | F_HUMIDITY):                     # I021/220
        items.add("220")
        b.append((0xC0 if fl & F_WIND else 0) | (0x20 if fl & F_OAT else 0))
        if fl & F_WIND:
            b += _be(f["wind_speed"], 2) + _be(sv["wd"], 2)
        if fl & F_OAT:
            b += _be(sv["oat"], 2)
    if nav & (NAV_FMS_ALT | NAV_MCP_ALT):                                                         # I021/146
        items.add("146")
        mcp = bool(nav & NAV_MCP_ALT)
        alt = sv["mcp"] if mcp else sv["fms"]
        b += [(0xC0 if mcp else 0xE0) | ((alt & 0x1F00) >> 8), alt & 0xFF]
    cc_tc = f["op_cc_tc"] & 3
    if (op & OP_VALID) and ((op & (OP_OM_ACAS_RA | OP_CC_TS | OP_CC_ARV | OP_CC_CDTI)) or cc_tc or not op & OP_CC_ACAS):   # I021/008
        items.add("008")
        b.append((0x80 if op & OP_OM_ACAS_RA else 0) | cc_tc << 5 | (0x10 if op & OP_CC_TS else 0) | (8 if op & OP_CC_ARV else 0)
                 | (4 if op & OP_CC_CDTI else 0) | (0 if op & OP_CC_ACAS else 2))
    if rid:                                                                                       # I021/400
        items.add("400")
        b.append(rid & 0xFF)
    fspec = [0] * 7
    for name in items:
        k, bit = FSPEC_BITS[name]
        fspec[k] |= 1 << bit
    flen = 1
    for k in range(5, -1, -1):
        if fspec[k + 1]:
            fspec[k] |= 1
            flen += 1
    total = len(b) + 3 + flen
    return bytes([21, total >> 8, total & 0xFF] + fspec[:flen] + [x & 0xFF for x in b]), items


def asterix_reference(msgs, fields, now_ms, positions=None, verdict=None, ids=None, ac_baro_alt=None, ac_category=None, remote=False, want_items=False):
    """-> (stream bytes, record length per message (0: none), deferred[] {index, offset}, the number of skipped messages[, the items
    of every record written])"""
    n = len(msgs)
    assert len(fields) == n and 0 <= now_ms < MS_END
    cls = asterix_classes(fields, positions, verdict, ac_baro_alt)
    sv = {k: _trunc(v) for k, v in scaled_values(fields, positions, ac_baro_alt).items()}
    sv["baro_ft"] = _idiv25(fields["baro_alt"])
    sv["mcp"] = _idiv25(_wrap32(fields["nav_mcp_altitude"]))
    sv["fms"] = _idiv25(_wrap32(fields["nav_fms_altitude"]))
    for k in ("brate", "grate"):
        sv[k] = _wrap16(sv[k]) >> 1
    sv = {k: v.tolist() for k, v in sv.items()}
    cols = {k: fields[k].tolist() for k in _NAMES}
    ts = msgs["sysTimestamp"].tolist()
    has_pos = np.isin(positions["method"], POS_METHODS).tolist() if positions is not None else [False] * n
    idl = np.asarray(ids).astype(np.uint64).tolist() if ids is not None else [0] * n
    acc = np.asarray(ac_category).astype(np.uint8).tolist() if ac_category is not None else [0] * n
    midnight = int(now_ms) // 1000 // 86400 * DAY_MS
    tod_now = _tod(now_ms, midnight)
    recs, length, all_items = [], np.zeros(n, dtype=np.int64), []
    for i in np.nonzero(cls == LINE)[0].tolist():
        rec, items = asterix_record({k: cols[k][i] for k in _NAMES}, {k: v[i] for k, v in sv.items()}, has_pos[i], _tod(ts[i], midnight), tod_now,
                                    idl[i], acc[i], remote)
        assert len(rec) <= RECORD_MAX
        recs.append(rec)
        all_items.append(items)
        length[i] = len(rec)
    start = np.cumsum(length) - length
    dsel = cls == DEFER
    out = np.zeros(int(dsel.sum()), dtype=DEFERRED)
    out["index"], out["offset"] = np.nonzero(dsel)[0], start[dsel]
    res = (b"".join(recs), length, out, int((cls == SKIP).sum()))
    return res + (all_items,) if want_items else res


def asterix_of(c, now_ms=NOW_MS, gated=True, **kw):
    """asterix_reference on a case set."""
    return asterix_reference(c["msgs"], c["fields"], now_ms, positions=c["positions"], verdict=c["verdict"] if gated else None, ids=c["ids"],
                             ac_baro_alt=c["ac_baro_alt"], ac_category=c["ac_category"], **kw)


def split_records(stream):
    """The records of a stream by their own length fields."""
    out, k = [], 0
    while k < len(stream):
        assert stream[k] == 21
        l = stream[k + 1] << 8 | stream[k + 2]
        assert l >= 3 + 4 and k + l <= len(stream)
        out.append(stream[k:k + l])
        k += l
    return out


# ---- case generators ---------------------------------------------------------------------------------------------------------------

KEYS = ("msgs", "fields", "positions", "verdict", "ids", "ac_baro_alt", "ac_category")
FORWARD = np.uint8(GATE_FORWARD | su.GATE_RELIABLE | su.GATE_POSSIBLE | su.GATE_CERTAIN)


def empty_cases(n):
    return {"msgs": np.zeros(n, dtype=MSG), "fields": np.zeros(n, dtype=FIELDS), "positions": np.zeros(n, dtype=POSITION),
            "verdict": np.full(n, FORWARD, dtype=np.uint8), "ids": np.zeros(n, dtype=np.uint64), "ac_baro_alt": np.zeros(n, dtype=np.int32),
            "ac_category": np.zeros(n, dtype=np.uint8)}


def _base(n):
    c = empty_cases(n)
    c["fields"]["msgtype"], c["fields"]["metype"], c["fields"]["addr"], c["fields"]["source"] = 17, 11, 0x4840D6, SOURCE_ADSB
    c["fields"]["flags"] = F_ALT_Q_BIT
    c["msgs"]["sysTimestamp"] = NOW_MS - 876
    return c


def fuzz_cases(per_item, seed):
    """(a) field records of fuzzed frames of every DF / ME type and of Comm-B registers through the oracle's field decode, picked so that
    every item of the record is present in at least per_item records and absent in as many; gate-like verdicts, candidate positions on
    the records that carry a CPR word, receiver ids, aircraft state."""
    import fields_util as fu
    rng = np.random.default_rng(seed)
    parts = [fu.fuzz_frames(40 * per_item, seed + 1, dfs=(17, 18)), fu.fuzz_frames(8 * per_item, seed + 2, dfs=(0, 4, 5, 11, 16, 20, 21, 24, 27, 31)),
             fu.commb_frames(100 * per_item, seed + 3)]
    # ME types a uniform draw gives 1 in 32 of: operational status (31, subtypes 0 and 1) and velocity over ground (19, subtypes 1 and 2)
    for k, (me, sub_lo) in enumerate(((31, 0), (19, 1))):
        es_frames, es_bits = fu.fuzz_frames(20 * per_item, seed + 5 + k, dfs=(17, 18))
        es_frames[:, 4] = (me << 3) | (sub_lo + (es_frames[:, 4] & 1))
        parts.append((fu.seal(es_frames), es_bits))
    frames, bits = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    fields = fu.oracle_fields(frames, bits).view(FIELDS)
    n_all = len(fields)
    positions = np.zeros(n_all, dtype=POSITION)
    has_cpr = (fields["flags"] & F_CPR) != 0
    positions["method"] = np.where(has_cpr, rng.integers(0, 5, size=n_all), 0)
    ids = np.where(rng.random(n_all) < 0.5, 0, rng.integers(1, 1 << 63, size=n_all, dtype=np.uint64))
    ac_cat = np.where(rng.random(n_all) < 0.5, 0, rng.integers(1, 256, size=n_all)).astype(np.uint8)
    pres = item_presence(fields, positions, ids, ac_cat)
    pick = np.zeros(n_all, dtype=bool)
    for name, p in sorted(pres.items()):
        for side in (p, ~p):
            if name in ("010", "040", "080", "090", "077") and side is not p:
                continue
            short = per_item - int((pick & side).sum())                 # what earlier picks leave to do
            idx = np.nonzero(side & ~pick)[0]
            assert len(idx) >= short, (name, len(idx), {k: int(v.sum()) for k, v in pres.items()})
            if short > 0:
                pick[rng.permutation(idx)[:short]] = True
    pick = rng.permutation(np.nonzero(pick)[0])
    n = len(pick)
    c = empty_cases(n)
    c["fields"], c["positions"] = fields[pick].copy(), positions[pick].copy()
    c["ids"][:], c["ac_category"][:] = ids[pick], ac_cat[pick]
    c["msgs"]["msg"], c["msgs"]["raw"], c["msgs"]["msgbits"] = frames[pick], frames[pick], bits[pick]
    c["msgs"]["msgtype"], c["msgs"]["addr"] = c["fields"]["msgtype"], c["fields"]["addr"]
    c["msgs"]["sysTimestamp"] = NOW_MS - 40000000 + np.cumsum(rng.integers(0, 5000, size=n))
    c["msgs"]["timestamp"] = 12000 * (c["msgs"]["sysTimestamp"] - (NOW_MS - 40000000))
    c["verdict"][:] = gate_like_verdicts(n, seed + 4)
    placed = np.isin(c["positions"]["method"], POS_METHODS)
    c["positions"]["lat"] = np.where(placed, rng.uniform(-90, 90, size=n), 0.0)
    c["positions"]["lon"] = np.where(placed, rng.uniform(-180, 180, size=n), 0.0)
    c["ac_baro_alt"][:] = rng.integers(-1000, 45000, size=n)
    return c


def clock_cases():
    """sysTimestamps on both sides of NOW_MS's midnight and of the 32-bit wrap of the difference, with a position (I021/073) and with a
    ground vector (I021/075); the golden runs them at every now_ms of CLOCKS besides."""
    mid = NOW_MS // 1000 // 86400 * DAY_MS
    stamps = [mid, mid - 1, mid + 1, mid + DAY_MS - 1, mid + DAY_MS, mid - DAY_MS, mid - DAY_MS - 1, mid + (1 << 31) - 1, mid + (1 << 31), mid + (1 << 31) + 1,
              mid - (1 << 31), mid - (1 << 31) - 1, mid - (1 << 31) + DAY_MS, mid - (1 << 31) + DAY_MS - 1, mid + (1 << 32), mid + (1 << 32) - 1, 0, -1, NOW_MS,
              (1 << 63) - 1, -(1 << 63), MS_END - 1, mid + 7, mid + 8, mid + 15, mid + 16, mid + 125, mid + 1000]
    c = _base(2 * len(stamps))
    c["msgs"]["sysTimestamp"] = stamps + stamps
    c["positions"]["method"][:len(stamps)] = 1
    c["positions"]["lat"], c["positions"]["lon"] = 52.25, 4.75
    f = c["fields"]
    f["flags"][len(stamps):] |= F_GS | F_HEADING
    f["heading_type"], f["gs_v0"], f["heading"] = HEADING_GROUND_TRACK, 431.5, 271.25
    return c


def edge_cases(seed):
    """(b) the edges: see tests/golden/make_asterix_golden.py."""
    rng = np.random.default_rng(seed)
    parts = []
    # every category byte with category_valid (every (tc, ca) pair and the bits above them), and not valid; aircraft category 0 and not
    c = _base(256 * 4)
    k = np.arange(256 * 4)
    c["fields"]["category"] = k & 255
    c["fields"]["flags"] |= np.where(k & 256, F_CATEGORY, 0).astype(np.uint32)
    c["ac_category"][:] = np.where(k & 512, (k & 255) | 1, 0)
    parts.append(c)
    # I021/090: every combination of its seven inputs, with small and with byte-filling values
    c = _base(128 * 3 * 2)
    k = np.arange(len(c["verdict"]))
    m, st, big = k & 127, (k >> 7) % 3, k >= 384
    f = c["fields"]
    f["acc_flags"] = (np.where(m & 1, ACC_NAC_V_VALID, 0) | np.where(m & 2, ACC_NIC_BARO_VALID, 0) | np.where(m & 4, ACC_NIC_BARO, 0)
                      | np.where(m & 8, ACC_NAC_P_VALID, 0) | np.where(m & 16, ACC_SDA_VALID, 0) | np.where(m & 32, ACC_GVA_VALID, 0)).astype(np.uint16)
    f["sil_type"] = np.where(m & 64, st + 1, 0)
    f["nac_v"], f["nac_p"], f["sil"], f["sda"], f["gva"] = np.where(big, 255, 1 + m % 4), np.where(big, 255, 1 + m % 11), np.where(big, 255, 1 + m % 3), \
        np.where(big, 255, 1 + m % 3), np.where(big, 255, 1 + m % 2)
    parts.append(c)
    # the same with zero values behind set valid flags: extensions that stay empty
    c = _base(128)
    m = np.arange(128)
    c["fields"]["acc_flags"] = (np.where(m & 1, ACC_NAC_V_VALID, 0) | np.where(m & 2, ACC_NIC_BARO_VALID, 0) | np.where(m & 8, ACC_NAC_P_VALID, 0)
                                | np.where(m & 16, ACC_SDA_VALID, 0) | np.where(m & 32, ACC_GVA_VALID, 0)).astype(np.uint16)
    c["fields"]["sil_type"] = np.where(m & 64, 1 + (m & 4) // 2, 0)
    parts.append(c)
    # I021/040: address types, the non-ICAO bit, the Q bit, every airground
    rows = [(at, ni, q, ag) for at in range(16) for ni in (0, 1) for q in (0, 1) for ag in range(4)]
    c = _base(len(rows))
    f = c["fields"]
    f["addrtype"], f["airground"] = [r[0] for r in rows], [r[3] for r in rows]
    f["addr"] = [0xABCDEF | (NON_ICAO if r[1] else 0) for r in rows]
    f["flags"] = [F_ALT_Q_BIT if r[2] else 0 for r in rows]
    parts.append(c)
    # FSPEC lengths 4, 5, 6 by each item of the last two bytes alone and together
    c = _base(32)
    k = np.arange(32)
    f = c["fields"]
    c["ac_category"][:] = 7
    f["flags"] |= (np.where(k & 1, F_CALLSIGN, 0) | np.where(k & 2, F_HUMIDITY, 0)).astype(np.uint32)
    f["nav_flags"] = np.where(k & 4, NAV_FMS_ALT, 0)
    f["op_flags"] = np.where(k & 8, OP_VALID, 0) | OP_CC_ACAS * ((k & 24) == 8)
    c["ids"][:] = np.where(k & 16, 0x2A, 0)
    f["callsign"] = b"FSPEC   "
    parts.append(c)
    parts.append(clock_cases())
    # all 4096 squawks, and each with bit patterns of squawkHex above and between the twelve bits the item takes
    digits = np.arange(4096)
    hexes = ((digits >> 9) & 7) << 12 | ((digits >> 6) & 7) << 8 | ((digits >> 3) & 7) << 4 | (digits & 7)
    c = _base(4096 * 4)
    c["fields"]["flags"] |= F_SQUAWK
    c["fields"]["squawkHex"] = np.concatenate([hexes, hexes | 0x8000, hexes | 0x0888, hexes | 0x8888])
    parts.append(c)
    # callsigns: the whole AIS set, bytes outside it, NULs in every place, bytes above 127
    names = [AIS[k:k + 8].encode() for k in range(0, 64, 8)] + [b"KLM 1023", b"", b"A", b"AB\0DEFGH", b"\0BCDEFGH", b"abcdefgh", b"\xff\x80\x7f\x01`{~\xc1",
                                                                   b"@@@@@@@@", b"????????", b"        ", b"\x1f\x20\x3f\x40\x5f\x60\x00\x41"]
    c = _base(len(names))
    c["fields"]["callsign"] = names
    c["fields"]["flags"] |= F_CALLSIGN
    parts.append(c)
    # I021/210: every source and address type, every version byte's low bits and a few above them; the operational status bits of I021/008
    rows = [(src, at, ver) for src in range(12) for at in range(16) for ver in (0, 1, 2, 7, 8, 255)]
    c = _base(len(rows))
    f = c["fields"]
    f["source"], f["addrtype"], f["op_version"] = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    f["op_flags"] = OP_VALID | OP_CC_ACAS
    parts.append(c)
    c = _base(64 * 6)
    k = np.arange(64 * 6)
    f = c["fields"]
    f["op_flags"] = (np.where(k & 1, OP_VALID, 0) | np.where(k & 2, OP_OM_ACAS_RA, 0) | np.where(k & 4, OP_CC_TS, 0) | np.where(k & 8, OP_CC_ARV, 0)
                     | np.where(k & 16, OP_CC_CDTI, 0) | np.where(k & 32, OP_CC_ACAS, 0)).astype(np.uint16)
    f["op_cc_tc"] = np.array([0, 1, 2, 3, 4, 255])[k >> 6]
    parts.append(c)
    # receiver ids
    idv = [0, 1, 0x100, 0x1FF, (1 << 64) - 1, 0xFF, 0xFFFFFFFFFFFFFF00, 1 << 63]
    c = _base(len(idv))
    c["ids"][:] = np.array(idv, dtype=np.uint64)
    parts.append(c)
    # I021/200: every combination of its inputs; every emergency value
    c = _base(256 * 2)
    k = np.arange(512)
    f = c["fields"]
    f["flags"] |= (np.where(k & 1, F_SPI_VALID, 0) | np.where(k & 2, F_SPI, 0) | np.where(k & 4, F_ALERT_VALID, 0) | np.where(k & 8, F_ALERT, 0)
                   | np.where(k & 16, F_EMERGENCY, 0)).astype(np.uint32)
    f["nav_flags"] = np.where(k & 32, NAV_MODES, 0)
    f["nav_modes"] = np.where(k & 64, 2, 61)
    f["emergency"] = np.where(k & 256, 255, (k >> 7) * 5 + 1)
    parts.append(c)
    # I021/146 and the integer divisions: selected altitudes and barometric altitudes around multiples of 25, negative, at the ends
    alts = [0, 1, 24, 25, 26, 49, 50, 36000, 65535, 65536, 204799, 204800, INT32_MAX, 1 << 31, (1 << 32) - 1, (1 << 32) - 24, (1 << 32) - 25, (1 << 32) - 26]
    c = _base(len(alts) * 3)
    f = c["fields"]
    f["nav_mcp_altitude"] = alts * 3
    f["nav_fms_altitude"] = alts[::-1] * 3
    f["nav_flags"] = np.repeat([NAV_MCP_ALT, NAV_FMS_ALT, NAV_MCP_ALT | NAV_FMS_ALT], len(alts))
    f["baro_alt"] = _wrap32(np.array(alts * 3))
    f["flags"] |= F_BARO_ALT
    parts.append(c)
    # I021/220: every combination of the five valid flags
    c = _base(32)
    k = np.arange(32)
    f = c["fields"]
    f["flags"] |= (np.where(k & 1, F_WIND, 0) | np.where(k & 2, F_OAT, 0) | np.where(k & 4, F_TURBULENCE, 0) | np.where(k & 8, F_STATIC_PRESSURE, 0)
                   | np.where(k & 16, F_HUMIDITY, 0)).astype(np.uint32)
    f["wind_speed"], f["wind_direction"], f["oat"] = 0xABCD, 359.9, -56.75
    parts.append(c)
    # geometric height by the aircraft's barometric altitude: sums that wrap, both units, vertical rates at the ends
    vals = [0, 1, -1, 6, 7, -6, -7, 38000, -1000, 204793, 204794, -204800, -204801, INT32_MAX, INT32_MIN]
    rows = [(a, d) for a in vals for d in vals]
    c = _base(len(rows) * 2)
    f = c["fields"]
    f["geom_delta"] = [r[1] for r in rows] * 2
    f["geom_alt"] = [r[0] for r in rows] * 2
    c["ac_baro_alt"][:] = [r[0] for r in rows] * 2
    f["flags"][:len(rows)] |= F_GEOM_DELTA | F_BARO_RATE | F_GEOM_RATE
    f["flags"][len(rows):] |= F_GEOM_ALT | F_GEOM_DELTA
    f["geom_alt_unit"][len(rows):] = np.arange(len(rows)) % 3
    f["baro_rate"], f["geom_rate"] = f["geom_alt"], f["geom_delta"]
    parts.append(c)
    # speeds: every kind of I021/150 / 151
    ias = [0, 1, 219, 220, 450, 1023, 65535]
    c = _base(len(ias) * 4)
    f = c["fields"]
    f["ias"], f["tas"] = ias * 4, [65535 - v for v in ias] * 4
    f["mach"] = 0.82
    f["flags"] |= np.repeat([F_IAS, F_MACH, F_IAS | F_MACH | F_TAS, F_TAS], len(ias)).astype(np.uint32)
    parts.append(c)
    # the longest record
    c = _base(2)
    f = c["fields"]
    f["flags"] = (F_BARO_ALT | F_GEOM_ALT | F_HEADING | F_GS | F_IAS | F_TAS | F_BARO_RATE | F_GEOM_RATE | F_SQUAWK | F_CALLSIGN | F_CATEGORY | F_SPI_VALID | F_ROLL | F_MACH
                  | F_WIND | F_OAT)
    f["heading_type"], f["airground"], f["category"], f["callsign"] = HEADING_GROUND_TRACK, 1, 0xA3, b"LONGEST1"
    f["acc_flags"], f["sil_type"], f["nac_p"], f["sda"] = ACC_NAC_P_VALID | ACC_SDA_VALID, 2, 9, 2
    f["op_flags"], f["nav_flags"] = OP_VALID, NAV_MCP_ALT
    c["positions"]["method"], c["positions"]["lat"], c["positions"]["lon"] = 1, -33.9, 151.2
    c["ids"][:] = 0x1234
    f["heading_type"][1] = HEADING_MAGNETIC
    parts.append(c)
    # flag combinations at random over plausible values
    n = 1500
    c = _base(n)
    f = c["fields"]
    f["flags"] = rng.integers(0, 1 << 29, size=n) & rng.integers(0, 1 << 29, size=n)
    f["acc_flags"], f["nav_flags"] = rng.integers(0, 1 << 12, size=n), rng.integers(0, 32, size=n)
    f["op_flags"] = rng.integers(0, 1 << 14, size=n) | (rng.random(n) < 0.5)
    for name in ("addrtype", "source", "airground", "category", "emergency", "baro_alt_unit", "geom_alt_unit", "sil_type", "nac_p", "nac_v", "sil", "gva", "sda",
                 "op_version", "op_cc_tc", "nav_modes"):
        f[name] = rng.integers(0, 16, size=n)
    f["heading_type"] = rng.integers(0, 6, size=n)
    f["squawkHex"], f["ias"], f["tas"], f["wind_speed"] = rng.integers(0, 65536, size=n), rng.integers(0, 600, size=n), rng.integers(0, 600, size=n), rng.integers(0, 300, size=n)
    f["baro_alt"], f["geom_alt"], f["geom_delta"] = rng.integers(-1000, 50000, size=n), rng.integers(-1000, 50000, size=n), rng.integers(-2000, 2000, size=n)
    f["baro_rate"], f["geom_rate"] = rng.integers(-40000, 40000, size=n), rng.integers(-40000, 40000, size=n)
    f["gs_v0"], f["heading"], f["roll"], f["mach"] = rng.uniform(0, 1200, size=n), rng.uniform(0, 360, size=n), rng.uniform(-90, 90, size=n), rng.uniform(0, 4, size=n)
    f["oat"], f["wind_direction"] = rng.uniform(-128, 128, size=n), rng.uniform(0, 360, size=n)
    f["nav_mcp_altitude"], f["nav_fms_altitude"] = rng.integers(0, 65536, size=n) * 16, rng.integers(0, 65536, size=n) * 16
    f["callsign"] = [bytes(rng.choice(list(b"ABCXYZ019 _"), size=8).tolist()) for _ in range(n)]
    f["addr"] = rng.integers(0, 1 << 25, size=n)
    c["positions"]["method"] = rng.integers(0, 5, size=n)
    c["positions"]["lat"], c["positions"]["lon"] = rng.uniform(-90, 90, size=n), rng.uniform(-180, 180, size=n)
    c["msgs"]["sysTimestamp"] = NOW_MS - rng.integers(0, 3 * DAY_MS, size=n)
    c["ids"][:] = np.where(rng.random(n) < 0.5, 0, rng.integers(0, 1 << 16, size=n)).astype(np.uint64)
    c["ac_baro_alt"][:], c["ac_category"][:] = rng.integers(-1000, 50000, size=n), np.where(rng.random(n) < 0.5, 0, 0xA1)
    c["verdict"][:] = gate_like_verdicts(n, seed + 1)
    parts.append(c)
    return concat_cases(parts)


def _neighbours(x, dtype):
    x = np.asarray(x, dtype=dtype)
    return np.concatenate([x, np.nextafter(x, dtype(np.inf)), np.nextafter(x, dtype(-np.inf))])


def _sources_at(scale, targets, dtype, op="mul"):
    """Source values (of dtype) whose product with (quotient by) `scale` lies next to each integer target: the nearest source and both
    of its neighbours in the source type."""
    t = np.asarray(targets, dtype=np.float64)
    x = (t / scale if op == "mul" else t * scale).astype(dtype)
    return _neighbours(x, dtype)


LIMIT = 2147483648.0


def tie_cases(seed):
    """(c) for each scaled item the values whose product sits on and on either side of an integer, zeros of both signs, the ends of the
    domain (the largest magnitudes below 2^31 after scaling)."""
    rng = np.random.default_rng(seed)
    ints = np.concatenate([np.arange(-40, 41), rng.integers(-70000, 70000, size=160), [255, 256, 32767, 32768, 65535, 65536, -32768, -32769, -65536,
                           (1 << 31) - 1, -(1 << 31) + 1, (1 << 31) - 200, 1 << 24, -(1 << 24)]]).astype(np.float64)
    f32, f64 = np.float32, np.float64
    zeros32, zeros64 = np.array([0.0, -0.0, 1e-45, -1e-45], dtype=f32), np.array([0.0, -0.0, 5e-324, -5e-324])
    parts = []

    def below(x, scaled, dtype):
        """x stepped towards zero until scaled(x) is inside the domain"""
        x = np.asarray(x, dtype=dtype)
        for _ in range(8):
            bad = ~(np.abs(scaled(x)) < LIMIT)
            x = np.where(bad, np.nextafter(x, dtype(0)), x)
        return x

    def float_set(scale, scaled):
        x = np.concatenate([_sources_at(scale, ints, f32), zeros32, below(np.array([LIMIT / scale, -LIMIT / scale], dtype=f32), scaled, f32)])
        x = x[np.abs(scaled(x)) < LIMIT]
        return x

    # roll * 100 and oat * 4: float products
    for name, flag, scale in (("roll", F_ROLL, 100.0), ("oat", F_OAT, 4.0)):
        x = float_set(scale, lambda v, s=scale: (v.astype(f32) * f32(s)).astype(f64))
        c = _base(len(x))
        c["fields"][name] = x
        c["fields"]["flags"] |= flag
        parts.append(c)
    # mach * 1000, heading * 182.0444 (magnetic), heading * (65536 / 360.0) and gs_v0 * 4.5511 (ground track), wind_direction: floats widened
    x = float_set(1000.0, lambda v: v.astype(f64) * 1000.0)
    c = _base(len(x))
    c["fields"]["mach"] = x
    c["fields"]["flags"] |= F_MACH
    parts.append(c)
    x = float_set(182.0444, lambda v: v.astype(f64) * 182.0444)
    c = _base(len(x))
    c["fields"]["heading"], c["fields"]["heading_type"] = x, HEADING_MAGNETIC
    c["fields"]["flags"] |= F_HEADING
    parts.append(c)
    xh = float_set(65536 / 360.0, lambda v: v.astype(f64) * (65536 / 360.0))
    xg = float_set(4.5511, lambda v: v.astype(f64) * 4.5511)
    n = max(len(xh), len(xg))
    c = _base(n)
    c["fields"]["heading"], c["fields"]["gs_v0"], c["fields"]["heading_type"] = np.resize(xh, n), np.resize(xg, n), HEADING_GROUND_TRACK
    c["fields"]["flags"] |= F_HEADING | F_GS
    parts.append(c)
    x = float_set(1.0, lambda v: v.astype(f64))
    c = _base(len(x))
    c["fields"]["wind_direction"], c["fields"]["wind_speed"] = x, 77
    c["fields"]["flags"] |= F_WIND
    parts.append(c)
    # ias / 3600.0 * 16384: every value whose product is an integer (multiples of 225) with its neighbours, the ends
    ias = np.unique(np.clip(np.concatenate([np.arange(0, 65536, 225), np.arange(0, 65536, 225) + 1, np.arange(225, 65536, 225) - 1, [65535, 7, 8]]), 0, 65535))
    c = _base(len(ias))
    c["fields"]["ias"] = ias
    c["fields"]["flags"] |= F_IAS
    parts.append(c)
    # the integer sources: geom_alt / 6.25 and / 20.5053, rates / 3.125, baro_alt * 3.2808 (metres), baro_alt / 25
    iv = np.unique(np.concatenate([np.arange(-60, 61), (ints[np.abs(ints) < 70000] * 6.25).astype(np.int64), (ints[np.abs(ints) < 70000] * 20.5053).astype(np.int64),
                                   (ints[np.abs(ints) < 70000] * 3.125).astype(np.int64) + rng.integers(-1, 2, size=int((np.abs(ints) < 70000).sum())),
                                   (ints[np.abs(ints) < 70000] / 3.2808).astype(np.int64), [INT32_MAX, INT32_MIN, 654561585, 654561586, -654561585, -654561586,
                                                                                          204799, 204800, 204806, -204800, -204806, 102400, 102396]]))
    c = _base(len(iv) * 2)
    f = c["fields"]
    f["geom_alt"], f["baro_alt"], f["baro_rate"], f["geom_rate"] = (np.tile(iv, 2),) * 4
    f["flags"] |= F_GEOM_ALT | F_BARO_ALT | F_BARO_RATE | F_GEOM_RATE
    f["geom_alt_unit"], f["baro_alt_unit"] = np.repeat([0, 1], len(iv)), np.repeat([0, 1], len(iv))
    inside = asterix_classes(f) != SKIP
    parts.append({k: v[inside] for k, v in c.items()})
    # positions: lat / (180 / 2^23) next to integers, zeros, the ends of the domain
    unit = 180 / 2.0 ** 23
    la = np.concatenate([_sources_at(unit, ints[np.abs(ints) <= 1 << 22], f64, op="div"), zeros64, [90.0, -90.0, np.nextafter(90.0, 0), np.nextafter(-90.0, 0)]])
    lo = np.concatenate([_sources_at(unit, ints[np.abs(ints) <= 1 << 24], f64, op="div"), zeros64, [360.0, -360.0, 180.0, -180.0, np.nextafter(360.0, 0), np.nextafter(-360.0, 0)]])
    la, lo = la[np.abs(la) <= 90.0], lo[np.abs(lo) <= 360.0]
    n = max(len(la), len(lo))
    c = _base(n)
    c["positions"]["method"] = 1 + np.arange(n) % 3
    c["positions"]["lat"], c["positions"]["lon"] = np.resize(la, n), np.resize(lo, n)
    parts.append(c)
    c = concat_cases(parts)
    assert (asterix_classes(c["fields"], c["positions"]) == LINE).all()
    return c


def outside_cases():
    """(d) records outside the domain, and their twins whose offending value belongs to an item the record does not have."""
    f32 = np.float32
    bad = np.array([np.inf, -np.inf, np.nan, 3.0e38, -3.0e38], dtype=f32)
    def edge(scale, scaled):
        """the float32 values of least magnitude whose scaled value is outside the domain, both signs"""
        x = np.array([LIMIT / scale, -LIMIT / scale], dtype=f32)
        for _ in range(8):
            x = np.where(np.abs(scaled(x)) < LIMIT, np.nextafter(x, f32([np.inf, -np.inf])), x)
        assert not (np.abs(scaled(x)) < LIMIT).any()
        return x
    wide = lambda s: (lambda v: v.astype(np.float64) * s)                                          # noqa: E731
    narrow = lambda s: (lambda v: (v.astype(f32) * f32(s)).astype(np.float64))                      # noqa: E731
    rows = []                                       # (member, value, flags, heading_type)
    for name, flag, scale, fn in (("roll", F_ROLL, 100.0, narrow), ("oat", F_OAT, 4.0, narrow), ("mach", F_MACH, 1000.0, wide), ("wind_direction", F_WIND, 1.0, wide)):
        for x in np.concatenate([bad, edge(scale, fn(scale))]):
            rows += [(name, x, flag, 0), (name, x, 0, 0)]
    for ht, scale in ((HEADING_MAGNETIC, 182.0444), (HEADING_GROUND_TRACK, 65536 / 360.0)):
        for x in np.concatenate([bad, edge(scale, wide(scale))]):
            rows += [("heading", x, F_HEADING | F_GS, ht), ("heading", x, F_GS, ht), ("heading", x, F_HEADING | F_GS, 2)]
    for x in np.concatenate([bad, edge(4.5511, wide(4.5511))]):
        rows += [("gs_v0", x, F_HEADING | F_GS, HEADING_GROUND_TRACK), ("gs_v0", x, F_HEADING | F_GS, HEADING_MAGNETIC), ("gs_v0", x, F_GS, HEADING_GROUND_TRACK)]
    c = _base(len(rows))
    for k, (name, x, flag, ht) in enumerate(rows):
        c["fields"][name][k], c["fields"]["heading_type"][k] = x, ht
        c["fields"]["flags"][k] |= flag
    parts = [c]
    # metres beyond the domain, feet never
    alts = [654561586, -654561586, INT32_MAX, INT32_MIN, 654561585, -654561585]
    c = _base(len(alts) * 2)
    c["fields"]["baro_alt"], c["fields"]["baro_alt_unit"] = alts * 2, np.repeat([1, 0], len(alts))
    c["fields"]["flags"] |= F_BARO_ALT
    parts.append(c)
    bad_p = [(np.nan, 0), (0, np.nan), (np.inf, 0), (0, -np.inf), (90.00000000000001, 0), (-90.00000000000001, 0), (0, 360.00000000000006),
             (0, -360.00000000000006), (90.0, 360.0), (-90.0, -360.0), (1e300, 1e300)]
    c = _base(2 * len(bad_p))
    for k, (la, lo) in enumerate(bad_p):
        for m, method in enumerate((2, 4)):
            c["positions"]["lat"][2 * k + m], c["positions"]["lon"][2 * k + m], c["positions"]["method"][2 * k + m] = la, lo, method
    parts.append(c)
    c = concat_cases(parts)
    c["verdict"][::3] = GATE_DEFER
    c["verdict"][1::7] = su.GATE_DROP
    return c


def hostile_cases(n, seed):
    """Random bytes as field and position records, with enough of them steered back into the domain that records of every kind appear."""
    rng = np.random.default_rng(seed)
    c = empty_cases(n)
    c["fields"] = rng.integers(0, 256, size=n * FIELDS.itemsize, dtype=np.uint8).view(FIELDS).copy()
    c["positions"] = rng.integers(0, 256, size=n * POSITION.itemsize, dtype=np.uint8).view(POSITION).copy()
    f = c["fields"]
    tame = rng.random(n) < 0.85
    k = int(tame.sum())
    f["roll"][tame], f["oat"][tame], f["mach"][tame] = rng.uniform(-90, 90, size=k), rng.uniform(-128, 128, size=k), rng.uniform(0, 4, size=k)
    f["heading"][tame], f["gs_v0"][tame], f["wind_direction"][tame] = rng.uniform(-400, 400, size=k), rng.uniform(-700, 2000, size=k), rng.uniform(0, 360, size=k)
    f["baro_alt"][tame] = rng.integers(-100000000, 100000000, size=k)
    f["heading_type"][tame] = rng.integers(0, 6, size=k)
    c["positions"]["method"] = rng.integers(0, 6, size=n)
    c["positions"]["lat"][tame], c["positions"]["lon"][tame] = rng.uniform(-90, 90, size=k), rng.uniform(-360, 360, size=k)
    sparse = rng.random(n) < 0.3                                     # records with few items, as real ones
    f["flags"][sparse] &= rng.integers(0, 1 << 32, size=int(sparse.sum()), dtype=np.uint32) & rng.integers(0, 1 << 32, size=int(sparse.sum()), dtype=np.uint32)
    c["msgs"]["sysTimestamp"] = np.where(rng.random(n) < 0.8, NOW_MS - rng.integers(0, 2 * DAY_MS, size=n), rng.integers(-(1 << 63), (1 << 63) - 1, size=n))
    c["verdict"][:] = rng.integers(0, 256, size=n, dtype=np.uint8)
    c["verdict"][rng.random(n) < 0.5] = FORWARD
    c["ids"][:] = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    c["ids"][rng.random(n) < 0.3] = 0
    c["ac_baro_alt"][:] = rng.integers(INT32_MIN, INT32_MAX, size=n).astype(np.int32)
    c["ac_category"][:] = np.where(rng.random(n) < 0.5, 0, rng.integers(0, 256, size=n)).astype(np.uint8)
    return c


def longest_cases(n):
    """n records of RECORD_MAX bytes."""
    c = _base(n)
    f = c["fields"]
    f["flags"] = (F_BARO_ALT | F_GEOM_ALT | F_HEADING | F_GS | F_IAS | F_TAS | F_BARO_RATE | F_GEOM_RATE | F_SQUAWK | F_CALLSIGN | F_CATEGORY | F_SPI_VALID | F_ROLL | F_MACH
                  | F_WIND | F_OAT)
    f["heading_type"], f["airground"], f["category"], f["callsign"] = HEADING_GROUND_TRACK, 1, 0xA3, b"LONGEST1"
    f["acc_flags"], f["sil_type"], f["nac_p"], f["sda"] = ACC_NAC_P_VALID | ACC_SDA_VALID, 2, 9, 2
    f["op_flags"], f["nav_flags"] = OP_VALID, NAV_MCP_ALT
    f["squawkHex"], f["baro_alt"], f["geom_alt"], f["gs_v0"], f["heading"] = 0x7421 + (np.arange(n) & 0xF), 38000 + np.arange(n), 39000, 447.0, 123.4 + np.arange(n) % 200
    c["positions"]["method"], c["positions"]["lat"], c["positions"]["lon"] = 1, -33.9, 151.2
    c["ids"][:] = 0x1200 + np.arange(n)
    return c


# ---- the golden file ------------------------------------------------------------------------------------------------------------------

GOLDEN = os.path.join(helpers.GOLDEN_DIR, "asterix_cases.npz")
GROUPS = ("a", "b", "c", "d")
# (now_ms, remote) of every stored reference run of groups a-c; the clock group of (b) is run at each of CLOCKS besides
RUNS = ((NOW_MS, 0), (NOW_MS, 1))
_MID = NOW_MS // 1000 // 86400 * DAY_MS
CLOCKS = (_MID, _MID + 999, _MID + 1000, _MID + DAY_MS - 1, _MID - 1, 0, 999, MS_END - 1, _MID + 7, _MID + 8)


def in_domain(c):
    keep = asterix_classes(c["fields"], c["positions"], None, c["ac_baro_alt"]) != SKIP
    return {k: v[keep] for k, v in c.items()}


def load_golden():
    """-> (the case sets by group, the stored streams by name (ref_<group>_r<remote> and ref_clock_<now_ms>: the reference's own bytes
    of the in-domain records, without verdicts), the class of every record by group)"""
    z = np.load(GOLDEN)
    sets = {g: {k: z[f"{g}_{k}"] for k in KEYS} for g in GROUPS}
    streams = {k: z[k].tobytes() for k in z.files if k.startswith("ref_")}
    return sets, streams, {g: z[f"cls_{g}"] for g in GROUPS}


# ---- the reference's own writer (tests/host_stub/asterix_ref_harness.c) ---------------------------------------------------------------

HARNESS_SRC = os.path.join(helpers.ROOT, "tests", "host_stub", "asterix_ref_harness.c")
HARNESS_CASE = np.dtype([("sysTimestamp", "<i8"), ("lat", "<f8"), ("lon", "<f8"), ("id", "<u8"), ("ac_baro_alt", "<i4"), ("has_pos", "u1"),
                         ("ac_category", "u1"), ("pad", "u1", 2), ("fields", FIELDS)])
have_ref_full = su.have_ref_full


def build_ref_harness(workdir):
    """tests/host_stub/asterix_ref_harness.c — which includes the reference's net_io.c — compiled with the flags of `make -C oracle full`
    and linked against that build's other objects, readsb.o with its main renamed in a copy."""
    exe = os.path.join(workdir, "asterix_ref_harness")
    main_o = os.path.join(workdir, "readsb_nomain_asterix.o")
    subprocess.run(["objcopy", "--redefine-sym", "main=readsb_main", os.path.join(su.REF_FULL, "readsb.o"), main_o], check=True)
    objs, flags = su._full_build()
    subprocess.run(["gcc", *flags, "-I" + os.path.join(helpers.ORACLE_DIR, "stub_full"), "-I/root/reference", "-I" + os.path.join(helpers.ROOT, "include"),
                    HARNESS_SRC, main_o, *[os.path.join(su.REF_FULL, o + ".o") for o in objs], "-o", exe, "-pthread", "-lpthread", "-lm", "-lrt",
                    "-l:libzstd.so.1", "-lz"], check=True)
    return exe


def run_ref_harness(exe, c, now_ms=NOW_MS, remote=False, workdir=None):
    """Every record of the case set through modesSendAsterixOutput.  -> (the bytes written, the length written per record)"""
    n = len(c["msgs"])
    rec = np.zeros(n, dtype=HARNESS_CASE)
    rec["sysTimestamp"], rec["fields"] = c["msgs"]["sysTimestamp"], c["fields"]
    rec["has_pos"] = np.isin(c["positions"]["method"], POS_METHODS)
    rec["lat"], rec["lon"] = c["positions"]["lat"], c["positions"]["lon"]
    rec["id"], rec["ac_baro_alt"], rec["ac_category"] = c["ids"], c["ac_baro_alt"], c["ac_category"]
    path = os.path.join(workdir, "asterix_cases.bin")
    rec.tofile(path)
    r = subprocess.run([exe, path, str(int(now_ms)), str(int(remote))], check=True, capture_output=True)
    lens = np.frombuffer(r.stdout[: 4 * n], dtype=np.int32)
    return r.stdout[4 * n:], lens
