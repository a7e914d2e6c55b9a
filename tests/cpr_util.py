"""Position decode (kernels/cpr.inc, include/modes_gpu.h: mgpu_cpr_*): a float64 numpy restatement of cpr.c's three decoders, a CPR
encoder (DO-260B / ICAO 9871 §A.2.6, the inverse of the decoders), the cases of tests/golden/cpr_cases.npz, position frames for the
walk's tests and a message-by-message restatement of the pairing rules the header states."""
import os
import subprocess

import numpy as np

import fields_util as fu
import helpers
from readsb_amd.binding import CPR_CASE_DTYPE, CPR_RESULT_DTYPE, FIELDS_DTYPE, MSG_DTYPE, POSITION_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(helpers.GOLDEN_DIR, "cpr_cases.npz")
REF_OBJECT = os.path.join(ROOT, "oracle", "_ref", "full", "cpr.o")
HARNESS_SRC = os.path.join(ROOT, "tests", "host_stub", "cpr_ref_harness.c")

# the NL table of 1090-WP-9-14 as cpr.c:84-144 writes it: NL = 59 - (thresholds <= |lat|)
NL_THRESHOLDS = np.array([
    10.47047130, 14.82817437, 18.18626357, 21.02939493, 23.54504487, 25.82924707, 27.93898710, 29.91135686, 31.77209708, 33.53993436,
    35.22899598, 36.85025108, 38.41241892, 39.92256684, 41.38651832, 42.80914012, 44.19454951, 45.54626723, 46.86733252, 48.16039128,
    49.42776439, 50.67150166, 51.89342469, 53.09516153, 54.27817472, 55.44378444, 56.59318756, 57.72747354, 58.84763776, 59.95459277,
    61.04917774, 62.13216659, 63.20427479, 64.26616523, 65.31845310, 66.36171008, 67.39646774, 68.42322022, 69.44242631, 70.45451075,
    71.45986473, 72.45884545, 73.45177442, 74.43893416, 75.42056257, 76.39684391, 77.36789461, 78.33374083, 79.29428225, 80.24923213,
    81.19801349, 82.13956981, 83.07199445, 83.99173563, 84.89166191, 85.75541621, 86.53536998, 87.00000000])
assert len(NL_THRESHOLDS) == 58

NONE, GLOBAL, LOCAL_RECEIVER, LOCAL_AIRCRAFT, BAD = 0, 1, 2, 3, 4
NOT_TRIED = 1
PARTNER_NONE, PARTNER_EARLIER = 0xFFFFFFFF, 0xFFFFFFFE
CPR_SURFACE, CPR_AIRBORNE = 1, 2
F_GS_VALID, F_CPR_VALID, F_CPR_ODD = 1 << 3, 1 << 10, 1 << 11
LOCAL_TTL_MS = 10 * 60 * 1000


# ---- cpr.c restated: np.floor, np.fmod, plain division, float64, the reference's order of operations ----
def nl(lat):
    return 59 - np.searchsorted(NL_THRESHOLDS, np.abs(lat), side="right")


def _n(lat, fflag):
    return np.maximum(nl(lat) - fflag, 1)


def _dlon(lat, fflag, surface):
    return np.where(surface, 90.0, 360.0) / _n(lat, fflag)


def _mod_double(a, b):
    r = np.fmod(a, b)
    return np.where(r < 0, r + b, r)


def _global(surface, reflat, reflon, even_lat, even_lon, odd_lat, odd_lon, fflag):
    """decodeCPRairborne (surface False) / decodeCPRsurface (True), cpr.c:170-319 -> (rc, lat, lon)"""
    span = 90.0 if surface else 360.0
    dlat0, dlat1 = span / 60.0, span / 59.0
    lat0, lon0, lat1, lon1 = (np.asarray(x, dtype=np.float64) for x in (even_lat, even_lon, odd_lat, odd_lon))
    j = np.floor(((59 * lat0 - 60 * lat1) / 131072) + 0.5).astype(np.int64)
    rlat0 = dlat0 * (np.mod(j, 60) + lat0 / 131072)
    rlat1 = dlat1 * (np.mod(j, 59) + lat1 / 131072)
    if surface:
        def quadrant(r):
            at_zero = np.where(reflat < -45, -90.0, np.where(reflat > 45, 90.0, r))
            return np.where(r == 0, at_zero, np.where((r - reflat) > 45, r - 90, r))
        rlat0, rlat1 = quadrant(rlat0), quadrant(rlat1)
    else:
        rlat0 = np.where(rlat0 >= 270, rlat0 - 360, rlat0)
        rlat1 = np.where(rlat1 >= 270, rlat1 - 360, rlat1)
    bad = (rlat0 < -90) | (rlat0 > 90) | (rlat1 < -90) | (rlat1 > 90)
    crossed = nl(rlat0) != nl(rlat1)
    odd = np.asarray(fflag) != 0
    rlat = np.where(odd, rlat1, rlat0)
    nlr = nl(rlat)
    ni = _n(rlat, odd.astype(np.int64))
    m = np.floor((((lon0 * (nlr - 1)) - (lon1 * nlr)) / 131072) + 0.5).astype(np.int64)
    rlon = _dlon(rlat, odd.astype(np.int64), surface) * (np.mod(m, ni) + np.where(odd, lon1, lon0) / 131072)
    if surface:
        rlon = rlon + np.floor((reflon - rlon + 45) / 90) * 90
    rlon = rlon - np.floor((rlon + 180) / 360) * 360
    rc = np.where(bad, -2, np.where(crossed, -1, 0))
    return rc, np.where(rc == 0, rlat, 0.0), np.where(rc == 0, rlon, 0.0)


def _relative(reflat, reflon, cprlat, cprlon, fflag, surface):
    """decodeCPRrelative, cpr.c:331-374 -> (rc, lat, lon)"""
    flat = np.asarray(cprlat, dtype=np.float64) / 131072.0
    flon = np.asarray(cprlon, dtype=np.float64) / 131072.0
    odd, surface = np.asarray(fflag) != 0, np.asarray(surface) != 0
    dlat = np.where(surface, 90.0, 360.0) / np.where(odd, 59.0, 60.0)
    j = (np.floor(reflat / dlat) + np.floor(0.5 + _mod_double(reflat, dlat) / dlat - flat)).astype(np.int64)
    rlat = dlat * (j + flat)
    rlat = np.where(rlat >= 270, rlat - 360, rlat)
    fail = (rlat < -90) | (rlat > 90) | (np.abs(rlat - reflat) > (dlat / 2))
    rlat_safe = np.where(fail, 0.0, rlat)
    dlon = _dlon(rlat_safe, odd.astype(np.int64), surface)
    m = (np.floor(reflon / dlon) + np.floor(0.5 + _mod_double(reflon, dlon) / dlon - flon)).astype(np.int64)
    rlon = dlon * (m + flon)
    rlon = np.where(rlon > 180, rlon - 360, rlon)
    fail = fail | (np.abs(rlon - reflon) > (dlon / 2))
    rc = np.where(fail, -1, 0)
    return rc, np.where(fail, 0.0, rlat), np.where(fail, 0.0, rlon)


def decode_cases(cases):
    """struct mgpu_cpr_case records -> struct mgpu_cpr_result records, as mgpu_cpr_decode defines them."""
    cases = np.asarray(cases, dtype=CPR_CASE_DTYPE)
    out = np.zeros(len(cases), dtype=CPR_RESULT_DTYPE)
    with np.errstate(all="ignore"):
        for fn in (0, 1, 2):
            sel = np.nonzero(cases["fn"] == fn)[0]
            if not len(sel):
                continue
            c = cases[sel]
            if fn == 2:
                rc, lat, lon = _relative(c["reflat"], c["reflon"], c["even_lat"], c["even_lon"], c["fflag"], c["surface"])
            else:
                rc, lat, lon = _global(fn == 1, c["reflat"], c["reflon"], c["even_lat"], c["even_lon"], c["odd_lat"], c["odd_lon"], c["fflag"])
            out["rc"][sel], out["lat"][sel], out["lon"][sel] = rc, lat, lon
    return out


# ---- the encoder ----
def encode(lat, lon, odd, surface):
    """True position -> the 17-bit words (YZ, XZ) an aircraft transmits.  Surface positions are encoded with 19 bits over 360 degrees,
    of which the low 17 are sent: the same as 17 bits over 90 degrees."""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    odd, surface = np.asarray(odd).astype(np.int64), np.asarray(surface) != 0
    span = np.where(surface, 90.0, 360.0)
    dlat = span / (60 - odd)
    yz = np.floor(131072 * (np.mod(lat, dlat) / dlat) + 0.5)
    rlat = dlat * (yz / 131072 + np.floor(lat / dlat))
    dlon = span / np.maximum(nl(rlat) - odd, 1)
    xz = np.floor(131072 * (np.mod(lon, dlon) / dlon) + 0.5)
    return yz.astype(np.int64) & 0x1FFFF, xz.astype(np.int64) & 0x1FFFF


def move(lat, lon, km, bearing):
    """`km` along `bearing` (radians) on a flat patch: good enough to put a second fix a few kilometres on."""
    lat2 = np.clip(lat + km * np.cos(bearing) / 111.2, -90.0, 90.0)
    lon2 = lon + km * np.sin(bearing) / (111.2 * np.maximum(np.cos(np.radians(lat)), 0.01))
    return lat2, (lon2 + 180.0) % 360.0 - 180.0


# ---- the golden's cases ----
def _cases(fn, reflat, reflon, even, odd, fflag, surface):
    n = len(np.atleast_1d(fflag))
    c = np.zeros(n, dtype=CPR_CASE_DTYPE)
    c["fn"], c["reflat"], c["reflon"], c["fflag"], c["surface"] = fn, reflat, reflon, fflag, surface
    c["even_lat"], c["even_lon"] = even
    c["odd_lat"], c["odd_lon"] = odd
    return c


def _pair_cases(lat, lon, lat2, lon2, surface, reflat=0.0, reflon=0.0):
    """even word of (lat, lon), odd word of (lat2, lon2) — and the other way round — decoded with both fflags"""
    out = []
    for first_odd in (0, 1):
        la_e, lo_e = (lat, lon) if not first_odd else (lat2, lon2)
        la_o, lo_o = (lat2, lon2) if not first_odd else (lat, lon)
        ev, od = encode(la_e, lo_e, 0, surface), encode(la_o, lo_o, 1, surface)
        for fflag in (0, 1):
            out.append(_cases(1 if surface else 0, reflat, reflon, ev, od, np.full(len(lat), fflag), 0))
    return out


def golden_cases():
    """The cases of tests/golden/cpr_cases.npz (deterministic): see tests/golden/make_cpr_golden.py for what they cover."""
    rng = np.random.default_rng(20241018)
    parts = []
    # (a) every NL threshold, latitudes just below and just above it, both hemispheres, both parities; airborne, surface, relative
    t = np.repeat(NL_THRESHOLDS, 6)
    delta = np.tile(np.array([-1e-3, -1e-4, -3e-5, 3e-5, 1e-4, 1e-3]), 58)
    for sign in (1.0, -1.0):
        lat = sign * (t + delta)
        lon = rng.uniform(-180, 180, size=len(lat))
        lat2, lon2 = move(lat, lon, rng.uniform(0, 0.05, size=len(lat)), rng.uniform(0, 2 * np.pi, size=len(lat)))
        parts += _pair_cases(lat, lon, lat2, lon2, False)[:2]
        parts += _pair_cases(lat, lon, lat2, lon2, True, reflat=lat + rng.uniform(-0.3, 0.3, size=len(lat)), reflon=lon + rng.uniform(-0.3, 0.3, size=len(lat)))[2:]
        for surface in (0, 1):
            odd = rng.integers(0, 2, size=len(lat))
            parts.append(_cases(2, lat2 + rng.uniform(-0.2, 0.2, size=len(lat)), lon2 + rng.uniform(-0.2, 0.2, size=len(lat)),
                                encode(lat, lon, odd, surface), (0, 0), odd, surface))
    # (b) pairs from true positions, the second fix 0-3 km on: everywhere, and the poles, the equator, +-180
    n = 700
    lat = np.degrees(np.arcsin(rng.uniform(-1, 1, size=n)))
    lon = rng.uniform(-180, 180, size=n)
    special_lat = np.array([90.0, -90.0, 89.9999, -89.9999, 87.0, -87.0, 86.99999, 0.0, 1e-7, -1e-7, 0.0, 0.0, 45.0, -45.0, 30.0, 60.0, 44.2, 0.0, 51.5, -33.9])
    special_lon = np.array([0.0, 10.0, -120.0, 77.0, 179.99999, -180.0, 0.0, 0.0, 180.0, -180.0, 179.9999, -179.9999, 90.0, -90.0, 0.0, 1e-7, -1e-7, -0.0001, 180.0, -180.0])
    lat, lon = np.concatenate([lat, np.repeat(special_lat, 5)]), np.concatenate([lon, np.repeat(special_lon, 5)])
    lat2, lon2 = move(lat, lon, rng.uniform(0, 3, size=len(lat)), rng.uniform(0, 2 * np.pi, size=len(lat)))
    parts += _pair_cases(lat, lon, lat2, lon2, False)
    rl, ro = move(lat, lon, rng.uniform(0, 60, size=len(lat)), rng.uniform(0, 2 * np.pi, size=len(lat)))
    parts += _pair_cases(lat, lon, lat2, lon2, True, reflat=rl, reflon=ro)
    # (c) surface: the reference in each of the four longitude quadrants, and at reflat +-45 (and a hair beside it)
    n = 150
    lat, lon = rng.uniform(-89, 89, size=n), rng.uniform(-180, 180, size=n)
    lat2, lon2 = move(lat, lon, rng.uniform(0, 1, size=n), rng.uniform(0, 2 * np.pi, size=n))
    for q in (0.0, 90.0, 180.0, -90.0):
        parts += _pair_cases(lat, lon, lat2, lon2, True, reflat=lat, reflon=(lon + q + rng.uniform(-40, 40, size=n) + 180.0) % 360.0 - 180.0)[::3]
    for reflat in (45.0, -45.0, 45.0 + 1e-9, -45.0 - 1e-9, 44.999, -44.999):
        la = np.concatenate([rng.uniform(-89, 89, size=60), np.zeros(5), np.full(5, 90.0), np.full(5, -90.0), reflat + 45 + rng.uniform(-1e-3, 1e-3, size=15)])
        la = np.clip(la, -90, 90)
        lo = rng.uniform(-180, 180, size=len(la))
        la2, lo2 = move(la, lo, rng.uniform(0, 0.5, size=len(la)), rng.uniform(0, 2 * np.pi, size=len(la)))
        parts += _pair_cases(la, lo, la2, lo2, True, reflat=reflat, reflon=lo + rng.uniform(-30, 30, size=len(la)))[1:3]
    # (d) relative: the reference 0.49 and 0.51 of a cell from the truth, in latitude and in longitude; and plainly near
    n = 130
    for surface in (0, 1):
        span = 90.0 if surface else 360.0
        for odd in (0, 1):
            lat, lon = rng.uniform(-88, 88, size=n), rng.uniform(-179, 179, size=n)
            word = encode(lat, lon, np.full(n, odd), surface)
            dlat = span / (60 - odd)
            dlon = span / np.maximum(nl(lat) - odd, 1)
            for frac in (0.49, 0.51, -0.49, -0.51):
                parts.append(_cases(2, lat + frac * dlat, lon, word, (0, 0), np.full(n, odd), surface))
                parts.append(_cases(2, lat, lon + frac * dlon, word, (0, 0), np.full(n, odd), surface))
            parts.append(_cases(2, lat + rng.uniform(-0.3, 0.3, size=n) * dlat, lon + rng.uniform(-0.3, 0.3, size=n) * dlon, word, (0, 0), np.full(n, odd), surface))
    # (e) uniformly random words (and references): the failing codes.  A relative decode always finds a position within half a cell
    # of its reference unless that lies beyond a pole: references within half a cell of one
    n = 400
    parts.append(_cases(2, rng.choice([-1.0, 1.0], size=n) * rng.uniform(87, 90, size=n), rng.uniform(-180, 180, size=n),
                        (rng.integers(0, 131072, size=n), rng.integers(0, 131072, size=n)), (0, 0), rng.integers(0, 2, size=n), 0))
    for fn, n in ((0, 500), (1, 700), (2, 300)):
        words = rng.integers(0, 131072, size=(4, n))
        parts.append(_cases(fn, rng.uniform(-90, 90, size=n), rng.uniform(-180, 180, size=n), (words[0], words[1]), (words[2], words[3]),
                            rng.integers(0, 2, size=n), rng.integers(0, 2, size=n) if fn == 2 else 0))
    cases = np.concatenate(parts)
    cases["reflat"][cases["fn"] == 0] = 0                 # the fields a function does not read stay zero
    cases["reflon"][cases["fn"] == 0] = 0
    return cases


def ref_available():
    from shutil import which
    return os.path.exists(REF_OBJECT) and which("gcc") is not None


def run_ref_harness(cases, workdir):
    """The REFERENCE's decoders (oracle/_ref/full/cpr.o behind tests/host_stub/cpr_ref_harness.c) on the cases."""
    exe = os.path.join(workdir, "cpr_ref_harness")
    subprocess.run(["gcc", "-O2", "-std=c11", "-no-pie", "-o", exe, HARNESS_SRC, REF_OBJECT, "-lm"], check=True)
    fin, fout = os.path.join(workdir, "cases.bin"), os.path.join(workdir, "results.bin")
    np.ascontiguousarray(cases, dtype=CPR_CASE_DTYPE).tofile(fin)
    subprocess.run([exe, fin, fout], check=True)
    out = np.fromfile(fout, dtype=CPR_RESULT_DTYPE)
    assert len(out) == len(cases)
    return out


def load_golden():
    z = np.load(GOLDEN)
    cases = np.frombuffer(z["cases"].tobytes(), dtype=CPR_CASE_DTYPE)
    results = np.zeros(len(cases), dtype=CPR_RESULT_DTYPE)
    results["lat"], results["lon"], results["rc"] = z["lat_bits"].view(np.float64), z["lon_bits"].view(np.float64), z["rc"]
    return cases, results


def assert_same_results(got, want, what=""):
    assert len(got) == len(want)
    bad = np.nonzero((got["rc"] != want["rc"]) | (got["lat"].view(np.uint64) != want["lat"].view(np.uint64)) |
                     (got["lon"].view(np.uint64) != want["lon"].view(np.uint64)))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} cases differ, first {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}"


# ---- position frames and message lists for the walk ----
def position_frames(addr, lat_w, lon_w, odd, surface, df=17, low3=5, movement=0):
    """DF17 / DF18 position squitters: airborne ME type 11 with an altitude, surface ME type 6 with `movement` (0: no speed,
    1: stopped, 100: 78 kt).  low3 = CA (DF17) or CF (DF18).  Parity sealed."""
    addr, lat_w, lon_w, odd, surface, df, low3, movement = (np.atleast_1d(np.asarray(x)).astype(np.uint64) for x in
                                                            np.broadcast_arrays(addr, lat_w, lon_w, odd, surface, df, low3, movement))
    u = np.uint64
    air = (u(11) << u(51)) | (u(0x5D5) << u(36))
    sfc = (u(6) << u(51)) | (movement << u(44))
    me = np.where(surface != 0, sfc, air) | (odd << u(34)) | (lat_w << u(17)) | lon_w
    fr = np.zeros((len(me), 14), dtype=np.uint8)
    fr[:, 0] = (df << u(3)) | low3
    fr[:, 1], fr[:, 2], fr[:, 3] = (addr >> u(16)) & u(0xFF), (addr >> u(8)) & u(0xFF), addr & u(0xFF)
    for k in range(7):
        fr[:, 4 + k] = (me >> u(8 * (6 - k))) & u(0xFF)
    return fu.seal(fr)


def ident_frames(addr):
    """DF17 identification squitters (ME type 4): an aircraft's messages that carry no position."""
    addr = np.atleast_1d(np.asarray(addr)).astype(np.uint64)
    fr = np.zeros((len(addr), 14), dtype=np.uint8)
    fr[:, 0] = (17 << 3) | 5
    fr[:, 1], fr[:, 2], fr[:, 3] = (addr >> np.uint64(16)) & np.uint64(0xFF), (addr >> np.uint64(8)) & np.uint64(0xFF), addr & np.uint64(0xFF)
    fr[:, 4:11] = (0x20, 0x04, 0x20, 0xF1, 0xCB, 0x38, 0x20)
    return fu.seal(fr)


def message_list(frames, t_ms, modeac=None):
    """Message records (what the gate's and the encoder's tests hand to the library) of sealed frames at sysTimestamp t_ms;
    modeac: a mask of entries that become Mode A/C replies instead."""
    n = len(frames)
    msgs = np.zeros(n, dtype=MSG_DTYPE)
    t_ms = np.asarray(t_ms, dtype=np.int64)
    msgs["sysTimestamp"] = t_ms
    msgs["timestamp"] = 772 + (t_ms - t_ms.min()) * 12000 + np.arange(n)
    msgs["msg"] = frames
    msgs["raw"] = frames
    df = frames[:, 0] >> 3
    msgs["msgtype"] = df
    msgs["msgbits"] = np.where(df >= 16, 112, 56)
    msgs["addr"] = (frames[:, 1].astype(np.uint32) << 16) | (frames[:, 2].astype(np.uint32) << 8) | frames[:, 3]
    if modeac is not None:
        msgs["msgtype"][modeac], msgs["msgbits"][modeac], msgs["addr"][modeac] = 77, 16, 0
        msgs["msg"][modeac, 2:] = 0
    return msgs


# ---- the pairing rules (include/modes_gpu.h, mgpu_cpr_track), message by message ----
class CprModel:
    """Rules 1-4 over message lists, the state kept from call to call like the library's table.  Two numpy calls per list: every
    global decode, then every local decode (a local decode reads global results only)."""

    def __init__(self, ref_lat=0.0, ref_lon=0.0, ref_valid=0, airborne_max_elapsed_ms=0):
        self.ref_lat, self.ref_lon, self.ref_valid = float(ref_lat), float(ref_lon), int(ref_valid)
        self.air_max = int(airborne_max_elapsed_ms) or 10000
        self.slots = {}       # (addr, odd) -> (lat word, lon word, cpr_type, source, t, index in the current call | PARTNER_EARLIER)
        self.ref = {}         # addr -> (lat, lon, t) of the last GLOBAL result

    def reset(self):
        self.slots.clear()
        self.ref.clear()

    def track(self, msgs, fields):
        n = len(msgs)
        out = np.zeros(n, dtype=POSITION_DTYPE)
        is_pos = ((fields["flags"] & F_CPR_VALID) != 0) & ((msgs["msgtype"] == 17) | (msgs["msgtype"] == 18))
        pos = np.nonzero(is_pos)[0]
        for key in list(self.slots):
            self.slots[key] = self.slots[key][:5] + (PARTNER_EARLIER,)
        tried = []            # (message, case)
        for i in pos:
            f = fields[i]
            addr, odd = int(f["addr"]) & 0x1FFFFFF, 1 if f["flags"] & F_CPR_ODD else 0
            now, surface = int(msgs["sysTimestamp"][i]), int(f["cpr_type"]) == CPR_SURFACE
            me = (int(f["cpr_lat"]), int(f["cpr_lon"]), int(f["cpr_type"]) & 3, int(f["source"]), now, int(i))
            self.slots[(addr, odd)] = me
            out["flags"][i] = odd | (2 if surface else 0)
            out["partner"][i], out["global_result"][i], out["local_result"][i] = PARTNER_NONE, NOT_TRIED, NOT_TRIED
            if surface:
                max_elapsed = 50000 if (f["flags"] & F_GS_VALID) and f["gs_selected"] <= 25 else 25000
            else:
                max_elapsed = self.air_max
            other = self.slots.get((addr, 1 - odd))
            if other is None or other[2] != me[2] or other[3] != me[3] or abs(now - other[4]) > max_elapsed:
                continue
            out["partner"][i], out["partner_dt_ms"][i] = other[5], now - other[4]
            even, od = (other, me) if odd else (me, other)
            c = np.zeros(1, dtype=CPR_CASE_DTYPE)
            c["fn"], c["fflag"], c["reflat"], c["reflon"] = (1 if surface else 0), odd, self.ref_lat, self.ref_lon
            c["even_lat"], c["even_lon"], c["odd_lat"], c["odd_lon"] = even[0], even[1], od[0], od[1]
            tried.append((i, c[0]))
        if tried:
            res = decode_cases(np.array([c for _, c in tried], dtype=CPR_CASE_DTYPE))
            for (i, c), r in zip(tried, res):
                rc = int(r["rc"]) if (c["fn"] == 0 or self.ref_valid) else -1
                out["global_result"][i] = rc
                if rc == 0:
                    out["method"][i], out["lat"][i], out["lon"][i] = GLOBAL, r["lat"], r["lon"]
                elif rc == -2:
                    out["method"][i] = BAD
        local = []
        for i in pos:
            addr = int(fields["addr"][i]) & 0x1FFFFFF
            now = int(msgs["sysTimestamp"][i])
            if out["method"][i] == GLOBAL:
                self.ref[addr] = (float(out["lat"][i]), float(out["lon"][i]), now)
            if out["method"][i] != NONE:
                continue
            surface = int(out["flags"][i]) & 2
            g = self.ref.get(addr)
            if g is not None and now < g[2] + LOCAL_TTL_MS:
                how, rlat, rlon = LOCAL_AIRCRAFT, g[0], g[1]
            elif not surface and self.ref_valid:
                how, rlat, rlon = LOCAL_RECEIVER, self.ref_lat, self.ref_lon
            else:
                continue
            c = np.zeros(1, dtype=CPR_CASE_DTYPE)
            c["fn"], c["fflag"], c["surface"], c["reflat"], c["reflon"] = 2, int(out["flags"][i]) & 1, 1 if surface else 0, rlat, rlon
            c["even_lat"], c["even_lon"] = fields["cpr_lat"][i], fields["cpr_lon"][i]
            local.append((i, how, c[0]))
        if local:
            res = decode_cases(np.array([c for _, _, c in local], dtype=CPR_CASE_DTYPE))
            for (i, how, _), r in zip(local, res):
                out["local_result"][i] = r["rc"]
                if r["rc"] == 0:
                    out["method"][i], out["lat"][i], out["lon"][i] = how, r["lat"], r["lon"]
        return out


def assert_same_positions(got, want, what=""):
    assert got.dtype == POSITION_DTYPE and len(got) == len(want)
    g, w = got.view(np.uint8).reshape(len(got), -1), want.view(np.uint8).reshape(len(want), -1)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} records differ, first at {bad[:5]}:\n got {got[bad[:5]]}\nwant {want[bad[:5]]}"
