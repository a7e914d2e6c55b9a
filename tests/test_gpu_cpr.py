"""-m gpu: position decode on the device (kernels/cpr.inc; include/modes_gpu.h: mgpu_cpr_decode, mgpu_cpr_track).
The decoders against tests/golden/cpr_cases.npz (what the reference's own cpr.o returns): result codes equal, latitudes and longitudes
equal as bit patterns.  The pairing against tests/cpr_util.py's message-by-message restatement of the rules the header states, whole
records byte for byte, over lists of sealed DF17 / DF18 position frames run through mgpu_decode_fields — at the shapes at which a walk
of 64 messages per step can go wrong."""
import ctypes as C

import numpy as np
import pytest

import cpr_util as cu

pytestmark = pytest.mark.gpu

REF = (52.0, 4.5)                 # the receiver
A0 = 0x484000


@pytest.fixture(scope="module")
def dev(built):
    import helpers
    import readsb_amd
    d = readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=1 << 20)
    yield d
    d.close()


class ListBuilder:
    """Rows in any order -> a message list in time order (stable)."""

    def __init__(self):
        self.rows = []        # (t_ms, kind 0 position / 1 identification / 2 Mode A/C, addr, lat, lon, odd, surface, df, low3, movement, words or None)

    def pos(self, t, addr, lat, lon, odd, surface=0, df=17, low3=5, movement=0, words=None):
        self.rows.append((int(t), 0, addr, lat, lon, int(odd), int(surface), df, low3, movement, words))

    def ident(self, t, addr):
        self.rows.append((int(t), 1, addr, 0.0, 0.0, 0, 0, 17, 5, 0, None))

    def modeac(self, t):
        self.rows.append((int(t), 2, 0, 0.0, 0.0, 0, 0, 0, 0, 0, None))

    def flight(self, addr, t0, n, lat=52.3, lon=4.8, period=500, surface=0, first_odd=0, step_km=0.1, bearing=1.0, **kw):
        for k in range(n):
            la, lo = cu.move(lat, lon, step_km * k, bearing)
            self.pos(t0 + k * period, addr, float(la), float(lo), (k + first_odd) & 1, surface, **kw)

    def build(self):
        rows = sorted(self.rows, key=lambda r: r[0])
        n = len(rows)
        col = lambda k, dt: np.array([r[k] for r in rows], dtype=dt)
        t, kind, addr = col(0, np.int64), col(1, np.int64), col(2, np.uint64)
        odd, surface = col(5, np.int64), col(6, np.int64)
        yz, xz = cu.encode(col(3, np.float64), col(4, np.float64), odd, surface)
        for k, r in enumerate(rows):
            if r[10] is not None:
                yz[k], xz[k] = r[10]
        frames = cu.position_frames(addr, yz, xz, odd, surface, col(7, np.uint64), col(8, np.uint64), col(9, np.uint64))
        if (kind == 1).any():
            frames[kind == 1] = cu.ident_frames(addr[kind == 1])
        import helpers
        return cu.message_list(frames, helpers.STARTUP_MS + t, modeac=(kind == 2) if (kind == 2).any() else None)


def model_for(ref, air_max=0):
    return cu.CprModel(*(ref if ref else (0.0, 0.0)), 1 if ref else 0, air_max)


def run_and_check(dev, msgs, ref=REF, air_max=0, what=""):
    """One call on a fresh table against the restatement; returns (records, field records)."""
    fields = dev.decode_fields(msgs)
    want = model_for(ref, air_max).track(msgs, fields)
    dev.cpr_reset()
    got = dev.cpr_track(msgs, ref=ref, airborne_max_elapsed_ms=air_max)
    cu.assert_same_positions(got, want, what)
    return got, fields


# ---- the decoders ----
def test_decoders_equal_the_reference_on_every_golden_case(dev):
    cases, want = cu.load_golden()
    cu.assert_same_results(dev.cpr_decode(cases), want, "mgpu_cpr_decode against the golden")
    for n in (0, 1, 63, 64, 65):
        cu.assert_same_results(dev.cpr_decode(cases[5000:5000 + n]), want[5000:5000 + n], f"n = {n}")


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


class DeviceArrays:
    def __init__(self, *sizes):
        self.hip, self.ptrs = _hip(), []
        for s in sizes:
            p = C.c_void_p()
            assert self.hip.hipMalloc(C.byref(p), max(int(s), 16)) == 0
            self.ptrs.append(p)

    def put(self, k, arr):
        assert self.hip.hipMemcpy(self.ptrs[k], arr.ctypes.data, arr.nbytes, 1) == 0

    def get(self, k, n, dtype):
        out = np.empty(n, dtype=dtype)
        assert self.hip.hipMemcpy(out.ctypes.data, self.ptrs[k], out.nbytes, 2) == 0
        return out

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)


def test_device_forms_equal_the_host_forms(dev):
    import readsb_amd
    cases, want = cu.load_golden()
    cases = np.ascontiguousarray(cases[:3001])
    b = ListBuilder()
    for a in range(40):
        b.flight(A0 + a, 100 * a, 9 + a % 5, lat=51.0 + 0.05 * a, surface=a % 3 == 0, movement=1)
    msgs = np.ascontiguousarray(b.build())
    n = len(msgs)
    host, fields = run_and_check(dev, msgs)
    mem = DeviceArrays(cases.nbytes, len(cases) * 24, msgs.nbytes, n * readsb_amd.FIELDS_DTYPE.itemsize, n * 32)
    try:
        mem.put(0, cases)
        dev.cpr_decode_device(mem.ptrs[0].value, len(cases), mem.ptrs[1].value)
        cu.assert_same_results(mem.get(1, len(cases), cu.CPR_RESULT_DTYPE), want[:3001], "mgpu_cpr_decode_device")
        mem.put(2, msgs)
        dev.decode_fields_device(mem.ptrs[2].value, n, mem.ptrs[3].value)
        dev.cpr_reset()
        dev.cpr_track_device(mem.ptrs[2].value, mem.ptrs[3].value, n, mem.ptrs[4].value, ref=REF)
        cu.assert_same_positions(mem.get(4, n, cu.POSITION_DTYPE), host, "mgpu_cpr_track_device")
    finally:
        mem.free()


def test_arguments(dev):
    from readsb_amd.binding import CprConfig
    b = ListBuilder()
    b.flight(A0, 0, 4)
    msgs = np.ascontiguousarray(b.build())
    out = np.zeros(len(msgs), dtype=cu.POSITION_DTYPE)
    lib, ctx = dev.lib, dev.ctx
    ok = CprConfig(52.0, 4.0, 1, 0)
    assert lib.mgpu_cpr_track(ctx, C.byref(ok), None, 0, None) == 0                                  # n == 0 is MGPU_OK
    assert lib.mgpu_cpr_track_device(ctx, C.byref(ok), None, None, 0, None) == 0
    assert lib.mgpu_cpr_decode(ctx, None, 0, None) == 0
    assert lib.mgpu_cpr_track(ctx, None, C.c_void_p(msgs.ctypes.data), len(msgs), C.c_void_p(out.ctypes.data)) == -1     # MGPU_E_INVAL
    for bad in (CprConfig(float("nan"), 4.0, 1, 0), CprConfig(52.0, float("inf"), 0, 0)):
        assert lib.mgpu_cpr_track(ctx, C.byref(bad), C.c_void_p(msgs.ctypes.data), len(msgs), C.c_void_p(out.ctypes.data)) == -1
    assert len(dev.cpr_track(msgs[:0])) == 0


# ---- the walk ----
@pytest.mark.parametrize("ref", [REF, None])
def test_runs_of_one_address(dev, ref):
    """1, 2, 64, 65, 128 and 129 position messages of one address: alone in a call, and all six addresses interleaved in one."""
    lengths = (1, 2, 64, 65, 128, 129)
    both = ListBuilder()
    for k, n in enumerate(lengths):
        b = ListBuilder()
        b.flight(A0 + k, 0, n, first_odd=k & 1)
        both.flight(A0 + k, 7 * k, n, first_odd=k & 1)
        got, _ = run_and_check(dev, b.build(), ref=ref, what=f"run of {n}")
        assert (got["method"] == cu.GLOBAL).sum() == n - 1                      # every message but the first has its partner right before it
        assert got["method"][0] == (cu.LOCAL_RECEIVER if ref else cu.NONE)
        assert np.array_equal(got["partner"][1:], np.arange(n - 1, dtype=np.uint32))
    got, _ = run_and_check(dev, both.build(), ref=ref, what="six runs interleaved")
    assert (got["method"] == cu.GLOBAL).sum() == sum(lengths) - len(lengths)


def test_partner_in_the_previous_step_and_far_below(dev):
    """63 odd messages, one even, 66 odd: the even message is lane 63 of the first step, the partner of every message of the second
    and third step.  The airborne window is opened to 60 s so that all of them pair."""
    b = ListBuilder()
    for k in range(130):
        la, lo = cu.move(52.3, 4.8, 0.05 * k, 2.0)
        b.pos(300 * k, A0, float(la), float(lo), 0 if k == 63 else 1)
    got, _ = run_and_check(dev, b.build(), air_max=60000, what="one even among odds")
    assert (got["partner"][:63] == cu.PARTNER_NONE).all() and got["partner"][63] == 62
    assert (got["partner"][64:] == 63).all() and (got["method"][64:] == cu.GLOBAL).all()
    assert np.array_equal(got["partner_dt_ms"][64:], 300 * (np.arange(64, 130) - 63))
    # with the default 10 s only the messages up to 33 places behind it pair; the others fall back on the last global result
    got, _ = run_and_check(dev, b.build(), what="one even among odds, 10 s")
    assert (got["method"][64:97] == cu.GLOBAL).all() and (got["method"][97:] == cu.LOCAL_AIRCRAFT).all()
    assert (got["global_result"][97:] == cu.NOT_TRIED).all()


def _random_traffic(n_aircraft, seed, per_aircraft=(2, 24)):
    rng = np.random.default_rng(seed)
    b = ListBuilder()
    for a in range(n_aircraft):
        addr = A0 + 0x100 + a
        n = int(rng.integers(*per_aircraft))
        surface = int(rng.random() < 0.3)
        lat, lon = (REF[0] + rng.uniform(-1.5, 1.5), REF[1] + rng.uniform(-2, 2)) if rng.random() < 0.8 else (rng.uniform(-80, 80), rng.uniform(-180, 180))
        t = np.sort(rng.integers(0, 40000, size=n))
        odd = rng.integers(0, 2, size=n)
        polar = a % 50 == 7                                # near a pole a local decode of a garbled word runs off the globe: result -1
        if polar:                                          # (a pair, then odd messages only, outside the pair's window)
            lat, surface, n = (89.95 if a % 100 == 7 else -89.95), 0, 12
            t, odd = np.array([0, 500] + [11000 + 100 * k for k in range(10)]), np.array([0] + [1] * 11)
        for k in range(n):
            la, lo = cu.move(lat, lon, 0.2 * k, 0.5 + a)
            garbage = (int(rng.integers(0, 131072)), int(rng.integers(0, 131072))) if rng.random() < (0.5 if polar and k >= 2 else 0.06) else None
            b.pos(t[k], addr, float(la), float(lo), odd[k], surface, movement=int(rng.choice([0, 1, 100])), words=garbage)
        if rng.random() < 0.3:
            b.ident(int(rng.integers(0, 40000)), addr)
    for _ in range(n_aircraft // 4):
        b.modeac(int(rng.integers(0, 40000)))
    return b.build()


@pytest.mark.parametrize("ref", [REF, None])
def test_300_aircraft_interleaved(dev, ref):
    msgs = _random_traffic(300, 11)
    got, fields = run_and_check(dev, msgs, ref=ref, what="300 aircraft")
    methods = set(np.unique(got["method"]))
    assert {cu.NONE, cu.GLOBAL, cu.LOCAL_AIRCRAFT, cu.BAD} <= methods and ((cu.LOCAL_RECEIVER in methods) == (ref is not None))
    assert (got["global_result"] == -1).any() and (got["local_result"] == -1).any()
    other = ((fields["flags"] & cu.F_CPR_VALID) == 0)
    assert other.sum() > 50 and not got[other].view(np.uint8).any(), "messages without a position get all-zero records"


def test_one_list_in_one_call_two_calls_and_message_by_message(dev):
    """The table carries the slots and the reference from call to call: the same records however the list is cut — but for
    `partner`, which counts in the call's own list (MGPU_CPR_PARTNER_EARLIER for a message of an earlier call)."""
    msgs = _random_traffic(60, 5, per_aircraft=(2, 14))
    n = len(msgs)
    whole, fields = run_and_check(dev, msgs)

    def in_calls(cuts):
        dev.cpr_reset()
        model, parts = model_for(REF), []
        for a, b in zip(cuts[:-1], cuts[1:]):
            got = dev.cpr_track(msgs[a:b], ref=REF)
            cu.assert_same_positions(got, model.track(msgs[a:b], fields[a:b]), f"call [{a}, {b})")
            got = got.copy()
            own = got["partner"] < cu.PARTNER_EARLIER
            inside = own & ((fields["flags"][a:b] & cu.F_CPR_VALID) != 0)      # (the other messages' records are all zero)
            got["partner"][inside] += a
            parts.append(got)
        return np.concatenate(parts)

    for cuts in ([0, n // 2, n], [0, 1, 2, 3, 64, 65, n - 1, n], list(range(n + 1))):
        cut = in_calls(cuts)
        earlier = cut["partner"] == cu.PARTNER_EARLIER
        assert earlier.any() and (whole["partner"][earlier] < cu.PARTNER_EARLIER).all()
        cut["partner"][earlier] = whole["partner"][earlier]
        cu.assert_same_positions(cut, whole, f"{len(cuts) - 1} calls against one")


@pytest.mark.parametrize("ref", [REF, None])
def test_windows_types_sources_and_addresses(dev, ref):
    b, expect = ListBuilder(), {}
    addr = [A0 + 0x1000]

    def pair(dt, tried, first=None, second=None, t0=1000):
        a = addr[0]
        addr[0] += 1
        first, second = dict(first or {}), dict(second or {})
        a2 = second.pop("addr", a)
        b.pos(t0, a, 52.2, 4.9, 0, **first)
        b.pos(t0 + dt, a2, 52.2, 4.9, 1, **second)
        expect[(a2, t0 + dt)] = tried

    sfc_slow, sfc_fast, sfc_unknown = dict(surface=1, movement=1), dict(surface=1, movement=100), dict(surface=1, movement=0)
    for dt, tried in ((10000, True), (10001, False)):                           # airborne: the 10 s fallback
        pair(dt, tried)
    for kind, limit in ((sfc_slow, 50000), (sfc_fast, 25000), (sfc_unknown, 25000)):
        pair(limit, True, kind, kind)
        pair(limit + 1, False, kind, kind)
    pair(25001, True, sfc_fast, sfc_slow)                                      # the window is the second message's own
    pair(25001, False, sfc_slow, sfc_fast)
    pair(500, False, {}, sfc_slow)                                             # airborne, then surface: types differ
    pair(500, False, {}, dict(df=18, low3=6))                                  # ADS-B, then ADS-R: sources differ
    pair(500, True, dict(df=18, low3=6), dict(df=18, low3=6))
    a = addr[0]
    pair(500, False, {}, dict(df=18, low3=1, addr=a))                          # DF18 CF 1: the same 24 bits as a non-ICAO address
    msgs = b.build()
    got, fields = run_and_check(dev, msgs, ref=ref, what="pairs")
    assert {8, 9, 10} >= set(np.unique(fields["source"])) >= {9, 10} and ((fields["addr"] >> 24) & 1).sum() == 1
    import helpers
    seen = 0
    for k in range(len(msgs)):
        key = (int(msgs["addr"][k]), int(msgs["sysTimestamp"][k]) - helpers.STARTUP_MS)
        if key in expect and fields["flags"][k] & cu.F_CPR_ODD:
            seen += 1
            assert (got["global_result"][k] != cu.NOT_TRIED) == expect[key], f"message {k} {key}: {got[k]}"
            if expect[key]:
                surface = got["flags"][k] & 2
                assert got["method"][k] == (cu.GLOBAL if (ref or not surface) else cu.NONE)
                assert got["global_result"][k] == (0 if (ref or not surface) else -1)
    assert seen == len(expect)
    # the airborne window from the configuration
    for air_max, dt, tried in ((7000, 7000, True), (7000, 7001, False), (30000, 30000, True), (30000, 30001, False)):
        c = ListBuilder()
        c.pos(0, A0, 52.2, 4.9, 1)
        c.pos(dt, A0, 52.2, 4.9, 0)
        got, _ = run_and_check(dev, c.build(), ref=ref, air_max=air_max, what=f"airborne window {air_max}")
        assert (got["global_result"][1] != cu.NOT_TRIED) == tried


@pytest.mark.parametrize("ref", [REF, None])
def test_only_evens_and_the_age_of_the_last_global_result(dev, ref):
    b = ListBuilder()
    b.flight(A0 + 1, 0, 70, period=2000, step_km=0.0)                                                # (alternating: a reference from t = 2 s on)
    for k in range(70):
        b.pos(1000 + 2000 * k, A0 + 2, 52.4, 4.7, 0)                                                  # only evens
    ttl = cu.LOCAL_TTL_MS
    for a, late in ((A0 + 3, ttl - 1), (A0 + 4, ttl)):
        b.pos(0, a, 52.1, 4.6, 0)
        b.pos(1000, a, 52.1, 4.6, 1)                                                                  # GLOBAL at t = 1 s
        b.pos(1000 + late, a, 52.1, 4.6, 1)
    msgs = b.build()
    got, fields = run_and_check(dev, msgs, ref=ref, what="evens / ages")
    evens = fields["addr"] == A0 + 2
    assert (got["global_result"][evens] == cu.NOT_TRIED).all() and (got["partner"][evens] == cu.PARTNER_NONE).all()
    assert (got["method"][evens] == (cu.LOCAL_RECEIVER if ref else cu.NONE)).all()
    last = {a: np.nonzero(fields["addr"] == a)[0][-1] for a in (A0 + 3, A0 + 4)}
    assert got["method"][last[A0 + 3]] == cu.LOCAL_AIRCRAFT and got["global_result"][last[A0 + 3]] == cu.NOT_TRIED
    assert got["method"][last[A0 + 4]] == (cu.LOCAL_RECEIVER if ref else cu.NONE)
    # the same ages across calls: the reference comes out of the table
    dev.cpr_reset()
    model = model_for(ref)
    for part in (msgs[: len(msgs) - 2], msgs[len(msgs) - 2:]):
        f = dev.decode_fields(part)
        cu.assert_same_positions(dev.cpr_track(part, ref=ref), model.track(part, f), "ages, two calls")


def test_other_messages_touch_nothing_and_reset_forgets(dev):
    b = ListBuilder()
    for a in range(30):
        b.flight(A0 + a, 13 * a, 6 + a % 4, period=700, lat=51.5 + 0.03 * a)
    plain = b.build()
    for a in range(30):
        b.ident(13 * a + 350, A0 + a)
        b.ident(13 * a + 1050, A0 + a)
        b.modeac(13 * a + 360)
    mixed = b.build()
    got_plain, _ = run_and_check(dev, plain, what="positions only")
    got_mixed, fields = run_and_check(dev, mixed, what="positions among others")
    is_pos = (fields["flags"] & cu.F_CPR_VALID) != 0
    assert (~is_pos).sum() == 90 and not got_mixed[~is_pos].view(np.uint8).any()
    sub, want = got_mixed[is_pos].copy(), got_plain.copy()
    assert np.array_equal(np.nonzero(is_pos)[0][want["partner"][want["partner"] < cu.PARTNER_EARLIER]], sub["partner"][sub["partner"] < cu.PARTNER_EARLIER])
    sub["partner"], want["partner"] = 0, 0
    cu.assert_same_positions(sub, want, "the position messages' records with and without the others")
    # the same list again without a reset: every first message now has a partner from the call before; after a reset, not
    again = dev.cpr_track(plain, ref=REF)
    assert (again["partner"] == cu.PARTNER_EARLIER).sum() == 30 and not np.array_equal(again, got_plain)
    dev.cpr_reset()
    cu.assert_same_positions(dev.cpr_track(plain, ref=REF), got_plain, "after mgpu_cpr_reset")
