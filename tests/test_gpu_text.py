"""-m gpu: the text outputs on the device (kernels/text.inc, mgpu_sbs_encode_ex* / mgpu_raw_encode_ex*), byte for byte against
tests/sbs_util.py's checker, which tests/test_text_reference.py pins to the reference's own writers on the CPU.  No tolerance anywhere.

Shapes: a workgroup is 256 messages, a wave 64, and nothing else in these kernels depends on the size of the list — so the lists are
0, 1, a wave -1 / exact / +1, a workgroup -1 / exact / +1 and three workgroups + 5 long, with every message, no message and only a
workgroup's last lane having a line; the whole golden case set (every line form, every exact tie of %1.6f and %.0f) in one call; the
output at every alignment with a capacity that is exact, one short and zero, between guard bytes; random bytes as records.
The readsb_gpu_ifile --raw --mlat comparison the raw output could have had is not made: that program prints displayModesMessage's
line (mode_s.c:1834-1847, lower-case payload), which is not the network writer's, and keeps printing it (tests/test_gpu_host_cli.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import beast_util as bu
import helpers
import sbs_util as su

pytestmark = pytest.mark.gpu

GUARD = 256
DEF_GUARD = 16
SIZES = [0, 1, 63, 64, 65, su.BLOCK - 1, su.BLOCK, su.BLOCK + 1, 3 * su.BLOCK + 5]


@pytest.fixture(scope="module")
def ctx(built):
    import readsb_amd
    d = readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=16 * 131072)
    hip = bu.Hip()
    try:
        yield d, hip
    finally:
        hip.free_all()
        d.close()


@functools.lru_cache(maxsize=None)
def _golden():
    return su.load_golden()


@functools.lru_cache(maxsize=None)
def _mixed():
    """Groups (a), (b), (d) and a stretch of (c), shuffled: lines of every form next to each other; and what the checker makes of it."""
    sets = _golden()[0]
    c = su.concat_cases([sets["a"], sets["b"], sets["d"], su.slice_cases(sets["c"], 0, 1500)])
    order = np.random.default_rng(5).permutation(len(c["msgs"]))
    c = {k: v[order] for k, v in c.items()}
    return c, su.sbs_of(c, use_gnss=True)


def _first_diff(got, want):
    if len(got) != len(want):
        return f"{len(got)} bytes, want {len(want)}"
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    k = int(np.nonzero(a != b)[0][0])
    return f"first difference at byte {k} of {len(want)}: got {got[max(k - 60, 0):k + 16]!r} want {want[max(k - 60, 0):k + 16]!r}"


def _same(got, want):
    assert got == want, _first_diff(got, want)


def _same_deferred(got, want):
    assert len(got) == len(want), (len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} of {len(want)} deferred entries differ, first at {bad[:3]}: got {got[bad[:3]]} want {want[bad[:3]]}"


def _sbs_device(d, hip, c, want, k=0, cap=None, deferred_cap=None, use_gnss=True, with_verdict=True, override_squawk=-1):
    """mgpu_sbs_encode_ex_device into guard | k bytes | cap bytes | guard, all 0xA5 before the call, the deferred list before DEF_GUARD
    entries of 0xA5; the C entry itself, so that an error's outputs can be looked at.  want: the checker's result for the same arguments."""
    from readsb_amd.binding import SbsArgs, SBS_USE_GNSS
    wstream, _, wdef, wskip = want
    n, T, D = len(c["msgs"]), len(wstream), len(wdef)
    cap = T if cap is None else cap
    dcap = D if deferred_cap is None else deferred_cap
    total = GUARD + k + max(cap, T) + GUARD
    ptrs = [hip.upload(c[name]) for name in ("msgs", "fields", "positions", "verdict", "geom_delta")]
    d_buf, d_def = hip.malloc(total), hip.malloc((dcap + DEF_GUARD) * bu.DEFERRED.itemsize)
    try:
        hip.fill(d_buf, 0xA5, total)
        hip.fill(d_def, 0xA5, (dcap + DEF_GUARD) * bu.DEFERRED.itemsize)
        nb, nd, ns = C.c_uint64(12345), C.c_uint64(12345), C.c_uint64(12345)
        a = SbsArgs(C.sizeof(SbsArgs), SBS_USE_GNSS if use_gnss else 0, ptrs[0], ptrs[1], ptrs[2], ptrs[3] if with_verdict else None, ptrs[4], n, su.NOW_MS,
                    override_squawk, d_buf + GUARD + k, cap, C.pointer(nb), d_def, dcap, C.pointer(nd), C.pointer(ns))
        rc = int(d.lib.mgpu_sbs_encode_ex_device(d.ctx, C.byref(a)))
        buf = hip.download(d_buf, total)
        got_def = hip.download(d_def, (dcap + DEF_GUARD) * bu.DEFERRED.itemsize, dtype=bu.DEFERRED)
    finally:
        for p in ptrs + [d_buf, d_def]:
            hip.free(p)
    at = GUARD + k
    assert (nb.value, nd.value, ns.value) == (T, D, wskip), (nb.value, nd.value, ns.value, T, D, wskip)
    assert (buf[:at] == 0xA5).all(), f"bytes before the output were written (offset {k})"
    assert (buf[at + min(cap, T):] == 0xA5).all(), f"bytes behind the stream or at / beyond the capacity {cap} were written (offset {k})"
    _same(buf[at:at + min(cap, T)].tobytes(), wstream[:min(cap, T)])          # on overflow too: the prefix below the capacity is the stream's
    listed = min(dcap, D)
    _same_deferred(got_def[:listed], wdef[:listed])
    assert (got_def[listed:].view(np.uint8) == 0xA5).all(), "entries behind the list were written"
    assert rc == (su.MGPU_E_OVERFLOW if cap < T or dcap < D else 0), rc
    return rc


def _sbs_host(d, c, use_gnss=True, **kw):
    return d.sbs_encode(c["msgs"], su.NOW_MS, fields=c["fields"], positions=c["positions"], verdict=c["verdict"], geom_delta=c["geom_delta"],
                        use_gnss=use_gnss, **kw)


def _check_host(d, c, want, use_gnss=True):
    stream, deferred, nskipped = _sbs_host(d, c, use_gnss)
    _same(stream, want[0])
    _same_deferred(deferred, want[2])
    assert nskipped == want[3]


# ---- sizes ----------------------------------------------------------------------------------------------------------------------------

def _lined(n, seed):
    """n records that all have a line, of every form."""
    c, (_, length, _, _) = _mixed()
    idx = np.nonzero(length > 0)[0]
    idx = idx[np.random.default_rng(seed).permutation(len(idx))[:n]]
    assert len(idx) == n
    return {k: v[idx] for k, v in c.items()}


@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, n):
    d, hip = ctx
    every = _lined(n, n)
    none = {k: v.copy() for k, v in every.items()}
    none["verdict"][:] = su.GATE_DROP
    last = {k: v.copy() for k, v in every.items()}
    last["verdict"][:] = su.GATE_FORWARD                                       # forwarded, yet no aircraft: no line
    last["verdict"][su.BLOCK - 1::su.BLOCK] = su.VERDICTS[4]
    for what, c in (("every", every), ("none", none), ("last lane", last)):
        want = su.sbs_of(c, use_gnss=True)
        lines = int((want[1] > 0).sum())
        assert lines == {"every": n, "none": 0, "last lane": n // su.BLOCK}[what]
        _check_host(d, c, want)
        if n:
            _sbs_device(d, hip, c, want, k=n % 4)
    stream, deferred, nskipped = d.sbs_encode(every["msgs"], su.NOW_MS, fields=every["fields"])          # no verdicts, positions or geom_delta
    _same(stream, su.sbs_reference(every["msgs"], every["fields"], su.NOW_MS)[0])
    assert len(deferred) == 0


# ---- the golden cases ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_gnss", [False, True])
def test_golden_cases_in_one_call(ctx, use_gnss):
    d, _ = ctx
    sets = _golden()[0]
    c = su.concat_cases([sets[g] for g in su.GROUPS])
    want = su.sbs_of(c, use_gnss=use_gnss)
    assert len(c["msgs"]) > 40000 and want[3] == 26 and len(want[2]) > 100
    _check_host(d, c, want, use_gnss)
    b = su.override_cases(sets["b"])
    for o in su.OVERRIDES:
        _same(_sbs_host(d, b, False, override_squawk=o)[0], su.sbs_of(b, override_squawk=o)[0])


# ---- misalignment and capacity ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(4))
def test_misalignment_and_capacity(ctx, k):
    d, hip = ctx
    c, _ = _mixed()
    c = su.slice_cases(c, 100 * k, 100 * k + 5 * su.BLOCK + 77)
    want = su.sbs_of(c, use_gnss=True)
    T = len(want[0])
    starts = (np.cumsum(want[1]) - want[1])[::su.BLOCK]
    assert T > 5 * su.BLOCK * 40 and len(set(((starts + k) % 4).tolist())) >= 2        # workgroups start at several alignments
    assert _sbs_device(d, hip, c, want, k=k, cap=T) == 0
    assert _sbs_device(d, hip, c, want, k=k, cap=T - 1) == su.MGPU_E_OVERFLOW
    assert _sbs_device(d, hip, c, want, k=k, cap=0) == su.MGPU_E_OVERFLOW
    assert _sbs_device(d, hip, c, want, k=k) == 0                                        # the context encodes correctly afterwards


# ---- the deferred list -----------------------------------------------------------------------------------------------------------------

def test_deferred_list(ctx):
    d, hip = ctx
    c, _ = _mixed()
    c = su.slice_cases(c, 2000, 2000 + 4 * su.BLOCK + 9)
    c = {k: v.copy() for k, v in c.items()}
    ends = np.concatenate([np.arange(0, len(c["msgs"]), su.BLOCK) + lane for lane in (0, 63, 64, 255)])
    ends = ends[ends < len(c["msgs"])]
    c["verdict"][ends] = su.GATE_DEFER | su.GATE_POSSIBLE                      # at the ends of waves and workgroups
    want = su.sbs_of(c, use_gnss=True)
    D = len(want[2])
    assert D > 20
    for dcap in (0, 1, D, D + 100):
        _sbs_device(d, hip, c, want, deferred_cap=dcap)
    # without verdicts nothing is deferred and no list is needed
    plain = su.sbs_reference(c["msgs"], c["fields"], su.NOW_MS, positions=c["positions"], geom_delta=c["geom_delta"], use_gnss=True)
    _sbs_device(d, hip, c, plain, with_verdict=False, deferred_cap=0)


# ---- hostile records -------------------------------------------------------------------------------------------------------------------

def test_hostile_records(ctx):
    d, hip = ctx
    c = su.hostile_cases(6 * su.BLOCK + 31, 77)
    for use_gnss in (False, True):
        want = su.sbs_of(c, use_gnss=use_gnss)
        assert (want[1] > 0).sum() > 200 and want[3] > 100 and len(want[2]) > 50 and want[1].max() <= su.SBS_LINE_MAX
        _sbs_device(d, hip, c, want, k=1 + use_gnss, use_gnss=use_gnss)
    _sbs_device(d, hip, c, su.sbs_of(c, override_squawk=-(1 << 31)), use_gnss=False, override_squawk=-(1 << 31))


def test_longest_lines_fill_a_workgroup(ctx):
    """Every lane a line of the full 176 bytes: the LDS buffer's limit."""
    d, hip = ctx
    c = su._base(2 * su.BLOCK + 3)
    f = c["fields"]
    f["flags"] = (su.F_CALLSIGN | su.F_GEOM_ALT | su.F_GS | su.F_HEADING | su.F_GEOM_RATE | su.F_SQUAWK | su.F_ALERT_VALID | su.F_ALERT | su.F_SPI_VALID
                  | su.F_SPI)
    f["callsign"], f["geom_alt"], f["geom_rate"], f["gs_selected"], f["heading"], f["heading_type"] = b"WWWWWWWW", su.INT32_MIN, su.INT32_MIN, -2147483520.0, -2147483520.0, 1
    f["airground"], f["addr"], f["squawkDec"], f["squawkHex"] = 1, 0xFEFFFFFF, 7700, 0x7700
    c["positions"]["method"], c["positions"]["lat"], c["positions"]["lon"] = 1, -89.9999995, -359.9999995
    want = su.sbs_of(c, use_gnss=True, override_squawk=-(1 << 31))
    assert (want[1] == su.SBS_LINE_MAX).all()
    for k in range(4):
        _sbs_device(d, hip, c, want, k=k, override_squawk=-(1 << 31))


# ---- cut lists ---------------------------------------------------------------------------------------------------------------------------

def test_cut_lists(ctx):
    d, _ = ctx
    c, (whole, length, _, _) = _mixed()
    n = len(c["msgs"])
    _same(_sbs_host(d, c)[0], whole)
    for cut in (1, 255, 256, 1000):
        lo, hi = (n // 2, n // 2 + 200) if cut == 1 else (0, n)
        got = b"".join(_sbs_host(d, su.slice_cases(c, k, min(k + cut, hi)))[0] for k in range(lo, hi, cut))
        start = int(length[:lo].sum())
        _same(got, whole[start:start + int(length[lo:hi].sum())])


# ---- the two forms, and the library's own field decode -----------------------------------------------------------------------------------

def test_forms_agree(ctx):
    d, hip = ctx
    a = _golden()[0]["a"]
    fields = d.decode_fields(a["msgs"])
    assert fields.tobytes() == a["fields"].tobytes()                           # group (a) holds the decode of its own frames
    with_fields = d.sbs_encode(a["msgs"], su.NOW_MS, fields=fields, positions=a["positions"], verdict=a["verdict"], geom_delta=a["geom_delta"])
    without = d.sbs_encode(a["msgs"], su.NOW_MS, positions=a["positions"], verdict=a["verdict"], geom_delta=a["geom_delta"])
    want = su.sbs_of(a)
    for got in (with_fields, without):
        _same(got[0], want[0])
        _same_deferred(got[1], want[2])
        assert got[2] == want[3]
    _sbs_device(d, hip, a, want, use_gnss=False)


def test_arguments(ctx):
    from readsb_amd.binding import SbsArgs, RawArgs
    d, hip = ctx
    c = _lined(10, 1)
    out = np.zeros(4096, dtype=np.uint8)
    nb, nd = C.c_uint64(7), C.c_uint64(7)

    def sbs(size=C.sizeof(SbsArgs), flags=0, n=10, now=su.NOW_MS, fields=c["fields"].ctypes.data, bytes_=C.pointer(nb), ndef=C.pointer(nd), device=False):
        a = SbsArgs(size, flags, c["msgs"].ctypes.data, fields, None, c["verdict"].ctypes.data, None, n, now, -1, out.ctypes.data, out.size, bytes_, None, 0, ndef, None)
        return int((d.lib.mgpu_sbs_encode_ex_device if device else d.lib.mgpu_sbs_encode_ex)(d.ctx, C.byref(a)))
    assert sbs() == 0 and nb.value == len(su.sbs_reference(c["msgs"], c["fields"], su.NOW_MS, verdict=c["verdict"])[0])
    assert sbs(n=0) == 0 and nb.value == 0
    assert sbs(n=0, device=True, fields=None) == 0
    assert sbs(size=C.sizeof(SbsArgs) - 8) == su.MGPU_E_INVAL
    assert sbs(flags=2) == su.MGPU_E_INVAL
    assert sbs(now=-1) == su.MGPU_E_INVAL and sbs(now=su.MS_END) == su.MGPU_E_INVAL and sbs(now=su.MS_END - 1) == 0
    assert sbs(bytes_=None) == su.MGPU_E_INVAL and sbs(ndef=None) == su.MGPU_E_INVAL
    assert sbs(device=True, fields=None) == su.MGPU_E_INVAL                    # only the host form decodes the fields itself
    m = c["msgs"]

    def raw(size=C.sizeof(RawArgs), flags=0, n=10):
        a = RawArgs(size, flags, m.ctypes.data, None, n, out.ctypes.data, out.size, C.pointer(nb), None, 0, None)
        return int(d.lib.mgpu_raw_encode_ex(d.ctx, C.byref(a)))
    assert raw() == 0 and raw(n=0) == 0 and nb.value == 0
    assert raw(size=C.sizeof(RawArgs) - 8) == su.MGPU_E_INVAL and raw(flags=8) == su.MGPU_E_INVAL


# ---- end to end --------------------------------------------------------------------------------------------------------------------------

def test_end_to_end_on_a_capture(ctx):
    """feed -> decode_fields_device -> track_gate_device -> cpr_track_device -> sbs_encode_device, everything resident, against the
    checker on the same stages' host results."""
    import readsb_amd
    _, hip = ctx
    iq = helpers.synth(seconds=2.0, seed=4242, rate=2500.0)
    d = readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=16 * 131072)          # a stream of its own
    try:
        _end_to_end(d, hip, iq)
    finally:
        d.close()


def _end_to_end(d, hip, iq):
    import readsb_amd
    msgs, _ = d.demodulate_capture(iq)
    n = len(msgs)
    ref = (52.0, 4.0)
    d.track_gate_reset()
    d.cpr_reset()
    fields, verdict, positions = d.decode_fields(msgs), d.track_gate(msgs), d.cpr_track(msgs, ref=ref)
    d.track_gate_reset()
    d.cpr_reset()
    want = su.sbs_reference(msgs, fields, su.NOW_MS, positions=positions, verdict=verdict, use_gnss=True)
    cap = len(want[0]) + 64
    d_msgs = hip.upload(msgs)
    d_fields, d_verdict, d_pos = hip.malloc(n * readsb_amd.FIELDS_DTYPE.itemsize), hip.malloc(n), hip.malloc(n * readsb_amd.POSITION_DTYPE.itemsize)
    d_out, d_def = hip.malloc(cap), hip.malloc((len(want[2]) + 1) * bu.DEFERRED.itemsize)
    try:
        d.decode_fields_device(d_msgs, n, d_fields)
        d.track_gate_device(d_msgs, d_fields, n, d_verdict)
        d.cpr_track_device(d_msgs, d_fields, n, d_pos, ref=ref)
        nb, nd, ns = d.sbs_encode_device(d_msgs, d_fields, n, su.NOW_MS, d_out, cap, d_positions_ptr=d_pos, d_verdict_ptr=d_verdict, use_gnss=True,
                                         d_deferred_ptr=d_def, deferred_cap=len(want[2]) + 1)
        stream = hip.download(d_out, nb).tobytes()
        deferred = hip.download(d_def, nd * bu.DEFERRED.itemsize, dtype=bu.DEFERRED)
    finally:
        for p in (d_msgs, d_fields, d_verdict, d_pos, d_out, d_def):
            hip.free(p)
        d.track_gate_reset()
        d.cpr_reset()
    _same(stream, want[0])
    _same_deferred(deferred, want[2])
    assert ns == want[3] == 0
    lines = stream.split(b"\r\n")[:-1]
    assert len(lines) >= 100
    due = want[1] > 0
    present = set(su.sbs_msg_type(int(a), int(b)) for a, b in zip(fields["msgtype"][due].tolist(), fields["metype"][due].tolist()))
    contained = set(su.sbs_msg_type(int(a), int(b)) for a, b in zip(fields["msgtype"].tolist(), fields["metype"].tolist())) - {0}
    assert present == contained and len(contained) >= 3, (present, contained)
    for t in contained:
        assert any(l.startswith(b"MSG,%d," % t) for l in lines), t
    assert any(l.split(b",")[14] != b"" and l.split(b",")[15] != b"" for l in lines), "no line carries a position"


# ---- raw -----------------------------------------------------------------------------------------------------------------------------------

def _raw_device(d, hip, msgs, verdict, want, k, cap=None, deferred_cap=None, **flags):
    wstream, _, wdef = want
    T, D = len(wstream), len(wdef)
    cap = T if cap is None else cap
    dcap = D if deferred_cap is None else deferred_cap
    total = GUARD + k + max(cap, T) + GUARD
    d_in, d_v = hip.upload(msgs), hip.upload(verdict) if verdict is not None else None
    d_buf, d_def = hip.malloc(total), hip.malloc((dcap + DEF_GUARD) * bu.DEFERRED.itemsize)
    try:
        hip.fill(d_buf, 0xA5, total)
        hip.fill(d_def, 0xA5, (dcap + DEF_GUARD) * bu.DEFERRED.itemsize)
        from readsb_amd.binding import RawArgs
        nb, nd = C.c_uint64(12345), C.c_uint64(12345)
        a = RawArgs(C.sizeof(RawArgs), d._raw_flags(**flags), d_in, d_v, len(msgs), d_buf + GUARD + k, cap, C.pointer(nb), d_def, dcap, C.pointer(nd))
        rc = int(d.lib.mgpu_raw_encode_ex_device(d.ctx, C.byref(a)))
        buf = hip.download(d_buf, total)
        got_def = hip.download(d_def, (dcap + DEF_GUARD) * bu.DEFERRED.itemsize, dtype=bu.DEFERRED)
    finally:
        for p in (d_in, d_v, d_buf, d_def):
            if p is not None:
                hip.free(p)
    at = GUARD + k
    assert (nb.value, nd.value) == (T, D), (nb.value, nd.value, T, D)
    assert (buf[:at] == 0xA5).all() and (buf[at + min(cap, T):] == 0xA5).all(), "bytes outside the stream, or at / beyond the capacity, were written"
    _same(buf[at:at + min(cap, T)].tobytes(), wstream[:min(cap, T)])
    listed = min(dcap, D)
    _same_deferred(got_def[:listed], wdef[:listed])
    assert (got_def[listed:].view(np.uint8) == 0xA5).all(), "entries behind the list were written"
    assert rc == (su.MGPU_E_OVERFLOW if cap < T or dcap < D else 0), rc


@pytest.mark.parametrize("mlat,net_rule,verbatim", su.RAW_VARIANTS)
def test_raw(ctx, mlat, net_rule, verbatim):
    d, hip = ctx
    flags = dict(mlat=mlat, net_rule=net_rule, verbatim=verbatim)
    gm, gv = _golden()[1]
    pool = bu.hostile_records(5 * su.BLOCK + 5, 99)                            # every length, timestamps at and above 2^48 and negative
    pool_v = bu.random_verdicts(len(pool), 98)
    # the golden cases: the reference's own bytes where it has them
    for verdict in (None, gv):
        want = su.raw_reference(gm, verdict=verdict, **flags)
        got = d.raw_encode(gm, verdict=verdict, **flags)
        _same(got[0], want[0])
        _same_deferred(got[1], want[2])
    if not net_rule:
        carried = gm[np.isin(gm["msgbits"], (16, 56, 112))]
        _same(d.raw_encode(carried, mlat=mlat, verbatim=verbatim)[0], _golden()[2][f"ref_raw_m{int(mlat)}v{int(verbatim)}"])
    # sizes: every message, none, only a workgroup's last lane
    for n in SIZES:
        m, v = pool[:n].copy(), pool_v[:n]
        m["msgbits"] = np.array([16, 56, 112])[np.arange(n) % 3]
        m["correctedbits"] = 0
        last = m.copy()
        last["msgbits"] = 0
        last["msgbits"][su.BLOCK - 1::su.BLOCK] = 112
        for what, mm, vv in (("every", m, None), ("none", m, np.zeros(n, dtype=np.uint8)), ("last lane", last, None), ("verdicts", m, v)):
            want = su.raw_reference(mm, verdict=vv, **flags)
            lines = int((want[1] > 0).sum())
            if what != "verdicts":
                assert lines == {"every": n, "none": n if verbatim else 0, "last lane": n // su.BLOCK}[what]
            got = d.raw_encode(mm, verdict=vv, **flags)
            _same(got[0], want[0])
            _same_deferred(got[1], want[2])
    # hostile records on the device: misalignment, capacity, the deferred list
    want = su.raw_reference(pool, verdict=pool_v, **flags)
    T, D = len(want[0]), len(want[2])
    assert T > 3000 and (verbatim or D > 20)
    for k in range(4):
        _raw_device(d, hip, pool, pool_v, want, k, **flags)
    _raw_device(d, hip, pool, pool_v, want, 1, cap=T - 1, **flags)
    _raw_device(d, hip, pool, pool_v, want, 2, cap=0, **flags)
    if D:
        for dcap in (0, 1, D + 10):
            _raw_device(d, hip, pool, pool_v, want, 3, deferred_cap=dcap, **flags)
    # cut lists
    whole = su.raw_reference(pool, verdict=pool_v, **flags)[0]
    for cut in (255, 256, 1000):
        _same(b"".join(d.raw_encode(pool[s:s + cut], verdict=pool_v[s:s + cut], **flags)[0] for s in range(0, len(pool), cut)), whole)
    _same(b"".join(d.raw_encode(pool[s:s + 1], verdict=pool_v[s:s + 1], **flags)[0] for s in range(300, 400)),
          su.raw_reference(pool[300:400], verdict=pool_v[300:400], **flags)[0])


# ---- the host program ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _cli_capture():
    """A capture and, from the host-array stages on its whole message list, the SBS stream with the deferred messages dropped."""
    import readsb_amd
    iq = helpers.synth(seconds=2.0, seed=515, rate=2500.0)
    ref = (52.0, 4.0)
    d = readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=16 * 131072)
    try:
        msgs, _ = d.demodulate_capture(iq)
        fields, verdict = d.decode_fields(msgs), d.track_gate(msgs)
        want = {}
        for with_ref in (False, True):
            d.cpr_reset()
            positions = d.cpr_track(msgs, ref=ref if with_ref else None)
            for gnss in (False, True):
                want[with_ref, gnss] = su.sbs_reference(msgs, fields, su.NOW_MS, positions=positions, verdict=verdict, use_gnss=gnss)
    finally:
        d.close()
    return iq, ref, want


@pytest.mark.parametrize("chunk,with_ref,gnss", [(256, True, False), (7, True, True), (3, False, False)])
def test_host_program_sbs_out(built, tmp_path, chunk, with_ref, gnss):
    """readsb_gpu_ifile --sbs-out: the file is the checker's stream for the capture — one feed or many — and --help says that
    deferred messages are dropped."""
    import os
    import subprocess
    cli = os.path.join(helpers.ROOT, "readsb_amd", "host", "readsb_gpu_ifile")
    iq, ref, want = _cli_capture()
    stream, length, deferred, nskipped = want[with_ref, gnss]
    cap, out = tmp_path / "cap.iq", tmp_path / "out.sbs"
    iq.tofile(cap)
    cmd = [cli, "--device-type", "ifile", "--ifile", str(cap), "--iformat", "UC8", "--fix", "--startup-time-ms", str(helpers.STARTUP_MS),
           "--gpu-chunk-buffers", str(chunk), "--sbs-out", str(out), "--sbs-now-ms", str(su.NOW_MS), "--stats"]
    cmd += ["--lat", str(ref[0]), "--lon", str(ref[1])] if with_ref else []
    cmd += ["--gnss"] if gnss else []
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == ""
    _same(out.read_bytes(), stream)
    lines = stream.split(b"\r\n")[:-1]
    assert len(lines) >= 100 and nskipped == 0
    if with_ref:
        assert any(l.split(b",")[14] != b"" for l in lines), "no line carries a position"
    assert f"{len(deferred)} message(s) left to a position tracker dropped" in r.stderr
    assert "Mode-S message preambles received" in r.stderr
    if chunk == 256:
        h = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=30)
        assert h.returncode == 0 and "--sbs-out" in h.stdout and "DROPPED" in h.stdout
