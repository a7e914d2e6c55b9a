"""-m gpu: SBS input on the device (kernels/sbs_in.inc, mgpu_sbs_decode / mgpu_sbs_decode_device): the records, their source lines, the
counters and the deferred list compared with == on bytes against what the reference's readAscii + decodeSbsLine left
(tests/golden/sbs_in_cases.npz, which tests/test_sbs_in_reference.py holds to the live reference on the CPU) and, for built streams,
against the library's host parser (which the same CPU tests hold to the reference).

Shapes: a tile is 8192 bytes of text, a lane takes the lines that start in 32 of them, the halo is 256 bytes, a load 16 bytes, a line
is decided by 201 bytes at the most.  The golden groups are 39 to 56 KB (5 to 7 tiles); the cutting stream is about 4 300 lines (50
tiles); the tile-edge streams are three tiles at every misalignment of the text."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import beast_util as bu
import helpers
import sbs_in_util as su
import sbs_util

pytestmark = pytest.mark.gpu

GUARD = 4                                        # records, line indices in front of and behind every array
CANARY = 0xA5A5A5A5A5A5A5A5
CLI = os.path.join(helpers.ROOT, "readsb_amd", "host", "readsb_gpu_sbs_in")
FULL = dict(callsign="BAW123  ", alt="35000", gs="451", trk="271", lat="51.477500", lon="-0.461389", vr="-64", sq="4721", f19="0", f20="0", f21="0", f22="0")


@pytest.fixture(scope="module")
def ctx(built):
    import readsb_amd
    d = readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=131072)
    hip = bu.Hip()
    try:
        yield d, hip
    finally:
        hip.free_all()
        d.close()


@pytest.fixture(scope="module")
def golden():
    return su.load_golden()


def call(d, form, text_ptr, nbytes, recs_ptr, line_ptr, recs_cap, deferred_cap=0, source="sbs", pass_bytes=0, size=None, counters=True):
    """The C entry itself -> (rc, dict of the counters, the deferred list as far as it was written)."""
    from readsb_amd import binding
    c = [C.c_uint64(0xDEAD) for _ in range(5)]
    deferred = np.full(deferred_cap + 4, CANARY, dtype=np.uint64)
    ptrs = [C.pointer(x) for x in c] if counters else [None] * 5
    a = binding.SbsInArgs(C.sizeof(binding.SbsInArgs) if size is None else size, su.SOURCES.get(source, source), text_ptr, nbytes, su.NOW_MS, recs_ptr, line_ptr, recs_cap,
                          deferred.ctypes.data if deferred_cap else None, deferred_cap, *ptrs, pass_bytes)
    f = d.lib.mgpu_sbs_decode if form == "host" else d.lib.mgpu_sbs_decode_device
    rc = int(f(d.ctx, C.byref(a)))
    n = dict(zip(("consumed", "nlines", "nrecs", "ninvalid", "ndeferred"), (int(x.value) for x in c)))
    assert (deferred[deferred_cap:] == CANARY).all(), "a deferred index beyond the list's capacity"
    return rc, n, deferred[: min(n["ndeferred"], deferred_cap)] if rc != su.MGPU_E_INVAL else deferred[:0]


def run(d, hip, form, text, source="sbs", recs_cap=None, deferred_cap=None, text_off=0, recs_off=0, pass_bytes=0):
    """One call with every array between canaries -> dict(rc, counters..., recs, line_of, deferred, intact).  recs_off: 0 or 8, the
    records' place modulo 16."""
    text = bytes(text)
    most = len(text) // 21 + 1
    recs_cap = most if recs_cap is None else recs_cap
    deferred_cap = most if deferred_cap is None else deferred_cap
    rec_bytes, line_bytes = (recs_cap + 2 * GUARD) * 96 + 16, (recs_cap + 2 * GUARD) * 8
    lo = GUARD * 96 + recs_off
    if form == "host":
        src = np.frombuffer(b"\n" * text_off + text + b"\nMSG,3,1,1,4AC8B3,1,,,,,,,,,,,,,,,,\n", dtype=np.uint8)       # (a line behind the text: nothing beyond nbytes may count)
        raw = np.full(rec_bytes, 0xA5, dtype=np.uint8)
        lines = np.full(recs_cap + 2 * GUARD, CANARY, dtype=np.uint64)
        rc, n, deferred = call(d, form, src.ctypes.data + text_off if text else None, len(text), raw.ctypes.data + lo, lines.ctypes.data + 8 * GUARD, recs_cap, deferred_cap,
                               source, pass_bytes)
    else:
        d_text = hip.upload(np.frombuffer(b"\n" * text_off + text + b"\nMSG,3,1,1,4AC8B3,1,,,,,,,,,,,,,,,,\n", dtype=np.uint8))
        d_recs, d_lines = hip.malloc(rec_bytes), hip.malloc(line_bytes)
        hip.fill(d_recs, 0xA5, rec_bytes)
        hip.fill(d_lines, 0xA5, line_bytes)
        rc, n, deferred = call(d, form, d_text + text_off, len(text), d_recs + lo, d_lines + 8 * GUARD, recs_cap, deferred_cap, source)
        raw, lines = hip.download(d_recs, rec_bytes), hip.download(d_lines, line_bytes, dtype=np.uint64)
        for p in (d_text, d_recs, d_lines):
            hip.free(p)
    nrec = min(n["nrecs"], recs_cap) if rc != su.MGPU_E_INVAL else 0
    intact = (raw[:lo] == 0xA5).all() and (raw[lo + 96 * nrec:] == 0xA5).all() and (lines[:GUARD] == CANARY).all() and (lines[GUARD + nrec:] == CANARY).all()
    return dict(n, rc=rc, recs=raw[lo: lo + 96 * nrec].copy().view(su.REC), line_of=lines[GUARD: GUARD + nrec].copy(), deferred=deferred, intact=bool(intact))


def stream_expected(stream, source="sbs"):
    """(records, line_of, invalid lines, lines, consumed) of a stream by the host parser of the library, every number resolved: what a
    call must give for a stream in which nothing is deferred."""
    import readsb_amd
    lib = readsb_amd.load_library()
    one = np.zeros(1, dtype=su.REC)
    recs, line_of, invalid = [], [], 0
    lines = su.split_lines(stream)
    for k, x in enumerate(lines):
        src = np.frombuffer(x, dtype=np.uint8)
        rc = int(lib.mgpu_sbs_parse_line_host(src.ctypes.data if len(x) else None, len(x), su.SOURCES[source], su.NOW_MS, one.ctypes.data))
        assert rc in (0, 1)
        if rc:
            recs.append(one.copy())
            line_of.append(k)
        else:
            body = x[:-1] if len(x) >= 2 and x.endswith(b"\r") else x
            invalid += len(body) >= 2
    consumed = max(stream.rfind(b"\n"), stream.rfind(b"\0")) + 1
    return (np.concatenate(recs) if recs else np.zeros(0, dtype=su.REC)), np.array(line_of, dtype=np.uint64), invalid, len(lines), consumed


def same(res, want):
    recs, line_of, invalid, nlines, consumed = want
    assert res["rc"] == su.MGPU_OK and res["intact"]
    assert (res["consumed"], res["nlines"], res["nrecs"], res["ninvalid"], res["ndeferred"]) == (consumed, nlines, len(recs), invalid, 0)
    assert res["recs"].tobytes() == recs.tobytes() and (res["line_of"] == line_of).all()


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("group", su.GROUPS)
def test_golden_groups(ctx, golden, group, form):
    """Every golden group and source through the C entry of either form: records, source lines, counters, the deferred list; for group
    (c) nothing but the list, and mgpu_sbs_parse_host settles every listed line to the reference's record."""
    d, hip = ctx
    from readsb_amd import binding
    stream, by_source = golden[group]
    for s, (head, line_of, recs) in by_source.items():
        deferred = line_of.tolist() if group == "c" else []
        want_line_of, want_recs = su.without(line_of, recs, deferred)
        res = run(d, hip, form, stream, source=s, recs_off=8 if s == "mlat" else 0)
        assert res["rc"] == su.MGPU_OK and res["intact"], (group, s)
        assert (res["consumed"], res["nlines"], res["nrecs"], res["ninvalid"], res["ndeferred"]) == (int(head[0]), int(head[1]), len(want_recs), int(head[3]), len(deferred)), (group, s)
        assert res["recs"].tobytes() == want_recs.tobytes() and (res["line_of"] == want_line_of).all() and res["deferred"].tolist() == deferred, (group, s)
        if deferred:
            src = np.frombuffer(stream, dtype=np.uint8)
            a = binding.SbsInArgs(size=C.sizeof(binding.SbsInArgs), source=su.SOURCES[s], text=src.ctypes.data, nbytes=src.size, now_ms=su.NOW_MS)
            settled = np.zeros(len(deferred), dtype=su.REC)
            for k, index in enumerate(res["deferred"].tolist()):
                assert d.lib.mgpu_sbs_parse_host(C.byref(a), index, settled[k: k + 1].ctypes.data) == 1
            assert settled.tobytes() == recs.tobytes(), (group, s)


def test_binding_settles(ctx, golden):
    """Demodulator.sbs_decode: the reference's records with the deferred lines' spliced in, on group (c) alone and between two copies
    of group (a); settle=False leaves them out and lists them."""
    d, hip = ctx
    a_stream, a_by = golden["a"]
    c_stream, c_by = golden["c"]
    for s in ("sbs", "mlat"):
        res = d.sbs_decode(c_stream, source=s, now_ms=su.NOW_MS)
        assert res["recs"].tobytes() == c_by[s][2].tobytes() and (res["line_of"] == c_by[s][1]).all() and len(res["deferred"]) == len(c_by[s][2])
        stream = a_stream + c_stream + a_stream
        na, nc = int(a_by[s][0][1]), int(c_by[s][0][1])
        want = np.concatenate([a_by[s][2], c_by[s][2], a_by[s][2]])
        want_lines = np.concatenate([a_by[s][1], c_by[s][1] + na, a_by[s][1] + na + nc])
        res = d.sbs_decode(stream, source=s, now_ms=su.NOW_MS, pass_bytes=30000)
        assert res["recs"].tobytes() == want.tobytes() and (res["line_of"] == want_lines).all() and res["consumed"] == len(stream) and res["nlines"] == 2 * na + nc
        res = d.sbs_decode(stream, source=s, now_ms=su.NOW_MS, settle=False)
        assert res["recs"].tobytes() == np.concatenate([a_by[s][2], a_by[s][2]]).tobytes() and (res["deferred"] == c_by[s][1] + na).all()


def test_cut_at_every_byte_of_a_line(ctx):
    """A stream of about 50 tiles cut in two at every byte of one line (and a few bytes around it), the unconsumed rest carried into
    the second call, gives the records of one call: this is `consumed`."""
    d, hip = ctx
    lines = su.feed(4300, seed=3)
    stream = b"".join(lines)
    assert 48 * su.TILE < len(stream) < 56 * su.TILE
    whole = run(d, hip, "device", stream, source="mlat")
    same(whole, stream_expected(stream, "mlat"))
    assert whole["nrecs"] == len(lines)
    ends = np.cumsum([len(x) for x in lines])
    lo = int(ends[2149]) - 3
    d_text = hip.upload(np.frombuffer(stream, dtype=np.uint8))
    cap = len(lines)
    d_recs, d_lines = hip.malloc((cap + 1) * 96), hip.malloc((cap + 1) * 8)
    for cut in range(lo, lo + len(lines[2150]) + 6):
        hip.fill(d_recs, 0xA5, (cap + 1) * 96)
        hip.fill(d_lines, 0xA5, (cap + 1) * 8)
        rc, n1, _ = call(d, "device", d_text, cut, d_recs, d_lines, cap, source="mlat")
        want_consumed = int(ends[ends <= cut].max())
        assert rc == su.MGPU_OK and n1["consumed"] == want_consumed and n1["nlines"] == n1["nrecs"] == int((ends <= cut).sum()), cut
        rc, n2, _ = call(d, "device", d_text + n1["consumed"], len(stream) - n1["consumed"], d_recs + 96 * n1["nrecs"], d_lines + 8 * n1["nrecs"], cap - n1["nrecs"], source="mlat")
        assert rc == su.MGPU_OK and n1["nrecs"] + n2["nrecs"] == cap and n2["consumed"] == len(stream) - n1["consumed"], cut
        got, got_lines = hip.download(d_recs, (cap + 1) * 96), hip.download(d_lines, (cap + 1) * 8, dtype=np.uint64)
        assert got[: cap * 96].tobytes() == whole["recs"].tobytes() and (got[cap * 96:] == 0xA5).all(), cut
        got_lines[n1["nrecs"]: cap] += n1["nlines"]
        assert (got_lines[:cap] == whole["line_of"]).all() and got_lines[cap] == CANARY, cut
    for p in (d_text, d_recs, d_lines):
        hip.free(p)


def edge_stream(kind, first):
    """Three tiles and more of drawn lines with a crafted place at stream position `first` (a tile's last or first byte): filler lines
    (valid, 81 to 199 bytes) end right before it."""
    lines = su.feed(260, seed=5)
    head, at = [], 0
    for x in lines:
        if at + len(x) > first - 210:
            break
        head.append(x)
        at += len(x)
    rest = lines[len(head):]
    # start: a line's first byte at `first` (a tile's last byte), the terminator before it at first - 1; terminator / nul: a '\n' / NUL
    # at `first` (a tile's first byte); long: a 199-byte line and its '\r' from a tile's last byte on — 201 bytes decide it, in the halo
    total = first - at + (kind in ("terminator", "nul"))             # bytes of filler, terminators included
    assert 200 < total <= 400
    sizes = [total // 2, total - total // 2]
    pad = su.padded(sizes[0] - 1, alt="1") + su.padded(sizes[1] - 1, end=b"\0" if kind == "nul" else b"\n", alt="1")
    special = su.padded(199, end=b"\r\n", **FULL) + su.padded(200, end=b"\r\n", **FULL) if kind == "long" else su.sbs(**FULL)
    stream = b"".join(head) + pad + special + b"".join(rest)
    assert len(stream) > 3 * su.TILE
    return stream


@pytest.mark.parametrize("kind", ["start", "terminator", "long", "nul"])
def test_tile_edges(ctx, kind):
    """A line's first byte on a tile's last byte; a terminator on a tile's first byte; a 199-byte line with '\\r' reaching into the halo;
    a NUL terminator at a tile edge: the device form at every misalignment 0-15 of the text, the host form once."""
    d, hip = ctx
    for tile in (1, 2):
        first = tile * su.TILE - 1 if kind in ("start", "long") else tile * su.TILE
        stream = edge_stream(kind, first)
        if kind in ("start", "long"):
            assert stream[first - 1: first + 4] == b"\nMSG,"
        else:
            assert stream[first: first + 5] == (b"\0MSG," if kind == "nul" else b"\nMSG,")
        want = stream_expected(stream)
        assert want[2] == (1 if kind == "long" else 0)
        for text_off in range(16):
            same(run(d, hip, "device", stream, text_off=text_off, recs_off=8 * (text_off & 1)), want)
        same(run(d, hip, "host", stream), want)


@pytest.mark.parametrize("form", ["host", "device"])
def test_capacities_one_short(ctx, golden, form):
    """Each capacity exact, then one short: MGPU_E_OVERFLOW with what is needed, nothing beyond the capacity touched, the records
    below it as they would be."""
    d, hip = ctx
    stream = golden["a"][0] + golden["c"][0] + golden["b"][0]
    full = run(d, hip, form, stream)
    assert full["rc"] == su.MGPU_OK and full["intact"] and full["ndeferred"] == len(golden["c"][1]["sbs"][2])
    need = (full["nrecs"], full["ndeferred"])
    exact = run(d, hip, form, stream, recs_cap=need[0], deferred_cap=need[1])
    assert exact["rc"] == su.MGPU_OK and exact["intact"] and exact["recs"].tobytes() == full["recs"].tobytes() and exact["deferred"].tolist() == full["deferred"].tolist()
    for kw in (dict(recs_cap=need[0] - 1), dict(deferred_cap=need[1] - 1), dict(recs_cap=0, deferred_cap=0), dict(recs_cap=7, deferred_cap=3)):
        res = run(d, hip, form, stream, **{**dict(recs_cap=need[0], deferred_cap=need[1]), **kw})
        assert res["rc"] == su.MGPU_E_OVERFLOW and res["intact"], kw
        assert (res["nrecs"], res["ndeferred"], res["nlines"], res["consumed"]) == (need[0], need[1], full["nlines"], len(stream)), kw
        assert res["recs"].tobytes() == full["recs"][: len(res["recs"])].tobytes() and (res["line_of"] == full["line_of"][: len(res["line_of"])]).all()
        assert res["deferred"].tolist() == full["deferred"].tolist()[: len(res["deferred"])]


@pytest.mark.parametrize("form", ["host", "device"])
def test_bad_arguments_and_empty(ctx, form):
    d, hip = ctx
    from readsb_amd import binding
    text = su.sbs(**FULL) * 3
    buf = np.frombuffer(text, dtype=np.uint8)
    d_text, d_recs, d_lines = hip.upload(buf), hip.malloc(8 * 96), hip.malloc(8 * 8)
    host_recs, host_lines = np.zeros(8, dtype=su.REC), np.zeros(8, dtype=np.uint64)
    tp, rp, lp = (buf.ctypes.data, host_recs.ctypes.data, host_lines.ctypes.data) if form == "host" else (d_text, d_recs, d_lines)
    f = d.lib.mgpu_sbs_decode if form == "host" else d.lib.mgpu_sbs_decode_device
    assert call(d, form, tp, len(text), rp, lp, 8)[0] == su.MGPU_OK
    assert f(None, None) == su.MGPU_E_INVAL and f(d.ctx, None) == su.MGPU_E_INVAL
    assert call(d, form, tp, len(text), rp, lp, 8, size=C.sizeof(binding.SbsInArgs) - 8)[0] == su.MGPU_E_INVAL
    assert call(d, form, tp, len(text), rp, lp, 8, size=0)[0] == su.MGPU_E_INVAL
    for source in (0, 1, 2, 5, 7, 10, 12, 64 + 3, 0xFFFFFFFF):
        assert call(d, form, tp, len(text), rp, lp, 8, source=source)[0] == su.MGPU_E_INVAL, source
    assert call(d, form, None, len(text), rp, lp, 8)[0] == su.MGPU_E_INVAL
    assert call(d, form, tp, len(text), None, lp, 8)[0] == su.MGPU_E_INVAL
    assert call(d, form, tp, len(text), rp, lp, 8, counters=False)[0] == su.MGPU_E_INVAL
    if form == "device":
        assert call(d, form, tp, len(text), rp + 4, lp, 4)[0] == su.MGPU_E_INVAL                    # records off their alignment
    # a deferred_cap without its list or its counter
    c = [C.c_uint64(0) for _ in range(4)]
    a = binding.SbsInArgs(C.sizeof(binding.SbsInArgs), 3, tp, len(text), 0, rp, lp, 8, None, 4, *[C.pointer(x) for x in c], None, 0)
    assert f(d.ctx, C.byref(a)) == su.MGPU_E_INVAL
    for p in (d_text, d_recs, d_lines):
        hip.free(p)
    # nbytes == 0, with and without pointers; text without any terminator
    for t in (b"", su.sbs(end=b"", **FULL), su.sbs(end=b"", **FULL) * 100):
        res = run(d, hip, form, t)
        assert (res["rc"], res["consumed"], res["nlines"], res["nrecs"], res["ninvalid"], res["ndeferred"], res["intact"]) == (su.MGPU_OK, 0, 0, 0, 0, 0, True)
    rc, n, _ = call(d, form, None, 0, None, None, 0)
    assert rc == su.MGPU_OK and set(n.values()) == {0}


def test_host_form_in_small_passes(ctx, golden):
    """The host form with pass_bytes far below the stream, down to 1 (every pass grows until it holds a line), equals one device call;
    bytes behind the last terminator are left."""
    d, hip = ctx
    stream = golden["b"][0] + golden["c"][0] + golden["a"][0] + b"MSG,3,1,1,4AC8B3,1,a tail without its terminator"
    one = run(d, hip, "device", stream, source="mlat")
    assert one["rc"] == su.MGPU_OK and one["consumed"] == len(stream) - 48 and one["ndeferred"] == len(golden["c"][1]["mlat"][2])
    for pass_bytes in (1, 250, 8191, 8192, 20000):
        part = stream[:30000] + stream[-48:] if pass_bytes == 1 else stream
        ref = run(d, hip, "device", part, source="mlat") if pass_bytes == 1 else one
        res = run(d, hip, "host", part, source="mlat", pass_bytes=pass_bytes)
        assert res["rc"] == su.MGPU_OK and res["intact"], pass_bytes
        assert all(res[k] == ref[k] for k in ("consumed", "nlines", "nrecs", "ninvalid", "ndeferred")), pass_bytes
        assert res["recs"].tobytes() == ref["recs"].tobytes() and (res["line_of"] == ref["line_of"]).all() and res["deferred"].tolist() == ref["deferred"].tolist(), pass_bytes


def test_round_trip_through_the_sbs_writer(ctx):
    """A short synthetic capture's message list through the existing mgpu_sbs_encode_ex, those lines through the new decoder: the
    records equal the host parser's, and addr, callsign, altitude and squawk equal the field records the lines were printed from."""
    d, hip = ctx
    from readsb_amd import binding
    iq = helpers.synth(seconds=2.0, seed=7)                                                        # (drawn ME fields: four valid callsigns in two seconds)
    msgs, _ = d.demodulate_capture(iq)
    fields = d.decode_fields(msgs)
    stream, deferred, _ = d.sbs_encode(msgs, su.NOW_MS, fields=fields)
    assert len(deferred) == 0
    cls, _ = sbs_util.sbs_classes(fields, msgs["sysTimestamp"], None, None)                        # net_io.c:3191, :3207-3245: who gets a line
    printed = cls == sbs_util.LINE
    f = fields[printed]
    lines = su.split_lines(stream)
    assert len(lines) == len(f) > 100
    res = run(d, hip, "device", stream)
    same(res, stream_expected(stream))
    r = res["recs"]
    assert len(r) == len(f) and (r["addr"] == f["addr"]).all()
    flag = lambda bit: (f["flags"] >> bit) & 1 == 1                                               # noqa: E731
    # the writer prints every callsign the Mode S decode takes ('/', '@', '-', '.' among them); the reader's rule is narrower (:3042-3044)
    read_back = (r["flags"] >> 9) & 1 == 1
    assert flag(9).sum() >= 2 and read_back.sum() >= 1 and (read_back & ~flag(9)).sum() == 0
    for got, want, valid, again in zip(r["callsign"], f["callsign"], flag(9), read_back):
        assert got.rstrip(b" ") == (want.rstrip(b" ") if valid else b"")
        assert not valid or bool(again) == all(c in b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 " for c in want)
    alt = flag(0)
    assert (r["baro_alt"][alt] == f["baro_alt"][alt]).all() and alt.sum() > 10
    sq = flag(8) & (f["squawkDec"] > 0)
    assert (((r["flags"] >> 8) & 1 == 1) == sq).all() and (r["squawkDec"][sq] == f["squawkDec"][sq]).all() and (r["squawkHex"][sq] == f["squawkHex"][sq]).all()
    assert (r["sysTimestamp"] == su.NOW_MS).all() and (r["source"] == 3).all() and (r["addrtype"] == 6).all()
    assert binding.SBS_REC_DTYPE == su.REC


def test_command_line_against_the_library(ctx, golden):
    """readsb_gpu_sbs_in as a child process on golden groups equals the library: the records with the deferred ones in place, with a
    block smaller than the stream so that lines are carried between calls; --stats prints the counts."""
    d, hip = ctx
    for g, s, block in (("a", "mlat", 4096), ("b", "sbs", 700), ("c", "sbs", 5000), ("b", "prio", 1 << 20)):
        stream, by_source = golden[g]
        head, line_of, recs = by_source[s]
        lib = d.sbs_decode(stream, source=s, now_ms=su.NOW_MS)
        assert lib["recs"].tobytes() == recs.tobytes()
        r = subprocess.run([CLI, "--source", s, "--now", str(su.NOW_MS), "--block", str(block)], input=stream + b"MSG,3,no terminator", capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr[-500:]
        assert r.stdout == lib["recs"].tobytes(), (g, s)
        r = subprocess.run([CLI, "--source", s, "--now", str(su.NOW_MS), "--block", str(block), "--stats"], input=stream, capture_output=True, timeout=120)
        assert r.returncode == 0 and r.stdout.decode().split() == ["lines", str(int(head[1])), "records", str(len(recs)), "invalid", str(int(head[3])), "deferred",
                                                                    str(len(lib["deferred"])), "bytes", str(len(stream))], r.stdout
