"""-m gpu: ASTERIX input on the device (kernels/asterix_in.inc, mgpu_asterix_decode / mgpu_asterix_decode_device): the records, their
frames, every counter and the stop compared with == on bytes against what the reference's readAsterix + decodeAsterixMessage left
(tests/golden/asterix_in_cases.npz, which tests/test_asterix_in_reference.py holds to the live reference on the CPU) and, for built
streams, against the framing rule restated in tests/asterix_in_util.py with the library's host parser (which the same CPU tests hold to
the reference).

Shapes: a tile is 65536 bytes, a group 32 tiles, a lane classifies the starts in 64 bytes, a frame is decided by 1 KiB at the most.
The streams are 3 to 5 tiles; one has 40 tiles, so that the chain crosses a group's edge; the time values' stream has 11."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import asterix_in_util as au
import beast_util as bu
import helpers

pytestmark = pytest.mark.gpu

GUARD = 4                                        # records, frame indices in front of and behind every array
CANARY = 0xA5A5A5A5A5A5A5A5
CLI = os.path.join(helpers.ROOT, "readsb_amd", "host", "readsb_gpu_asterix_in")
TILE = au.TILE
ADDR = {"080": b"\x4a\xc8\xb3"}


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
    return au.load_golden()


def call(d, form, data_ptr, nbytes, recs_ptr, frame_ptr, recs_cap, source=au.SOURCE, now_ms=au.NOWS[0], pass_bytes=0, size=None, drop=None):
    """The C entry itself -> (rc, dict of the counters)."""
    from readsb_amd import binding
    a, c = au.args_for(binding, (data_ptr, nbytes), source, now_ms, recs_ptr, frame_ptr, recs_cap, pass_bytes)
    if size is not None:
        a.size = size
    if drop:
        setattr(a, drop, None)
    f = d.lib.mgpu_asterix_decode if form == "host" else d.lib.mgpu_asterix_decode_device
    rc = int(f(d.ctx, C.byref(a)))
    return rc, {k: int(v.value) for k, v in c.items()}


def run(d, hip, form, data, recs_cap=None, data_off=0, now_ms=au.NOWS[0], pass_bytes=0, frames=True):
    """One call with every array between canaries -> dict(rc, counters..., recs, frame_of, intact).  Behind the stream lies a record
    that must not count."""
    data = bytes(data)
    if recs_cap is None:
        recs_cap = len(data) // 3 + 1 if len(data) < 30000 else len(data) // 8
    rec_bytes, frame_bytes = (recs_cap + 2 * GUARD) * 128, (recs_cap + 2 * GUARD) * 8
    lo = GUARD * 128
    src = np.frombuffer(b"\xee" * data_off + data + au.frame(ADDR), dtype=np.uint8)
    if form == "host":
        raw = np.full(rec_bytes, 0xA5, dtype=np.uint8)
        fo = np.full(recs_cap + 2 * GUARD, CANARY, dtype=np.uint64)
        rc, n = call(d, form, src.ctypes.data + data_off if data else None, len(data), raw.ctypes.data + lo, fo.ctypes.data + 8 * GUARD if frames else None, recs_cap,
                     now_ms=now_ms, pass_bytes=pass_bytes)
    else:
        d_data = hip.upload(src)
        d_recs, d_fo = hip.malloc(rec_bytes), hip.malloc(frame_bytes)
        hip.fill(d_recs, 0xA5, rec_bytes)
        hip.fill(d_fo, 0xA5, frame_bytes)
        rc, n = call(d, form, d_data + data_off, len(data), d_recs + lo, d_fo + 8 * GUARD if frames else None, recs_cap, now_ms=now_ms)
        raw, fo = hip.download(d_recs, rec_bytes), hip.download(d_fo, frame_bytes, dtype=np.uint64)
        for p in (d_data, d_recs, d_fo):
            hip.free(p)
    nrec = min(n["nrecs"], recs_cap) if rc != au.MGPU_E_INVAL else 0
    nfo = nrec if frames else 0
    intact = (raw[:lo] == 0xA5).all() and (raw[lo + 128 * nrec:] == 0xA5).all() and (fo[:GUARD] == CANARY).all() and (fo[GUARD + nfo:] == CANARY).all()
    return dict(n, rc=rc, recs=raw[lo: lo + 128 * nrec].copy().view(au.REC), frame_of=fo[GUARD: GUARD + nfo].copy(), intact=bool(intact))


COUNTERS = ("consumed", "nframes", "nrecs", "nother", "nundefined", "stop")


def same(res, want, what=None):
    assert res["rc"] == au.MGPU_OK and res["intact"], what
    assert tuple(res[k] for k in COUNTERS) == (want["consumed"], want["nframes"], len(want["recs"]), want["nother"], want["nundefined"], want["stop"]), what
    assert res["recs"].tobytes() == want["recs"].tobytes() and (res["frame_of"] == want["frame_of"]).all(), what


def expected(stream, now_ms=au.NOWS[0]):
    return au.expect(au.load_host_lib(), stream, now_ms=now_ms)


def other(nbytes, cat=48):
    """A frame of another category of exactly nbytes bytes."""
    assert 3 <= nbytes <= 65535
    return bytes([cat]) + au.len_bytes(nbytes) + b"\x5a" * (nbytes - 3)


def fill_to(parts, target):
    """Frames of another category up to the stream position `target`."""
    have = sum(len(p) for p in parts)
    while target - have > 60000:
        parts.append(other(50000))
        have += 50000
    if target > have:
        parts.append(other(target - have))
    assert sum(len(p) for p in parts) == target


PREFIX = [other(30000), other(30001), other(30002)]


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("group", au.GROUPS)
def test_golden_groups(ctx, golden, group, form):
    """Every golden group at both clocks through the C entry of either form, behind 90 003 bytes of other frames so that it crosses
    tile edges: records, frames, every counter, the stop."""
    d, hip = ctx
    stream, by_now = golden[group]
    pre = b"".join(PREFIX)
    for now_ms, (head, frame_of, recs) in by_now.items():
        res = run(d, hip, form, pre + stream, now_ms=now_ms)
        want = dict(consumed=len(pre) + int(head[0]), nframes=3 + int(head[1]), recs=recs, frame_of=frame_of + 3, nother=3 + int(head[3]), nundefined=0, stop=int(head[4]))
        same(res, want, (group, now_ms))
    res = run(d, hip, form, stream)                                                                 # and alone: one tile for (a), (c)
    head, frame_of, recs = by_now[au.NOWS[0]]
    same(res, dict(consumed=int(head[0]), nframes=int(head[1]), recs=recs, frame_of=frame_of, nother=int(head[3]), nundefined=0, stop=int(head[4])), group)


def edge_stream():
    rng = np.random.default_rng(5)
    parts = au.feed(300, seed=11)
    fill_to(parts, TILE - 1)
    parts.append(au.frame({**ADDR, "145": au.be(100, 2)}))                                         # its first byte is the tile's last
    parts += au.feed(200, seed=12)
    fill_to(parts, 2 * TILE - 2)
    parts.append(au.frame({**ADDR, "145": au.be(101, 2)}))                                         # its length bytes straddle the edge
    fill_to(parts, 3 * TILE + 1)
    parts.append(other(65535))                                                                     # 65535 bytes from offset 1: the next starts at 4 * TILE
    assert sum(len(p) for p in parts) == 4 * TILE
    parts.append(au.frame({**ADDR, "170": au.be(0x0c2d35c71c60, 6)}))
    fill_to(parts, 5 * TILE - 21)
    parts.append(b"\x02\x00\x02" + b"\x00\x02" * 20)                                               # frames of length 2 over the edge: 02 00 02 | 02 00 02 | 02 00 02 ..
    parts.append(b"\x00\x09\x01\x10\x01\x02\x03\x04")                                              # .. the last one, 02 00 09, leaves the run
    parts.append(b"\x15\x00\x01" + b"\x01\x10\xaa\xbb\xcc" + b"\0" * (0x101 - 2 - 5))               # a frame of length 1 and the frame inside it
    fill_to(parts, 6 * TILE - 5)
    parts.append(bytes([21]) + au.len_bytes(5) + b"\xff\xfe")                                      # its items lie in the next tile
    parts += au.feed(50, seed=13)
    parts.append(au.frame(au.every_item(rng)))
    return b"".join(parts)


def test_tile_edges_at_every_misalignment(ctx):
    """Records on, over and around tile edges, the device form at every misalignment of the stream, the host form once."""
    d, hip = ctx
    stream = edge_stream()
    want = expected(stream)
    starts, _, _ = au.frames_of(stream)
    assert {TILE - 1, 2 * TILE - 2, 3 * TILE + 1, 4 * TILE, 6 * TILE - 5} <= set(starts) and want["stop"] == au.STOP_END and want["consumed"] == len(stream)
    assert sum(1 for s in starts if 5 * TILE - 21 <= s < 5 * TILE + 21) >= 20 and len(want["recs"]) > 550
    for mis in range(16):
        same(run(d, hip, "device", stream, data_off=mis), want, mis)
    same(run(d, hip, "host", stream, data_off=3), want)
    same(run(d, hip, "device", stream, frames=False), dict(want, frame_of=want["frame_of"][:0]))


def test_a_chain_across_groups(ctx):
    """40 tiles: the chain enters the second group of 32 through the composed map, at an offset that is not 0."""
    d, hip = ctx
    parts = []
    for t in range(1, 40):
        parts += au.feed(3, seed=100 + t)
        fill_to(parts, t * TILE + 7 * t)
    parts += au.feed(20, seed=99)
    stream = b"".join(parts)
    assert len(stream) > (au.GROUP_TILES + 7) * TILE
    same(run(d, hip, "device", stream), expected(stream))


def test_cut_in_two_at_every_byte(ctx):
    """The stream cut at every byte of one record and the bytes around it, the tail carried into a second call: together the result of
    one call.  (Records that do not overrun: the bytes behind a call's data read as 0.)"""
    d, hip = ctx
    parts = au.feed(1500, seed=3)
    fill_to(parts, 3 * TILE + 11)
    parts += au.feed(1500, seed=4)
    stream = b"".join(parts)
    whole = run(d, hip, "device", stream)
    same(whole, expected(stream))
    starts, _, _ = au.frames_of(stream)
    k = next(i for i, s in enumerate(starts) if s > 3 * TILE + 200)                                # a drawn record in the fourth tile
    assert starts[k + 1] - starts[k] < 100
    for cut in range(starts[k] - 3, starts[k + 1] + 4):
        one = run(d, hip, "device", stream[:cut])
        two = run(d, hip, "device", stream[one["consumed"]:])
        assert one["rc"] == two["rc"] == au.MGPU_OK and one["intact"] and two["intact"] and one["stop"] == au.STOP_END
        assert one["consumed"] == max(s for s in starts + [len(stream)] if s <= cut) and one["consumed"] + two["consumed"] == len(stream)
        assert one["nframes"] + two["nframes"] == whole["nframes"] and one["recs"].tobytes() + two["recs"].tobytes() == whole["recs"].tobytes(), cut
        assert (np.concatenate([one["frame_of"], two["frame_of"] + one["nframes"]]) == whole["frame_of"]).all(), cut


@pytest.mark.parametrize("kind", ["random", "ff", "chains"])
def test_hostile_tiles(ctx, kind):
    """Four tiles of uniformly random bytes, of 0xFF, and of category-21 frames whose FSPEC never ends (undefined: no record)."""
    d, hip = ctx
    if kind == "random":
        stream = np.random.default_rng(77).integers(0, 256, 4 * TILE, dtype=np.uint8).tobytes()
    elif kind == "ff":
        stream = b"\xff" * (4 * TILE)
    else:
        stream = b"".join(bytes([21]) + au.len_bytes(n) + b"\xff" * (n - 3) for n in (5000, 60000, 197, 65535, 300, 70000 - 65535, 40000, 30000, 3000))
        stream += au.frame(ADDR) + bytes([21]) + au.len_bytes(198) + b"\xff" * 195
    want = expected(stream)
    if kind == "chains":
        assert want["nundefined"] == 10 and len(want["recs"]) == 1
    for form in ("device", "host"):
        same(run(d, hip, form, stream), want, (kind, form))


def stop_streams():
    body = au.feed(2500, seed=21)
    closed = au.frame({"145": au.be(77, 2)})
    out = {}
    for name, bad in (("zero", b"\x15\x00\x00\x01\x10"), ("closed", closed)):
        out[name + "_start"] = bad + b"".join(body[:2000])
        out[name + "_middle"] = b"".join(body[:1800]) + bad + b"".join(body[1800:])
        out[name + "_last"] = b"".join(body) + bad
    for name, bad in (("end", au.frame(ADDR)[:-1]), ("end2", b"\x15\x00"), ("end3", other(65535)[:40000])):   # (the end is the end: no middle)
        out[name + "_start"] = bad
        out[name + "_last"] = b"".join(body) + bad
    out["exact_end"] = b"".join(body)
    parts = body[:100]
    fill_to(parts, 2 * TILE)                                                                       # the chain ends AT a tile's first byte, behind the stream
    out["tile_end"] = b"".join(parts)
    return out


def test_each_stop(ctx):
    """A length of 0, a record without an address, a record that does not fit and a header that does not, at the stream's start, in
    its middle (nothing behind it is framed) and in its last frame."""
    d, hip = ctx
    for name, stream in stop_streams().items():
        want = expected(stream)
        kind = {"zero": au.STOP_ZERO_LEN, "closed": au.STOP_CLOSED}.get(name.split("_")[0], au.STOP_END)
        assert want["stop"] == kind, name
        if name.endswith("_start") and kind != au.STOP_CLOSED:
            assert want["consumed"] == 0 and want["nframes"] == 0
        for form in ("device", "host"):
            same(run(d, hip, form, stream), want, (name, form))


def test_capacities_exact_and_one_short(ctx):
    d, hip = ctx
    stream = b"".join(PREFIX + au.feed(2000, seed=31))
    want = expected(stream)
    n = len(want["recs"])
    for form in ("device", "host"):
        same(run(d, hip, form, stream, recs_cap=n), want, form)
        for cap in (n - 1, 1, 0):
            res = run(d, hip, form, stream, recs_cap=cap)
            assert res["rc"] == au.MGPU_E_OVERFLOW and res["intact"] and res["nrecs"] == n and res["nframes"] == want["nframes"], (form, cap)
            assert res["recs"].tobytes() == want["recs"][:cap].tobytes() and (res["frame_of"] == want["frame_of"][:cap]).all()


def test_bad_arguments_and_the_empty_call(ctx):
    d, hip = ctx
    from readsb_amd import binding
    stream = b"".join(au.feed(10))
    src = np.frombuffer(stream, dtype=np.uint8)
    recs = np.zeros(16, dtype=au.REC)
    d_data, d_recs = hip.upload(src), hip.malloc(16 * 128 + 16)
    for form, data, out in (("host", src.ctypes.data, recs.ctypes.data), ("device", d_data, d_recs)):
        assert call(d, form, data, len(stream), out, None, 16)[0] == au.MGPU_OK
        assert call(d, form, data, len(stream), out, None, 16, size=C.sizeof(binding.AsterixInArgs) - 8)[0] == au.MGPU_E_INVAL
        assert call(d, form, None, len(stream), out, None, 16)[0] == au.MGPU_E_INVAL
        assert call(d, form, data, len(stream), None, None, 16)[0] == au.MGPU_E_INVAL
        assert call(d, form, data, len(stream), out, None, 16, source=12)[0] == au.MGPU_E_INVAL
        assert call(d, form, data, len(stream), out, None, 16, source=11)[0] == au.MGPU_OK
        assert call(d, form, data, len(stream), out, None, 16, now_ms=-1)[0] == au.MGPU_E_INVAL
        assert call(d, form, data, len(stream), out, None, 16, now_ms=253402300800000)[0] == au.MGPU_E_INVAL
        for name in ("consumed", "nframes", "nrecs", "stop"):
            assert call(d, form, data, len(stream), out, None, 16, drop=name)[0] == au.MGPU_E_INVAL, name
        for name in ("nother", "nundefined"):
            assert call(d, form, data, len(stream), out, None, 16, drop=name)[0] == au.MGPU_OK, name
        rc, n = call(d, form, data, 0, out, None, 16)
        assert rc == au.MGPU_OK and n == dict(consumed=0, nframes=0, nrecs=0, stop=0, nother=0, nundefined=0)
        assert call(d, form, None, 0, None, None, 0)[0] == au.MGPU_OK
    assert call(d, "device", d_data, len(stream), d_recs + 8, None, 15)[0] == au.MGPU_E_INVAL          # recs 16-byte aligned
    assert call(d, "device", d_data, len(stream), d_recs, d_recs + 4, 1)[0] == au.MGPU_E_INVAL         # frame_of 8-byte aligned
    assert d.lib.mgpu_asterix_decode(None, None) == au.MGPU_E_INVAL


def test_host_passes_against_one_device_call(ctx, golden):
    """The host form staging 1, 250, 65535, 65536 and 200000 bytes per pass (a pass grows until a record fits, and carries its tail)
    against one device call, on the hostile group, whose items overrun their records."""
    d, hip = ctx
    stream = b"".join(PREFIX) + golden["b"][0] + b"".join(au.feed(1000, seed=41)) + golden["b"][0]
    whole = run(d, hip, "device", stream)
    same(whole, expected(stream))
    for pass_bytes in (1, 250, 65535, 65536, 200000):
        res = run(d, hip, "host", stream, pass_bytes=pass_bytes)
        same(res, dict(whole, recs=whole["recs"], nframes=whole["nframes"]), pass_bytes)


def test_time_values_against_the_host_parser(ctx):
    """65 536 I021/071 values: every multiple of 16 in a range (where raw / .128 is a whole number) and drawn ones, at a clock just
    behind midnight."""
    d, hip = ctx
    rng = np.random.default_rng(71)
    raws = np.concatenate([np.arange(0xa80000, 0xa80000 + 16 * 32768, 16), rng.integers(0, 1 << 24, 32768)])
    assert len(raws) == 65536
    head = bytes([21]) + au.len_bytes(11) + b"\x09\x10"
    stream = b"".join(head + au.be(int(r), 3) + b"\x4a\xc8\xb3" for r in raws)
    now_ms = au.NOWS[1]
    res = run(d, hip, "device", stream, now_ms=now_ms)
    same(res, expected(stream, now_ms=now_ms))
    assert len(res["recs"]) == 65536 and len(set(res["recs"]["sysTimestamp"].tolist())) > 60000


def test_round_trip_through_the_asterix_writer(ctx):
    """A short synthetic capture's message list through the existing mgpu_asterix_encode_ex, those records through the new decoder:
    the records equal the host parser's; the address and the I021/130 position are what the writer was given (DESIGN.md says which
    other members survive)."""
    d, hip = ctx
    from readsb_amd import binding
    iq = helpers.synth(seconds=2.0, seed=7)
    msgs, _ = d.demodulate_capture(iq)
    fields = d.decode_fields(msgs)
    rng = np.random.default_rng(9)
    pos = np.zeros(len(msgs), dtype=binding.POSITION_DTYPE)
    pos["lat"], pos["lon"], pos["method"] = rng.uniform(-89, 89, len(msgs)), rng.uniform(-179, 179, len(msgs)), 1
    now_ms = au.NOWS[0]
    msgs = msgs.copy()
    msgs["sysTimestamp"] = now_ms - 100
    stream, deferred, skipped = d.asterix_encode(msgs, now_ms, fields=fields, positions=pos)
    assert len(deferred) == 0 and skipped == 0
    res = run(d, hip, "device", stream, now_ms=now_ms)
    want = expected(stream, now_ms=now_ms)
    same(res, want)
    r = res["recs"]
    assert len(r) == len(msgs) > 100 and res["nframes"] == len(msgs) and res["consumed"] == len(stream)
    assert ((r["addr"] & 0xffffff) == (fields["addr"] & 0xffffff)).all()
    lsb = 180.0 / (1 << 23)
    assert (r["ast_flags"] & binding.AST_POS_VALID).all()
    assert (r["decoded_lat"] == np.trunc(pos["lat"] / lsb) * lsb).all() and (r["decoded_lon"] == np.trunc(pos["lon"] / lsb) * lsb).all()


def test_command_line_against_the_library(ctx, golden):
    """readsb_gpu_asterix_in as a child process equals the library, with a block smaller than the stream so that tails are carried
    between calls; --stats prints the counts; it stops where the stop is not the stream's end."""
    d, hip = ctx
    feed = b"".join(au.feed(3000, seed=51))
    for stream, block in ((feed, 4096), (feed + b"\x15\x00", 100000), (golden["c1"][0], 300), (feed[:5000] + b"\x15\x00\x00" + feed[5000:], 1 << 20)):
        lib = d.asterix_decode(stream, source=au.SOURCE, now_ms=au.NOWS[0])
        want = expected(stream)
        assert lib["recs"].tobytes() == want["recs"].tobytes() and lib["stop"] == want["stop"] and lib["consumed"] == want["consumed"]
        r = subprocess.run([CLI, "--source", str(au.SOURCE), "--now", str(au.NOWS[0]), "--block", str(block)], input=stream, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr[-500:]
        assert r.stdout == lib["recs"].tobytes()
        r = subprocess.run([CLI, "--source", str(au.SOURCE), "--now", str(au.NOWS[0]), "--block", str(block), "--stats"], input=stream, capture_output=True, timeout=120)
        assert r.returncode == 0 and r.stdout.decode().split() == ["frames", str(want["nframes"]), "records", str(len(want["recs"])), "other", str(want["nother"]),
                                                                    "undefined", str(want["nundefined"]), "bytes", str(want["consumed"]), "stop", str(want["stop"])], r.stdout
