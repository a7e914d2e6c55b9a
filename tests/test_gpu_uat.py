"""-m gpu: UAT input on the device (kernels/uat.inc, mgpu_uat_encode / mgpu_uat_encode_device): the AVR lines, the counters, the
records, the signal bytes, the source lines and the deferred list compared with == against the bytes the reference's uat2esnt
printed (tests/golden/uat_cases.npz, which tests/test_uat_reference.py holds to the live reference on the CPU).

Shapes: a tile is 8192 bytes of text, a lane takes the lines that start in 32 of them, the halo is 256 bytes, a load 16 bytes.  The
golden groups are 8 KB to 177 KB (1 to 22 tiles); the cutting stream is about 4 000 lines (50 tiles); the tile-edge streams put a
line's first byte on a tile's last byte and a '\\n' on a tile's first, at every misalignment class of the text and the output."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import beast_util as bu
import fields_util as fu
import helpers
import uat_util as uu

pytestmark = pytest.mark.gpu

GUARD = 256
NOW_MS = 1700000000123
CLI = os.path.join(helpers.ROOT, "readsb_amd", "host", "readsb_gpu_uat2esnt")


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
    return uu.load_golden()


def call(d, form, text_ptr, nbytes, out_ptr, cap, msgs_ptr=None, sig_ptr=None, line_ptr=None, msgs_cap=0, deferred_cap=0, pass_bytes=0):
    """The C entry itself -> (rc, dict of the counters, the deferred list as far as it was written)."""
    from readsb_amd import binding
    c = [C.c_uint64(0xDEAD) for _ in range(6)]
    deferred = np.full(deferred_cap + 4, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    a = binding.UatArgs(C.sizeof(binding.UatArgs), 0, text_ptr, nbytes, out_ptr, cap, msgs_ptr, sig_ptr, line_ptr, msgs_cap,
                        deferred.ctypes.data if deferred_cap else None, deferred_cap, NOW_MS, *[C.pointer(x) for x in c], pass_bytes)
    f = d.lib.mgpu_uat_encode if form == "host" else d.lib.mgpu_uat_encode_device
    rc = int(f(d.ctx, C.byref(a)))
    names = ("bytes", "consumed", "nlines", "nframes", "nshort", "ndeferred")
    n = dict(zip(names, (int(x.value) for x in c)))
    assert (deferred[deferred_cap:] == 0xA5A5A5A5A5A5A5A5).all(), "a deferred index beyond the list's capacity"
    return rc, n, deferred[: min(n["ndeferred"], deferred_cap)]


def run(d, hip, form, text, cap=None, msgs_cap=None, deferred_cap=None, text_off=0, out_off=0, pass_bytes=0):
    """One call with every optional array, between canaries -> dict(rc, counters..., text, msgs, sig, line_of, deferred, intact)."""
    from readsb_amd import binding
    text = bytes(text)
    most = len(text) * 4 // 37 + 4
    cap = most * uu.FRAME_TEXT if cap is None else cap
    msgs_cap = most if msgs_cap is None else msgs_cap
    deferred_cap = len(text) // 14 + 1 if deferred_cap is None else deferred_cap
    if form == "host":
        src = np.frombuffer(b"\0" * text_off + text, dtype=np.uint8)
        out = np.full(GUARD + out_off + cap + GUARD, 0xA5, dtype=np.uint8)
        msgs = np.frombuffer(b"\xa5" * ((msgs_cap + 2) * 64), dtype=binding.MSG_DTYPE).copy()
        sig = np.full(msgs_cap + GUARD, 0xA5, dtype=np.uint8)
        line_of = np.full(msgs_cap + 4, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        rc, n, deferred = call(d, form, src.ctypes.data + text_off if text else None, len(text), out.ctypes.data + GUARD + out_off, cap, msgs.ctypes.data, sig.ctypes.data,
                               line_of.ctypes.data, msgs_cap, deferred_cap, pass_bytes)
    else:
        d_text = hip.upload(np.frombuffer(b"\0" * text_off + text + b"\n-" * 64, dtype=np.uint8))     # (lines behind the text: nothing beyond nbytes may count)
        d_out, d_msgs, d_sig, d_line = hip.malloc(GUARD + out_off + cap + GUARD), hip.malloc((msgs_cap + 2) * 64), hip.malloc(msgs_cap + GUARD), hip.malloc((msgs_cap + 4) * 8)
        for p, size in ((d_out, GUARD + out_off + cap + GUARD), (d_msgs, (msgs_cap + 2) * 64), (d_sig, msgs_cap + GUARD), (d_line, (msgs_cap + 4) * 8)):
            hip.fill(p, 0xA5, size)
        rc, n, deferred = call(d, form, d_text + text_off, len(text), d_out + GUARD + out_off, cap, d_msgs, d_sig, d_line, msgs_cap, deferred_cap)
        out = hip.download(d_out, GUARD + out_off + cap + GUARD)
        msgs = hip.download(d_msgs, (msgs_cap + 2) * 64, dtype=binding.MSG_DTYPE)
        sig = hip.download(d_sig, msgs_cap + GUARD)
        line_of = hip.download(d_line, (msgs_cap + 4) * 8, dtype=np.uint64)
        for p in (d_text, d_out, d_msgs, d_sig, d_line):
            hip.free(p)
    lo = GUARD + out_off
    wrote, nrec = min(n["bytes"], cap), min(n["nframes"], msgs_cap)
    intact = (out[:lo] == 0xA5).all() and (out[lo + wrote:] == 0xA5).all() and msgs[nrec:].tobytes() == b"\xa5" * ((msgs_cap + 2 - nrec) * 64) \
        and (sig[nrec:] == 0xA5).all() and (line_of[nrec:] == 0xA5A5A5A5A5A5A5A5).all()
    return dict(n, rc=rc, text=out[lo: lo + wrote].tobytes(), msgs=msgs[:nrec], sig=sig[:nrec], line_of=line_of[:nrec], deferred=deferred, intact=bool(intact))


def check_records(res, text=None):
    """Every record is what decodeHexMessage + decodeModesMessage leave for its line of the text."""
    sig, frames = uu.frames_of(res["text"] if text is None else text)
    m = res["msgs"]
    assert len(m) == len(frames) and (res["sig"] == sig).all()
    assert (m["msg"] == frames).all() and (m["raw"] == frames).all()
    assert (m["timestamp"] == uu.UAT_TIMESTAMP).all() and (m["sysTimestamp"] == NOW_MS).all() and (m["msgtype"] == 18).all() and (m["msgbits"] == 112).all()
    assert not m["correctedbits"].any() and not m["score"].any() and not m["phase"].any() and (m["sig_len"] == 1).all()
    assert (m["sig_sumsq"] == (257 * sig.astype(np.uint64)) ** 2).all()
    assert (m["addr"] == (frames[:, 1].astype(np.uint32) << 16 | frames[:, 2].astype(np.uint32) << 8 | frames[:, 3])).all()


def check_decode(d, msgs, text):
    """mgpu_decode_fields of the records equals the project's oracle on the same frames, and equals the decode of the same frames in
    records as the demodulator leaves them (an existing DF18 path); the beast encoder's signal byte of every record is the line's."""
    from readsb_amd import binding
    sig, frames = uu.frames_of(text)
    assert len(msgs) == len(frames) and len(frames)
    fields = d.decode_fields(msgs)
    want = fu.oracle_fields(np.ascontiguousarray(frames), np.full(len(frames), 112, dtype=np.int32))
    assert fields.tobytes() == want.tobytes()
    plain = np.zeros(len(frames), dtype=binding.MSG_DTYPE)
    plain["msg"], plain["raw"], plain["msgbits"], plain["msgtype"], plain["sig_len"], plain["sig_sumsq"] = frames, frames, 112, 18, 268, 1 << 20
    plain["timestamp"], plain["addr"] = 12345, msgs["addr"]
    assert d.decode_fields(plain).tobytes() == fields.tobytes()
    beast = helpers.beast_frames(d.beast_encode(msgs))
    assert len(beast) == len(frames) and [b[3] for b in beast] == sig.tolist() and all(b[2] == uu.UAT_TIMESTAMP for b in beast)


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("group", uu.GROUPS)
def test_golden_groups(ctx, golden, group, form):
    """Every golden group through the C entry of either form: text, counters, records, signal bytes, source lines, the deferred list;
    every record through mgpu_decode_fields and the beast encoder (check_decode) — for group (f) the records the host formatter
    settles the deferred lines to."""
    d, hip = ctx
    from readsb_amd import binding
    stream, out, lens = golden[group]
    deferred = list(range(len(lens))) if group == "f" else []
    want_text, want_line_of = uu.expected(out, lens, deferred)
    res = run(d, hip, form, stream)
    assert res["rc"] == uu.MGPU_OK and res["intact"]
    assert (res["bytes"], res["consumed"], res["nlines"], res["nframes"], res["nshort"], res["ndeferred"]) == \
        (len(want_text), len(stream), len(lens), len(want_text) // uu.FRAME_TEXT, 0, len(deferred))
    assert res["text"] == want_text and (res["line_of"] == want_line_of).all() and res["deferred"].tolist() == deferred
    check_records(res)
    if not deferred:
        check_decode(d, res["msgs"], res["text"])
        return
    # the host formatter settles the listed lines to the reference's bytes, and their records are the text's
    src = np.frombuffer(stream, dtype=np.uint8)
    a = binding.UatArgs(C.sizeof(binding.UatArgs), 0, src.ctypes.data, src.size)
    a.now_ms = NOW_MS
    buf, recs, sig = np.empty(4 * uu.FRAME_TEXT, dtype=np.uint8), np.zeros(4, dtype=binding.MSG_DTYPE), C.c_uint8(0)
    settled, msgs, sigs = {}, [], []
    for k in res["deferred"].tolist():
        n = int(d.lib.mgpu_uat_format_host(C.byref(a), k, buf.ctypes.data, buf.size, recs.ctypes.data, C.addressof(sig)))
        assert n == int(lens[k])
        settled[k] = buf[:n].tobytes()
        msgs.append(recs[: n // uu.FRAME_TEXT].copy())
        sigs += [sig.value] * (n // uu.FRAME_TEXT)
    assert uu.merge_deferred(res["text"], res["line_of"], settled) == out
    both = dict(text=out, msgs=np.concatenate(msgs), sig=np.array(sigs, dtype=np.uint8))
    check_records(both)
    check_decode(d, both["msgs"], out)


def test_binding_settles(ctx, golden):
    """Demodulator.uat_encode over groups (a) and (f): the reference's bytes with the deferred lines in place, their records too."""
    d, hip = ctx
    for g in ("a", "f"):
        stream, out, lens = golden[g]
        res = d.uat_encode(stream, now_ms=NOW_MS)
        assert res["text"] == out and res["consumed"] == len(stream) and res["nlines"] == len(lens)
        assert (res["line_of"] == np.repeat(np.arange(len(lens)), lens // uu.FRAME_TEXT)).all()
        check_records(res)
        check_decode(d, res["msgs"], out)


@pytest.mark.parametrize("form", ["host", "device"])
def test_dense_short_lines(ctx, form):
    """Lines of MDB types 11-31 with 4 payload bytes are 11 bytes long and give one frame each: up to three frame-giving lines start in
    one lane's 32 bytes, and a tile gives 745 frames.  Several tiles of them, then mixed with 37-byte lines (type 0, 17 payload bytes,
    three frames: the densest text there is) and empty lines, at two alignments."""
    d, hip = ctx
    rng = np.random.default_rng(31)
    short = [uu.line(uu.payload(11 + int(rng.integers(0, 21)), int(rng.integers(0, 8)), addr=1 + int(rng.integers(0, 0xFFFFFF)), nbytes=4), extra="") for _ in range(2600)]
    assert all(len(x) == 11 for x in short)
    dense = [uu.line(uu.payload(0, 0, addr=1 + k, raw_a=0x0C8 + k, nbytes=17), extra="") for k in range(700)]
    assert all(len(x) == 37 for x in dense)
    mixed = []
    for k in range(900):
        mixed += [short[k], dense[k % 700]] + ([b"\n"] if k % 5 == 0 else []) + ([short[k + 900]] * (k % 3))
    for lines in (short, dense, mixed):
        stream = b"".join(lines)
        assert len(stream) > 3 * uu.TILE
        ref = stream_expected(stream)
        assert len(ref[1]) >= len(lines) - 200
        for text_off, out_off in ((0, 0), (5, 11)):
            res = run(d, hip, form, stream, text_off=text_off, out_off=out_off)
            assert res["rc"] == uu.MGPU_OK and res["intact"] and res["nshort"] == 0 and res["ndeferred"] == 0
            assert res["text"] == ref[0] and (res["line_of"] == ref[1]).all() and res["nlines"] == len(lines)
            check_records(res)
    check_decode(d, res["msgs"], res["text"])


def test_cut_at_every_carry_point(ctx):
    """A stream of about 4 000 lines cut in two at every byte of a small window, the unconsumed rest carried into the second call,
    gives the bytes of one call: this is `consumed`.  Both forms; the host form in passes smaller than the stream, too."""
    d, hip = ctx
    lines = uu.feed(4000, seed=3)
    stream = b"".join(lines)
    whole = run(d, hip, "device", stream)
    assert whole["rc"] == uu.MGPU_OK and whole["intact"] and whole["consumed"] == len(stream) and whole["nlines"] == len(lines) and whole["nframes"] > 8000
    check_records(whole)
    ends = np.cumsum([len(x) for x in lines])
    lo = int(ends[1999]) - 150                                   # the window holds three line ends
    d_text = hip.upload(np.frombuffer(stream, dtype=np.uint8))
    cap = len(whole["text"])
    d_out = hip.malloc(cap + GUARD)
    for cut in range(lo, lo + 300):
        hip.fill(d_out, 0xA5, cap + GUARD)
        rc, n1, _ = call(d, "device", d_text, cut, d_out, cap)
        want_consumed = int(ends[ends <= cut].max())
        assert rc == uu.MGPU_OK and n1["consumed"] == want_consumed and n1["nlines"] == int((ends <= cut).sum()), cut
        rc, n2, _ = call(d, "device", d_text + n1["consumed"], len(stream) - n1["consumed"], d_out + n1["bytes"], cap - n1["bytes"])
        assert rc == uu.MGPU_OK and n1["bytes"] + n2["bytes"] == cap and n1["nlines"] + n2["nlines"] == len(lines), cut
        got = hip.download(d_out, cap + GUARD)
        assert got[:cap].tobytes() == whole["text"] and (got[cap:] == 0xA5).all(), cut
    hip.free(d_text)
    hip.free(d_out)
    for pass_bytes in (1, 300, 8191, 100000):                    # (1: every pass grows until it holds a line)
        part = stream[: 40000 if pass_bytes == 1 else len(stream)] + b"-tail without a newline"
        res = run(d, hip, "host", part, pass_bytes=pass_bytes)
        one = run(d, hip, "device", part)
        assert res["rc"] == uu.MGPU_OK and res["intact"] and res["consumed"] == one["consumed"] == part.rfind(b"\n") + 1
        assert res["text"] == one["text"] and (res["line_of"] == one["line_of"]).all() and res["msgs"].tobytes() == one["msgs"].tobytes(), pass_bytes


@pytest.mark.parametrize("form", ["host", "device"])
def test_tile_edges(ctx, form):
    """More than three tiles.  In one copy a line's first byte is a tile's last byte, in the other its '\\n' before it is the next
    tile's first byte; both at every alignment class of the text and of the output, both with a line that reaches 256 bytes."""
    d, hip = ctx
    lines = uu.feed(400, seed=5)
    long_line = uu.line(uu.payload(1, 0), extra="rssi=-12.3;t=" + "7" * 172 + ";")
    assert len(long_line) - 1 == uu.DEV_LINE_MAX
    for first in (uu.TILE - 1, uu.TILE + 1, 2 * uu.TILE - 1, 2 * uu.TILE + 1):          # where the crafted line starts (the '\n' before it is at first - 1)
        for special in (lines[7], long_line):
            head, at = [], 0
            for x in lines:
                if at + len(x) > first - 40:
                    break
                head.append(x)
                at += len(x)
            pad = b"#" * (first - at - 1) + b"\n"                                        # a comment line that ends right before `first`
            stream = b"".join(head) + pad + special + b"".join(lines[len(head):])
            assert stream[first - 1: first + 1] == b"\n-" and len(stream) > 3 * uu.TILE
            ref = stream_expected(stream)
            for text_off, out_off in ((0, 0), (1, 3), (7, 8), (15, 15)):
                res = run(d, hip, form, stream, text_off=text_off, out_off=out_off)
                assert res["rc"] == uu.MGPU_OK and res["intact"], (first, text_off)
                assert res["text"] == ref[0] and (res["line_of"] == ref[1]).all() and res["nlines"] == stream.count(b"\n"), (first, text_off)


def stream_expected(stream):
    """(text, line_of) of a stream without deferred lines, by the host formatter of the library (which the CPU tests hold to the reference)."""
    import readsb_amd
    lib = readsb_amd.load_library()
    buf = np.empty(4 * uu.FRAME_TEXT, dtype=np.uint8)
    parts, line_of = [], []
    for k, x in enumerate(uu.split_lines(stream)):
        src = np.frombuffer(x, dtype=np.uint8)
        n = int(lib.mgpu_uat_format_line_host(src.ctypes.data if len(x) else None, len(x), NOW_MS, buf.ctypes.data, buf.size, None, None))
        assert n >= 0
        parts.append(buf[:n].tobytes())
        line_of += [k] * (n // uu.FRAME_TEXT)
    return b"".join(parts), np.array(line_of, dtype=np.uint64)


@pytest.mark.parametrize("form", ["host", "device"])
def test_no_newline_and_empty_and_short(ctx, form):
    d, hip = ctx
    body = uu.line(uu.payload(1, 0))[:-1]
    for text in (body, body * 200, b"-", b""):                   # nothing is consumed, nothing written
        res = run(d, hip, form, text)
        assert (res["rc"], res["bytes"], res["consumed"], res["nlines"], res["nframes"], res["nshort"], res["ndeferred"], res["intact"]) == (uu.MGPU_OK, 0, 0, 0, 0, 0, 0, True)
    # short payloads: counted, no frame; the same line one byte longer is taken
    lines = []
    for t in range(32):
        lines += [uu.line(uu.payload(t, 0, nbytes=uu.NEEDED[t] - 1)), uu.line(uu.payload(t, 0, nbytes=uu.NEEDED[t])), b"-;\n"]
    stream = b"".join(lines)
    ref = stream_expected(stream)
    res = run(d, hip, form, stream)
    assert res["rc"] == uu.MGPU_OK and res["intact"] and res["nshort"] == 64 and res["text"] == ref[0] and (res["line_of"] == ref[1]).all()
    assert set((res["line_of"] % 3).tolist()) == {1}


@pytest.mark.parametrize("form", ["host", "device"])
def test_capacities_one_short(ctx, golden, form):
    d, hip = ctx
    stream = golden["a"][0] + golden["f"][0]
    full = run(d, hip, form, stream)
    assert full["rc"] == uu.MGPU_OK and full["ndeferred"] == len(golden["f"][2])
    need = (full["bytes"], full["nframes"], full["ndeferred"])
    exact = run(d, hip, form, stream, cap=need[0], msgs_cap=need[1], deferred_cap=need[2])
    assert exact["rc"] == uu.MGPU_OK and exact["intact"] and exact["text"] == full["text"] and exact["deferred"].tolist() == full["deferred"].tolist()
    for kw in (dict(cap=need[0] - 1), dict(msgs_cap=need[1] - 1), dict(deferred_cap=need[2] - 1), dict(cap=0, msgs_cap=0, deferred_cap=0)):
        res = run(d, hip, form, stream, **{**dict(cap=need[0], msgs_cap=need[1], deferred_cap=need[2]), **kw})
        assert res["rc"] == uu.MGPU_E_OVERFLOW and res["intact"], kw
        assert (res["bytes"], res["nframes"], res["ndeferred"]) == need, kw
        assert res["text"] == full["text"][: len(res["text"])] and res["msgs"].tobytes() == full["msgs"][: len(res["msgs"])].tobytes()
    # bad arguments with a live context
    buf = np.zeros(4096, dtype=np.uint8)
    assert call(d, form, buf.ctypes.data, 1000, buf.ctypes.data + 500, 1000)[0] == uu.MGPU_E_INVAL        # out overlaps text
    assert call(d, form, None, 10, buf.ctypes.data, 100)[0] == uu.MGPU_E_INVAL


def test_command_line_against_the_golden(built, golden):
    """readsb_gpu_uat2esnt as a child process: every golden stream in, the reference's bytes out, with a block smaller than the
    stream so that lines are carried between calls; a last line without '\\n' gives nothing."""
    for g, block in (("a", 4096), ("b", 60000), ("f", 700), ("e", 1 << 20)):
        stream, out, _ = golden[g]
        r = subprocess.run([CLI, "--block", str(block)], input=stream + b"-00", capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr[-500:]
        assert r.stdout == out, g
