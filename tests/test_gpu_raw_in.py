"""-m gpu: raw input on the device (kernels/raw_in.inc, mgpu_raw_decode / mgpu_raw_decode_device): the accepted messages, their source
lines, the signal doubles' bit patterns, the class of every line and the counters compared with == on bytes against what the
reference's readAscii + processHexMessage left (tests/golden/raw_in_cases.npz, which tests/test_raw_in_reference.py holds to the live
reference on the CPU) and, for built streams, against the library's sequential resolver (which the same CPU tests hold to the
reference).

Shapes: a tile is 8192 bytes of text, a lane takes the lines that start in 32 of them, the halo is 256 bytes, a load 16 bytes; the
passes over the candidates run in workgroups of 256.  The golden groups are 40 to 60 KB (5 to 7 tiles, 1 100 to 1 800 candidates);
the tile-edge streams are three tiles at every misalignment of the text."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import beast_util as bu
import filter_util
import frames_util as fr
import helpers
import raw_in_util as ru

pytestmark = pytest.mark.gpu

GUARD = 4                                        # records, line indices, doubles in front of and behind every array
CANARY = 0xA5A5A5A5A5A5A5A5
EXTERNAL = 2                                     # MGPU_FILTER_CLOCK_EXTERNAL: the filter starts empty, as the harness's does
CLI = os.path.join(helpers.ROOT, "readsb_amd", "host", "readsb_gpu_raw_in")
TAIL = b"*8D4840D6202CC371C32CE0576098;"         # bytes behind the last terminator: nothing of them may count


@pytest.fixture(scope="module")
def ctxs(built):
    import readsb_amd
    hip = bu.Hip()
    made = {}

    def get(cfg):
        if cfg not in made:
            made[cfg] = readsb_amd.Demodulator(nfix_crc=cfg[0], fix_df=cfg[1], mode_ac=cfg[2], startup_time_ms=helpers.STARTUP_MS, max_samples=131072, filter_clock=EXTERNAL)
        made[cfg].reset()
        return made[cfg]
    try:
        yield get, hip
    finally:
        hip.free_all()
        for d in made.values():
            d.close()


@pytest.fixture(scope="module")
def golden():
    return ru.load_golden()


def prepare(d, ops):
    for op in ops:
        d.filter_expire() if op < 0 else d.filter_add(op)


def call(d, form, text_ptr, nbytes, msgs_ptr, line_ptr, sig_ptr, msgs_cap, cls_ptr=None, cls_cap=0, pass_bytes=0, size=None, counters=True, now_ms=ru.NOW_MS):
    """The C entry itself -> (rc, dict of the counts, the seven counters)."""
    from readsb_amd import binding
    c = [C.c_uint64(0xDEAD) for _ in range(3)]
    cn = binding.RawInCounters()
    a = binding.RawInArgs(C.sizeof(binding.RawInArgs) if size is None else size, 0, text_ptr, nbytes, now_ms, msgs_ptr, line_ptr, sig_ptr, msgs_cap, cls_ptr, cls_cap,
                          *([C.pointer(x) for x in c] if counters else [None] * 3), C.pointer(cn) if counters else None, pass_bytes)
    f = d.lib.mgpu_raw_decode if form == "host" else d.lib.mgpu_raw_decode_device
    rc = int(f(d.ctx, C.byref(a)))
    n = dict(zip(("consumed", "nlines", "nmsgs"), (int(x.value) for x in c)))
    n["counters"] = [int(cn.remote_received_modes), int(cn.remote_received_modeac), int(cn.remote_rejected_unknown_icao), int(cn.remote_rejected_bad), *[int(x) for x in cn.remote_accepted]]
    return rc, n


def run(d, hip, form, text, msgs_cap=None, cls_cap=None, text_off=0, msgs_off=0, pass_bytes=0):
    """One call with every array between canaries -> dict(rc, counts, msgs, line_of, signal (as uint64), cls, intact).  msgs_off: 0 or
    8, the records' place modulo 16."""
    text = bytes(text)
    most = len(text) // 6 + 1
    nl = text.count(b"\n") + text.count(b"\0")
    msgs_cap = most if msgs_cap is None else msgs_cap
    cls_cap = nl if cls_cap is None else cls_cap
    rec_bytes, word_bytes, cls_bytes = (msgs_cap + 2 * GUARD) * 64 + 16, (msgs_cap + 2 * GUARD) * 8, cls_cap + 2 * 16
    lo = GUARD * 64 + msgs_off
    src = np.frombuffer(b"\n" * text_off + text + TAIL, dtype=np.uint8)
    if form == "host":
        raw = np.full(rec_bytes, 0xA5, dtype=np.uint8)
        lines, sig = np.full(msgs_cap + 2 * GUARD, CANARY, dtype=np.uint64), np.full(msgs_cap + 2 * GUARD, CANARY, dtype=np.uint64)
        cls = np.full(cls_bytes, 0xA5, dtype=np.uint8)
        rc, n = call(d, form, src.ctypes.data + text_off if text else None, len(text), raw.ctypes.data + lo, lines.ctypes.data + 8 * GUARD, sig.ctypes.data + 8 * GUARD, msgs_cap,
                     cls.ctypes.data + 16, cls_cap, pass_bytes)
    else:
        d_text = hip.upload(src)
        d_recs, d_lines, d_sig, d_cls = hip.malloc(rec_bytes), hip.malloc(word_bytes), hip.malloc(word_bytes), hip.malloc(cls_bytes)
        for p, nb in ((d_recs, rec_bytes), (d_lines, word_bytes), (d_sig, word_bytes), (d_cls, cls_bytes)):
            hip.fill(p, 0xA5, nb)
        rc, n = call(d, form, d_text + text_off, len(text), d_recs + lo, d_lines + 8 * GUARD, d_sig + 8 * GUARD, msgs_cap, d_cls + 16, cls_cap)
        raw, lines, sig, cls = hip.download(d_recs, rec_bytes), hip.download(d_lines, word_bytes, dtype=np.uint64), hip.download(d_sig, word_bytes, dtype=np.uint64), hip.download(d_cls, cls_bytes)
        for p in (d_text, d_recs, d_lines, d_sig, d_cls):
            hip.free(p)
    ok = rc != ru.MGPU_E_INVAL
    nmsg = min(n["nmsgs"], msgs_cap) if ok else 0
    ncls = min(n["nlines"], cls_cap) if ok else 0
    intact = ((raw[:lo] == 0xA5).all() and (raw[lo + 64 * nmsg:] == 0xA5).all() and (lines[:GUARD] == CANARY).all() and (lines[GUARD + nmsg:] == CANARY).all() and
              (sig[:GUARD] == CANARY).all() and (sig[GUARD + nmsg:] == CANARY).all() and (cls[:16] == 0xA5).all() and (cls[16 + ncls:] == 0xA5).all())
    return dict(n, rc=rc, msgs=raw[lo: lo + 64 * nmsg].copy().view(ru.MSG), line_of=lines[GUARD: GUARD + nmsg].copy(), signal=sig[GUARD: GUARD + nmsg].copy(),
                cls=cls[16: 16 + ncls].copy(), intact=bool(intact))


def same(res, want, what=None):
    """want: a golden entry or a result of ru.host_decode"""
    head = want["head"] if "head" in want else np.array([want["consumed"], want["nlines"], want["nmsgs"], *want["counters"]], dtype=np.uint64)
    assert res["rc"] == ru.MGPU_OK and res["intact"], what
    assert [res["consumed"], res["nlines"], res["nmsgs"], *res["counters"]] == [int(x) for x in head], (what, res["counters"], head)
    assert res["cls"].tobytes() == np.asarray(want["cls"], dtype=np.uint8).tobytes(), (what, np.nonzero(res["cls"] != want["cls"])[0][:8])
    assert (res["line_of"] == want["line_of"]).all(), what
    assert res["msgs"].tobytes() == want["msgs"].tobytes(), what
    assert res["signal"].tobytes() == np.asarray(want["signal"], dtype=np.float64).tobytes(), what


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("group", ru.GROUPS)
def test_golden_groups(ctxs, golden, group, form):
    """Every golden group under every configuration through the C entry of either form: records, source lines, the signal doubles'
    bit patterns, the class of every line, all the counters.  After group (d) a second call with one Address/Parity frame per
    prepared address: the context's filter stands where the reference's does."""
    get, hip = ctxs
    for k, cfg in enumerate(ru.CONFIGS[group]):
        d = get(cfg)
        prepare(d, ru.ops_of(group))
        g = golden[ru.key(group, cfg)]
        same(run(d, hip, form, g["stream"], msgs_off=8 * (k & 1)), g, (group, cfg))
        if group == "d":
            g2 = golden[ru.key("d2", cfg)]
            same(run(d, hip, form, g2["stream"]), g2, ("d2", cfg))


def test_growth_is_where_the_model_puts_it(golden):
    """The case tests what it says: by the model of icao_filter.c the stream of group (d) crosses two growths, and frames of
    inactive-generation addresses are accepted in front of the first and rejected behind it (the golden's classes, the reference's)."""
    lines, lstar, lstar2, probes = ru.group_d()
    cls = golden[ru.key("d", (1, 1, 0))]["cls"]
    inactive = set(int(x) for x in ru.D_INACTIVE)
    assert sum(1 for ln, a, ok in probes if a in inactive and ln < lstar and ok) >= 20 and sum(1 for ln, a, ok in probes if a in inactive and ln > lstar and not ok) >= 20
    assert all(cls[ln] == (ru.ACCEPT if ok else ru.UNKNOWN) for ln, a, ok in probes) and lstar < lstar2
    assert [int(cls[lstar + k]) for k in (-2, -1, 1, 2, 3)] == [ru.ACCEPT, ru.ACCEPT, ru.UNKNOWN, ru.ACCEPT, ru.ACCEPT]


def test_binding_and_host_passes(ctxs, golden):
    """Demodulator.raw_decode gives the golden; the host form with pass_bytes small enough to cut group (c) into four passes (the
    filter carries from pass to pass) and down to 1 (every pass grows until it holds a line) gives the bytes of one pass."""
    get, hip = ctxs
    cfg = (1, 1, 0)
    g = golden[ru.key("c", cfg)]
    d = get(cfg)
    res = d.raw_decode(g["stream"], now_ms=ru.NOW_MS)
    assert res["msgs"].tobytes() == g["msgs"].tobytes() and (res["line_of"] == g["line_of"]).all() and res["signal_level"].tobytes() == g["signal"].tobytes()
    assert res["line_class"].tobytes() == g["cls"].tobytes() and res["consumed"] == len(g["stream"]) and res["counters"]["remote_accepted"] == [int(x) for x in g["head"][7:10]]
    for pass_bytes in (len(g["stream"]) // 4 + 1, 8192, 1000):
        same(run(get(cfg), hip, "host", g["stream"], pass_bytes=pass_bytes), g, pass_bytes)
    part = g["stream"][:6000]
    want = ru.host_decode(d.lib, part, cfg)
    same(run(get(cfg), hip, "host", part, pass_bytes=1), want, 1)


@pytest.mark.parametrize("form", ["host", "device"])
def test_optional_arrays_left_out(ctxs, golden, form):
    """line_of, signal_level and line_class NULL (and a line_class_cap that then means nothing): the messages and the counts of the
    golden, in one pass and, in the host form, in small ones."""
    get, hip = ctxs
    cfg = (1, 1, 0)
    g = golden[ru.key("c", cfg)]
    src = np.frombuffer(g["stream"] + TAIL, dtype=np.uint8)
    n = len(g["msgs"])
    for pass_bytes in ((0, 9000) if form == "host" else (0,)):
        d = get(cfg)
        if form == "host":
            msgs = np.full((n + 1) * 64, 0xA5, dtype=np.uint8)
            rc, c = call(d, form, src.ctypes.data, len(g["stream"]), msgs.ctypes.data, None, None, n, None, 0, pass_bytes)
        else:
            d_text, d_msgs = hip.upload(src), hip.malloc((n + 1) * 64)
            hip.fill(d_msgs, 0xA5, (n + 1) * 64)
            rc, c = call(d, form, d_text, len(g["stream"]), d_msgs, None, None, n, None, 0)
            msgs = hip.download(d_msgs, (n + 1) * 64)
            hip.free(d_text)
            hip.free(d_msgs)
        assert rc == ru.MGPU_OK and [c["consumed"], c["nlines"], c["nmsgs"], *c["counters"]] == [int(x) for x in g["head"]], (form, pass_bytes)
        assert msgs[: n * 64].tobytes() == g["msgs"].tobytes() and (msgs[n * 64:] == 0xA5).all(), (form, pass_bytes)


def edge_stream(kind, first, rng):
    """Three tiles and more of traffic with a crafted place at stream position `first` (a tile's last or first byte)."""
    pool = ru.POOL
    head, at = [], 0
    while True:
        x = ru.filler(rng, 1, pool)[0]
        if at + len(x) > first - 300:
            break
        head.append(x)
        at += len(x)
    # an adder of a new address, then filler so that the next line begins (start, long) or ends (terminator, nul) exactly at `first`
    new = 0x7A0000 + first
    total = first - at + (kind in ("terminator", "nul"))
    adder = ru.avr(ru.es(new, 3))
    assert 200 < total - len(adder) <= 400
    rest_bytes = total - len(adder)
    pad = b" " * (rest_bytes // 2 - 1) + b"\n" + b"\t" * (rest_bytes - rest_bytes // 2 - 1) + (b"\0" if kind == "nul" else b"\n")
    if kind == "long":                                                                       # 256 bytes from a tile's last byte on: decided in the halo
        special = b" " * (256 - 17) + ru.avr(ru.ap(4, new, 1), end=b" \n") + b" " * (257 - 16) + ru.avr(ru.ap(4, new, 2))
        assert [len(x) for x in special.split(b"\n")[:2]] == [256, 257]
    else:
        special = ru.avr(ru.ap(20, new, 1)) + ru.avr(ru.ap(4, new, 2), b"<")
    stream = b"".join(head) + adder + pad + special
    stream += b"".join(ru.pad_to([], 3 * ru.TILE + 100 - len(stream), rng, pool))
    assert 3 * ru.TILE < len(stream) < 3 * ru.TILE + 200
    return stream


@pytest.mark.parametrize("kind", ["start", "terminator", "long", "nul"])
def test_tile_edges(ctxs, kind):
    """A line's first byte on a tile's last byte; a terminator on a tile's first byte; a 256-byte line reaching through the halo (and
    a 257-byte one, which is not a frame); a NUL terminator at a tile edge — each a conditional frame whose adder stands in the tile
    before: the device form at every misalignment 0-15 of the text, the host form once."""
    get, hip = ctxs
    cfg = (1, 1, 0)
    rng = np.random.default_rng(21)
    for tile in (1, 2):
        first = tile * ru.TILE - 1 if kind in ("start", "long") else tile * ru.TILE
        stream = edge_stream(kind, first, rng)
        if kind in ("start", "long"):
            assert stream[first - 1] in b"\n" and stream[first] in (b"* " if kind == "start" else b" ")
        else:
            assert stream[first: first + 1] == (b"\0" if kind == "nul" else b"\n")
        want = ru.host_decode(get(cfg).lib, stream, cfg)
        assert want["rc"] == ru.MGPU_OK and want["nmsgs"] > 300
        for text_off in range(16):
            same(run(get(cfg), hip, "device", stream, text_off=text_off, msgs_off=8 * (text_off & 1)), want, (kind, tile, text_off))
        same(run(get(cfg), hip, "host", stream), want, (kind, tile))


def test_long_lines_are_not_frames(ctxs):
    """The documented departure: a line longer than 256 bytes is "not a frame" on the device and on the host alike."""
    get, hip = ctxs
    cfg = (1, 1, 0)
    stream = b"".join(ru.LONG_LINES) + ru.avr(ru.es(ru.A, 3))
    want = ru.host_decode(get(cfg).lib, stream, cfg)
    assert want["cls"].tolist() == [ru.NONE] * len(ru.LONG_LINES) + [ru.ACCEPT]
    same(run(get(cfg), hip, "device", stream), want)


def filter_state(d, hip, addrs):
    """Which of the addresses the context's filter holds, asked with Address/Parity frames (which add nothing)."""
    stream = b"".join(ru.avr(ru.ap(4, int(a), k)) for k, a in enumerate(addrs))
    return run(d, hip, "device", stream)["cls"].tolist()


@pytest.mark.parametrize("form", ["host", "device"])
def test_capacities_one_short(ctxs, golden, form):
    """Each capacity exact, then one short: MGPU_E_OVERFLOW with what is needed, nothing stored at or beyond a capacity, the filter
    unchanged; and the same call with room then gives the golden."""
    get, hip = ctxs
    cfg = (1, 1, 0)
    g = golden[ru.key("d", cfg)]
    need, nlines = len(g["msgs"]), int(g["head"][1])
    asked = np.concatenate([ru.D_INACTIVE[:12], ru.D_ACTIVE[:4], ru.D_NEW[:12]])
    d = get(cfg)
    prepare(d, ru.ops_of("d"))
    state0 = filter_state(d, hip, asked)
    assert state0 == [ru.ACCEPT] * 16 + [ru.UNKNOWN] * 12
    for kw in (dict(msgs_cap=need - 1), dict(cls_cap=nlines - 1), dict(msgs_cap=0, cls_cap=0), dict(msgs_cap=7), dict(msgs_cap=need // 2, pass_bytes=9000)):
        if "pass_bytes" in kw and form == "device":
            continue
        res = run(d, hip, form, g["stream"], **{**dict(msgs_cap=need, cls_cap=nlines), **kw})
        assert res["rc"] == ru.MGPU_E_OVERFLOW and res["intact"], kw
        assert (res["nmsgs"], res["nlines"], res["consumed"], res["counters"]) == (need, nlines, len(g["stream"]), [int(x) for x in g["head"][3:]]), kw
        assert res["msgs"].tobytes() == g["msgs"][: len(res["msgs"])].tobytes() and (res["line_of"] == g["line_of"][: len(res["line_of"])]).all(), kw
        assert res["cls"].tobytes() == g["cls"][: len(res["cls"])].tobytes(), kw
        assert filter_state(d, hip, asked) == state0, kw                                     # the filter is where it stood
    same(run(d, hip, form, g["stream"], msgs_cap=need, cls_cap=nlines), g, "exact")
    assert filter_state(d, hip, asked) == [ru.UNKNOWN] * 7 + [ru.ACCEPT] + [ru.UNKNOWN] * 3 + [ru.ACCEPT] + [ru.ACCEPT] * 16


@pytest.mark.parametrize("form", ["host", "device"])
def test_bad_arguments_and_empty(ctxs, form):
    get, hip = ctxs
    from readsb_amd import binding
    d = get((1, 1, 0))
    text = ru.avr(ru.es(ru.A, 3)) * 3
    buf = np.frombuffer(text, dtype=np.uint8)
    d_text, d_recs, d_lines, d_sig = hip.upload(buf), hip.malloc(8 * 64), hip.malloc(8 * 8), hip.malloc(8 * 8)
    h_recs, h_lines, h_sig = np.zeros(8, dtype=ru.MSG), np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.float64)
    tp, rp, lp, sp = (buf.ctypes.data, h_recs.ctypes.data, h_lines.ctypes.data, h_sig.ctypes.data) if form == "host" else (d_text, d_recs, d_lines, d_sig)
    f = d.lib.mgpu_raw_decode if form == "host" else d.lib.mgpu_raw_decode_device
    rc, n = call(d, form, tp, len(text), rp, lp, sp, 8)
    assert rc == ru.MGPU_OK and n["nmsgs"] == 3 and n["counters"] == [3, 0, 0, 0, 3, 0, 0]
    assert f(None, None) == ru.MGPU_E_INVAL and f(d.ctx, None) == ru.MGPU_E_INVAL
    assert call(d, form, tp, len(text), rp, lp, sp, 8, size=C.sizeof(binding.RawInArgs) - 8)[0] == ru.MGPU_E_INVAL
    assert call(d, form, tp, len(text), rp, lp, sp, 8, size=0)[0] == ru.MGPU_E_INVAL
    assert call(d, form, None, len(text), rp, lp, sp, 8)[0] == ru.MGPU_E_INVAL
    assert call(d, form, tp, len(text), None, lp, sp, 8)[0] == ru.MGPU_E_INVAL
    assert call(d, form, tp, len(text), rp, lp, sp, 8, counters=False)[0] == ru.MGPU_E_INVAL
    assert call(d, form, tp, len(text), rp, lp, sp, 8, cls_ptr=None, cls_cap=5)[0] == ru.MGPU_E_INVAL
    for now in (-1, 253402300800000):
        assert call(d, form, tp, len(text), rp, lp, sp, 8, now_ms=now)[0] == ru.MGPU_E_INVAL
    if form == "device":
        assert call(d, form, tp, len(text), rp + 4, lp, sp, 4)[0] == ru.MGPU_E_INVAL                # records off their alignment
    for p in (d_text, d_recs, d_lines, d_sig):
        hip.free(p)
    # nbytes == 0, with and without pointers; text without any terminator
    for t in (b"", TAIL, TAIL * 100):
        res = run(d, hip, form, t)
        assert (res["rc"], res["consumed"], res["nlines"], res["nmsgs"], res["counters"], res["intact"]) == (ru.MGPU_OK, 0, 0, 0, [0] * 7, True)
    rc, n = call(d, form, None, 0, None, None, None, 0)
    assert rc == ru.MGPU_OK and (n["consumed"], n["nlines"], n["nmsgs"]) == (0, 0, 0)
    # a tail without its terminator behind lines: not consumed
    res = run(d, hip, form, text + TAIL[:-1])
    assert res["rc"] == ru.MGPU_OK and (res["consumed"], res["nlines"], res["nmsgs"]) == (len(text), 3, 3) and res["intact"]


def test_the_demodulator_sees_network_learnt_addresses(ctxs):
    """One capture with a DF4 of an address learnt from the raw feed, demodulated after the raw call, is accepted by mgpu_feed_iq; the
    same capture on a fresh context is not."""
    get, hip = ctxs
    import readsb_amd
    addr = 0x4CA2D6
    frames = fr.ap_frames(np.array([4, 4, 5]), addr, payload_seed=5)
    iq = filter_util.modulate_buffers([(frames, np.full(3, 56))])
    got = {}
    for learnt in (False, True):
        d = readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=8 * helpers.BUF_SAMPLES, filter_clock=EXTERNAL)
        try:
            if learnt:
                res = d.raw_decode(ru.avr(ru.es(addr, 1)), now_ms=ru.NOW_MS)
                assert res["line_class"].tolist() == [ru.ACCEPT]
            msgs, counters = d.demodulate_capture(iq)
            got[learnt] = msgs
        finally:
            d.close()
    assert len(got[False]) == 0
    assert len(got[True]) == 3 and (got[True]["addr"] == addr).all() and got[True]["msg"].tobytes() == frames[:, :14].tobytes()


def test_command_line_against_the_library(ctxs, golden):
    """readsb_gpu_raw_in as a child process on golden groups equals the library: the accepted messages as the beast stream
    mgpu_beast_encode makes of them, with a block smaller than the stream so that lines are carried between calls and the filter from
    block to block; the counters on stderr."""
    get, hip = ctxs
    for g, cfg, flags, block in (("c", (1, 1, 0), ["--fix"], 5000), ("b", (2, 1, 0), ["--aggressive"], 700), ("b", (1, 0, 0), ["--no-fix-df"], 1 << 20),
                                 ("a", (1, 1, 1), ["--modeac"], 4096)):
        e = golden[ru.key(g, cfg)]
        want = get(cfg).beast_encode(e["msgs"])
        r = subprocess.run([CLI, *flags, "--now", str(ru.NOW_MS), "--block", str(block)], input=e["stream"] + TAIL, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr[-500:]
        assert r.stdout == bytes(want), (g, cfg)
        head = [int(x) for x in e["head"]]
        assert r.stderr.decode().split() == ["lines", str(head[1]), "messages", str(head[2]), "bytes", str(head[0]), "remote_received_modes", str(head[3]),
                                             "remote_received_modeac", str(head[4]), "remote_rejected_unknown_icao", str(head[5]), "remote_rejected_bad", str(head[6]),
                                             "remote_accepted", str(head[7]), str(head[8]), str(head[9])], r.stderr
