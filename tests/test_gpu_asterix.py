"""-m gpu: the ASTERIX CAT021 output on the device (kernels/asterix.inc, mgpu_asterix_encode_ex*), byte for byte against
tests/asterix_util.py's checker, which tests/test_asterix_reference.py pins to the reference's own writer on the CPU.  No tolerance
anywhere.

Shapes as in tests/test_gpu_text.py (the passes are the same, the job is new): a workgroup is 256 messages, a wave 64, and nothing else
depends on the size of the list — lists of 0, 1, a wave -1 / exact / +1, a workgroup -1 / exact / +1 and three workgroups + 5, with
every message, no message and only a workgroup's last lane having a record; the whole golden case set in one call with either flag
value; the output at every alignment with a capacity that is exact, one short and zero, between guard bytes; random bytes as records;
a workgroup of records of the full 74 bytes."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import asterix_util as au
import beast_util as bu
import helpers
from sbs_util import MGPU_E_INVAL, MGPU_E_OVERFLOW

pytestmark = pytest.mark.gpu

GUARD = 256
DEF_GUARD = 16
SIZES = [0, 1, 63, 64, 65, au.BLOCK - 1, au.BLOCK, au.BLOCK + 1, 3 * au.BLOCK + 5]
OPTIONAL = ("positions", "verdict", "ids", "ac_baro_alt", "ac_category")


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
    return au.load_golden()


@functools.lru_cache(maxsize=None)
def _mixed():
    """Groups (a), (d) and stretches of (b) and (c), shuffled: records of every form next to each other; and the checker's result."""
    sets = _golden()[0]
    b, c = sets["b"], sets["c"]
    squawk_only = b["fields"]["flags"] == (au.F_ALT_Q_BIT | au.F_SQUAWK)
    keep = ~squawk_only | (np.cumsum(squawk_only) <= 1000)                             # all of (b) but most of its 16384 squawks
    b = {k: v[keep] for k, v in b.items()}
    c = au.concat_cases([sets["a"], b, sets["d"], au.slice_cases(c, 0, 1500)])
    order = np.random.default_rng(5).permutation(len(c["msgs"]))
    c = {k: v[order] for k, v in c.items()}
    return c, au.asterix_of(c)


def _first_diff(got, want):
    if len(got) != len(want):
        return f"{len(got)} bytes, want {len(want)}"
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    k = int(np.nonzero(a != b)[0][0])
    return f"first difference at byte {k} of {len(want)}: got {got[max(k - 60, 0):k + 16].hex()} want {want[max(k - 60, 0):k + 16].hex()}"


def _same(got, want):
    assert got == want, _first_diff(got, want)


def _same_deferred(got, want):
    assert len(got) == len(want), (len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} of {len(want)} deferred entries differ, first at {bad[:3]}: got {got[bad[:3]]} want {want[bad[:3]]}"


def _device(d, hip, c, want, k=0, cap=None, deferred_cap=None, remote=False, without=()):
    """mgpu_asterix_encode_ex_device into guard | k bytes | cap bytes | guard, all 0xA5 before the call, the deferred list before
    DEF_GUARD entries of 0xA5; the C entry itself, so that an error's outputs can be looked at.  want: the checker's result for the same
    arguments; without: the optional arrays passed as NULL."""
    from readsb_amd.binding import AsterixArgs, ASTERIX_REMOTE
    wstream, _, wdef, wskip = want
    n, T, D = len(c["msgs"]), len(wstream), len(wdef)
    cap = T if cap is None else cap
    dcap = D if deferred_cap is None else deferred_cap
    total = GUARD + k + max(cap, T) + GUARD
    ptrs = {name: hip.upload(c[name]) for name in au.KEYS}
    d_buf, d_def = hip.malloc(total), hip.malloc((dcap + DEF_GUARD) * bu.DEFERRED.itemsize)
    try:
        hip.fill(d_buf, 0xA5, total)
        hip.fill(d_def, 0xA5, (dcap + DEF_GUARD) * bu.DEFERRED.itemsize)
        nb, nd, ns = C.c_uint64(12345), C.c_uint64(12345), C.c_uint64(12345)
        opt = [None if name in without else ptrs[name] for name in OPTIONAL]
        a = AsterixArgs(C.sizeof(AsterixArgs), ASTERIX_REMOTE if remote else 0, ptrs["msgs"], ptrs["fields"], *opt, n, au.NOW_MS, d_buf + GUARD + k, cap,
                        C.pointer(nb), d_def, dcap, C.pointer(nd), C.pointer(ns))
        rc = int(d.lib.mgpu_asterix_encode_ex_device(d.ctx, C.byref(a)))
        buf = hip.download(d_buf, total)
        got_def = hip.download(d_def, (dcap + DEF_GUARD) * bu.DEFERRED.itemsize, dtype=bu.DEFERRED)
    finally:
        for p in list(ptrs.values()) + [d_buf, d_def]:
            hip.free(p)
    at = GUARD + k
    assert (nb.value, nd.value, ns.value) == (T, D, wskip), (nb.value, nd.value, ns.value, T, D, wskip)
    assert (buf[:at] == 0xA5).all(), f"bytes before the output were written (offset {k})"
    assert (buf[at + min(cap, T):] == 0xA5).all(), f"bytes behind the stream or at / beyond the capacity {cap} were written (offset {k})"
    _same(buf[at:at + min(cap, T)].tobytes(), wstream[:min(cap, T)])          # on overflow too: the prefix below the capacity is the stream's
    listed = min(dcap, D)
    _same_deferred(got_def[:listed], wdef[:listed])
    assert (got_def[listed:].view(np.uint8) == 0xA5).all(), "entries behind the list were written"
    assert rc == (MGPU_E_OVERFLOW if cap < T or dcap < D else 0), rc
    return rc


def _host(d, c, remote=False, without=(), **kw):
    opt = {name: None if name in without else c[name] for name in OPTIONAL}
    return d.asterix_encode(c["msgs"], au.NOW_MS, fields=c["fields"], remote=remote, **opt, **kw)


def _check_host(d, c, want, **kw):
    stream, deferred, nskipped = _host(d, c, **kw)
    _same(stream, want[0])
    _same_deferred(deferred, want[2])
    assert nskipped == want[3]


# ---- sizes ----------------------------------------------------------------------------------------------------------------------------

def _with_records(n, seed):
    """n messages that all have a record, of every form."""
    c, (_, length, _, _) = _mixed()
    idx = np.nonzero(length > 0)[0]
    idx = idx[np.random.default_rng(seed).permutation(len(idx))[:n]]
    assert len(idx) == n
    return {k: v[idx] for k, v in c.items()}


@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, n):
    d, hip = ctx
    every = _with_records(n, n)
    none = {k: v.copy() for k, v in every.items()}
    none["verdict"][:] = au.su.GATE_DROP
    last = {k: v.copy() for k, v in every.items()}
    last["verdict"][:] = au.su.GATE_DROP | au.su.GATE_POSSIBLE
    last["verdict"][au.BLOCK - 1::au.BLOCK] = au.FORWARD
    for what, c in (("every", every), ("none", none), ("last lane", last)):
        want = au.asterix_of(c)
        records = int((want[1] > 0).sum())
        assert records == {"every": n, "none": 0, "last lane": n // au.BLOCK}[what]
        _check_host(d, c, want)
        if n:
            _device(d, hip, c, want, k=n % 4)
    stream, deferred, nskipped = d.asterix_encode(every["msgs"], au.NOW_MS, fields=every["fields"])      # none of the optional arrays
    _same(stream, au.asterix_reference(every["msgs"], every["fields"], au.NOW_MS)[0])
    assert len(deferred) == 0


# ---- the golden cases ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("remote", [False, True])
def test_golden_cases_in_one_call(ctx, remote):
    d, _ = ctx
    sets, streams, _ = _golden()
    c = au.concat_cases([sets[g] for g in au.GROUPS])
    want = au.asterix_of(c, remote=remote)
    assert len(c["msgs"]) > 30000 and want[3] >= 40 and len(want[2]) > 100
    _check_host(d, c, want, remote=remote)
    # and without verdicts the reference's own bytes, group by group
    for g in ("a", "b", "c"):
        _same(_host(d, sets[g], remote=remote, without=("verdict",))[0], streams[f"ref_{g}_r{int(remote)}"])


def test_clocks(ctx):
    """sysTimestamp and now_ms on both sides of midnight and of the 32-bit wrap: the reference's bytes at every clock of the golden."""
    d, _ = ctx
    streams = _golden()[1]
    clock = au.clock_cases()
    for now_ms in au.CLOCKS:
        got = d.asterix_encode(clock["msgs"], now_ms, fields=clock["fields"], positions=clock["positions"])
        _same(got[0], streams[f"ref_clock_{now_ms}"])


# ---- misalignment and capacity ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(4))
def test_misalignment_and_capacity(ctx, k):
    d, hip = ctx
    c, _ = _mixed()
    c = au.slice_cases(c, 100 * k, 100 * k + 5 * au.BLOCK + 77)
    want = au.asterix_of(c)
    T = len(want[0])
    starts = (np.cumsum(want[1]) - want[1])[::au.BLOCK]
    assert T > 5 * au.BLOCK * 10 and len(set(((starts + k) % 4).tolist())) >= 2        # workgroups start at several alignments
    assert _device(d, hip, c, want, k=k, cap=T) == 0
    assert _device(d, hip, c, want, k=k, cap=T - 1) == MGPU_E_OVERFLOW
    assert _device(d, hip, c, want, k=k, cap=0) == MGPU_E_OVERFLOW
    assert _device(d, hip, c, want, k=k) == 0                                          # the context encodes correctly afterwards


# ---- the deferred list -----------------------------------------------------------------------------------------------------------------

def test_deferred_list(ctx):
    d, hip = ctx
    c, _ = _mixed()
    c = au.slice_cases(c, 2000, 2000 + 4 * au.BLOCK + 9)
    c = {k: v.copy() for k, v in c.items()}
    ends = np.concatenate([np.arange(0, len(c["msgs"]), au.BLOCK) + lane for lane in (0, 63, 64, 255)])
    ends = ends[ends < len(c["msgs"])]
    c["verdict"][ends] = au.GATE_DEFER                                          # at the ends of waves and workgroups
    want = au.asterix_of(c)
    D = len(want[2])
    assert D > 20
    for dcap in (0, 1, D, D + 100):
        _device(d, hip, c, want, deferred_cap=dcap)
    # without verdicts nothing is deferred and no list is needed
    _device(d, hip, c, au.asterix_of(c, gated=False), without=("verdict",), deferred_cap=0)


# ---- hostile records -------------------------------------------------------------------------------------------------------------------

def test_hostile_records(ctx):
    d, hip = ctx
    c = au.hostile_cases(6 * au.BLOCK + 31, 77)
    plain = au.asterix_classes(c["fields"], c["positions"], None, c["ac_baro_alt"])
    assert (plain != au.SKIP).mean() >= 0.6, "at least 60 % of the records lie in the domain"
    assert (plain == au.SKIP).mean() >= 0.1
    for remote in (False, True):
        want = au.asterix_of(c, remote=remote)
        assert (want[1] > 0).sum() > 300 and want[3] > 100 and len(want[2]) > 50 and want[1].max() <= au.RECORD_MAX
        _device(d, hip, c, want, k=1 + remote, remote=remote)
    items = set().union(*au.asterix_of(c, want_items=True)[4])
    assert items == set(au.FSPEC_BITS), "records of every kind"


def test_longest_records_fill_a_workgroup(ctx):
    """Every lane a record of the full 74 bytes: the LDS buffer's limit."""
    d, hip = ctx
    c = au.longest_cases(2 * au.BLOCK + 3)
    want = au.asterix_of(c)
    assert (want[1] == au.RECORD_MAX).all()
    for k in range(4):
        _device(d, hip, c, want, k=k)


# ---- the two forms, the optional arrays, the library's own field decode -------------------------------------------------------------------

def test_forms_agree(ctx):
    d, hip = ctx
    a = _golden()[0]["a"]
    fields = d.decode_fields(a["msgs"])
    assert fields.tobytes() == a["fields"].tobytes()                           # group (a) holds the decode of its own frames
    opt = {name: a[name] for name in OPTIONAL}
    with_fields = d.asterix_encode(a["msgs"], au.NOW_MS, fields=fields, **opt)
    without = d.asterix_encode(a["msgs"], au.NOW_MS, **opt)
    want = au.asterix_of(a)
    for got in (with_fields, without):
        _same(got[0], want[0])
        _same_deferred(got[1], want[2])
        assert got[2] == want[3]
    _device(d, hip, a, want)


@pytest.mark.parametrize("missing", OPTIONAL + (OPTIONAL,))
def test_optional_arrays(ctx, missing):
    """Each optional array NULL, and all of them: no position, every message a record, no receiver id, a fresh aircraft's zeros."""
    d, hip = ctx
    without = missing if isinstance(missing, tuple) else (missing,)
    c, _ = _mixed()
    c = au.slice_cases(c, 500, 500 + 3 * au.BLOCK + 17)
    kw = {k: None if k in without else c[k] for k in OPTIONAL}
    want = au.asterix_reference(c["msgs"], c["fields"], au.NOW_MS, **kw)
    full = au.asterix_of(c)
    assert want[0] != full[0], "the array matters to this stretch"
    _check_host(d, c, want, without=without)
    _device(d, hip, c, want, k=3, without=without)


def test_cut_lists(ctx):
    d, _ = ctx
    c, (whole, length, _, _) = _mixed()
    n = len(c["msgs"])
    _same(_host(d, c)[0], whole)
    for cut in (1, 255, 256, 1000):
        lo, hi = (n // 2, n // 2 + 200) if cut == 1 else (0, n)
        got = b"".join(_host(d, au.slice_cases(c, k, min(k + cut, hi)))[0] for k in range(lo, hi, cut))
        start = int(length[:lo].sum())
        _same(got, whole[start:start + int(length[lo:hi].sum())])


def test_arguments(ctx):
    from readsb_amd.binding import AsterixArgs
    d, hip = ctx
    c = _with_records(10, 1)
    out = np.zeros(4096, dtype=np.uint8)
    nb, nd = C.c_uint64(7), C.c_uint64(7)

    def enc(size=C.sizeof(AsterixArgs), flags=0, n=10, now=au.NOW_MS, fields=c["fields"].ctypes.data, bytes_=C.pointer(nb), ndef=C.pointer(nd), device=False,
            msgs=c["msgs"].ctypes.data, outp=out.ctypes.data):
        a = AsterixArgs(size, flags, msgs, fields, None, c["verdict"].ctypes.data, None, None, None, n, now, outp, out.size, bytes_, None, 0, ndef, None)
        return int((d.lib.mgpu_asterix_encode_ex_device if device else d.lib.mgpu_asterix_encode_ex)(d.ctx, C.byref(a)))
    assert enc() == 0 and nb.value == len(au.asterix_reference(c["msgs"], c["fields"], au.NOW_MS, verdict=c["verdict"])[0])
    assert enc(n=0) == 0 and nb.value == 0
    assert enc(n=0, device=True, fields=None) == 0
    assert enc(size=C.sizeof(AsterixArgs) - 8) == MGPU_E_INVAL
    assert enc(flags=2) == MGPU_E_INVAL and enc(flags=1) == 0
    assert enc(now=-1) == MGPU_E_INVAL and enc(now=au.MS_END) == MGPU_E_INVAL and enc(now=au.MS_END - 1) == 0
    assert enc(bytes_=None) == MGPU_E_INVAL and enc(ndef=None) == MGPU_E_INVAL
    assert enc(msgs=None) == MGPU_E_INVAL and enc(outp=None) == MGPU_E_INVAL
    assert enc(device=True, fields=None) == MGPU_E_INVAL                       # only the host form decodes the fields itself


# ---- end to end --------------------------------------------------------------------------------------------------------------------------

def test_end_to_end_on_a_capture(ctx):
    """feed -> decode_fields_device -> track_gate_device -> cpr_track_device -> asterix_encode_device, everything resident, against the
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
    want = au.asterix_reference(msgs, fields, au.NOW_MS, positions=positions, verdict=verdict, want_items=True)
    cap = len(want[0]) + 64
    d_msgs = hip.upload(msgs)
    d_fields, d_verdict, d_pos = hip.malloc(n * readsb_amd.FIELDS_DTYPE.itemsize), hip.malloc(n), hip.malloc(n * readsb_amd.POSITION_DTYPE.itemsize)
    d_out, d_def = hip.malloc(cap), hip.malloc((len(want[2]) + 1) * bu.DEFERRED.itemsize)
    try:
        d.decode_fields_device(d_msgs, n, d_fields)
        d.track_gate_device(d_msgs, d_fields, n, d_verdict)
        d.cpr_track_device(d_msgs, d_fields, n, d_pos, ref=ref)
        nb, nd, ns = d.asterix_encode_device(d_msgs, d_fields, n, au.NOW_MS, d_out, cap, d_positions_ptr=d_pos, d_verdict_ptr=d_verdict,
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
    records = au.split_records(stream)
    assert len(records) >= 100 and len(records) == int((want[1] > 0).sum())
    items = set().union(*want[4])
    assert {"130", "073", "145", "070", "200"} <= items, items                   # positions, altitudes, squawks, status of the drawn traffic


# ---- the host program ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _cli_capture():
    """A capture and, from the host-array stages on its whole message list, the CAT021 stream with the deferred messages dropped."""
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
            want[with_ref] = au.asterix_reference(msgs, fields, au.NOW_MS, positions=positions, verdict=verdict)
    finally:
        d.close()
    return iq, ref, want


@pytest.mark.parametrize("chunk,with_ref", [(256, True), (7, True), (3, False)])
def test_host_program_asterix_out(built, tmp_path, chunk, with_ref):
    """readsb_gpu_ifile --asterix-out: the file is the checker's stream for the capture — one feed or many — and --help names the option."""
    cli = os.path.join(helpers.ROOT, "readsb_amd", "host", "readsb_gpu_ifile")
    iq, ref, want = _cli_capture()
    stream, length, deferred, nskipped = want[with_ref]
    cap, out = tmp_path / "cap.iq", tmp_path / "out.asterix"
    iq.tofile(cap)
    cmd = [cli, "--device-type", "ifile", "--ifile", str(cap), "--iformat", "UC8", "--fix", "--startup-time-ms", str(helpers.STARTUP_MS),
           "--gpu-chunk-buffers", str(chunk), "--asterix-out", str(out), "--asterix-now-ms", str(au.NOW_MS), "--stats"]
    cmd += ["--lat", str(ref[0]), "--lon", str(ref[1])] if with_ref else []
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == ""
    _same(out.read_bytes(), stream)
    records = au.split_records(stream)
    assert len(records) >= 100 and nskipped == 0
    if with_ref:
        assert any(r_[3] & 0x04 for r_ in records), "no record carries a position"
    assert f"{len(deferred)} message(s) left to a position tracker dropped" in r.stderr
    assert "Mode-S message preambles received" in r.stderr
    if chunk == 256:
        h = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=30)
        assert h.returncode == 0 and "--asterix-out" in h.stdout and "--sbs-out" in h.stdout
