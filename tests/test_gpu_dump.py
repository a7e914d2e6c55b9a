"""-m gpu: the decoded-message dump on the device (kernels/dump.inc, mgpu_dump_encode_ex*), byte for byte against the bytes the
reference's displayModesMessage printed for the same cases (tests/golden/dump_cases.npz; tests/test_dump_reference.py pins the file
to the live reference and runs the same formatter on the CPU).  No tolerance anywhere.

Shapes: a workgroup is 256 messages, a wave 64; the scan takes a second round beyond 1024 workgroups (run in ONLYADDR mode, seven
bytes a message); the write pass's sink works on 8-byte words of the absolute address, so the output is tried at all eight
alignments, with the longest and the shortest dump as neighbours in both orders, and with a capacity that is exact, one short and
zero, between guard bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

import beast_util as bu
import dump_util as du
import helpers
import sbs_util as su

pytestmark = pytest.mark.gpu

GUARD = 64
DEF_GUARD = 16
NAMES = ("msgs", "fields", "reduce_forward", "receiver_ids", "positions", "decoded_nic", "decoded_rc")
SIZES = [0, 1, 63, 64, 65, du.BLOCK - 1, du.BLOCK, du.BLOCK + 1, 2 * du.BLOCK + 1]


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
    sets, ref, near = du.load_golden()
    chunks = {key: du.chunks(*val) for key, val in ref.items()}
    return sets, chunks, near


@functools.lru_cache(maxsize=None)
def _all():
    """Every group in one list -> (cases, {mode: the reference's dump per case})"""
    sets, chunks, _ = _golden()
    return du.concat_cases([sets[g] for g in du.GROUPS]), {mode: sum((chunks[(g, mode)] for g in du.GROUPS), []) for mode in du.MODES}


@functools.lru_cache(maxsize=None)
def _cycle(n, mode="full"):
    """n dumped, never deferred cases: the longest and the shortest dump of the golden as neighbours in both orders, then the rest in
    a fixed shuffle, repeated as often as needed."""
    c, chunks = _all()
    cls = du.classes(c, du.MODES[mode])
    lens = np.array([len(t) for t in chunks[mode]])
    idx = np.nonzero(cls == du.LINE)[0]
    hi, lo = idx[np.argmax(lens[idx])], idx[np.argmin(lens[idx])]
    rest = idx[np.random.default_rng(11).permutation(len(idx))]
    order = np.resize(np.concatenate([[hi, lo, hi], rest]), n)
    return du.take_cases(c, order), [chunks[mode][i] for i in order]


def _first_diff(got, want):
    if len(got) != len(want):
        return f"{len(got)} bytes, want {len(want)}"
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    k = int(np.nonzero(a != b)[0][0])
    return f"first difference at byte {k} of {len(want)}: got {got[max(k - 80, 0):k + 16]!r} want {want[max(k - 80, 0):k + 16]!r}"


def _same(got, want):
    assert got == want, _first_diff(got, want)


def _same_deferred(got, want):
    assert len(got) == len(want), (len(got), len(want))
    assert (got == want).all(), (got[:4], want[:4])


def _device(d, hip, c, chunks, flags, k=0, cap=None, deferred_cap=None, show_only=0, optional=True):
    """mgpu_dump_encode_ex_device into guard | k bytes | cap bytes | guard, all 0xA5 before the call, the deferred list before DEF_GUARD
    entries of 0xA5; the C entry itself, so that an error's outputs can be looked at.  -> (rc, the expectation)"""
    from readsb_amd.binding import DumpArgs
    want = du.expected(c, flags, chunks, show_only)
    wstream, wdef, wskip, _ = want
    n, T, D = len(c["msgs"]), len(wstream), len(wdef)
    cap = T if cap is None else cap
    dcap = D if deferred_cap is None else deferred_cap
    total = GUARD + 8 + max(cap, T) + GUARD
    ptrs = [hip.upload(c[name]) if n and (optional or name in ("msgs", "fields")) else None for name in NAMES]
    d_buf, d_def = hip.malloc(total), hip.malloc((dcap + DEF_GUARD) * bu.DEFERRED.itemsize)
    try:
        hip.fill(d_buf, 0xA5, total)
        hip.fill(d_def, 0xA5, (dcap + DEF_GUARD) * bu.DEFERRED.itemsize)
        nb, nd, ns = C.c_uint64(12345), C.c_uint64(12345), C.c_uint64(12345)
        a = DumpArgs(C.sizeof(DumpArgs), flags, *ptrs, n, show_only, d_buf + GUARD + k, cap, C.pointer(nb), d_def, dcap, C.pointer(nd), C.pointer(ns))
        rc = int(d.lib.mgpu_dump_encode_ex_device(d.ctx, C.byref(a)))
        buf = hip.download(d_buf, total)
        got_def = hip.download(d_def, (dcap + DEF_GUARD) * bu.DEFERRED.itemsize, dtype=bu.DEFERRED)
    finally:
        for p in ptrs + [d_buf, d_def]:
            if p is not None:
                hip.free(p)
    at = GUARD + k
    assert (nb.value, nd.value, ns.value) == (T, D, wskip), (nb.value, nd.value, ns.value, T, D, wskip)
    assert (buf[:at] == 0xA5).all(), f"bytes before the output were written (offset {k})"
    assert (buf[at + min(cap, T):] == 0xA5).all(), f"bytes behind the stream or at / beyond the capacity {cap} were written (offset {k})"
    _same(buf[at:at + min(cap, T)].tobytes(), wstream[:min(cap, T)])          # on overflow too: the prefix below the capacity is the stream's
    listed = min(dcap, D)
    _same_deferred(got_def[:listed], wdef[:listed])
    assert (got_def[listed:].view(np.uint8) == 0xA5).all(), "entries behind the list were written"
    assert rc == (du.MGPU_E_OVERFLOW if cap < T or dcap < D else 0), rc
    return rc, want


def _host(d, c, flags, optional=True, fields=True, **kw):
    opt = {name: c[name] for name in du.OPTIONAL} if optional else {}
    return d.dump_encode(c["msgs"], flags, fields=c["fields"] if fields else None, **opt, **kw)


def _check_host(d, c, chunks, flags, **kw):
    want = du.expected(c, flags, chunks, kw.get("show_only", 0))
    stream, deferred, nskipped = _host(d, c, flags, **kw)
    _same(stream, want[0])
    _same_deferred(deferred, want[1])
    assert nskipped == want[2]
    return stream, deferred


# ---- golden parity --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(du.MODES))
@pytest.mark.parametrize("group", du.GROUPS)
def test_golden(ctx, group, mode):
    """Every golden group in every mode, host form and device form: the reference's bytes, the skipped and the deferred as the rules say."""
    d, hip = ctx
    sets, chunks, near = _golden()
    c, flags = sets[group], du.MODES[mode]
    _, (_, wdef, wskip, _) = _device(d, hip, c, chunks[(group, mode)], flags)
    _check_host(d, c, chunks[(group, mode)], flags)
    assert wdef["index"].tolist() == (near.tolist() if group == "e" and not flags & (du.RAW | du.ONLYADDR) else [])
    assert wskip == int((du.classes(c, flags) == du.SKIP).sum())


@pytest.mark.parametrize("mode", ["full", "mlat"])
def test_deferred_spliced_by_the_host(ctx, mode):
    """Group (e): exactly the near cases are deferred, with their indices and offsets, and mgpu_dump_format_host's text put in at the
    offsets gives what the reference printed for the whole group."""
    d, _ = ctx
    sets, chunks, near = _golden()
    c, flags = sets["e"], du.MODES[mode]
    stream, deferred = _check_host(d, c, chunks[("e", mode)], flags)
    assert deferred["index"].tolist() == near.tolist()
    texts = [d.dump_format_host(int(i), c["msgs"], c["fields"], flags, **{name: c[name] for name in du.OPTIONAL}) for i in deferred["index"]]
    _same(du.splice(stream, deferred, texts), b"".join(chunks[("e", mode)]))


def test_everything_in_one_call(ctx):
    """All groups as one list, shuffled: every form of dump next to every other, at an odd output address."""
    d, hip = ctx
    c, chunks = _all()
    order = np.random.default_rng(3).permutation(len(c["msgs"]))
    _device(d, hip, du.take_cases(c, order), [chunks["mlat"][i] for i in order], du.MLAT, k=3)


def test_fields_decoded_by_the_library(ctx):
    """Host form with fields == NULL: group (a)'s records are the decode of its frames, so the dumps are the same."""
    d, _ = ctx
    sets, chunks, _ = _golden()
    _check_host(d, sets["a"], chunks[("a", "full")], 0, fields=False)


def test_optional_arrays_absent(ctx):
    """NULL for the five optional arrays is zeros: groups (d) and (e) carry zeros there."""
    d, hip = ctx
    sets, chunks, _ = _golden()
    for g in ("d", "e"):
        assert all(not sets[g][name].view(np.uint8).any() for name in du.OPTIONAL)
        _device(d, hip, sets[g], chunks[(g, "full")], 0, optional=False)
        _check_host(d, sets[g], chunks[(g, "full")], 0, optional=False)


def test_quiet_shows_one_address(ctx):
    d, hip = ctx
    c, chunks = _cycle(700)
    addr = int(c["fields"]["addr"][5])
    want = _device(d, hip, c, chunks, du.QUIET, show_only=addr)[1]
    assert 0 < len(want[0]) < sum(len(t) for t in chunks) and want[2] == 0
    _check_host(d, c, chunks, du.QUIET, show_only=addr)
    assert _device(d, hip, c, chunks, du.QUIET, show_only=0xFF123456)[1][0] == b""


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, n):
    d, hip = ctx
    c, chunks = _cycle(n)
    _device(d, hip, c, chunks, 0, k=n % 8)
    _check_host(d, c, chunks, 0)


def test_scan_takes_a_second_round(ctx):
    """One workgroup more than the scan's threads: ONLYADDR keeps the stream at seven bytes a message."""
    d, hip = ctx
    n = du.BLOCK * du.SCAN_THREADS + 1
    c, chunks = _cycle(n, "onlyaddr")
    _device(d, hip, c, chunks, du.ONLYADDR, k=1)


# ---- capacity ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(8))
def test_alignment_and_capacity(ctx, k):
    """The output at each of the eight byte offsets from an aligned allocation: the same bytes; a capacity equal to the need passes,
    one less is MGPU_E_OVERFLOW with *bytes = the need and nothing at or beyond the capacity written."""
    d, hip = ctx
    c, chunks = _cycle(du.BLOCK + 37)
    need = sum(len(t) for t in chunks)
    assert _device(d, hip, c, chunks, 0, k=k)[0] == 0
    assert _device(d, hip, c, chunks, 0, k=k, cap=need - 1)[0] == du.MGPU_E_OVERFLOW


@pytest.mark.parametrize("cap", [0, 1, 7, 8, 9, 2599, 100000])
def test_capacity_cuts_anywhere(ctx, cap):
    d, hip = ctx
    c, chunks = _cycle(2 * du.BLOCK + 1)
    assert _device(d, hip, c, chunks, 0, k=5, cap=cap)[0] == du.MGPU_E_OVERFLOW


def test_host_form_overflow(ctx):
    d, _ = ctx
    from readsb_amd.binding import MgpuError
    c, chunks = _cycle(300)
    need = sum(len(t) for t in chunks)
    assert len(_host(d, c, 0, cap=need)[0]) == need
    with pytest.raises(MgpuError):
        _host(d, c, 0, cap=need - 1)


def test_deferred_capacity(ctx):
    """A list shorter than the count: MGPU_E_OVERFLOW, *ndeferred the count, the first deferred_cap entries written."""
    d, hip = ctx
    sets, chunks, near = _golden()
    assert len(near) > 3
    for dcap in (0, 1, len(near) - 1):
        assert _device(d, hip, sets["e"], chunks[("e", "full")], 0, deferred_cap=dcap)[0] == du.MGPU_E_OVERFLOW
    assert _device(d, hip, sets["e"], chunks[("e", "full")], 0, deferred_cap=len(near) + 5)[0] == 0


# ---- reuse ------------------------------------------------------------------------------------------------------------------------------

def test_reuse_of_a_context(ctx):
    """Small, large, small again on one context: the scratch regrows and no stale byte or length shows; a dump call between two SBS
    calls leaves their output unchanged."""
    d, hip = ctx
    for n in (5, 40 * du.BLOCK + 3, 5, 1):
        c, chunks = _cycle(n)
        _check_host(d, c, chunks, 0)
        _device(d, hip, c, chunks, 0, k=2)
    tsets = su.load_golden()[0]
    t = tsets["a"]
    before = d.sbs_encode(t["msgs"], su.NOW_MS, fields=t["fields"], positions=t["positions"], verdict=t["verdict"], geom_delta=t["geom_delta"])
    c, chunks = _cycle(700)
    _check_host(d, c, chunks, 0)
    after = d.sbs_encode(t["msgs"], su.NOW_MS, fields=t["fields"], positions=t["positions"], verdict=t["verdict"], geom_delta=t["geom_delta"])
    assert before[0] == after[0] and (before[1] == after[1]).all() and before[2] == after[2]


# ---- arguments --------------------------------------------------------------------------------------------------------------------------

def test_arguments(ctx):
    d, hip = ctx
    from readsb_amd.binding import DumpArgs
    c, _ = _cycle(4)
    p_msgs, p_fields, p_out = hip.upload(c["msgs"]), hip.upload(c["fields"]), hip.malloc(4 * du.DUMP_MAX)
    try:
        def call(fn=d.lib.mgpu_dump_encode_ex_device, **kw):
            nb = C.c_uint64(0)
            v = dict(size=C.sizeof(DumpArgs), flags=0, msgs=p_msgs, fields=p_fields, n=4, out=p_out, cap=4 * du.DUMP_MAX, bytes=C.pointer(nb))
            v.update(kw)
            return int(fn(d.ctx, C.byref(DumpArgs(**v)))), nb.value
        assert call()[0] == 0
        assert call(size=C.sizeof(DumpArgs) - 8)[0] == du.MGPU_E_INVAL
        assert call(fields=None)[0] == du.MGPU_E_INVAL                       # the device form decodes nothing
        assert call(out=None)[0] == du.MGPU_E_INVAL
        assert call(flags=16)[0] == du.MGPU_E_INVAL
        assert call(deferred=None, deferred_cap=1)[0] == du.MGPU_E_INVAL
        assert call(bytes=None)[0] == du.MGPU_E_INVAL
        rc, need = call(out=None, cap=0)                                     # a sizing call: what the stream needs
        assert rc == du.MGPU_E_OVERFLOW and need == call()[1]
        assert call(n=0) == (0, 0)
        assert call(fn=d.lib.mgpu_dump_encode_ex, msgs=c["msgs"].ctypes.data, fields=None, out=None, cap=1)[0] == du.MGPU_E_INVAL
    finally:
        for p in (p_msgs, p_fields, p_out):
            hip.free(p)


# ---- the host program -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk,extra,flags", [(256, [], 0), (5, ["--mlat"], du.MLAT), (256, ["--raw", "--mlat"], du.RAW | du.MLAT)])
def test_host_program_dump_out(built, tmp_path, chunk, extra, flags):
    """readsb_gpu_ifile --dump-out on a 1 s synthetic capture — one feed or many — writes what the plain-Python model
    (dump_util.model_dump, pinned to the reference's bytes by tests/test_dump_reference.py) prints for the list mgpu_collect returns for
    the same capture, no message left out; the host-array entry with the deferred spliced in gives the same; stdout stays empty and
    --help says what differs from the reference program."""
    import os
    import subprocess
    import readsb_amd
    cli = os.path.join(helpers.ROOT, "readsb_amd", "host", "readsb_gpu_ifile")
    iq = helpers.synth(seconds=1.0, seed=616, rate=2500.0)
    d = readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=16 * 131072)
    try:
        msgs, _ = d.demodulate_capture(iq)
        fields = d.decode_fields(msgs)
        stream, deferred, nskipped = d.dump_encode(msgs, flags, fields=fields)
        spliced = du.splice(stream, deferred, [d.dump_format_host(int(i), msgs, fields, flags) for i in deferred["index"]])
    finally:
        d.close()
    c = du.empty_cases(len(msgs))
    c["msgs"], c["fields"] = msgs, fields
    assert (du.classes(c, flags) != du.SKIP).all()
    want = b"".join(du.model_chunks(c, flags, optional=False))
    _same(spliced, want)
    assert len(msgs) >= 100 and nskipped == 0
    assert want.startswith((b"@%012X" % int(msgs["timestamp"][0]) if flags & du.MLAT else b"*") + msgs["msg"][0, :msgs["msgbits"][0] // 8].tobytes().hex().encode() + b";\n")
    assert want.count(b";\n") == len(msgs) and (flags & du.RAW or want.count(b"\n\n") == len(msgs))
    cap, out = tmp_path / "cap.iq", tmp_path / "out.txt"
    iq.tofile(cap)
    cmd = [cli, "--device-type", "ifile", "--ifile", str(cap), "--iformat", "UC8", "--fix", "--startup-time-ms", str(helpers.STARTUP_MS),
           "--gpu-chunk-buffers", str(chunk), "--dump-out", str(out), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    _same(out.read_bytes(), want)
    assert f"dump: {len(msgs)} messages, {len(want)} bytes, {len(deferred)} message(s) formatted on the host, 0 outside" in r.stderr
    if chunk == 256:
        h = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=30)
        assert h.returncode == 0 and "--dump-out" in h.stdout and "EXCEPT" in h.stdout
