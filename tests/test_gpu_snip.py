"""-m gpu: `readsb --snip` on the device (kernels/snip.inc, mgpu_snip / mgpu_snip_device), bytes and the final quiet-run counter
compared with == against tests/snip_util.py's model, which tests/test_snip_reference.py pins to the reference program on the CPU; the
first case and the command line are compared with the reference program itself here too.

Shapes: a tile is 8192 samples (128 words of 64), a workgroup takes 4 of them, the halo is one word, a 16-byte load 8 samples.  The
crafted stream puts run starts and the 32/33 boundary on every residue mod 64 and across tile edges; the random streams are 1 Mi
samples = 32 workgroups, so the offsets go through the scan; the small sizes are 1, 2, a word -1 / exact / +1, a tile -1 / +1 and a
workgroup's share -1 / +1; the output starts at every kind of misalignment of a 16-byte vector between canaries."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import beast_util as bu
import helpers
import snip_util as su

pytestmark = pytest.mark.gpu

GUARD = 256
CLI = os.path.join(helpers.ROOT, "readsb_amd", "host", "readsb_gpu_ifile")


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


@functools.lru_cache(maxsize=None)
def _crafted(level):
    iq = su.crafted(level)
    return iq, su.model(iq, level)


def snip_raw(d, form, iq_ptr, n, level, out_ptr, cap, c_in=0, pass_samples=0):
    """-> (return code, *nout, *quiet_run) of mgpu_snip ('host') or mgpu_snip_device ('device')."""
    from readsb_amd import binding
    nout, run = C.c_uint64(0), C.c_uint64(int(c_in))
    a = binding.SnipArgs(C.sizeof(binding.SnipArgs), int(level), iq_ptr, n, out_ptr, cap, C.pointer(nout), C.pointer(run), pass_samples)
    f = d.lib.mgpu_snip if form == "host" else d.lib.mgpu_snip_device
    return int(f(d.ctx, C.byref(a))), int(nout.value), int(run.value)


def device_snip(d, hip, iq, level, c_in=0, offset=0, cap=None):
    """mgpu_snip_device with the output `offset` bytes behind a 64-byte boundary, between canaries.
    -> (rc, nout, quiet_run, output bytes up to the capacity, canaries intact)"""
    iq = bytes(iq)
    n = len(iq) // 2
    cap = n if cap is None else cap
    d_iq = hip.upload(np.frombuffer(iq, dtype=np.uint8)) if n else hip.malloc(16)
    room = GUARD + offset + 2 * cap + GUARD
    d_out = hip.malloc(room + 64)
    base = (d_out + 63) // 64 * 64
    hip.fill(base, 0xA5, room)
    rc, nout, run = snip_raw(d, "device", d_iq, n, level, base + GUARD + offset, cap, c_in)
    got = hip.download(base, room).tobytes()
    hip.free(d_iq)
    hip.free(d_out)
    lo, hi = GUARD + offset, GUARD + offset + 2 * min(nout, cap)
    intact = got[:lo] == b"\xa5" * lo and got[GUARD + offset + 2 * cap:] == b"\xa5" * GUARD
    if rc == su.MGPU_OK:
        intact = intact and got[hi: GUARD + offset + 2 * cap] == b"\xa5" * (2 * (cap - nout))      # nothing behind the kept samples either
    return rc, nout, run, got[lo:hi], intact


def check_both_forms(d, hip, iq, level, c_in=0, want=None):
    want = want or su.model(iq, level, c_in)
    got, run = d.snip(np.frombuffer(iq, dtype=np.uint8), level, quiet_run=c_in)
    assert (got.tobytes(), run) == want, "host form"
    rc, nout, run, out, intact = device_snip(d, hip, iq, level, c_in)
    assert rc == su.MGPU_OK and intact and (out, run) == want and 2 * nout == len(want[0]), "device form"


@pytest.mark.parametrize("level", su.LEVELS)
def test_crafted_stream(ctx, level):
    d, hip = ctx
    iq, want = _crafted(level)
    check_both_forms(d, hip, iq, level, want=want)
    if level == su.LEVELS[0]:
        assert su.have_reference(), f"{su.FULL} is missing: the GPU run would not have consulted the reference program"
        assert want[0] == su.reference_snip(iq, level)


def test_crafted_stream_against_the_reference_program_at_a_level_with_both_kinds(ctx):
    """Level -5 (the first case) has no quiet sample; the same comparison where the 32/33 boundary is exercised."""
    d, hip = ctx
    iq, want = _crafted(2)
    assert su.have_reference(), f"{su.FULL} is missing"
    ref = su.reference_snip(iq, 2)
    assert d.snip(np.frombuffer(iq, dtype=np.uint8), 2)[0].tobytes() == ref == want[0]


@pytest.mark.parametrize("density", [0.0, 1e-4, 1 / 33, 0.5, 1.0])
def test_random_streams(ctx, density):
    d, hip = ctx
    iq = su.random_stream(1 << 20, density, seed=int(density * 1e6) + 11)
    check_both_forms(d, hip, iq, 4)


@pytest.mark.parametrize("c_in", [0, 31, 32, 33, 1 << 40])
def test_all_quiet_stream_with_a_carry(ctx, c_in):
    d, hip = ctx
    iq = bytes([127, 126]) * 20001
    want = su.model(iq, 2, c_in)
    assert want == (iq[: 2 * max(0, 32 - c_in)], c_in + 20001)
    check_both_forms(d, hip, iq, 2, c_in, want)


def test_all_loud_stream(ctx):
    d, hip = ctx
    iq = bytes([127, 129, 0, 127, 255, 255]) * 6667
    check_both_forms(d, hip, iq, 2, 77, (iq, 0))


def test_cut_into_calls_device_form(ctx):
    """The crafted stream in calls at seeded random points, 0-sample and 1-sample calls among them, the counter carried and the calls
    appending into one buffer (so every call's output starts where the last one's ended: 2-byte alignment only) = one call."""
    d, hip = ctx
    level = 2
    iq, want = _crafted(level)
    n = len(iq) // 2
    bounds = su.cut_points(n, 40, seed=5)
    assert any(b == a for a, b in zip(bounds, bounds[1:])) and any(b == a + 1 for a, b in zip(bounds, bounds[1:]))
    d_out = hip.malloc(2 * n + GUARD)
    hip.fill(d_out, 0xA5, 2 * n + GUARD)
    produced = run = 0
    for a, b in zip(bounds, bounds[1:]):
        d_iq = hip.upload(np.frombuffer(iq[2 * a: 2 * b], dtype=np.uint8)) if b > a else hip.malloc(16)
        nout, run = d.snip_device(d_iq, b - a, level, d_out + 2 * produced, n - produced, quiet_run=run)
        produced += nout
        hip.free(d_iq)
    got = hip.download(d_out, 2 * n + GUARD).tobytes()
    hip.free(d_out)
    assert (got[: 2 * produced], run) == want
    assert got[2 * produced:] == b"\xa5" * (len(got) - 2 * produced)


@pytest.mark.parametrize("pass_samples", [1, 63, 64, 4097])
def test_cut_into_calls_and_passes_host_form(ctx, pass_samples):
    """The same through the host form, every call in passes of pass_samples samples through the library's scratch.
    pass_samples = 1 takes the stream's first 30 011 samples, the others all of it: a pass costs a copy in, four launches, a
    synchronisation and a copy out whatever its size (about 37 us measured), 7.5 s for the whole stream one sample at a time.  With one
    sample per pass every sample stands at position 0 of its tile, so only the carried counter decides — and the prefix takes it
    through every run length of the stream some fifteen times."""
    d, hip = ctx
    level = 2
    iq, want = _crafted(level)
    if pass_samples == 1:
        iq = iq[: 2 * 30011]
        want = su.model(iq, level)
    n = len(iq) // 2
    bounds = su.cut_points(n, 12, seed=6 + pass_samples)
    out, run = [], 0
    for a, b in zip(bounds, bounds[1:]):
        got, run = d.snip(np.frombuffer(iq[2 * a: 2 * b], dtype=np.uint8), level, quiet_run=run, pass_samples=pass_samples)
        out.append(got.tobytes())
    assert (b"".join(out), run) == want


@pytest.mark.parametrize("offset", [2, 6, 14, 30])
def test_placement_and_small_sizes(ctx, offset):
    d, hip = ctx
    level = 2
    stream = _crafted(level)[0]
    for n in (1, 2, 63, 64, 65, su.TILE - 1, su.TILE + 1, su.GROUP - 1, su.GROUP + 1):
        for start in (0, 2 * 7):                            # from a loud sample, and from inside a quiet run
            iq = stream[2 * start: 2 * (start + n)]
            for c_in in (0, 40):
                want = su.model(iq, level, c_in)
                rc, nout, run, out, intact = device_snip(d, hip, iq, level, c_in, offset=offset)
                assert rc == su.MGPU_OK and intact and (out, run) == want, (n, start, c_in)
    # a zero-sample call: MGPU_OK, nothing written, the counter as it was
    rc, nout, run, out, intact = device_snip(d, hip, b"", level, 9, offset=offset, cap=4)
    assert (rc, nout, run, out, intact) == (su.MGPU_OK, 0, 9, b"", True)


def test_capacity(ctx):
    d, hip = ctx
    level = 2
    iq, want = _crafted(level)
    kept = len(want[0]) // 2
    rc, nout, run, out, intact = device_snip(d, hip, iq, level, 5, offset=6, cap=kept)
    assert rc == su.MGPU_OK and intact and nout == kept and (out, run) == su.model(iq, level, 5)
    rc, nout, run, out, intact = device_snip(d, hip, iq, level, 5, offset=6, cap=kept - 1)
    assert rc == su.MGPU_E_OVERFLOW and nout == kept and intact and run == 5
    # the host form likewise, with the overflow found in a later pass: *nout is still what the whole input needs
    src = np.frombuffer(iq, dtype=np.uint8)
    for cap, code in ((kept, su.MGPU_OK), (kept - 1, su.MGPU_E_OVERFLOW), (0, su.MGPU_E_OVERFLOW)):
        buf = np.full(2 * kept + GUARD, 0xA5, dtype=np.uint8)
        rc, nout, run = snip_raw(d, "host", src.ctypes.data, len(iq) // 2, level, buf.ctypes.data, cap, 5, pass_samples=50000)
        assert (rc, nout) == (code, kept) and run == (want[1] if code == su.MGPU_OK else 5)
        assert buf[2 * cap:].tobytes() == b"\xa5" * (buf.size - 2 * cap)
        if code == su.MGPU_OK:
            assert buf[: 2 * kept].tobytes() == su.model(iq, level, 5)[0]
    # bad arguments with a live context: a misaligned device input, out overlapping iq
    d_iq = hip.upload(src[:4096])
    assert snip_raw(d, "device", d_iq + 2, 100, level, d_iq + 2048, 100)[0] == su.MGPU_E_INVAL
    assert snip_raw(d, "device", d_iq, 1000, level, d_iq + 1000, 100)[0] == su.MGPU_E_INVAL
    hip.free(d_iq)


def test_command_line_against_the_reference_program(built):
    """readsb_gpu_ifile --snip 4 on an odd-length stdin = readsb_full --snip 4: identical stdout, both exit 0."""
    assert su.have_reference(), f"{su.FULL} is missing"
    iq = su.random_stream(300001, 1 / 33, seed=21) + b"\x80"
    r = subprocess.run([CLI, "--snip", "4"], input=iq, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-500:]
    want = su.reference_snip(iq, 4)
    assert r.stdout == want and 0 < len(want) < len(iq) - 1
