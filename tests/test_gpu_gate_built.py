"""-m gpu: the tracking gate on the device (kernels/gate.inc) on BUILT lists — tests/gate_util.py says which message sits where, and
tests/test_oracle_gate_built.py that the lists hold what they claim.  mgpu_track_gate_device with the caller's field records
against the CPU restatement (oracle/modes_oracle_gate.c) on the same arrays, every verdict byte with ==: the thresholds at the
limit and 1 ms beyond it with the two messages at chosen lanes of the walk's steps, runs that end on a step and beside it, the
batch cut, the buffer a message is counted in, the edge addresses at the sizes at which the sorting waves share the keys
differently, and lists handed over in several calls — the state a call leaves in the table only for the next one to read."""
import ctypes as C

import numpy as np
import pytest

import gate_util as gu

pytestmark = pytest.mark.gpu

_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipFree.argtypes = [C.c_void_p]
    return _hip


@pytest.fixture(scope="module")
def dev(built):
    import helpers
    import readsb_amd
    d = readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=1 << 20)
    yield d
    d.close()


def gate_calls(d, msgs, fields, cuts=()):
    """The list in HBM once, mgpu_track_gate_device on each call's slice of it (messages, field records, verdict bytes), on the
    table as it stands: -> all verdict bytes."""
    h = hip()
    msgs, fields = np.ascontiguousarray(msgs), np.ascontiguousarray(fields)
    n = len(msgs)
    d_msgs, d_fields, d_v = C.c_void_p(), C.c_void_p(), C.c_void_p()
    try:
        assert h.hipMalloc(C.byref(d_msgs), msgs.nbytes) == 0 and h.hipMalloc(C.byref(d_fields), fields.nbytes) == 0 and h.hipMalloc(C.byref(d_v), n) == 0
        assert h.hipMemcpy(d_msgs, msgs.ctypes.data, msgs.nbytes, 1) == 0 and h.hipMemcpy(d_fields, fields.ctypes.data, fields.nbytes, 1) == 0
        edges = [0] + [int(c) for c in cuts] + [n]
        for a, b in zip(edges[:-1], edges[1:]):
            assert a < b
            d.track_gate_device(d_msgs.value + a * msgs.itemsize, d_fields.value + a * fields.itemsize, b - a, d_v.value + a)
        v = np.empty(n, dtype=np.uint8)
        assert h.hipMemcpy(v.ctypes.data, d_v, n, 2) == 0
        return v
    finally:
        for p in (d_msgs, d_fields, d_v):
            if p.value:
                h.hipFree(p)


def run_case(dev, case, cuts=None):
    cuts = case.cuts if cuts is None else cuts
    dev.track_gate_reset()
    got = gate_calls(dev, case.msgs, case.fields, cuts)
    want = gu.oracle_gate_stepped(case.raw, cuts)
    diff = gu.first_difference(case, got, want)
    assert diff is None, diff
    return got


def check_by_hand(case, v):
    for i, want, what in case.expect:
        assert (v[i] & 3) == want, f"{what}: verdict {v[i] & 3}, by hand {want} ({case.row(i)})"


@pytest.mark.parametrize("name", list(gu.built_cases()))
def test_built_list(dev, name):
    """Every built list in the calls it is made for (one, unless the case is about the table a call leaves behind): thresholds and
    their lane matrix, batch cuts, buffers, runs alone / interleaved / on a primed table, addresses at the sort's sizes."""
    case = gu.built_case(name)
    v = run_case(dev, case)
    check_by_hand(case, v)


@pytest.mark.parametrize("name", ["pairs"] + [f"lanes_{k}" for k in gu.KINDS] + [f"primed_{n}_{p}" for n in gu.RUN_LENGTHS for p in gu.PRIMES])
def test_built_list_in_one_call(dev, name):
    """The lists that come in several calls, in one — and both ways the same verdicts."""
    case = gu.built_case(name)
    one = run_case(dev, case, cuts=[])
    assert np.array_equal(one, run_case(dev, case))
    check_by_hand(case, one)


def test_call_cuts(dev):
    """Three hours in one call, in two, and buffer by buffer: the same verdicts, and the restatement's stepped over the same cuts."""
    case = gu.built_case("callcut")
    one = run_case(dev, case, cuts=[])
    two = run_case(dev, case, cuts=case.note["two"])
    each = run_case(dev, case, cuts=case.note["each"])
    assert np.array_equal(one, two) and np.array_equal(one, each)


@pytest.mark.parametrize("kind", list(gu.KINDS))
def test_threshold_across_calls(dev, kind):
    """The referred message is the last of one call, the tested one the first of the next: what the first call wrote into the table
    (seen_lo / exists bit 0, seen_hi, cpr_first) decides, at the limit and 1 ms beyond it."""
    case = gu.built_case(f"cut_{kind}")
    assert case.cuts and case.expect[0][0] in case.cuts
    v = run_case(dev, case)
    check_by_hand(case, v)
    _, _, _, v_at, v_beyond, _ = gu.KINDS[kind]
    assert [int(v[i] & 3) for i, _, _ in case.expect] == [v_at, v_beyond]


def test_host_form(dev):
    """The list as sealed frames through mgpu_track_gate, which decodes the fields itself: equal to the device form on
    decode_fields' records, and to the restatement."""
    case = gu.built_case("host")
    msgs = case.msgs.copy()
    frames = gu.frames_of(case)
    msgs["msg"], msgs["raw"] = frames, frames
    fields = dev.decode_fields(msgs)
    assert np.array_equal(fields["addr"], case.raw["addr"]) and np.array_equal(fields["IID"], case.raw["iid"])
    assert np.array_equal((fields["flags"] & gu.F_CPR_VALID) != 0, case.raw["cpr"] != 0)
    want = gu.oracle_gate_stepped(case.raw)
    dev.track_gate_reset()
    host = dev.track_gate(msgs)
    diff = gu.first_difference(case, host, want)
    assert diff is None, diff
    dev.track_gate_reset()
    device = gate_calls(dev, msgs, fields)
    diff = gu.first_difference(case, device, want)
    assert diff is None, diff
    assert not gu.coverage_gaps(host)
