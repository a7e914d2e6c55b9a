"""-m gpu: the beast wire encoder (kernels/beast.inc, mgpu_beast_encode*) on record lists that no sample ever produced, byte for byte
against tests/beast_util.py's numpy encoder (pinned on the CPU by tests/test_beast_reference.py).  There is no tolerance anywhere.

What the lists reach that a demodulated capture does not: k_beast_scan with several entries per thread (more than 262 144 messages),
every alignment of the output pointer and of a workgroup's first byte, whole workgroups of 44-byte frames (the LDS buffer's limit),
workgroups of a few bytes (the byte-copy fallback), a capacity that cuts a workgroup, 0x1a in every timestamp byte, timestamps at
and above 2^48 and negative ones, the signal byte on both sides of each of its 255 rounding boundaries and on them, verdict bytes of
the caller's choosing with deferred messages at the ends of waves and workgroups, and a deferred list shorter than the count.
Device-path outputs lie between guard bytes, which must come back untouched.

The conditions on a generated list (a frame of every length from 11 to 44, at least 1 % of records without a frame; gated: at
least 10 % each of frames, deferred and dropped) are asserted on the reference's output, for every list that is encoded (_cut puts the
ladder's records into each cut of the pool) except the windows of test_sizes and test_reuse_of_a_context, which are cut from the
pool as it is (on which they hold), the named worst-case lists and the all-one-verdict lists, which are what they are.
sig_len == 0 is the only input class left out: the level is then an infinity or a NaN whose conversion to int is undefined in
the reference, and modes_gpu.h documents sig_len as 134 or 268."""
import functools

import numpy as np
import pytest

import beast_util as bu
import helpers

pytestmark = pytest.mark.gpu

GUARD = 256
LARGE = 3 * 262144 + 17


@pytest.fixture(scope="module")
def ctx(built):
    import readsb_amd
    d = readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=1 << 20)
    hip = bu.Hip()
    try:
        yield d, hip
    finally:
        hip.free_all()
        d.close()


@functools.lru_cache(maxsize=None)
def _pool():
    msgs = bu.hostile_records(LARGE, 2024)
    ref = bu.beast_reference(msgs)
    bu.check_lengths(msgs, ref[1])
    return msgs, ref


def _cut(start, n):
    """n records of the pool from `start` on, the ladder's records among them; the list conditions hold for the cut itself."""
    msgs = bu.with_ladder(_pool()[0][start:start + n].copy())
    bu.check_lengths(msgs)
    return msgs


def _first_diff(got, want):
    if len(got) != len(want):
        return f"{len(got)} bytes, want {len(want)}"
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    k = int(np.nonzero(a != b)[0][0])
    return f"first difference at byte {k} of {len(want)}: got {got[k:k + 16].hex()} want {want[k:k + 16].hex()}"


def _same(got, want):
    assert got == want, _first_diff(got, want)


def _device(d, hip, msgs, want, k=0, cap=None, expect_overflow=False, whole_before=None):
    """mgpu_beast_encode_device into guard | k bytes | cap bytes | guard, all 0xA5 before the call."""
    T = len(want)
    cap = T if cap is None else cap
    d_in = hip.upload(msgs)
    total = GUARD + k + max(cap, T) + GUARD
    d_buf = hip.malloc(total)
    try:
        hip.fill(d_buf, 0xA5, total)
        rc, nb, _ = bu.encode_raw(d, d_in, len(msgs), d_buf + GUARD + k, cap)
        buf = hip.download(d_buf, total)
    finally:
        hip.free(d_buf)
        hip.free(d_in)
    at = GUARD + k
    assert nb == T, (nb, T)
    assert (buf[:at] == 0xA5).all(), f"bytes before the output were written (offset {k})"
    if expect_overflow:
        assert rc == bu.MGPU_E_OVERFLOW, rc
        assert (buf[at + cap:] == 0xA5).all(), f"bytes at or beyond the capacity {cap} were written"
        _same(buf[at:at + whole_before].tobytes(), want[:whole_before])
    else:
        assert rc == 0, rc
        _same(buf[at:at + T].tobytes(), want)
        assert (buf[at + T:] == 0xA5).all(), f"bytes behind the stream were written (offset {k})"


# ---- sizes: the scan with one and with several entries per thread -----------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 262143, 262144, 262145, LARGE])
def test_sizes(ctx, n):
    d, hip = ctx
    pool, (pstream, plength, _) = _pool()
    if n < 1000:                                                     # a few windows of the list: single records need not have a frame
        starts = [0, 1000, 4321, 70001, 262144 - n, 524288 - n // 2, LARGE - n]
    else:
        starts = [0 if n != 262143 else 5]
    ends = np.cumsum(plength)
    nonempty = 0
    for s in starts:
        msgs = pool[s:s + n]
        want = pstream[int(ends[s] - plength[s]):int(ends[s + n - 1])]
        if n in (257, 262145):
            assert want == bu.beast_reference(msgs)[0]               # a slice of the list's stream is the slice's stream
        nonempty += len(want) > 0
        _same(d.beast_encode(msgs), want)
        if n >= 262145:
            assert bu.scan_per(n) >= 2
            _device(d, hip, msgs, want)
    assert nonempty >= len(starts) - 1
    assert (bu.scan_per(n) >= 2) == (n > 262144)


# ---- worst case: the LDS buffer full, workgroups of a few bytes -------------------------------------------------------------------

def _all_escaped(n):
    m = np.zeros(n, dtype=bu.MSG)
    m["msgbits"], m["timestamp"], m["msg"] = 112, 0x1A1A1A1A1A1A, 0x1A
    m["sig_sumsq"], m["sig_len"] = bu._sumsq_for(0x1A)
    return m


def _lead(length):
    """One frame of 11 (Mode A/C), 17 or 18 bytes (short, one or two doubled bytes)."""
    m = np.zeros(1, dtype=bu.MSG)
    m["msgbits"], m["sig_len"], m["sig_sumsq"] = (16 if length == 11 else 56), 134, 1 << 30
    m["timestamp"] = {11: 0x010203040506, 17: 0x01020304051A, 18: 0x0102031A051A}[length]
    m["msg"] = 0x42
    return m


def _one_per_workgroup(blocks):
    m = np.zeros(blocks * bu.BLOCK, dtype=bu.MSG)
    m["msgbits"] = 255
    m["sig_len"], m["sig_sumsq"], m["timestamp"] = 268, 1 << 30, 0x0A0B0C0D0E0F
    m["msg"] = np.arange(14) + 1
    for b in range(blocks):
        m["msgbits"][b * bu.BLOCK + (b * 37 + (255 if b == 1 else 0)) % bu.BLOCK] = (16, 56, 112)[b % 3]
    return m


def _single_mode_ac(n, at):
    m = np.zeros(n, dtype=bu.MSG)
    m["msgbits"], m["sig_len"] = 0, 134
    m[at] = _lead(11)[0]
    return m


WORST = {
    "all_44": lambda: _all_escaped(1024),
    "lead_11_then_44": lambda: np.concatenate([_lead(11), _all_escaped(1024)]),
    "lead_17_then_44": lambda: np.concatenate([_lead(17), _all_escaped(1024)]),
    "lead_18_then_44": lambda: np.concatenate([_lead(18), _all_escaped(1024)]),
    "one_frame_per_workgroup": lambda: _one_per_workgroup(9),
    "single_mode_ac_frame": lambda: _single_mode_ac(1, 0),
    "single_mode_ac_frame_among_300": lambda: _single_mode_ac(300, 299),
}


@pytest.mark.parametrize("name", sorted(WORST))
def test_worst_case(ctx, name):
    d, hip = ctx
    msgs = WORST[name]()
    want, length, _ = bu.beast_reference(msgs)
    if "44" in name:
        assert (length[-1024:] == 44).all()
        lead = int(name.split("_")[1]) if name.startswith("lead") else 0
        assert len(msgs) == 1024 + (lead > 0) and (lead == 0 or length[0] == lead)
        # every workgroup behind the first starts at the lead frame's alignment
        starts = (np.cumsum(length) - length)[bu.BLOCK::bu.BLOCK]
        assert len(starts) >= 3 and (starts % 4 == lead % 4).all()
    elif name == "one_frame_per_workgroup":
        per_block = (length.reshape(-1, bu.BLOCK) > 0).sum(axis=1)
        assert (per_block == 1).all() and set(length[length > 0].tolist()) == {11, 16, 23}
    else:
        assert len(want) == 11 and (length > 0).sum() == 1
    _same(d.beast_encode(msgs), want)
    for k in range(4):
        _device(d, hip, msgs, want, k=k)


# ---- alignment and stray writes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(8))
def test_output_alignment_and_guards(ctx, k):
    d, hip = ctx
    msgs = _cut(40000, 20 * bu.BLOCK + 99)
    want, length, _ = bu.beast_reference(msgs)
    starts = (np.cumsum(length) - length)[::bu.BLOCK]
    assert set((starts % 4).tolist()) == {0, 1, 2, 3}                # with the pointer's k: every misalignment, at every k
    _device(d, hip, msgs, want, k=k)


# ---- capacity ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [0, 3])
def test_capacity(ctx, k):
    d, hip = ctx
    msgs = _cut(90000, 12 * bu.BLOCK + 31)
    want, length, _ = bu.beast_reference(msgs)
    T = len(want)
    block_end = np.cumsum(np.add.reduceat(length, np.arange(0, len(msgs), bu.BLOCK)))
    assert block_end[-1] == T and T > 12 * 256 * 11
    _device(d, hip, msgs, want, k=k, cap=T)
    inside_first = int(block_end[0]) // 2 + 1
    for cap in (T - 1, T - 4, T // 2, inside_first, 0):
        whole = int(block_end[block_end <= cap].max()) if (block_end <= cap).any() else 0
        assert (cap >= block_end[0]) == (whole > 0)
        _device(d, hip, msgs, want, k=k, cap=cap, expect_overflow=True, whole_before=whole)
    _device(d, hip, msgs, want, k=k)                                  # the context encodes correctly afterwards
    _same(d.beast_encode(msgs), want)


# ---- the signal byte --------------------------------------------------------------------------------------------------------------------

def test_signal_byte_at_every_boundary(ctx):
    d, hip = ctx
    msgs = bu.signal_records(77)
    bu.check_lengths(msgs)
    want, length, _ = bu.beast_reference(msgs)
    framed = length > 0                                              # what follows: of the records that do produce a frame
    sig, x = bu.signal_byte(msgs["sig_sumsq"], msgs["sig_len"])
    sig, x, lens = sig[framed], x[framed], msgs["sig_len"][framed]
    assert framed.sum() >= 255 * 4 * 5 * 0.9 and set(sig.tolist()) == set(range(256))
    for ln in bu.SIG_LENS:
        assert 0x1A in sig[lens == ln]
    ties = (x == np.floor(x) + 0.5) & (x > 1) & (x < 255)
    assert (ties & (np.floor(x) % 2 == 0)).sum() >= 20 and (ties & (np.floor(x) % 2 == 1)).sum() >= 20
    _same(d.beast_encode(msgs), want)
    _device(d, hip, msgs, want, k=1)


# ---- the gated form, verdicts supplied ------------------------------------------------------------------------------------------------

DEF_GUARD = 16


def _gated(d, hip, msgs, verdict, net_rule, deferred_cap=None, k=0):
    """mgpu_beast_encode_gated_device; the deferred list lies before DEF_GUARD entries of 0xA5 bytes."""
    want, _, wdef = bu.beast_reference(msgs, verdict, net_rule)
    T, D = len(want), len(wdef)
    dcap = D if deferred_cap is None else deferred_cap
    d_in, d_v = hip.upload(msgs), hip.upload(verdict)
    total = GUARD + k + T + GUARD
    d_buf, d_def = hip.malloc(total), hip.malloc((dcap + DEF_GUARD) * bu.DEFERRED.itemsize)
    try:
        hip.fill(d_buf, 0xA5, total)
        hip.fill(d_def, 0xA5, (dcap + DEF_GUARD) * bu.DEFERRED.itemsize)
        if dcap >= D:
            nb, nd = d.beast_encode_gated_device(d_in, d_v, len(msgs), d_buf + GUARD + k, T, d_def, dcap, net_rule=net_rule)
            rc = 0
        else:
            rc, nb, nd = bu.encode_raw(d, d_in, len(msgs), d_buf + GUARD + k, T, d_verdict=d_v, net_rule=net_rule, d_deferred=d_def, deferred_cap=dcap)
        buf = hip.download(d_buf, total)
        got_def = hip.download(d_def, (dcap + DEF_GUARD) * bu.DEFERRED.itemsize, dtype=bu.DEFERRED)
    finally:
        for p in (d_buf, d_def, d_v, d_in):
            hip.free(p)
    at = GUARD + k
    assert (nb, nd) == (T, D), (nb, nd, T, D)
    assert rc == (0 if dcap >= D else bu.MGPU_E_OVERFLOW), rc
    assert (buf[:at] == 0xA5).all() and (buf[at + T:] == 0xA5).all(), "bytes outside the stream were written"
    listed = min(dcap, D)
    bad = np.nonzero(got_def[:listed] != wdef[:listed])[0]
    assert len(bad) == 0, f"{len(bad)} of {listed} deferred entries differ, first at {bad[:3]}: got {got_def[bad[:3]]} want {wdef[bad[:3]]}"
    assert (got_def[listed:].view(np.uint8) == 0xA5).all(), "entries behind the list were written"
    _same(buf[at:at + T].tobytes(), want)                            # also when the list overflowed: the stream had room
    return T, D


@pytest.mark.parametrize("net_rule", [False, True])
def test_gated_random_verdicts(ctx, net_rule):
    d, hip = ctx
    msgs = _cut(120000, 20000 + 3)
    v = bu.random_verdicts(len(msgs), 31)
    assert (v > 3).mean() > 0.9
    bu.check_gated(msgs, v, net_rule)
    T, D = _gated(d, hip, msgs, v, net_rule, k=int(net_rule) * 3)
    assert T > 0 and D > 0
    if net_rule:                                                     # correctedbits of 2 made a difference, for frames and for deferred entries
        s0, _, d0 = bu.beast_reference(msgs, v, False)
        assert len(s0) > T and len(d0) > D


@pytest.mark.parametrize("value", [0, 1, 2, 3])
def test_gated_all_one_verdict(ctx, value):
    d, hip = ctx
    msgs = _cut(200000, 5 * bu.BLOCK + 200)
    carried = int((bu.beast_reference(msgs)[1] > 0).sum())
    for upper in (0, 0xFC):
        v = np.full(len(msgs), value | upper, dtype=np.uint8)
        T, D = _gated(d, hip, msgs, v, False)
        assert (T > 0, D) == (value == 1, carried if value == 2 else 0)


def test_gated_deferred_at_the_ends_of_waves_and_workgroups(ctx):
    d, hip = ctx
    msgs = _cut(300000, 6 * bu.BLOCK + 77)
    v = bu.random_verdicts(len(msgs), 32)
    ends = np.concatenate([np.arange(0, len(msgs), bu.BLOCK) + lane for lane in (0, 63, 64, 255)] + [[6 * bu.BLOCK + 76]])
    ends = ends[ends < len(msgs)]
    v[ends] = (v[ends] & 0xFC) | 2
    msgs["msgbits"][ends] = np.array([112, 56, 16])[ends % 3]
    msgs["correctedbits"][ends] = 0
    bu.check_lengths(msgs)
    bu.check_gated(msgs, v, True)
    for net_rule in (False, True):
        wdef = bu.beast_reference(msgs, v, net_rule)[2]
        assert set(ends.tolist()) <= set(wdef["index"].tolist())
        _gated(d, hip, msgs, v, net_rule, k=1)


def test_gated_scan_with_several_entries_per_thread(ctx):
    d, hip = ctx
    n = 2 * 262144 + 300
    msgs = _cut(100, n)
    v = bu.random_verdicts(n, 33)
    assert bu.scan_per(n) >= 2
    bu.check_gated(msgs, v, True)
    T, D = _gated(d, hip, msgs, v, True)
    assert D > 262144 // 8


def test_gated_deferred_list_too_short(ctx):
    d, hip = ctx
    msgs = _cut(400000, 5000)
    v = bu.random_verdicts(len(msgs), 34)
    bu.check_gated(msgs, v, False)
    D = len(bu.beast_reference(msgs, v, False)[2])
    assert D > 500
    for dcap in (D, D - 1, 0):
        _gated(d, hip, msgs, v, False, deferred_cap=dcap)
    _gated(d, hip, msgs, v, False)


# ---- scratch grown once and reused ----------------------------------------------------------------------------------------------------

def test_reuse_of_a_context(built):
    import readsb_amd
    pool, _ = _pool()
    d = readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=1 << 20)
    try:
        for s, n in ((0, 300000), (300000, 100), (300100, 370000), (5, 300000)):   # 370 000 fits the scratch the first call reserved (n + n / 4 + 1024)
            msgs = pool[s:s + n]
            _same(d.beast_encode(msgs), bu.beast_reference(msgs)[0])
    finally:
        d.close()
