"""The aggregator's output on the GPU: the stable time merge of several receivers' lists (kernels/merge.inc) against numpy's stable
argsort over the concatenation, the beast encoder with receiver ids and --net-verbatim (kernels/beast.inc) against
tests/beast_ids_util.py, and the chain of both against the whole reference program's file — whole outputs, byte for byte.

Shapes: the merge's sorting waves own contiguous pieces of 64-key steps and there are 4 of them per 1024 keys (at most 1024), so
n = 1 .. 257 covers fewer keys than waves, a step that is not full and pieces of one step; 2 * 128 * 64 + 1 gives every wave
several steps.  The encoder's workgroups hold 256 messages: ids that change every 1 / 64 / 256 / 257 messages put the change
inside a wave, on a wave's edge, on a workgroup's edge and walking across both."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import beast_ids_util as biu
import beast_util as bu
import helpers

pytestmark = pytest.mark.gpu

GUARD = 256
MGPU_E_INVAL, MGPU_E_CAPACITY = -1, -6


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
    return bu.hostile_records(40000, 4711)


@functools.lru_cache(maxsize=None)
def _pool_ref(every, gated, net_rule=False):
    msgs = _pool()
    ids = biu.ids_changing_every(len(msgs), every, 3)
    verdict = bu.random_verdicts(len(msgs), 11) if gated else None
    return ids, verdict, biu.beast_reference(msgs, verdict, net_rule, ids=ids, last_id=0)


def _same(got, want):
    if got != want:
        a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
        m = min(len(a), len(b))
        diff = np.nonzero(a[:m] != b[:m])[0]
        k = int(diff[0]) if len(diff) else m
        raise AssertionError(f"{len(got)} bytes, want {len(want)}; first difference at byte {k}: got {got[k:k + 20].hex()} want {want[k:k + 20].hex()}")


# ---- the merge ------------------------------------------------------------------------------------------------------------------

def _merge_want(lists, ids, verdicts):
    allm = np.concatenate(lists) if lists else np.zeros(0, dtype=bu.MSG)
    order = np.argsort(allm["timestamp"], kind="stable")
    seg = np.repeat(np.arange(len(lists)), [len(m) for m in lists])
    want_ids = np.asarray(ids, dtype=np.uint64)[seg[order]] if len(lists) else np.zeros(0, dtype=np.uint64)
    want_v = np.concatenate(verdicts)[order] if verdicts is not None and len(lists) else None
    return allm[order], order.astype(np.uint64), want_ids, want_v


def _merge_device(d, hip, lists, ids, verdicts):
    """mgpu_merge_by_time_device on one allocation per list, every output between guards.  -> (records, perm, ids, verdicts)"""
    n = sum(len(m) for m in lists)
    d_lists = [hip.upload(m) for m in lists]
    d_ver = [hip.upload(v) for v in verdicts] if verdicts is not None else None
    sizes = [n * 64, n * 8, n * 8, n]
    bufs = [hip.malloc(2 * GUARD + s) for s in sizes]
    try:
        for b, s in zip(bufs, sizes):
            hip.fill(b, 0xA5, 2 * GUARD + s)
        got_n = d.merge_by_time_device(d_lists, [len(m) for m in lists], bufs[0] + GUARD, ids=ids, d_verdict_ptrs=d_ver, d_perm_ptr=bufs[1] + GUARD,
                                       d_ids_ptr=bufs[2] + GUARD, d_verdict_out_ptr=(bufs[3] + GUARD) if verdicts is not None else None)
        assert got_n == n
        raw = [hip.download(b, 2 * GUARD + s) for b, s in zip(bufs, sizes)]
    finally:
        for p in bufs + d_lists + (d_ver or []):
            hip.free(p)
    for r, s in zip(raw, sizes):
        assert (r[:GUARD] == 0xA5).all() and (r[GUARD + s:] == 0xA5).all(), "bytes outside an output were written"
    body = [r[GUARD:GUARD + s] for r, s in zip(raw, sizes)]
    return body[0].view(bu.MSG), body[1].view(np.uint64), body[2].view(np.uint64), body[3] if verdicts is not None else None


def _check_merge(d, hip, lists, ids=None, with_verdicts=True, passes=None):
    ids = [0x100 + 3 * k for k in range(len(lists))] if ids is None else ids
    rng = np.random.default_rng(len(lists))
    verdicts = [rng.integers(0, 256, size=len(m)).astype(np.uint8) for m in lists] if with_verdicts else None
    want = _merge_want(lists, ids, verdicts)
    got = _merge_device(d, hip, lists, ids, verdicts)
    assert np.array_equal(got[1], want[1]), "permutation"
    assert got[0].tobytes() == want[0].tobytes(), "records"
    assert np.array_equal(got[2], want[2]), "ids"
    if with_verdicts:
        assert np.array_equal(got[3], want[3]), "verdicts"
    if passes is not None:
        assert d.merge_last_passes() == passes
    return want


def _split(msgs, nseg, seed):
    cuts = np.sort(np.random.default_rng(seed).integers(0, len(msgs) + 1, size=nseg - 1))
    return [m.copy() for m in np.split(msgs, cuts)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 129, 257, 2 * 128 * 64 + 1])
def test_merge_sizes(ctx, n):
    """Three unsorted segments of the hostile list (stamps over all 64 bits, negative ones, 2^48 and above, many equal)."""
    d, hip = ctx
    msgs = _pool()[1000:1000 + n]
    if n > 2:
        assert (msgs["timestamp"] < 0).any() and (msgs["timestamp"] >= 1 << 48).any()
    _check_merge(d, hip, _split(msgs, 3, n))
    if n > 1000:
        assert d.merge_last_passes() == 8 and len(np.unique(msgs["timestamp"])) < n


def test_merge_one_sorted_segment_is_the_identity(ctx):
    d, hip = ctx
    msgs = _pool()[:3000].copy()
    msgs = msgs[np.argsort(msgs["timestamp"], kind="stable")]
    want = _check_merge(d, hip, [msgs])
    assert np.array_equal(want[1], np.arange(len(msgs), dtype=np.uint64))


def test_merge_256_segments_most_of_them_empty(ctx):
    d, hip = ctx
    msgs = _pool()[:5000]
    lists = [np.zeros(0, dtype=bu.MSG) for _ in range(256)]
    for k, part in zip((3, 4, 100, 254, 255), _split(msgs, 5, 8)):
        lists[k] = part
    _check_merge(d, hip, lists, ids=[(0x1A << 56) | k for k in range(256)])


def test_merge_all_stamps_equal_keeps_the_input_order(ctx):
    d, hip = ctx
    msgs = _pool()[:4097].copy()
    msgs["timestamp"] = -5
    want = _check_merge(d, hip, _split(msgs, 3, 1), passes=0)
    assert np.array_equal(want[1], np.arange(len(msgs), dtype=np.uint64))


@pytest.mark.parametrize("shift,passes", [(0, 1), (40, 6), (56, 8)])
def test_merge_stamps_that_differ_in_one_digit(ctx, shift, passes):
    """Only the digit passes up to the highest differing bit run: 1 for the lowest digit, all below it for a high one."""
    d, hip = ctx
    msgs = _pool()[:6000].copy()
    digit = np.random.default_rng(shift).integers(0, 256, size=len(msgs)).astype(np.uint64) << np.uint64(shift)
    msgs["timestamp"] = (np.uint64(0x0012345678123456) & ~(np.uint64(0xFF) << np.uint64(shift)) | digit).view(np.int64)
    _check_merge(d, hip, _split(msgs, 3, 2), passes=passes)


def test_merge_piecewise_ordered_segments(ctx):
    """As Mode A/C leaves a receiver's list: per sample buffer the Mode S messages in order, then the buffer's Mode A/C replies."""
    d, hip = ctx
    rng = np.random.default_rng(6)
    lists = []
    for r in range(2):
        parts = []
        for b in range(12):
            lo = 1000 + b * 655360 + r * 7
            parts += [np.sort(rng.integers(lo, lo + 655360, size=300)), np.sort(rng.integers(lo, lo + 655360, size=80))]
        m = _pool()[: 12 * 380].copy()
        m["timestamp"] = np.concatenate(parts)
        assert (np.diff(m["timestamp"]) < 0).sum() >= 12
        lists.append(m)
    _check_merge(d, hip, lists, passes=3)


def test_merge_host_arrays_equal_the_device_form(ctx):
    d, hip = ctx
    lists = _split(_pool()[:9000], 4, 5)
    ids = [0, 0x1A1A1A1A1A1A1A1A, biu.MASK64, 7]
    verdicts = [np.full(len(m), k, dtype=np.uint8) for k, m in enumerate(lists)]
    want = _merge_want(lists, ids, verdicts)
    out, perm, oid, vout = d.merge_by_time(lists, ids=ids, verdicts=verdicts)
    assert out.tobytes() == want[0].tobytes() and np.array_equal(perm, want[1]) and np.array_equal(oid, want[2]) and np.array_equal(vout, want[3])
    assert d.merge_by_time([])[0].size == 0


def test_merge_limits(ctx):
    d, _ = ctx
    one = (C.c_void_p * 4097)()
    counts = np.zeros(4097, dtype=np.uint64)
    rc = d.lib.mgpu_merge_by_time_device(d.ctx, C.cast(one, C.c_void_p), C.c_void_p(counts.ctypes.data), 4097, None, None, None, None, None, None)
    assert rc == MGPU_E_INVAL
    counts[:2] = 0xFFFFFFFF
    one[0] = one[1] = 0x1000
    rc = d.lib.mgpu_merge_by_time_device(d.ctx, C.cast(one, C.c_void_p), C.c_void_p(counts.ctypes.data), 2, None, None, C.c_void_p(0x1000), None, None, None)
    assert rc == MGPU_E_CAPACITY


# ---- the encoder ------------------------------------------------------------------------------------------------------------------

def _encode(d, hip, msgs, verdict=None, ids=None, net_rule=False, verbatim=False, last_id=0, cap=None, want_len=None):
    """mgpu_beast_encode_ex_device itself into guard | cap bytes | guard.  -> (rc, stream bytes up to *bytes or cap, *bytes, deferred[],
    *ndeferred, last id, everything behind those stream bytes up to the end of the trailing guard)"""
    from readsb_amd.binding import BeastArgs
    n = len(msgs)
    room = n * 62 + 64 if cap is None else max(cap, want_len or 0)
    cap = room if cap is None else cap
    d_in = hip.upload(msgs)
    d_v = hip.upload(verdict) if verdict is not None else None
    d_ids = hip.upload(np.asarray(ids, dtype=np.uint64)) if ids is not None else None
    d_def = hip.malloc(max(n, 1) * 16)
    d_buf = hip.malloc(2 * GUARD + room)
    try:
        hip.fill(d_buf, 0xA5, 2 * GUARD + room)
        nb, nd, last = C.c_uint64(0), C.c_uint64(7777), C.c_uint64(int(last_id))
        a = BeastArgs(C.sizeof(BeastArgs), (1 if net_rule else 0) | (2 if verbatim else 0), d_in, n, d_v, d_ids, C.pointer(last), d_buf + GUARD, cap,
                      C.pointer(nb), d_def, n, C.pointer(nd))
        rc = int(d.lib.mgpu_beast_encode_ex_device(d.ctx, C.byref(a)))
        buf = hip.download(d_buf, 2 * GUARD + room)
        deferred = hip.download(d_def, 16 * min(int(nd.value), n), bu.DEFERRED) if rc == 0 else None
    finally:
        for p in (d_in, d_v, d_ids, d_def, d_buf):
            if p is not None:
                hip.free(p)
    assert (buf[:GUARD] == 0xA5).all(), "bytes before the output were written"
    end = GUARD + min(int(nb.value), cap)
    return rc, buf[GUARD:end].tobytes(), int(nb.value), deferred, int(nd.value), int(last.value), buf[end:]


def _check_encode(d, hip, msgs, verdict, ids, net_rule=False, verbatim=False, last_id=0):
    want, _, wdef, wlast, _ = biu.beast_reference(msgs, verdict, net_rule, verbatim, ids, last_id)
    rc, got, nb, deferred, nd, last, behind = _encode(d, hip, msgs, verdict, ids, net_rule, verbatim, last_id)
    assert rc == 0 and nb == len(want), (rc, nb, len(want))
    _same(got, want)
    assert (behind == 0xA5).all(), "bytes behind the stream were written"
    assert nd == len(wdef) and np.array_equal(deferred, wdef)
    if ids is not None:
        assert last == wlast
    return want


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("every", [1, 64, 256, 257, 0])
def test_ids_on_the_hostile_list(ctx, every, gated):
    d, hip = ctx
    msgs = _pool()
    ids, verdict, (want, total, wdef, wlast, plen) = _pool_ref(every, gated)
    if every:
        assert (plen > 10).sum() >= 5 and (plen == 10).sum() >= 5
        assert every != 1 or total.max() >= 55
    else:
        assert (plen > 0).sum() == 1
    rc, got, nb, deferred, nd, last, behind = _encode(d, hip, msgs, verdict, ids)
    assert rc == 0 and nb == len(want), (rc, nb, len(want))
    _same(got, want)
    assert (behind == 0xA5).all(), "bytes behind the stream were written"
    assert nd == len(wdef) and np.array_equal(deferred, wdef) and last == wlast
    if gated:
        assert len(wdef) > 1000


def test_ids_with_the_network_rule(ctx):
    d, hip = ctx
    ids, verdict, _ = _pool_ref(1, True)
    _check_encode(d, hip, _pool(), verdict, ids, net_rule=True, last_id=int(ids[0]))


@pytest.mark.parametrize("same", [True, False])
def test_three_workgroups_without_a_caller_between_two_callers(ctx, same):
    """The previous caller's id has to pass through workgroups that have none."""
    d, hip = ctx
    msgs = _pool()[: 5 * 256].copy()
    msgs["msgbits"] = 112
    verdict = np.zeros(len(msgs), dtype=np.uint8)
    a, b = 100, 4 * 256 + 50
    verdict[[a, b]] = 1
    ids = np.full(len(msgs), 0x55, dtype=np.uint64)                  # what the dropped messages carry must not matter
    ids[a] = 0x1A00000000000022
    ids[b] = ids[a] if same else 0x11
    want = _check_encode(d, hip, msgs, verdict, ids)
    assert [rid for rid, _ in biu.read_beast(want)] == [int(ids[a]), int(ids[b])]


@pytest.mark.parametrize("at", [255, 511, 63])
def test_a_record_the_format_does_not_carry_as_last_caller(ctx, at):
    """The reference's quirk at the end of a workgroup (and of a wave): such a caller writes nothing, not even a prefix, yet moves
    the writer's id — the next workgroup's first frame, of that id, has no prefix; of another id, has one."""
    d, hip = ctx
    msgs = _pool()[: 4 * 256].copy()
    msgs["msgbits"] = 56
    msgs["msgbits"][at] = 24
    for nxt in (0x77, 0x1A1A):
        ids = np.full(len(msgs), 0x1A1A, dtype=np.uint64)
        ids[at] = 0x77
        ids[at + 1:] = nxt
        want, _, _, _, plen = biu.beast_reference(msgs, ids=ids)
        assert plen[at] == 0 and (plen[at + 1] > 0) == (nxt != 0x77) and plen[0] > 0
        _check_encode(d, hip, msgs, None, ids)
    # ... and as the very last record of a call: the id is handed on
    ids = np.full(at + 1, 3, dtype=np.uint64)
    ids[at] = 0x1A
    rc, _, _, _, _, last, _ = _encode(d, hip, msgs[: at + 1], None, ids, last_id=3)
    assert rc == 0 and last == 0x1A


@pytest.mark.parametrize("cut", [1, 255, 256, 1000])
def test_cut_lists_give_the_bytes_of_one_call(ctx, cut):
    """7000 records in one call and in calls of `cut` with last_id threaded through: the same bytes, the same final id."""
    d, hip = ctx
    msgs = _pool()[20000:27000]
    ids = biu.ids_changing_every(len(msgs), 3, 5)
    verdict = bu.random_verdicts(len(msgs), 6)
    want, _, _, wlast, _ = biu.beast_reference(msgs, verdict, ids=ids, last_id=9)
    out, last = bytearray(), 9
    for a in range(0, len(msgs), cut):
        stream, _, last = d.beast_encode_ex(msgs[a:a + cut], verdict=verdict[a:a + cut], ids=ids[a:a + cut], last_id=last)
        out += stream
    _same(bytes(out), want)
    assert last == wlast
    if cut == 1000:
        whole, _, last1 = d.beast_encode_ex(msgs, verdict=verdict, ids=ids, last_id=9)
        _same(whole, want)
        assert last1 == wlast


def test_capacity_one_byte_short(ctx):
    d, hip = ctx
    msgs = _pool()[:3000]
    ids = biu.ids_changing_every(len(msgs), 1, 2)
    want = biu.beast_reference(msgs, ids=ids)[0]
    T = len(want)
    rc, got, nb, _, _, _, behind = _encode(d, hip, msgs, None, ids, cap=T - 1, want_len=T)
    assert rc == bu.MGPU_E_OVERFLOW and nb == T
    assert (behind == 0xA5).all(), "bytes at or beyond the capacity were written"
    rc, got, nb, _, _, _, behind = _encode(d, hip, msgs, None, ids, cap=T, want_len=T)
    assert rc == 0 and nb == T and (behind == 0xA5).all()
    _same(got, want)


@pytest.mark.parametrize("with_ids", [False, True])
def test_verbatim_ignores_verdicts(ctx, with_ids):
    d, hip = ctx
    msgs = _pool().copy()
    rng = np.random.default_rng(12)
    msgs["raw"] = rng.choice(np.array([0x19, 0x1A, 0x1B, 0x00, 0xFF], dtype=np.uint8), size=(len(msgs), 14))
    ids = biu.ids_changing_every(len(msgs), 5, 1) if with_ids else None
    verdict = bu.random_verdicts(len(msgs), 13)
    want = _check_encode(d, hip, msgs, verdict, ids, net_rule=True, verbatim=True)
    assert want == biu.beast_reference(msgs, None, verbatim=True, ids=ids)[0] and want != biu.beast_reference(msgs, None, ids=ids)[0]
    rc, got, nb, _, nd, _, _ = _encode(d, hip, msgs, verdict, ids, verbatim=True)
    assert rc == 0 and nd == 0
    _same(got, want)


def test_without_ids_and_flags_the_old_entry_points(ctx):
    d, hip = ctx
    msgs = _pool()
    verdict = bu.random_verdicts(len(msgs), 21)
    d_in, d_v, d_out, d_def = hip.upload(msgs), hip.upload(verdict), hip.malloc(len(msgs) * 44), hip.malloc(len(msgs) * 16)
    try:
        for v, net_rule in ((None, False), (verdict, False), (verdict, True)):
            rc, nb, nd = bu.encode_raw(d, d_in, len(msgs), d_out, len(msgs) * 44, d_v if v is not None else None, net_rule, d_def, len(msgs))
            assert rc == 0
            old, old_def = hip.download(d_out, nb).tobytes(), hip.download(d_def, nd * 16, bu.DEFERRED)
            rc, got, nb2, deferred, nd2, _, _ = _encode(d, hip, msgs, v, None, net_rule)
            assert rc == 0 and (nb2, nd2) == (nb, nd if v is not None else 0)
            _same(got, old)
            if v is not None:
                assert np.array_equal(deferred, old_def)
            _same(old, bu.beast_reference(msgs, v, net_rule)[0])
    finally:
        for p in (d_in, d_v, d_out, d_def):
            hip.free(p)


def test_binding_keywords(ctx):
    d, _ = ctx
    msgs = _pool()[:2048]
    ids = biu.ids_changing_every(len(msgs), 2, 8)
    assert d.beast_encode(msgs) == bu.beast_reference(msgs)[0]
    assert d.beast_encode(msgs, verbatim=True) == biu.beast_reference(msgs, verbatim=True)[0]
    stream, last = d.beast_encode(msgs, receiver_ids=ids, last_id=4)
    want = biu.beast_reference(msgs, ids=ids, last_id=4)
    assert stream == want[0] and last == want[3]


# ---- the chain ------------------------------------------------------------------------------------------------------------------

def _demodulate(kw, opt):
    import readsb_amd
    iq = helpers.synth(threads=8, **kw)
    d = readsb_amd.Demodulator(nfix_crc=opt["nfix"], mode_ac=opt["mode_ac"], startup_time_ms=helpers.STARTUP_MS, max_samples=len(iq) // 2)
    try:
        return np.ascontiguousarray(d.demodulate_capture(iq)[0])
    finally:
        d.close()


def _chain(d, hip, lists, ids, verbatim):
    """records in HBM -> device merge with ids -> ex-encoder, nothing through the host in between"""
    n = sum(len(m) for m in lists)
    d_lists = [hip.upload(m) for m in lists]
    d_m, d_ids, d_out = hip.malloc(n * 64), hip.malloc(n * 8), hip.malloc(n * 62 + 64)
    try:
        d.merge_by_time_device(d_lists, [len(m) for m in lists], d_m, ids=ids, d_ids_ptr=d_ids)
        nb, nd, last = d.beast_encode_ex_device(d_m, n, d_out, n * 62 + 64, verbatim=verbatim, d_ids_ptr=d_ids)
        return hip.download(d_out, nb).tobytes(), last
    finally:
        for p in d_lists + [d_m, d_ids, d_out]:
            hip.free(p)


def test_chain_two_receivers(ctx):
    """Two receivers' seconds (one with Mode A/C: its list is only piecewise ordered), merged by time on the device with their ids,
    encoded with prefixes: the numpy merge + the numpy encoder."""
    d, hip = ctx
    a = _demodulate(dict(seconds=1.0, seed=31, rate=1500.0), dict(nfix=1, mode_ac=0))
    b = _demodulate(dict(seconds=1.0, seed=32, rate=700.0, dense=2), dict(nfix=2, mode_ac=1))
    assert len(a) > 500 and len(b) > 500 and (b["msgtype"] == 77).any() and (np.diff(b["timestamp"]) < 0).any()
    ids = [0x11, 0x1A00000000000022]
    merged, order, mids, _ = _merge_want([a, b], ids, None)                    # gather.merge_by_timestamp's list (numpy, stable)
    seg = (order >= len(a)).astype(np.int64)
    assert (np.diff(seg) != 0).sum() > 0.2 * len(merged)                       # the merged stream switches receiver all the time
    for verbatim in (False, True):
        want, _, _, wlast, _ = biu.beast_reference(merged, verbatim=verbatim, ids=mids)
        got, last = _chain(d, hip, [a, b], ids, verbatim)
        _same(got, want)
        assert last == wlast


def test_chain_one_receiver_equals_the_programs_verbatim_dump(ctx):
    """IQ -> messages -> device merge (one receiver, id 0) -> the encoder with MGPU_BEAST_VERBATIM and ids, on the GPU: the file the
    WHOLE reference program writes with --dump-beast --net-verbatim --net-receiver-id (tests/golden/beast_verbatim_uc8_fix_2s.bin)."""
    import gate_util as gu
    d, hip = ctx
    kw, opt = gu.CASES["uc8_fix_2s"]
    gold = open(os.path.join(helpers.GOLDEN_DIR, "beast_verbatim_uc8_fix_2s.bin"), "rb").read()
    msgs = _demodulate(kw, opt)
    got, last = _chain(d, hip, [msgs], [0], True)
    _same(got, gold)
    assert last == 0
    assert d.beast_encode(msgs) != gold


@pytest.mark.parametrize("mode", ["merge_id", "merge_verbatim", "id", "merge_id_forward_only"])
def test_c_gather_merge_receiver_id_verbatim_single_rank(ctx, tmp_path, mode):
    """readsb_gpu_gather --merge --receiver-id at world 1 (one run of the program per case): the stream of the chain above for one
    receiver — the prefix once, in front of the first frame; with --verbatim and id 0 the reference program's verbatim dump; without
    --merge the rank's own order; --forward-only --merge lists the deferred messages by {rank, index in the rank's list} through the
    merge's permutation."""
    import subprocess
    import gate_util as gu
    d, hip = ctx
    exe = os.path.join(helpers.ROOT, "readsb_amd", "host", "readsb_gpu_gather")
    kw, opt = gu.CASES["uc8_fix_2s"]
    iq = helpers.synth(threads=8, **kw)
    msgs = _demodulate(kw, opt)
    path, out, idf, dfile = tmp_path / "cap.iq", tmp_path / "beast.bin", tmp_path / "nccl.id", tmp_path / "deferred.bin"
    iq.tofile(path)
    rid = 0x1A00000000000022

    def run(*opts):
        r = subprocess.run([exe, "--rank", "0", "--world", "1", "--id-file", str(idf), "--ifile", str(path), "--fix", "--startup-time-ms",
                            str(helpers.STARTUP_MS), "--out", str(out)] + list(opts), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return out.read_bytes()

    order = np.argsort(msgs["timestamp"], kind="stable")
    ids = np.full(len(msgs), rid, dtype=np.uint64)
    if mode == "merge_id":
        _same(run("--merge", "--receiver-id", f"{rid:x}"), biu.beast_reference(msgs[order], ids=ids)[0])
    elif mode == "merge_verbatim":
        _same(run("--merge", "--receiver-id", "0", "--verbatim"), open(os.path.join(helpers.GOLDEN_DIR, "beast_verbatim_uc8_fix_2s.bin"), "rb").read())
    elif mode == "id":
        _same(run("--receiver-id", f"{rid:x}"), biu.beast_reference(msgs, ids=ids)[0])             # without --merge: the rank's own order
    else:
        d.track_gate_reset()
        v = d.track_gate(msgs)
        d.track_gate_reset()
        want, _, wdef, _, _ = biu.beast_reference(msgs[order], v[order], net_rule=True, ids=ids)
        _same(run("--merge", "--receiver-id", f"{rid:x}", "--forward-only", "--net-rule", "--deferred-out", str(dfile)), want)
        deferred = np.fromfile(dfile, dtype="<u8").reshape(-1, 3)
        assert (deferred[:, 0] == 0).all()
        assert np.array_equal(deferred[:, 1], order[wdef["index"].astype(np.int64)]) and np.array_equal(deferred[:, 2], wdef["offset"])
