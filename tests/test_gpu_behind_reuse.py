"""-m gpu: ONE context through every entry behind the message list (include/modes_gpu.h: the beast encoder plain / gated / _ex, the
field decode, the tracking gate, CPR track and decode, the time merge), host-array forms in turn and then their `_device` forms, at
list sizes 1, 300, 5000, 40, 20000, 1: the context's device scratch grows several times and is used again at small sizes, and every
host-array form stages its list over the one the form before it staged.

What is stateless (streams, field records, decoder results, the merge) is compared exactly with the numpy / CPU checkers of those
entries' own tests.  What carries an aircraft table from call to call — the gate's verdicts, the gated streams and deferred lists,
the CPR positions — is compared exactly with a second context that receives ONLY the calls that touch that table (track_gate,
beast_encode_gated and track_gate_device share the gate's; cpr_track and cpr_track_device the CPR table), in the same order: what
lies between two such calls on the first context, and how often its scratch was reallocated, must change nothing.  The gate's
verdicts are also what the CPU restatement (oracle/modes_oracle_gate.c) gives for the same sequence of calls.

The records are tests/test_gpu_cpr.py's random traffic (sealed DF17 / DF18 position frames of ~2000 aircraft, identification
squitters, Mode A/C replies), a fifth of them marked as repaired: a repaired frame is forwarded only for a known aircraft, so the
gate defers some, and the flights' even / odd frames pair."""
import ctypes as C
import functools

import numpy as np
import pytest

import beast_ids_util as biu
import beast_util as bu
import cpr_util as cu
import fields_util as fu
import gate_util as gu
import helpers

pytestmark = pytest.mark.gpu

SIZES = (1, 300, 5000, 40, 20000, 1)
REF = (52.0, 4.5)
SEG_IDS = [0x11, 0x1A00000000000022, 7]


@functools.lru_cache(maxsize=None)
def _records():
    from test_gpu_cpr import _random_traffic
    msgs = np.ascontiguousarray(_random_traffic(2100, 23))
    n = len(msgs)
    assert n >= sum(SIZES)
    rng = np.random.default_rng(29)
    msgs["correctedbits"] = rng.random(n) < 0.2
    msgs["sig_sumsq"], msgs["sig_len"] = rng.integers(1 << 20, 1 << 36, size=n), 268
    return msgs


def _oracle_view(m):
    """What gate_util.oracle_gate reads of an oracle message list, from message records."""
    o = np.zeros(len(m), dtype=[("msgtype", np.uint8), ("correctedbits", np.uint8), ("sys_rel_ms", np.int64), ("timestamp", np.int64)])
    o["msgtype"], o["correctedbits"], o["timestamp"] = m["msgtype"], m["correctedbits"], m["timestamp"]
    o["sys_rel_ms"] = m["sysTimestamp"].astype(np.int64) - helpers.STARTUP_MS
    return o


def _merge_want(lists, verdicts):
    allm = np.concatenate(lists)
    order = np.argsort(allm["timestamp"], kind="stable")
    seg = np.repeat(np.arange(len(lists)), [len(x) for x in lists])
    return allm[order], order.astype(np.uint64), np.asarray(SEG_IDS, dtype=np.uint64)[seg[order]], np.concatenate(verdicts)[order]


def test_every_entry_in_turn_while_the_scratch_regrows(built):
    import readsb_amd
    msgs_all = _records()
    cases_all, results_all = cu.load_golden()
    lib = helpers.oracle_lib()
    lib.modes_oracle_gate_new.restype = C.c_void_p
    lib.modes_oracle_gate_free.argtypes = [C.c_void_p]
    machine = C.c_void_p(lib.modes_oracle_gate_new())

    def context():
        return readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=1 << 20)

    d, gate_only, cpr_only = context(), context(), context()
    hip = bu.Hip()
    fsize, psize = readsb_amd.FIELDS_DTYPE.itemsize, cu.POSITION_DTYPE.itemsize
    at, last_id, ndeferred, npaired = 0, 0, 0, 0
    try:
        for step, n in enumerate(SIZES):
            m = np.ascontiguousarray(msgs_all[at:at + n])
            at += n
            what = f"call {step}, {n} messages"
            pick = (np.arange(n) + 977 * step) % len(cases_all)
            cases, want_results = np.ascontiguousarray(cases_all[pick]), results_all[pick]
            want_fields = fu.oracle_fields(np.ascontiguousarray(m["msg"]), m["msgbits"].astype(np.int32))
            plain = bu.beast_reference(m)[0]
            o = _oracle_view(m)

            # ---- the host-array forms, each staging over the one before ----
            assert d.beast_encode(m) == plain, what
            assert d.decode_fields(m).tobytes() == want_fields.tobytes(), what
            v = d.track_gate(m)
            assert np.array_equal(v, gate_only.track_gate(m)), what
            assert np.array_equal(v, gu.oracle_gate(o, want_fields, machine)), what
            stream, deferred = d.beast_encode_gated(m, net_rule=True)
            stream1, deferred1 = gate_only.beast_encode_gated(m, net_rule=True)
            assert stream == stream1 and np.array_equal(deferred, deferred1), what
            want_stream, _, want_deferred = bu.beast_reference(m, gu.oracle_gate(o, want_fields, machine), True)
            assert stream == want_stream and np.array_equal(deferred, want_deferred), what
            ndeferred += len(deferred)
            pos = d.cpr_track(m, ref=REF)
            cu.assert_same_positions(pos, cpr_only.cpr_track(m, ref=REF), what)
            npaired += int((pos["method"] == cu.GLOBAL).sum())
            cu.assert_same_results(d.cpr_decode(cases), want_results, what)
            lists, verdicts = [m[k::3].copy() for k in range(3)], [v[k::3].copy() for k in range(3)]
            merged, order, mids, mv = _merge_want(lists, verdicts)
            out, perm, oid, vout = d.merge_by_time(lists, ids=SEG_IDS, verdicts=verdicts)
            assert out.tobytes() == merged.tobytes() and np.array_equal(perm, order) and np.array_equal(oid, mids) and np.array_equal(vout, mv), what
            want_x, _, want_xdef, want_last, _ = biu.beast_reference(merged, mv, ids=mids, last_id=last_id)
            got_x, got_xdef, got_last = d.beast_encode_ex(out, verdict=vout, ids=oid, last_id=last_id)
            assert got_x == want_x and np.array_equal(got_xdef, want_xdef) and got_last == want_last, what

            # ---- one `_device` form of each on the same list ----
            cap = n * 62 + 64
            d_m, d_f, d_v, d_v1, d_out, d_def = hip.upload(m), hip.malloc(n * fsize), hip.malloc(n), hip.malloc(n), hip.malloc(cap), hip.malloc(n * 16)
            nb = d.beast_encode_device(d_m, n, d_out, cap)
            assert hip.download(d_out, nb).tobytes() == plain, what
            d.decode_fields_device(d_m, n, d_f)
            assert hip.download(d_f, n * fsize).tobytes() == want_fields.tobytes(), what
            d.track_gate_device(d_m, d_f, n, d_v)
            gate_only.track_gate_device(d_m, d_f, n, d_v1)
            v = hip.download(d_v, n)
            assert np.array_equal(v, hip.download(d_v1, n)) and np.array_equal(v, gu.oracle_gate(o, want_fields, machine)), what
            nb, nd = d.beast_encode_gated_device(d_m, d_v, n, d_out, cap, d_def, n)
            want_stream, _, want_deferred = bu.beast_reference(m, v)
            assert hip.download(d_out, nb).tobytes() == want_stream and np.array_equal(hip.download(d_def, nd * 16, bu.DEFERRED), want_deferred), what
            ndeferred += nd
            d_p, d_p1 = hip.malloc(n * psize), hip.malloc(n * psize)
            d.cpr_track_device(d_m, d_f, n, d_p, ref=REF)
            cpr_only.cpr_track_device(d_m, d_f, n, d_p1, ref=REF)
            pos = hip.download(d_p, n * psize, cu.POSITION_DTYPE)
            cu.assert_same_positions(pos, hip.download(d_p1, n * psize, cu.POSITION_DTYPE), what)
            npaired += int((pos["method"] == cu.GLOBAL).sum())
            d_c, d_r = hip.upload(cases), hip.malloc(n * cu.CPR_RESULT_DTYPE.itemsize)
            d.cpr_decode_device(d_c, n, d_r)
            cu.assert_same_results(hip.download(d_r, n * cu.CPR_RESULT_DTYPE.itemsize, cu.CPR_RESULT_DTYPE), want_results, what)
            lists, verdicts = [m[k::3].copy() for k in range(3)], [v[k::3].copy() for k in range(3)]
            merged, order, mids, mv = _merge_want(lists, verdicts)
            d_mo, d_perm, d_ids, d_vo = hip.malloc(n * 64), hip.malloc(n * 8), hip.malloc(n * 8), hip.malloc(n)
            d.merge_by_time_device([hip.upload(x) for x in lists], [len(x) for x in lists], d_mo, ids=SEG_IDS, d_verdict_ptrs=[hip.upload(x) for x in verdicts],
                                   d_perm_ptr=d_perm, d_ids_ptr=d_ids, d_verdict_out_ptr=d_vo)
            assert hip.download(d_mo, n * 64).tobytes() == merged.tobytes() and np.array_equal(hip.download(d_perm, n * 8, np.uint64), order), what
            assert np.array_equal(hip.download(d_ids, n * 8, np.uint64), mids) and np.array_equal(hip.download(d_vo, n), mv), what
            want_x, _, want_xdef, want_last, _ = biu.beast_reference(merged, mv, net_rule=True, ids=mids, last_id=last_id)
            nb, nd, got_last = d.beast_encode_ex_device(d_mo, n, d_out, cap, d_verdict_ptr=d_vo, net_rule=True, d_ids_ptr=d_ids, last_id=last_id,
                                                        d_deferred_ptr=d_def, deferred_cap=n)
            assert hip.download(d_out, nb).tobytes() == want_x and np.array_equal(hip.download(d_def, nd * 16, bu.DEFERRED), want_xdef), what
            assert got_last == want_last, what
            last_id = want_last
            hip.free_all()
    finally:
        hip.free_all()
        lib.modes_oracle_gate_free(machine)
        for x in (d, gate_only, cpr_only):
            x.close()
    # the stateful half is not vacuous: the gate deferred messages, and frames paired
    assert ndeferred > 0 and npaired > 0, (ndeferred, npaired)
    print(f"{sum(SIZES)} messages in {len(SIZES)} rounds: {ndeferred} deferred, {npaired} global decodes")
