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


# ---- the newer entries: text, ASTERIX and dump outputs, the five stream inputs --------------------------------------------------------

LIST_AT = ((0, 1), (40, 300), (2300, 40))           # (first record, records) of the three rounds' lists: grow, then small again
EXTERNAL = 2                                        # MGPU_FILTER_CLOCK_EXTERNAL: the filter starts empty, as the goldens' does
RAW_CFG, BEAST_CFG = (1, 1, 0), (1, 1, 0, 0)        # nfix_crc, fix_df, mode_ac (, net_ingest) of the raw and beast goldens used


def _passes(stream):
    """A pass_bytes that cuts the stream into three passes at least."""
    return max(len(stream) // 4 + 1, 1)


def _lines(stream, k, ends=(10,)):
    """The first k lines of a stream."""
    at = [i + 1 for i, b in enumerate(stream) if b in ends]
    return stream[:at[k - 1]]


def _same_results(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert (a[k].tobytes() == b[k].tobytes()) if isinstance(a[k], np.ndarray) else a[k] == b[k], (what, k)


def test_every_newer_entry_in_turn_over_shared_scratch(built):
    """-m gpu: ONE context through the text outputs (sbs_encode_ex, raw_encode_ex), asterix_encode_ex, dump_encode_ex and the five stream
    inputs (uat_encode, sbs_decode, raw_decode, beast_decode, asterix_decode), host-array forms in turn and then their `_device` forms,
    three rounds: lists of 1, 300, 40 records, streams of a few hundred bytes, 25 to 56 KB, about 2 KB.  The entries share their
    staging by role — one staged list, one set of optional arrays, one staged stream, one index array, one tile scratch — so every
    call stages over what another FORMAT left, in buffers that grew for a larger call; the host forms of the inputs run in three
    passes at least.

    Stateless entries are compared exactly with the reference's bytes and records: the dumps, the UAT text, the SBS and ASTERIX
    records with the goldens themselves (cut per message / per line where a round takes a part), the SBS, raw and ASTERIX outputs
    with the checkers of their own tests on golden cases, which tests/test_text_reference.py and test_asterix_reference.py pin to the
    goldens' streams.  raw_decode and beast_decode move the context's ICAO filter: they are compared exactly with a second context
    that receives ONLY those calls, in the same order, and the first of them — a whole golden stream on the fresh filter — with its
    golden as well."""
    import readsb_amd
    import asterix_in_util as ai
    import asterix_util as au
    import beast_in_util as bi
    import dump_util as du
    import raw_in_util as ru
    import sbs_in_util as si
    import sbs_util as su
    import uat_util as uu
    import test_gpu_asterix as t_asx
    import test_gpu_asterix_in as t_ai
    import test_gpu_beast_in as t_bi
    import test_gpu_dump as t_dump
    import test_gpu_raw_in as t_ri
    import test_gpu_sbs_in as t_si
    import test_gpu_text as t_text
    import test_gpu_uat as t_uat

    # the lists: golden cases of every form, with verdicts that defer some
    sbs_sets, (e_msgs, e_verdict), _, _ = su.load_golden()
    sbs_all = su.concat_cases([sbs_sets["a"], sbs_sets["b"]])
    asx_sets = au.load_golden()[0]
    asx_all = au.concat_cases([asx_sets["d"], asx_sets["a"]])
    dump_sets, dump_ref, _ = du.load_golden()
    dump_all = du.concat_cases([dump_sets["e"], dump_sets["a"], dump_sets["b"], dump_sets["c"], dump_sets["d"], dump_sets["e"], dump_sets["a"]])
    dump_chunks = sum((du.chunks(*dump_ref[(g, "full")]) for g in ("e", "a", "b", "c", "d", "e", "a")), [])
    # the streams of the three rounds, and what the stateless ones owe
    uat, sbs_in, ast_in = uu.load_golden(), si.load_golden(), ai.load_golden()
    raw_in, beast_in = ru.load_golden(), bi.load_golden()

    def uat_part(group, k, deferred):
        stream, out, lens = uat[group]
        k = len(lens) if k is None else k
        text, line_of = uu.expected(out[:int(np.sum(lens[:k]))], lens[:k], range(k) if deferred else ())
        return _lines(stream, k), text, line_of, list(range(k)) if deferred else [], k

    def sbs_in_part(group, k):
        stream, by_source = sbs_in[group]
        head, line_of, recs = by_source["sbs"]
        assert int(head[3]) == 0                                # no invalid line: a part's count is 0 as well
        k = int(head[1]) if k is None else k
        keep = line_of < k
        deferred = line_of[keep].tolist() if group == "c" else []
        want_line_of, want_recs = si.without(line_of[keep], recs[keep], deferred)
        return _lines(stream, k, ends=(10, 0)), want_recs, want_line_of, deferred, k

    uat_rounds = [uat_part("f", 3, True), uat_part("c", None, False), uat_part("e", 20, False)]
    sbs_in_rounds = [sbs_in_part("c", 2), sbs_in_part("a", None), sbs_in_part("a", 20)]
    ast_in_rounds = ["c2", "a", "c1"]
    raw_first = raw_in[ru.key("c", RAW_CFG)]
    raw_rounds = [raw_first["stream"], raw_in[ru.key("a", RAW_CFG)]["stream"], raw_in[ru.key("d2", RAW_CFG)]["stream"][:2000]]
    beast_rounds = [beast_in[bi.key("d2", BEAST_CFG)]["stream"][:200], beast_in[bi.key("a", BEAST_CFG)]["stream"], beast_in[bi.key("c", BEAST_CFG)]["stream"][:2000]]

    def context():
        return readsb_amd.Demodulator(nfix_crc=RAW_CFG[0], fix_df=RAW_CFG[1], mode_ac=RAW_CFG[2], startup_time_ms=helpers.STARTUP_MS, max_samples=1 << 20,
                                      filter_clock=EXTERNAL)

    d, filter_only = context(), context()
    hip = bu.Hip()
    produced = dict.fromkeys(("sbs", "raw", "asterix", "dump", "uat", "sbs_in", "raw_in", "beast_in", "asterix_in"), 0)
    deferred = dict.fromkeys(("sbs", "raw", "asterix", "dump", "uat", "sbs_in"), 0)
    try:
        for x in (d, filter_only):
            t_ri.prepare(x, ru.ops_of("c"))
        for step, (lo, n) in enumerate(LIST_AT):
            sbs_c, asx_c = su.slice_cases(sbs_all, lo, lo + n), au.slice_cases(asx_all, lo % 150, lo % 150 + n)
            dump_idx = np.arange(n) + (0 if step == 1 else lo)
            dump_c, chunks = du.take_cases(dump_all, dump_idx), [dump_chunks[i] for i in dump_idx]
            raw_idx = (np.arange(n) + lo) % len(e_msgs)
            raw_m, raw_v = np.ascontiguousarray(e_msgs[raw_idx]), np.ascontiguousarray(e_verdict[raw_idx])
            want_sbs, want_asx, want_raw = su.sbs_of(sbs_c, use_gnss=True), au.asterix_of(asx_c), su.raw_reference(raw_m, False, raw_v, True, False)
            want_dump = du.expected(dump_c, 0, chunks)
            u_stream, u_text, u_line_of, u_def, u_lines = uat_rounds[step]
            s_stream, s_recs, s_line_of, s_def, s_lines = sbs_in_rounds[step]
            a_stream, a_by_now = ast_in[ast_in_rounds[step]]
            a_head, a_frame_of, a_recs = a_by_now[ai.NOWS[0]]
            want_ast = dict(consumed=int(a_head[0]), nframes=int(a_head[1]), recs=a_recs, frame_of=a_frame_of, nother=int(a_head[3]), nundefined=0, stop=int(a_head[4]))
            for form in ("host", "device"):
                what = f"round {step}, {form} forms"
                # SBS lines, then the UAT input over what they staged
                if form == "host":
                    t_text._check_host(d, sbs_c, want_sbs)
                else:
                    t_text._sbs_device(d, hip, sbs_c, want_sbs)
                res = t_uat.run(d, hip, form, u_stream, pass_bytes=_passes(u_stream))
                assert res["rc"] == uu.MGPU_OK and res["intact"], what
                assert (res["bytes"], res["consumed"], res["nlines"], res["nframes"], res["nshort"], res["ndeferred"]) == \
                    (len(u_text), len(u_stream), u_lines, len(u_text) // uu.FRAME_TEXT, 0, len(u_def)), what
                assert res["text"] == u_text and (res["line_of"] == u_line_of).all() and res["deferred"].tolist() == u_def, what
                # raw lines, then the SBS input
                if form == "host":
                    stream, listed = d.raw_encode(raw_m, verdict=raw_v, net_rule=True)
                else:
                    cap = len(want_raw[0]) + 64
                    d_m, d_v, d_out, d_def = hip.upload(raw_m), hip.upload(raw_v), hip.malloc(cap), hip.malloc((n + 1) * 16)
                    nb, nd = d.raw_encode_device(d_m, n, d_out, cap, d_verdict_ptr=d_v, net_rule=True, d_deferred_ptr=d_def, deferred_cap=n)
                    stream, listed = hip.download(d_out, nb).tobytes(), hip.download(d_def, nd * 16, bu.DEFERRED)
                assert stream == want_raw[0] and np.array_equal(listed, want_raw[2]), what
                res = t_si.run(d, hip, form, s_stream, pass_bytes=_passes(s_stream))
                assert res["rc"] == si.MGPU_OK and res["intact"], what
                assert (res["consumed"], res["nlines"], res["nrecs"], res["ninvalid"], res["ndeferred"]) == (len(s_stream), s_lines, len(s_recs), 0, len(s_def)), what
                assert res["recs"].tobytes() == s_recs.tobytes() and (res["line_of"] == s_line_of).all() and res["deferred"].tolist() == s_def, what
                # ASTERIX reports, then the raw input (it moves the filter: the second context follows)
                if form == "host":
                    t_asx._check_host(d, asx_c, want_asx)
                else:
                    t_asx._device(d, hip, asx_c, want_asx)
                r_stream = raw_rounds[step]
                res = t_ri.run(d, hip, form, r_stream, pass_bytes=_passes(r_stream))
                _same_results(res, t_ri.run(filter_only, hip, form, r_stream, pass_bytes=_passes(r_stream)), what)
                assert res["rc"] == ru.MGPU_OK and res["intact"], what
                if step == 0 and form == "host":
                    t_ri.same(res, raw_first, what)             # the first filter-moving call: the golden itself
                produced["raw_in"] += res["nmsgs"]
                # dumps, then the beast input (likewise), then the ASTERIX input
                if form == "host":
                    t_dump._check_host(d, dump_c, chunks, 0)
                else:
                    t_dump._device(d, hip, dump_c, chunks, 0)
                b_stream = beast_rounds[step]
                res = t_bi.run(d, hip, form, b_stream, BEAST_CFG, pass_bytes=_passes(b_stream))
                _same_results(res, t_bi.run(filter_only, hip, form, b_stream, BEAST_CFG, pass_bytes=_passes(b_stream)), what)
                assert res["rc"] == bi.MGPU_OK and res["intact"], what
                produced["beast_in"] += res["nmsgs"]
                t_ai.same(t_ai.run(d, hip, form, a_stream, pass_bytes=_passes(a_stream)), want_ast, what)
                hip.free_all()
            for name, want in (("sbs", want_sbs), ("asterix", want_asx)):
                produced[name] += len(want[0])
                deferred[name] += len(want[2])
            produced["raw"], deferred["raw"] = produced["raw"] + len(want_raw[0]), deferred["raw"] + len(want_raw[2])
            produced["dump"], deferred["dump"] = produced["dump"] + len(want_dump[0]), deferred["dump"] + len(want_dump[1])
            produced["uat"], deferred["uat"] = produced["uat"] + len(u_text), deferred["uat"] + len(u_def)
            produced["sbs_in"], deferred["sbs_in"] = produced["sbs_in"] + len(s_recs), deferred["sbs_in"] + len(s_def)
            produced["asterix_in"] += len(a_recs)
    finally:
        hip.free_all()
        for x in (d, filter_only):
            x.close()
    # not vacuous: every format produced something, and every format that can defer deferred something
    assert all(v > 0 for v in produced.values()) and all(v > 0 for v in deferred.values()), (produced, deferred)
    print(f"{len(LIST_AT)} rounds x 2 forms: produced {produced}, deferred {deferred}")
