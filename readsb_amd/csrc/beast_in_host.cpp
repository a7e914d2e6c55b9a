// beast_in_host.cpp — the beast input (beast_in_format.h) on the host: mgpu_beast_parse_host and beast_in_decode_sequential, the
// SEQUENTIAL walk — readBeast's loop step by step, every handler call in order against a model of icao_filter.c: the plain statement
// of what kernels/beast_in.inc computes in parallel.  No HIP in this file: tests/host_stub/beast_in_format_check.cpp compiles it with
// plain g++ (with raw_in_host.cpp and tables.cpp), under ASan and UBSan too.
#include <cstring>

#include "beast_in_host.h"
#include "tables.h"

using namespace mgpu;

namespace mgpu {

// the stretch a (its arrays and capacities what the stretch may store)
static void beast_in_walk(const MsgInStretch &a, const struct mgpu_raw_in_config *cfg, IcaoFilter &flt, MsgInCounts &out) {
    const RawInTables tb = raw_in_tables_of(raw_in_host_tables(cfg->nfix_crc));
    const RawInConfig rc = {cfg->nfix_crc, cfg->fixDF, (int32_t) cfg->mode_ac};
    uint64_t *cn = out.cn;
    uint64_t som = 0, pending = 0, id = a.receiver_id_in;
    uint32_t stop = MGPU_BEAST_STOP_END;
    const uint64_t n = a.nbytes;
    bool left = false;                                                    // the loop was left by a break or a stop: som stands
    BeastInStep st;
    RawInLine r;
    while (som < n) {
        const uint32_t kind = beast_in_step(a.data, n, som, a.net_ingest, st);
        if (kind == BEAST_IN_GARBAGE) { ++pending; som = st.next; continue; }
        cn[7] += pending + st.garbage;                                   // memchr found this 0x1a: the run in front of it is garbage
        pending = 0;
        if (st.id_set) { id = st.id; ++cn[8]; }
        cn[9] += st.wcmd;
        som = st.next;
        if (kind == BEAST_IN_INCOMPLETE) { left = true; break; }
        if (kind == BEAST_IN_STOP_SYNTH || kind == BEAST_IN_STOP_UUID) { left = true; stop = kind == BEAST_IN_STOP_SYNTH ? MGPU_BEAST_STOP_SYNTH : MGPU_BEAST_STOP_UUID; break; }
        if (kind != BEAST_IN_FRAME) continue;
        uint32_t cls = beast_in_frame(st, a.now_ms, rc, tb, r);
        if (cls == MGPU_BEAST_IN_COND) cls = flt.test(r.addr) ? MGPU_BEAST_IN_ACCEPT : MGPU_BEAST_IN_UNKNOWN;
        if (cls == MGPU_BEAST_IN_MODEAC_OFF) ++cn[1];                     // counted though dropped (net_io.c:3825-3831)
        msg_in_unit(a, cls, r, id, st.frame, flt, out);
    }
    if (!left) som = n - pending;                                         // memchr found no 0x1a behind the trailing run: som stays in front of it
    if (stop == MGPU_BEAST_STOP_END && a.final && n - som > kBeastInTail) {  // net_io.c:5010-5015
        cn[7] += n - som;
        som = n;
    }
    out.consumed = som; out.stop_off = som; out.stop = stop; out.id = id;
}

int beast_in_decode_sequential(const struct mgpu_beast_in_args *a, const struct mgpu_raw_in_config *cfg, IcaoFilter &flt) {
    if (!a || a->size < sizeof(struct mgpu_beast_in_args) || !a->consumed || !a->nframes || !a->nmsgs || !a->stop || !a->stop_off || !a->receiver_id_out ||
        !a->counters || !raw_in_cfg_ok(cfg))
        return MGPU_E_INVAL;
    if ((a->nbytes && !a->data) || (a->msgs_cap && (!a->msgs || !a->receiver_id)) || (a->frames_cap && !a->frame_class && !a->frame_off)) return MGPU_E_INVAL;
    const MsgInStretch s = beast_in_stretch(*a);
    IcaoFilter::Snapshot before, pass_before;
    flt.snapshot(before);
    MsgInCounts all;
    all.id = s.receiver_id_in;
    if (s.nbytes)
        (void) stream_passes(s.nbytes, a->pass_bytes, false, all,
            [&](uint64_t at, uint64_t nb, bool final, const MsgInCounts &so_far, MsgInCounts &n) {
                flt.snapshot(pass_before);
                beast_in_walk(msg_in_slice(s, at, nb, 0, final, so_far), cfg, flt, n);
                return MGPU_OK;
            },
            [&] { flt.restore(pass_before); });
    beast_in_report(*a, all);
    if (msg_in_overflow(s, all)) { flt.restore(before); return MGPU_E_OVERFLOW; }
    return MGPU_OK;
}

}  // namespace mgpu

extern "C" {

int mgpu_beast_parse_host(const uint8_t *data, uint64_t nbytes, uint64_t offset, int64_t now_ms, const struct mgpu_beast_in_config *cfg, struct mgpu_beast_in_frame *out) {
    if (!data || !out || !cfg || cfg->size < sizeof(struct mgpu_beast_in_config) || cfg->nfix_crc < 0 || cfg->nfix_crc > 2 || offset >= nbytes) return MGPU_E_INVAL;
    memset(out, 0, sizeof *out);
    BeastInStep st;
    const uint32_t kind = beast_in_step(data, nbytes, offset, cfg->net_ingest, st);
    out->step = kind;                                                     // (MGPU_BEAST_STEP_* are BEAST_IN_*'s values)
    out->next = st.next;
    out->garbage = st.garbage;
    out->id_set = st.id_set;
    out->receiver_id = st.id;
    out->command = st.wcmd;
    if (kind != BEAST_IN_FRAME) return 0;
    const RawInTables tb = raw_in_tables_of(raw_in_host_tables(cfg->nfix_crc));
    const RawInConfig rc = {cfg->nfix_crc, cfg->fixDF, (int32_t) cfg->mode_ac};
    RawInLine r;
    const uint32_t cls = beast_in_frame(st, now_ms, rc, tb, r);
    out->frame_off = st.frame;
    out->cls = cls;
    if (cls == MGPU_BEAST_IN_MODEAC || cls == MGPU_BEAST_IN_ACCEPT || cls == MGPU_BEAST_IN_COND) out->msg = r.msg;
    out->signal_level = r.signal;
    out->addr = r.addr;
    out->adder = r.adder;
    return 1;
}

int mgpu_beast_decode_host(const struct mgpu_beast_in_args *a, const struct mgpu_raw_in_config *cfg, struct mgpu_raw_in_filter *f) {
    return msg_in_decode_host(beast_in_decode_sequential, a, cfg, f);
}

}  // extern "C"
