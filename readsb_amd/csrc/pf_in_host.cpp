// pf_in_host.cpp — the Planefinder input (pf_in_format.h) on the host: mgpu_pf_parse_host and pf_in_decode_sequential, the SEQUENTIAL
// walk — readPlanefinder's loop step by step, every handler call in order against a model of icao_filter.c: the plain statement of
// what kernels/pf_in.inc computes in parallel.  No HIP in this file: tests/host_stub/pf_in_format_check.cpp compiles it with plain g++
// (with raw_in_host.cpp and tables.cpp), under ASan and UBSan too.
#include <cstring>

#include "pf_in_host.h"
#include "tables.h"

using namespace mgpu;

namespace mgpu {

// the stretch a (a.nbytes framed, a.look bytes behind them the stream's too; its arrays and capacities what the stretch may store)
static void pf_in_walk(const MsgInStretch &a, const struct mgpu_raw_in_config *cfg, IcaoFilter &flt, MsgInCounts &out) {
    const RawInTables tb = raw_in_tables_of(raw_in_host_tables(cfg->nfix_crc));
    const RawInConfig rc = {cfg->nfix_crc, cfg->fixDF, (int32_t) cfg->mode_ac};
    uint64_t *cn = out.cn;
    uint64_t som = 0;
    const uint64_t nf = a.nbytes, n = nf + a.look;
    PfInStep st;
    PfInFields f;
    RawInLine r;
    while (som < nf) {
        const uint32_t kind = pf_in_step(a.data, nf, n, som, st);
        if (kind == PF_IN_END || kind == PF_IN_INCOMPLETE) break;
        som = st.next;
        if (kind == PF_IN_OTHER) ++cn[7];
        if (kind != PF_IN_FRAME) continue;
        uint32_t cls = pf_in_fields(a.data, n, st.frame, rc.mode_ac, f);
        cn[8] += f.past;
        if (!cls) cls = pf_in_frame(f, a.now_ms, rc, tb, r);
        if (cls == MGPU_PF_IN_COND) cls = flt.test(r.addr) ? MGPU_PF_IN_ACCEPT : MGPU_PF_IN_UNKNOWN;
        msg_in_unit(a, cls, r, 0, st.frame, flt, out);
    }
    out.consumed = som;
}

int pf_in_decode_sequential(const struct mgpu_pf_in_args *a, const struct mgpu_raw_in_config *cfg, IcaoFilter &flt) {
    if (!a || a->size < sizeof(struct mgpu_pf_in_args) || !a->consumed || !a->nframes || !a->nmsgs || !a->counters || !raw_in_cfg_ok(cfg)) return MGPU_E_INVAL;
    if ((a->nbytes && !a->data) || (a->msgs_cap && !a->msgs) || (a->frames_cap && !a->frame_class && !a->frame_off)) return MGPU_E_INVAL;
    const MsgInStretch s = pf_in_stretch(*a);
    IcaoFilter::Snapshot before, pass_before;
    flt.snapshot(before);
    MsgInCounts all;
    if (s.nbytes)
        (void) stream_passes(s.nbytes, a->pass_bytes, false, all,
            [&](uint64_t at, uint64_t nb, bool final, const MsgInCounts &so_far, MsgInCounts &n) {
                flt.snapshot(pass_before);
                pf_in_walk(msg_in_slice(s, at, nb, pf_in_look(s.nbytes + s.look, at, nb), final, so_far), cfg, flt, n);
                return MGPU_OK;
            },
            [&] { flt.restore(pass_before); });
    pf_in_report(*a, all);
    if (msg_in_overflow(s, all)) { flt.restore(before); return MGPU_E_OVERFLOW; }
    return MGPU_OK;
}

}  // namespace mgpu

extern "C" {

int mgpu_pf_parse_host(const uint8_t *data, uint64_t nbytes, uint64_t offset, int64_t now_ms, const struct mgpu_raw_in_config *cfg, struct mgpu_pf_in_frame *out) {
    if (!data || !out || !raw_in_cfg_ok(cfg) || offset >= nbytes) return MGPU_E_INVAL;
    memset(out, 0, sizeof *out);
    PfInStep st;
    const uint32_t kind = pf_in_step(data, nbytes, nbytes, offset, st);
    out->step = kind;                                                     // (MGPU_PF_STEP_* are PF_IN_*'s values)
    out->next = st.next;
    out->frame_off = st.frame;
    if (kind != PF_IN_FRAME) return 0;
    const RawInTables tb = raw_in_tables_of(raw_in_host_tables(cfg->nfix_crc));
    const RawInConfig rc = {cfg->nfix_crc, cfg->fixDF, (int32_t) cfg->mode_ac};
    PfInFields f;
    RawInLine r;
    uint32_t cls = pf_in_fields(data, nbytes, st.frame, rc.mode_ac, f);
    out->past_end = f.past;
    if (!cls) {
        cls = pf_in_frame(f, now_ms, rc, tb, r);
        if (cls == MGPU_PF_IN_MODEAC || cls == MGPU_PF_IN_ACCEPT || cls == MGPU_PF_IN_COND) out->msg = r.msg;
        out->signal_level = r.signal;
        out->addr = r.addr;
        out->adder = r.adder;
    }
    out->cls = cls;
    return 1;
}

int mgpu_pf_decode_host(const struct mgpu_pf_in_args *a, const struct mgpu_raw_in_config *cfg, struct mgpu_raw_in_filter *f) {
    return msg_in_decode_host(pf_in_decode_sequential, a, cfg, f);
}

}  // extern "C"
