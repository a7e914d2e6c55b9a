// pf_in_host.cpp — the Planefinder input (pf_in_format.h) on the host: mgpu_pf_parse_host and pf_in_decode_sequential, the SEQUENTIAL
// walk — readPlanefinder's loop step by step, every handler call in order against a model of icao_filter.c: the plain statement of
// what kernels/pf_in.inc computes in parallel.  No HIP in this file: tests/host_stub/pf_in_format_check.cpp compiles it with plain g++
// (with raw_in_host.cpp and tables.cpp), under ASan and UBSan too.
#include <cstring>

#include "pf_in_host.h"
#include "tables.h"

using namespace mgpu;

static bool pf_in_cfg_ok(const struct mgpu_raw_in_config *cfg) {
    return cfg && cfg->size >= sizeof(struct mgpu_raw_in_config) && cfg->nfix_crc >= 0 && cfg->nfix_crc <= 2;
}

namespace mgpu {

// the stretch a describes (a->nbytes framed, `look` bytes behind them the stream's too; its arrays and capacities what the stretch may
// store), frame_base and off_base added to frame_of and frame_off
static void pf_in_walk(const struct mgpu_pf_in_args *a, uint64_t look, const struct mgpu_raw_in_config *cfg, IcaoFilter &flt, uint64_t frame_base, uint64_t off_base,
                       PfInCounts &out) {
    const RawInTables tb = raw_in_tables_of(raw_in_host_tables(cfg->nfix_crc));
    const RawInConfig rc = {cfg->nfix_crc, cfg->fixDF, (int32_t) cfg->mode_ac};
    uint64_t *cn = out.cn;
    uint64_t nframes = 0, nmsgs = 0, som = 0;
    const uint64_t nf = a->nbytes, n = nf + look;
    PfInStep st;
    PfInFields f;
    RawInLine r;
    while (som < nf) {
        const uint32_t kind = pf_in_step(a->data, nf, n, som, st);
        if (kind == PF_IN_END || kind == PF_IN_INCOMPLETE) break;
        som = st.next;
        if (kind == PF_IN_OTHER) ++cn[7];
        if (kind != PF_IN_FRAME) continue;
        uint32_t cls = pf_in_fields(a->data, n, st.frame, rc.mode_ac, f);
        cn[8] += f.past;
        if (!cls) cls = pf_in_frame(f, a->now_ms, rc, tb, r);
        if (cls == MGPU_PF_IN_COND) cls = flt.test(r.addr) ? MGPU_PF_IN_ACCEPT : MGPU_PF_IN_UNKNOWN;
        if (cls == MGPU_PF_IN_MODEAC) ++cn[1];
        else if (cls <= MGPU_PF_IN_UNKNOWN) ++cn[0];
        if (cls == MGPU_PF_IN_UNKNOWN) ++cn[2];
        if (cls == MGPU_PF_IN_BAD) ++cn[3];
        if (cls == MGPU_PF_IN_ACCEPT) ++cn[4 + (r.msg.correctedbits < 3 ? r.msg.correctedbits : 2)];
        if (cls == MGPU_PF_IN_ACCEPT || cls == MGPU_PF_IN_MODEAC) {
            if (nmsgs < a->msgs_cap) {
                a->msgs[nmsgs] = r.msg;
                if (a->frame_of) a->frame_of[nmsgs] = frame_base + nframes;
                if (a->signal_level) a->signal_level[nmsgs] = r.signal;
            }
            ++nmsgs;
            if (r.adder) flt.add(r.addr);                                 // mode_s.c:766-779
        }
        if (nframes < a->frames_cap) {
            if (a->frame_class) a->frame_class[nframes] = (uint8_t) cls;
            if (a->frame_off) a->frame_off[nframes] = off_base + st.frame;
        }
        ++nframes;
    }
    out.frames = nframes; out.msgs = nmsgs; out.consumed = som;
}

int pf_in_decode_sequential(const struct mgpu_pf_in_args *a, const struct mgpu_raw_in_config *cfg, IcaoFilter &flt) {
    if (!a || a->size < sizeof(struct mgpu_pf_in_args) || !a->consumed || !a->nframes || !a->nmsgs || !a->counters || !pf_in_cfg_ok(cfg)) return MGPU_E_INVAL;
    if ((a->nbytes && !a->data) || (a->msgs_cap && !a->msgs) || (a->frames_cap && !a->frame_class && !a->frame_off)) return MGPU_E_INVAL;
    IcaoFilter::Snapshot before, pass_before;
    flt.snapshot(before);
    const bool want_frames = a->frame_class || a->frame_off;
    PfInCounts all;
    if (a->nbytes)
        (void) stream_passes(a->nbytes, a->pass_bytes, false, all,
            [&](uint64_t at, uint64_t nb, bool, const PfInCounts &so_far, PfInCounts &n) {
                flt.snapshot(pass_before);
                struct mgpu_pf_in_args d = *a;
                const uint64_t m = so_far.msgs < a->msgs_cap ? so_far.msgs : a->msgs_cap, f = so_far.frames < a->frames_cap ? so_far.frames : a->frames_cap;
                d.data = a->data + at; d.nbytes = nb;
                d.msgs = a->msgs ? a->msgs + m : nullptr; d.msgs_cap = a->msgs_cap - m;
                d.signal_level = a->signal_level ? a->signal_level + m : nullptr; d.frame_of = a->frame_of ? a->frame_of + m : nullptr;
                d.frame_class = a->frame_class ? a->frame_class + f : nullptr; d.frame_off = a->frame_off ? a->frame_off + f : nullptr; d.frames_cap = a->frames_cap - f;
                pf_in_walk(&d, pf_in_look(a->nbytes + a->look, at, nb), cfg, flt, so_far.frames, at, n);
                return MGPU_OK;
            },
            [&] { flt.restore(pass_before); });
    pf_in_counters_of(all, a->counters);
    *a->consumed = all.consumed; *a->nframes = all.frames; *a->nmsgs = all.msgs;
    if (all.msgs > a->msgs_cap || (want_frames && all.frames > a->frames_cap)) { flt.restore(before); return MGPU_E_OVERFLOW; }
    return MGPU_OK;
}

}  // namespace mgpu

extern "C" {

int mgpu_pf_parse_host(const uint8_t *data, uint64_t nbytes, uint64_t offset, int64_t now_ms, const struct mgpu_raw_in_config *cfg, struct mgpu_pf_in_frame *out) {
    if (!data || !out || !pf_in_cfg_ok(cfg) || offset >= nbytes) return MGPU_E_INVAL;
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
    if (!f || (f->n_active && !f->gen_active) || (f->n_inactive && !f->gen_inactive) || f->table_bits < 8 || f->table_bits > 20) return MGPU_E_INVAL;
    IcaoFilter::Snapshot s;
    s.members[0].assign(f->gen_active, f->gen_active + f->n_active);
    s.members[1].assign(f->gen_inactive, f->gen_inactive + f->n_inactive);
    s.active = 0; s.occupied = f->occupied; s.filter_bits = f->table_bits;
    IcaoFilter flt;
    flt.restore(s);
    const int rc = pf_in_decode_sequential(a, cfg, flt);
    if (rc != MGPU_OK) return rc;
    const std::vector<uint32_t> &ga = flt.members(true), &gi = flt.members(false);
    for (size_t k = 0; k < ga.size(); ++k) f->gen_active[k] = ga[k];
    for (size_t k = 0; k < gi.size(); ++k) f->gen_inactive[k] = gi[k];
    f->n_active = ga.size(); f->n_inactive = gi.size();
    f->occupied = flt.occupied(); f->table_bits = flt.table_bits();
    return MGPU_OK;
}

}  // extern "C"
