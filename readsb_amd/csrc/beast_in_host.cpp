// beast_in_host.cpp — the beast input (beast_in_format.h) on the host: mgpu_beast_parse_host and beast_in_decode_sequential, the
// SEQUENTIAL walk — readBeast's loop step by step, every handler call in order against a model of icao_filter.c: the plain statement
// of what kernels/beast_in.inc computes in parallel.  No HIP in this file: tests/host_stub/beast_in_format_check.cpp compiles it with
// plain g++ (with raw_in_host.cpp and tables.cpp), under ASan and UBSan too.
#include <cstring>

#include "beast_in_host.h"
#include "tables.h"

using namespace mgpu;

static bool beast_in_cfg_ok(const struct mgpu_raw_in_config *cfg) {
    return cfg && cfg->size >= sizeof(struct mgpu_raw_in_config) && cfg->nfix_crc >= 0 && cfg->nfix_crc <= 2;
}

namespace mgpu {

// the stretch a describes (its arrays and capacities what the stretch may store), frame_base and off_base added to frame_of and frame_off
static void beast_in_walk(const struct mgpu_beast_in_args *a, const struct mgpu_raw_in_config *cfg, IcaoFilter &flt, uint64_t frame_base, uint64_t off_base, bool final,
                          BeastInCounts &out) {
    const RawInTables tb = raw_in_tables_of(raw_in_host_tables(cfg->nfix_crc));
    const RawInConfig rc = {cfg->nfix_crc, cfg->fixDF, (int32_t) cfg->mode_ac};
    uint64_t *cn = out.cn;
    uint64_t nframes = 0, nmsgs = 0, som = 0, pending = 0, id = a->receiver_id_in;
    uint32_t stop = MGPU_BEAST_STOP_END;
    const uint64_t n = a->nbytes;
    bool left = false;                                                    // the loop was left by a break or a stop: som stands
    BeastInStep st;
    RawInLine r;
    while (som < n) {
        const uint32_t kind = beast_in_step(a->data, n, som, a->net_ingest, st);
        if (kind == BEAST_IN_GARBAGE) { ++pending; som = st.next; continue; }
        cn[7] += pending + st.garbage;                                   // memchr found this 0x1a: the run in front of it is garbage
        pending = 0;
        if (st.id_set) { id = st.id; ++cn[8]; }
        cn[9] += st.wcmd;
        som = st.next;
        if (kind == BEAST_IN_INCOMPLETE) { left = true; break; }
        if (kind == BEAST_IN_STOP_SYNTH || kind == BEAST_IN_STOP_UUID) { left = true; stop = kind == BEAST_IN_STOP_SYNTH ? MGPU_BEAST_STOP_SYNTH : MGPU_BEAST_STOP_UUID; break; }
        if (kind != BEAST_IN_FRAME) continue;
        uint32_t cls = beast_in_frame(st, a->now_ms, rc, tb, r);
        if (cls == MGPU_BEAST_IN_COND) cls = flt.test(r.addr) ? MGPU_BEAST_IN_ACCEPT : MGPU_BEAST_IN_UNKNOWN;
        if (cls == MGPU_BEAST_IN_MODEAC || cls == MGPU_BEAST_IN_MODEAC_OFF) ++cn[1];
        else if (cls <= MGPU_BEAST_IN_UNKNOWN) ++cn[0];
        if (cls == MGPU_BEAST_IN_UNKNOWN) ++cn[2];
        if (cls == MGPU_BEAST_IN_BAD) ++cn[3];
        if (cls == MGPU_BEAST_IN_ACCEPT) ++cn[4 + (r.msg.correctedbits < 3 ? r.msg.correctedbits : 2)];
        if (cls == MGPU_BEAST_IN_ACCEPT || cls == MGPU_BEAST_IN_MODEAC) {
            if (nmsgs < a->msgs_cap) {
                a->msgs[nmsgs] = r.msg;
                a->receiver_id[nmsgs] = id;
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
    if (!left) som = n - pending;                                         // memchr found no 0x1a behind the trailing run: som stays in front of it
    if (stop == MGPU_BEAST_STOP_END && final && n - som > kBeastInTail) {  // net_io.c:5010-5015
        cn[7] += n - som;
        som = n;
    }
    out.frames = nframes; out.msgs = nmsgs; out.consumed = som; out.stop_off = som; out.stop = stop; out.id = id;
}

int beast_in_decode_sequential(const struct mgpu_beast_in_args *a, const struct mgpu_raw_in_config *cfg, IcaoFilter &flt) {
    if (!a || a->size < sizeof(struct mgpu_beast_in_args) || !a->consumed || !a->nframes || !a->nmsgs || !a->stop || !a->stop_off || !a->receiver_id_out ||
        !a->counters || !beast_in_cfg_ok(cfg))
        return MGPU_E_INVAL;
    if ((a->nbytes && !a->data) || (a->msgs_cap && (!a->msgs || !a->receiver_id)) || (a->frames_cap && !a->frame_class && !a->frame_off)) return MGPU_E_INVAL;
    IcaoFilter::Snapshot before, pass_before;
    flt.snapshot(before);
    const bool want_frames = a->frame_class || a->frame_off;
    BeastInCounts all;
    all.id = a->receiver_id_in;
    if (a->nbytes)
        (void) stream_passes(a->nbytes, a->pass_bytes, false, all,
            [&](uint64_t at, uint64_t nb, bool final, const BeastInCounts &so_far, BeastInCounts &n) {
                flt.snapshot(pass_before);
                struct mgpu_beast_in_args d = *a;
                const uint64_t m = so_far.msgs < a->msgs_cap ? so_far.msgs : a->msgs_cap, f = so_far.frames < a->frames_cap ? so_far.frames : a->frames_cap;
                d.data = a->data + at; d.nbytes = nb; d.receiver_id_in = so_far.id;
                d.msgs = a->msgs ? a->msgs + m : nullptr; d.receiver_id = a->receiver_id ? a->receiver_id + m : nullptr; d.msgs_cap = a->msgs_cap - m;
                d.signal_level = a->signal_level ? a->signal_level + m : nullptr; d.frame_of = a->frame_of ? a->frame_of + m : nullptr;
                d.frame_class = a->frame_class ? a->frame_class + f : nullptr; d.frame_off = a->frame_off ? a->frame_off + f : nullptr; d.frames_cap = a->frames_cap - f;
                beast_in_walk(&d, cfg, flt, so_far.frames, at, final, n);
                return MGPU_OK;
            },
            [&] { flt.restore(pass_before); });
    beast_in_counters_of(all, a->counters);
    *a->consumed = all.consumed; *a->nframes = all.frames; *a->nmsgs = all.msgs; *a->stop = all.stop; *a->stop_off = all.stop_off; *a->receiver_id_out = all.id;
    if (all.msgs > a->msgs_cap || (want_frames && all.frames > a->frames_cap)) { flt.restore(before); return MGPU_E_OVERFLOW; }
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
    if (!f || (f->n_active && !f->gen_active) || (f->n_inactive && !f->gen_inactive) || f->table_bits < 8 || f->table_bits > 20) return MGPU_E_INVAL;
    IcaoFilter::Snapshot s;
    s.members[0].assign(f->gen_active, f->gen_active + f->n_active);
    s.members[1].assign(f->gen_inactive, f->gen_inactive + f->n_inactive);
    s.active = 0; s.occupied = f->occupied; s.filter_bits = f->table_bits;
    IcaoFilter flt;
    flt.restore(s);
    const int rc = beast_in_decode_sequential(a, cfg, flt);
    if (rc != MGPU_OK) return rc;
    const std::vector<uint32_t> &ga = flt.members(true), &gi = flt.members(false);
    for (size_t k = 0; k < ga.size(); ++k) f->gen_active[k] = ga[k];
    for (size_t k = 0; k < gi.size(); ++k) f->gen_inactive[k] = gi[k];
    f->n_active = ga.size(); f->n_inactive = gi.size();
    f->occupied = flt.occupied(); f->table_bits = flt.table_bits();
    return MGPU_OK;
}

}  // extern "C"
