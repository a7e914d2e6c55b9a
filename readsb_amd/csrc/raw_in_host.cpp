// raw_in_host.cpp — the raw input (raw_in_format.h) on the host: mgpu_raw_parse_line_host, the line splitter, and
// mgpu_raw_decode_host, the SEQUENTIAL resolver — every line in order against a model of icao_filter.c, the plain statement of the
// rule kernels/raw_in.inc resolves in parallel; and what the beast and the Planefinder walk share with it (raw_in_host.h).  No HIP in
// this file: tests/host_stub/raw_in_format_check.cpp and raw_in_resolve_check.cpp compile it with plain g++ (with tables.cpp), under
// ASan and UBSan too.
#include <cstring>
#include <mutex>
#include <vector>

#include "raw_in_host.h"
#include "tables.h"

namespace mgpu {

// the packed tables of an nfix_crc value, built once
const RawInHostTables &raw_in_host_tables(int nfix_crc) {
    static RawInHostTables cache[3];
    static std::once_flag once[3];
    const int n = nfix_crc < 0 ? 0 : nfix_crc > 2 ? 2 : nfix_crc;
    std::call_once(once[n], [n] {
        cache[n].tab_long = pack_syndrome_table(build_syndrome_table(112, n));
        cache[n].tab_short = pack_syndrome_table(build_syndrome_table(56, n));
    });
    return cache[n];
}

RawInTables raw_in_tables_of(const RawInHostTables &t) {
    return RawInTables{crc_tables().byte_table, t.tab_long.data(), t.tab_short.data(), (uint32_t) t.tab_long.size(), (uint32_t) t.tab_short.size()};
}

bool raw_in_cfg_ok(const struct mgpu_raw_in_config *cfg) {
    return cfg && cfg->size >= sizeof(struct mgpu_raw_in_config) && cfg->nfix_crc >= 0 && cfg->nfix_crc <= 2;
}

// ---- what the message inputs share ----

MsgInStretch msg_in_slice(const MsgInStretch &a, uint64_t at, uint64_t nb, uint64_t look, bool final, const MsgInCounts &so_far) {
    const uint64_t m = so_far.msgs < a.msgs_cap ? so_far.msgs : a.msgs_cap, u = so_far.units < a.units_cap ? so_far.units : a.units_cap;
    MsgInStretch d = a;
    d.data = a.data + at; d.nbytes = nb; d.look = look; d.final = final; d.receiver_id_in = so_far.id;
    d.msgs = a.msgs ? a.msgs + m : nullptr; d.ids = a.ids ? a.ids + m : nullptr; d.msgs_cap = a.msgs_cap - m;
    d.signal = a.signal ? a.signal + m : nullptr; d.index_of = a.index_of ? a.index_of + m : nullptr;
    d.unit_class = a.unit_class ? a.unit_class + u : nullptr; d.unit_off = a.unit_off ? a.unit_off + u : nullptr; d.units_cap = a.units_cap - u;
    d.unit_base = so_far.units; d.off_base = at;
    return d;
}

// one rule for the three formats: their classes are one set of values as far as the rule looks
static_assert(MGPU_BEAST_IN_MODEAC == MGPU_RAW_MODEAC && MGPU_BEAST_IN_BAD == MGPU_RAW_BAD && MGPU_BEAST_IN_ACCEPT == MGPU_RAW_ACCEPT &&
              MGPU_BEAST_IN_COND == MGPU_RAW_COND && MGPU_BEAST_IN_UNKNOWN == MGPU_RAW_UNKNOWN && MGPU_BEAST_IN_MODEAC_OFF > MGPU_RAW_UNKNOWN, "beast classes");
static_assert(MGPU_PF_IN_MODEAC == MGPU_RAW_MODEAC && MGPU_PF_IN_BAD == MGPU_RAW_BAD && MGPU_PF_IN_ACCEPT == MGPU_RAW_ACCEPT &&
              MGPU_PF_IN_COND == MGPU_RAW_COND && MGPU_PF_IN_UNKNOWN == MGPU_RAW_UNKNOWN && MGPU_PF_IN_MODEAC_OFF > MGPU_RAW_UNKNOWN, "Planefinder classes");
void msg_in_unit(const MsgInStretch &s, uint32_t cls, const RawInLine &r, uint64_t id, uint64_t off, IcaoFilter &flt, MsgInCounts &n) {
    if (cls == MGPU_RAW_MODEAC) ++n.cn[1];
    else if (cls != MGPU_RAW_NONE && cls <= MGPU_RAW_UNKNOWN) ++n.cn[0];             // every Mode S unit that reached the decode
    if (cls == MGPU_RAW_UNKNOWN) ++n.cn[2];
    if (cls == MGPU_RAW_BAD) ++n.cn[3];
    if (cls == MGPU_RAW_ACCEPT) ++n.cn[4 + (r.msg.correctedbits < 3 ? r.msg.correctedbits : 2)];
    if (cls == MGPU_RAW_ACCEPT || cls == MGPU_RAW_MODEAC) {
        if (n.msgs < s.msgs_cap) {
            s.msgs[n.msgs] = r.msg;
            if (s.ids) s.ids[n.msgs] = id;
            if (s.index_of) s.index_of[n.msgs] = s.unit_base + n.units;
            if (s.signal) s.signal[n.msgs] = r.signal;
        }
        ++n.msgs;
        if (r.adder) flt.add(r.addr);                                     // mode_s.c:766-779
    }
    if (n.units < s.units_cap) {
        if (s.unit_class) s.unit_class[n.units] = (uint8_t) cls;
        if (s.unit_off) s.unit_off[n.units] = s.off_base + off;
    }
    ++n.units;
}

bool raw_in_filter_load(const struct mgpu_raw_in_filter *f, IcaoFilter &flt) {
    if (!f || (f->n_active && !f->gen_active) || (f->n_inactive && !f->gen_inactive) || f->table_bits < 8 || f->table_bits > 20) return false;
    IcaoFilter::Snapshot s;
    s.members[0].assign(f->gen_active, f->gen_active + f->n_active);
    s.members[1].assign(f->gen_inactive, f->gen_inactive + f->n_inactive);
    s.active = 0; s.occupied = f->occupied; s.filter_bits = f->table_bits;
    flt.restore(s);
    return true;
}

void raw_in_filter_store(const IcaoFilter &flt, struct mgpu_raw_in_filter *f) {
    const std::vector<uint32_t> &ga = flt.members(true), &gi = flt.members(false);
    for (size_t k = 0; k < ga.size(); ++k) f->gen_active[k] = ga[k];
    for (size_t k = 0; k < gi.size(); ++k) f->gen_inactive[k] = gi[k];
    f->n_active = ga.size(); f->n_inactive = gi.size();
    f->occupied = flt.occupied(); f->table_bits = flt.table_bits();
}

// ---- the raw input ----

// raw_in_line over a line of any length (one beyond kRawInMaxLine is "not a frame")
static uint32_t raw_in_line_host(const uint8_t *line, uint64_t len, int64_t now_ms, const struct mgpu_raw_in_config *cfg, RawInLine &r) {
    const RawInTables tb = raw_in_tables_of(raw_in_host_tables(cfg->nfix_crc));
    const RawInConfig rc = {cfg->nfix_crc, cfg->fixDF, (int32_t) cfg->mode_ac};
    return raw_in_line(line, (uint32_t) (len > kRawInMaxLine ? kRawInMaxLine + 1 : len), now_ms, rc, tb, r);
}

int raw_in_decode_sequential(const struct mgpu_raw_in_args *a, const struct mgpu_raw_in_config *cfg, IcaoFilter &flt) {
    if (!a || a->size < sizeof(struct mgpu_raw_in_args) || !a->consumed || !a->nlines || !a->nmsgs || !a->counters || !raw_in_cfg_ok(cfg)) return MGPU_E_INVAL;
    if ((a->nbytes && !a->text) || (a->msgs_cap && !a->msgs) || (a->line_class_cap && !a->line_class)) return MGPU_E_INVAL;
    const MsgInStretch s = raw_in_stretch(*a);
    IcaoFilter::Snapshot before;
    flt.snapshot(before);
    MsgInCounts n;
    RawInLine r;
    const uint8_t *p = a->text, *end = a->text + a->nbytes;
    while (p < end) {
        const uint8_t *q = p;
        while (q < end && *q != '\n' && *q != 0) ++q;
        if (q >= end) break;                                              // bytes behind the last terminator are no line
        uint32_t cls = raw_in_line_host(p, (uint64_t) (q - p), a->now_ms, cfg, r);
        if (cls == MGPU_RAW_COND) cls = flt.test(r.addr) ? MGPU_RAW_ACCEPT : MGPU_RAW_UNKNOWN;
        msg_in_unit(s, cls, r, 0, 0, flt, n);
        p = q + 1;
        n.consumed = (uint64_t) (p - a->text);
    }
    raw_in_report(*a, n);
    if (msg_in_overflow(s, n)) { flt.restore(before); return MGPU_E_OVERFLOW; }
    return MGPU_OK;
}

}  // namespace mgpu

using namespace mgpu;

extern "C" {

int mgpu_raw_parse_line_host(const uint8_t *line, uint64_t len, int64_t now_ms, const struct mgpu_raw_in_config *cfg, struct mgpu_raw_in_line *out) {
    if ((len && !line) || !out || !raw_in_cfg_ok(cfg)) return MGPU_E_INVAL;
    memset(out, 0, sizeof *out);
    RawInLine r;
    const uint32_t cls = raw_in_line_host(line, len, now_ms, cfg, r);
    if (cls == MGPU_RAW_NONE) return 0;
    if (cls != MGPU_RAW_BAD) out->msg = r.msg;
    out->signal_level = r.signal;
    out->cls = cls;
    out->addr = r.addr;
    out->adder = r.adder;
    return 1;
}

int mgpu_raw_decode_host(const struct mgpu_raw_in_args *a, const struct mgpu_raw_in_config *cfg, struct mgpu_raw_in_filter *f) {
    return msg_in_decode_host(raw_in_decode_sequential, a, cfg, f);
}

}  // extern "C"
