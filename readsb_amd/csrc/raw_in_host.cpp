// raw_in_host.cpp — the raw input (raw_in_format.h) on the host: mgpu_raw_parse_line_host, the line splitter, and
// mgpu_raw_decode_host, the SEQUENTIAL resolver — every line in order against a model of icao_filter.c, the plain statement of the
// rule kernels/raw_in.inc resolves in parallel.  No HIP in this file: tests/host_stub/raw_in_format_check.cpp and
// raw_in_resolve_check.cpp compile it with plain g++ (with tables.cpp), under ASan and UBSan too.
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

}  // namespace mgpu

using namespace mgpu;

static bool raw_in_cfg_ok(const struct mgpu_raw_in_config *cfg) {
    return cfg && cfg->size >= sizeof(struct mgpu_raw_in_config) && cfg->nfix_crc >= 0 && cfg->nfix_crc <= 2;
}

namespace mgpu {

int raw_in_decode_sequential(const struct mgpu_raw_in_args *a, const struct mgpu_raw_in_config *cfg, IcaoFilter &flt) {
    if (!a || a->size < sizeof(struct mgpu_raw_in_args) || !a->consumed || !a->nlines || !a->nmsgs || !a->counters || !raw_in_cfg_ok(cfg)) return MGPU_E_INVAL;
    if ((a->nbytes && !a->text) || (a->msgs_cap && !a->msgs) || (a->line_class_cap && !a->line_class)) return MGPU_E_INVAL;
    IcaoFilter::Snapshot before;
    flt.snapshot(before);
    struct mgpu_raw_in_counters cn;
    memset(&cn, 0, sizeof cn);
    uint64_t consumed = 0, nlines = 0, nmsgs = 0;
    const uint8_t *p = a->text, *end = a->text + a->nbytes;
    while (p < end) {
        const uint8_t *q = p;
        while (q < end && *q != '\n' && *q != 0) ++q;
        if (q >= end) break;                                              // bytes behind the last terminator are no line
        struct mgpu_raw_in_line r;
        (void) mgpu_raw_parse_line_host(p, (uint64_t) (q - p), a->now_ms, cfg, &r);
        uint32_t cls = r.cls;
        if (cls == MGPU_RAW_COND) cls = flt.test(r.addr) ? MGPU_RAW_ACCEPT : MGPU_RAW_UNKNOWN;
        if (cls == MGPU_RAW_MODEAC) ++cn.remote_received_modeac;
        else if (cls != MGPU_RAW_NONE) ++cn.remote_received_modes;
        if (cls == MGPU_RAW_UNKNOWN) ++cn.remote_rejected_unknown_icao;
        if (cls == MGPU_RAW_BAD) ++cn.remote_rejected_bad;
        if (cls == MGPU_RAW_ACCEPT) ++cn.remote_accepted[r.msg.correctedbits < 3 ? r.msg.correctedbits : 2];
        if (cls == MGPU_RAW_ACCEPT || cls == MGPU_RAW_MODEAC) {
            if (nmsgs < a->msgs_cap) {
                a->msgs[nmsgs] = r.msg;
                if (a->line_of) a->line_of[nmsgs] = nlines;
                if (a->signal_level) a->signal_level[nmsgs] = r.signal_level;
            }
            ++nmsgs;
            if (r.adder) flt.add(r.addr);                                 // mode_s.c:766-779
        }
        if (a->line_class && nlines < a->line_class_cap) a->line_class[nlines] = (uint8_t) cls;
        ++nlines;
        p = q + 1;
        consumed = (uint64_t) (p - a->text);
    }
    *a->consumed = consumed; *a->nlines = nlines; *a->nmsgs = nmsgs; *a->counters = cn;
    if (nmsgs > a->msgs_cap || (a->line_class && nlines > a->line_class_cap)) { flt.restore(before); return MGPU_E_OVERFLOW; }
    return MGPU_OK;
}

}  // namespace mgpu

extern "C" {

int mgpu_raw_parse_line_host(const uint8_t *line, uint64_t len, int64_t now_ms, const struct mgpu_raw_in_config *cfg, struct mgpu_raw_in_line *out) {
    if ((len && !line) || !out || !raw_in_cfg_ok(cfg)) return MGPU_E_INVAL;
    memset(out, 0, sizeof *out);
    const RawInTables tb = raw_in_tables_of(raw_in_host_tables(cfg->nfix_crc));
    const RawInConfig rc = {cfg->nfix_crc, cfg->fixDF, (int32_t) cfg->mode_ac};
    RawInLine r;
    const uint32_t cls = raw_in_line(line, (uint32_t) (len > kRawInMaxLine ? kRawInMaxLine + 1 : len), now_ms, rc, tb, r);
    if (cls == MGPU_RAW_NONE) return 0;
    if (cls != MGPU_RAW_BAD) out->msg = r.msg;
    out->signal_level = r.signal;
    out->cls = cls;
    out->addr = r.addr;
    out->adder = r.adder;
    return 1;
}

int mgpu_raw_decode_host(const struct mgpu_raw_in_args *a, const struct mgpu_raw_in_config *cfg, struct mgpu_raw_in_filter *f) {
    if (!f || (f->n_active && !f->gen_active) || (f->n_inactive && !f->gen_inactive) || f->table_bits < 8 || f->table_bits > 20) return MGPU_E_INVAL;
    IcaoFilter::Snapshot s;
    s.members[0].assign(f->gen_active, f->gen_active + f->n_active);
    s.members[1].assign(f->gen_inactive, f->gen_inactive + f->n_inactive);
    s.active = 0; s.occupied = f->occupied; s.filter_bits = f->table_bits;
    IcaoFilter flt;
    flt.restore(s);
    const int rc = raw_in_decode_sequential(a, cfg, flt);
    if (rc != MGPU_OK) return rc;
    const std::vector<uint32_t> &ga = flt.members(true), &gi = flt.members(false);
    for (size_t k = 0; k < ga.size(); ++k) f->gen_active[k] = ga[k];
    for (size_t k = 0; k < gi.size(); ++k) f->gen_inactive[k] = gi[k];
    f->n_active = ga.size(); f->n_inactive = gi.size();
    f->occupied = flt.occupied(); f->table_bits = flt.table_bits();
    return MGPU_OK;
}

}  // extern "C"
