// raw_in_host.h — private to the library and its check programs: the host side of the raw input (raw_in_host.cpp), and what the three
// message inputs (raw, beast, Planefinder) share on the host: one stretch, one set of counts, the tail of a sequential walk, the
// filter's way through the C entries.  The sequential resolver below is NOT part of the installed C ABI (include/modes_gpu.h): it is
// the plain statement of the rule for the host-side checks and the tests, exported from the library only so that the tests reach it.
#pragma once
#include <cstdint>
#include <vector>

#include "icao_filter.h"
#include "raw_in_format.h"

namespace mgpu {

struct RawInHostTables {
    std::vector<uint64_t> tab_long, tab_short;
};
const RawInHostTables &raw_in_host_tables(int nfix_crc);     // the packed syndrome tables of an nfix_crc value, built once
RawInTables raw_in_tables_of(const RawInHostTables &t);

// ---- what the message inputs share (hidden: nothing of it is among the library's dynamic symbols) ----
#pragma GCC visibility push(hidden)

bool raw_in_cfg_ok(const struct mgpu_raw_in_config *cfg);    // the three inputs' configuration

// One stretch of a stream and where its results go, whatever the format: a call's own (raw_in_stretch, beast_in_stretch,
// pf_in_stretch map the public args onto it) or one pass of a host form.  A unit is what the format counts besides messages: a line
// (raw) or a handler call (beast, Planefinder).
struct MsgInStretch {
    const uint8_t *data;
    uint64_t nbytes, look;                                   // nbytes are framed; `look` bytes behind them are the stream's too (Planefinder)
    int64_t now_ms;
    mgpu_msg *msgs;                                          // per message, msgs_cap entries: the record, the receiver id (beast), the signal
    uint64_t *ids;                                           // level, the unit that gave it
    double *signal;
    uint64_t *index_of;
    uint64_t msgs_cap;
    uint8_t *unit_class;                                     // per unit, units_cap entries: its class, its offset (beast, Planefinder)
    uint64_t *unit_off;
    uint64_t units_cap;
    uint64_t unit_base, off_base;                            // added to every index_of and unit_off (a pass of a host form)
    bool final;                                              // the stretch ends the stream: beast's tail rule applies
    uint64_t receiver_id_in;                                 // beast: the id in force in front of the stretch, Modes.netIngest
    uint32_t net_ingest;
};

// The counts of a call or of one pass of it: units, bytes consumed, messages; beast's receiver id in force and its stop; the public
// counters in their struct's order (raw 7, Planefinder 9, beast 10).
struct MsgInCounts {
    uint64_t units = 0, consumed = 0, msgs = 0, id = 0, stop_off = 0;
    uint32_t stop = 0;                                       // MGPU_BEAST_STOP_END; nothing stops the other two
    uint64_t cn[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // for stream_passes (stream_passes.h, shared by the host forms over the device and the sequential walks with args->pass_bytes != 0):
    // a stretch is cut at the last unit that ends inside it (beast, Planefinder: at the som it reached); the receiver id is carried;
    // a stretch that consumes nothing (a line, a frame or a run without 0x1a longer than it) is the one that is repeated
    bool stopped() const { return stop != 0; }
    void add(const MsgInCounts &n) {
        units += n.units; msgs += n.msgs; id = n.id; stop = n.stop; stop_off = consumed;
        for (int k = 0; k < 10; ++k) cn[k] += n.cn[k];
    }
};

// The seven counters the three structs start with.
template <class Counters>
inline void msg_in_counters_of(const MsgInCounts &n, Counters *k) {
    k->remote_received_modes = n.cn[0]; k->remote_received_modeac = n.cn[1]; k->remote_rejected_unknown_icao = n.cn[2]; k->remote_rejected_bad = n.cn[3];
    for (int i = 0; i < 3; ++i) k->remote_accepted[i] = n.cn[4 + i];
}

// 0, or which capacity the counts exceed: 1 the per-message arrays', 2 the per-unit arrays'
inline int msg_in_overflow(const MsgInStretch &s, const MsgInCounts &n) {
    return n.msgs > s.msgs_cap ? 1 : (s.unit_class || s.unit_off) && n.units > s.units_cap ? 2 : 0;
}

// The stretch [at, at + nb) of a stream in HOST memory as a pass of stream_passes: a's arrays behind what so_far has stored.
MsgInStretch msg_in_slice(const MsgInStretch &a, uint64_t at, uint64_t nb, uint64_t look, bool final, const MsgInCounts &so_far);

// The tail every sequential walk shares, for one unit of class cls (MGPU_RAW_*, _COND resolved against the filter; the other two
// formats' classes have the same values up to _UNKNOWN, and their own beyond count nothing here) with r what the parser left: the
// counters, the record and its per-message entries below msgs_cap, the filter's add (mode_s.c:766-779), the unit's class and offset
// (off_base + off) below units_cap.
void msg_in_unit(const MsgInStretch &s, uint32_t cls, const RawInLine &r, uint64_t id, uint64_t off, IcaoFilter &flt, MsgInCounts &n);

inline MsgInStretch raw_in_stretch(const struct mgpu_raw_in_args &a) {
    return {a.text, a.nbytes, 0, a.now_ms, a.msgs, nullptr, a.signal_level, a.line_of, a.msgs_cap, a.line_class, nullptr, a.line_class_cap, 0, 0, true, 0, 0};
}
inline void raw_in_report(const struct mgpu_raw_in_args &a, const MsgInCounts &n) {
    *a.consumed = n.consumed; *a.nlines = n.units; *a.nmsgs = n.msgs;
    msg_in_counters_of(n, a.counters);
}
#pragma GCC visibility pop

// Every terminated line of a HOST-memory text in order through the parser and decodeModesMessage's filter questions, against `filter`
// (icao_filter.h: the library's own model), which is moved on as the reference's would be; the outputs as mgpu_raw_decode gives them
// (capacities as there: MGPU_E_OVERFLOW with what is needed and the filter as it was).
int raw_in_decode_sequential(const struct mgpu_raw_in_args *args, const struct mgpu_raw_in_config *cfg, IcaoFilter &filter);

}  // namespace mgpu

extern "C" {
// The same for a caller without C++ (the tests, through ctypes): the filter given and returned as its two generations (addresses
// below 2^24; room for n_active + the text's lines and n_inactive entries), its occupied count and log2 of its table size.
struct mgpu_raw_in_filter {
    uint32_t *gen_active, *gen_inactive;
    uint64_t n_active, n_inactive;
    uint32_t occupied, table_bits;
};
int mgpu_raw_decode_host(const struct mgpu_raw_in_args *args, const struct mgpu_raw_in_config *cfg, struct mgpu_raw_in_filter *filter);
}

namespace mgpu {
#pragma GCC visibility push(hidden)
bool raw_in_filter_load(const struct mgpu_raw_in_filter *f, IcaoFilter &flt);    // false: f is no filter
void raw_in_filter_store(const IcaoFilter &flt, struct mgpu_raw_in_filter *f);
// A sequential walk (raw_in_decode_sequential or one of its like) behind its C entry: the filter out of f, the walk, and unless it
// failed the generations written back.
template <class Args>
int msg_in_decode_host(int (*walk)(const Args *, const struct mgpu_raw_in_config *, IcaoFilter &), const Args *args, const struct mgpu_raw_in_config *cfg,
                       struct mgpu_raw_in_filter *f) {
    IcaoFilter flt;
    if (!raw_in_filter_load(f, flt)) return MGPU_E_INVAL;
    const int rc = walk(args, cfg, flt);
    if (rc == MGPU_OK) raw_in_filter_store(flt, f);
    return rc;
}
#pragma GCC visibility pop
}  // namespace mgpu
