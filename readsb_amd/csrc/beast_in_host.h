// beast_in_host.h — private to the library and its check programs: the host side of the beast input (beast_in_host.cpp).  The
// sequential resolver is NOT part of the installed C ABI (include/modes_gpu.h): it is the plain statement of what
// kernels/beast_in.inc computes in parallel, exported from the library only so that the tests reach it.
#pragma once
#include <cstdint>

#include "beast_in_format.h"
#include "icao_filter.h"
#include "raw_in_host.h"
#include "stream_passes.h"

namespace mgpu {

// A call as the stretch it is and its counts to the caller (raw_in_host.h: MsgInStretch, MsgInCounts; a unit is a handler call).
// Between passes (stream_passes.h) the receiver id is carried and the tail rule left to the stretch that ends the stream.
#pragma GCC visibility push(hidden)
inline MsgInStretch beast_in_stretch(const struct mgpu_beast_in_args &a) {
    return {a.data, a.nbytes, 0, a.now_ms, a.msgs, a.receiver_id, a.signal_level, a.frame_of, a.msgs_cap, a.frame_class, a.frame_off, a.frames_cap, 0, 0, true,
            a.receiver_id_in, a.net_ingest};
}
inline void beast_in_report(const struct mgpu_beast_in_args &a, const MsgInCounts &n) {
    *a.consumed = n.consumed; *a.nframes = n.units; *a.nmsgs = n.msgs; *a.stop = n.stop; *a.stop_off = n.stop_off; *a.receiver_id_out = n.id;
    struct mgpu_beast_in_counters *k = a.counters;
    msg_in_counters_of(n, k);
    k->remote_malformed_beast = n.cn[7]; k->nreceiver_ids = n.cn[8]; k->ncommands = n.cn[9];
}
#pragma GCC visibility pop

// One readBeast over a HOST-memory buffer, step by step, against `filter` (icao_filter.h), which is moved on as the reference's would
// be; the outputs as mgpu_beast_decode gives them (capacities as there: MGPU_E_OVERFLOW with what is needed and the filter as it was).
// args->pass_bytes != 0: in passes of that many bytes (stream_passes), which gives the same.
int beast_in_decode_sequential(const struct mgpu_beast_in_args *args, const struct mgpu_raw_in_config *cfg, IcaoFilter &filter);

}  // namespace mgpu

extern "C" {
// The same for a caller without C++ (the tests, through ctypes): the filter as mgpu_raw_decode_host takes it (room for n_active + the
// stream's messages).  cfg->mode_ac is the handler's Modes.mode_ac; net_ingest is args->net_ingest.
int mgpu_beast_decode_host(const struct mgpu_beast_in_args *args, const struct mgpu_raw_in_config *cfg, struct mgpu_raw_in_filter *filter);
}
