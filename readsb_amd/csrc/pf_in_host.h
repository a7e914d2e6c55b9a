// pf_in_host.h — private to the library and its check programs: the host side of the Planefinder input (pf_in_host.cpp).  The
// sequential walk is NOT part of the installed C ABI (include/modes_gpu.h): it is the plain statement of what kernels/pf_in.inc
// computes in parallel, exported from the library only so that the tests reach it.
#pragma once
#include <cstdint>

#include "pf_in_format.h"
#include "icao_filter.h"
#include "raw_in_host.h"
#include "stream_passes.h"

namespace mgpu {

// A call as the stretch it is and its counts to the caller (raw_in_host.h: MsgInStretch, MsgInCounts; a unit is a handler call).
#pragma GCC visibility push(hidden)
inline MsgInStretch pf_in_stretch(const struct mgpu_pf_in_args &a) {
    return {a.data, a.nbytes, a.look, a.now_ms, a.msgs, nullptr, a.signal_level, a.frame_of, a.msgs_cap, a.frame_class, a.frame_off, a.frames_cap, 0, 0, true, 0, 0};
}
inline void pf_in_report(const struct mgpu_pf_in_args &a, const MsgInCounts &n) {
    *a.consumed = n.consumed; *a.nframes = n.units; *a.nmsgs = n.msgs;
    struct mgpu_pf_in_counters *k = a.counters;
    msg_in_counters_of(n, k);
    k->nskipped = n.cn[7]; k->past_end = n.cn[8];
}
#pragma GCC visibility pop

// what a pass stages behind its nb bytes: the handler's reach, as far as the stream (args->nbytes + args->look bytes) goes
inline uint64_t pf_in_look(uint64_t total, uint64_t at, uint64_t nb) { return total - at - nb < kPfInReach ? total - at - nb : kPfInReach; }

// One readPlanefinder over a HOST-memory buffer, step by step, against `filter` (icao_filter.h), which is moved on as the reference's
// would be; the outputs as mgpu_pf_decode gives them (capacities as there: MGPU_E_OVERFLOW with what is needed and the filter as it
// was).  args->pass_bytes != 0: in passes of that many bytes (stream_passes), which gives the same.
int pf_in_decode_sequential(const struct mgpu_pf_in_args *args, const struct mgpu_raw_in_config *cfg, IcaoFilter &filter);

}  // namespace mgpu

extern "C" {
// The same for a caller without C++ (the tests, through ctypes): the filter as mgpu_raw_decode_host takes it (room for n_active + the
// stream's messages).
int mgpu_pf_decode_host(const struct mgpu_pf_in_args *args, const struct mgpu_raw_in_config *cfg, struct mgpu_raw_in_filter *filter);
}
