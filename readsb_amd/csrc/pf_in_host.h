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

// the counts of a call or of one pass of it
struct PfInCounts {
    uint64_t frames = 0, consumed = 0, msgs = 0;
    uint64_t cn[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};              // struct mgpu_pf_in_counters in its order
    // for stream_passes (stream_passes.h, shared by mgpu_pf_decode over the device and the sequential walk with args->pass_bytes != 0):
    // a stretch is cut at the som it reached; nothing stops a stream; a stretch that reaches no som (a frame longer than it) is the
    // one that is repeated
    bool stopped() const { return false; }
    void add(const PfInCounts &n) {
        frames += n.frames; msgs += n.msgs;
        for (int k = 0; k < 9; ++k) cn[k] += n.cn[k];
    }
};

inline void pf_in_counters_of(const PfInCounts &n, struct mgpu_pf_in_counters *k) {
    k->remote_received_modes = n.cn[0]; k->remote_received_modeac = n.cn[1]; k->remote_rejected_unknown_icao = n.cn[2]; k->remote_rejected_bad = n.cn[3];
    for (int i = 0; i < 3; ++i) k->remote_accepted[i] = n.cn[4 + i];
    k->nskipped = n.cn[7]; k->past_end = n.cn[8];
}

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
