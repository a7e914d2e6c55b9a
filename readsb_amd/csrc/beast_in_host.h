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

// the counts of a call or of one pass of it
struct BeastInCounts {
    uint64_t frames = 0, consumed = 0, msgs = 0, id = 0, stop_off = 0;
    uint32_t stop = MGPU_BEAST_STOP_END;
    uint64_t cn[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};          // struct mgpu_beast_in_counters in its order
    // for stream_passes (stream_passes.h, shared by mgpu_beast_decode over the device and the sequential walk with args->pass_bytes
    // != 0): a stretch is cut at the last som it reached; the receiver id is carried, the tail rule left to the stretch that ends the
    // stream; a stretch in which no som is reached (a frame or a run without 0x1a longer than it) is the one that is repeated
    bool stopped() const { return stop != MGPU_BEAST_STOP_END; }
    void add(const BeastInCounts &n) {
        frames += n.frames; msgs += n.msgs; id = n.id; stop = n.stop; stop_off = consumed;
        for (int k = 0; k < 10; ++k) cn[k] += n.cn[k];
    }
};

inline void beast_in_counters_of(const BeastInCounts &n, struct mgpu_beast_in_counters *k) {
    k->remote_received_modes = n.cn[0]; k->remote_received_modeac = n.cn[1]; k->remote_rejected_unknown_icao = n.cn[2]; k->remote_rejected_bad = n.cn[3];
    for (int i = 0; i < 3; ++i) k->remote_accepted[i] = n.cn[4 + i];
    k->remote_malformed_beast = n.cn[7]; k->nreceiver_ids = n.cn[8]; k->ncommands = n.cn[9];
}

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
