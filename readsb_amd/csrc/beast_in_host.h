// beast_in_host.h — private to the library and its check programs: the host side of the beast input (beast_in_host.cpp).  The
// sequential resolver is NOT part of the installed C ABI (include/modes_gpu.h): it is the plain statement of what
// kernels/beast_in.inc computes in parallel, exported from the library only so that the tests reach it.
#pragma once
#include <cstdint>

#include "beast_in_format.h"
#include "icao_filter.h"
#include "raw_in_host.h"

namespace mgpu {

// the counts of a call or of one pass of it
struct BeastInCounts {
    uint64_t frames = 0, consumed = 0, msgs = 0, id = 0, stop_off = 0;
    uint32_t stop = MGPU_BEAST_STOP_END;
    uint64_t cn[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};          // struct mgpu_beast_in_counters in its order
};

inline void beast_in_counters_of(const BeastInCounts &n, struct mgpu_beast_in_counters *k) {
    k->remote_received_modes = n.cn[0]; k->remote_received_modeac = n.cn[1]; k->remote_rejected_unknown_icao = n.cn[2]; k->remote_rejected_bad = n.cn[3];
    for (int i = 0; i < 3; ++i) k->remote_accepted[i] = n.cn[4 + i];
    k->remote_malformed_beast = n.cn[7]; k->nreceiver_ids = n.cn[8]; k->ncommands = n.cn[9];
}

// The host forms' passes (mgpu_beast_decode over the device, the sequential walk with args->pass_bytes != 0): the stream in stretches
// of `pass` bytes, each cut at the last som it reached — the next starts there, so the remainder is carried —, the receiver id carried,
// the tail rule left to the stretch that ends the stream: exactly the result of one call over the whole stream.  A stretch in which
// no som is reached (a frame or a run without 0x1a longer than it) is undone and repeated twice as long.
//   run(at, nb, final, all, n): the stretch [at, at + nb) with receiver id all.id, its results stored at all.msgs / all.frames of the
//     caller's arrays as far as they reach, its counts in n (n.consumed relative to at); undo(): the filter as before the last run.
template <class Run, class Undo>
int beast_in_passes(uint64_t nbytes, uint64_t pass, BeastInCounts &all, Run run, Undo undo) {
    if (pass == 0 || pass > nbytes) pass = nbytes;
    for (uint64_t at = 0;;) {
        const uint64_t nb = pass < nbytes - at ? pass : nbytes - at;
        const bool final = at + nb >= nbytes;
        BeastInCounts n;
        if (int rc = run(at, nb, final, all, n)) return rc;
        if (n.consumed == 0 && n.stop == MGPU_BEAST_STOP_END && !final) {
            undo();
            pass = pass > nbytes / 2 ? nbytes : 2 * pass;
            continue;
        }
        all.frames += n.frames; all.msgs += n.msgs; all.id = n.id;
        for (int k = 0; k < 10; ++k) all.cn[k] += n.cn[k];
        at += n.consumed;
        all.consumed = at; all.stop = n.stop; all.stop_off = at;
        if (final || n.stop != MGPU_BEAST_STOP_END) return MGPU_OK;
    }
}

// One readBeast over a HOST-memory buffer, step by step, against `filter` (icao_filter.h), which is moved on as the reference's would
// be; the outputs as mgpu_beast_decode gives them (capacities as there: MGPU_E_OVERFLOW with what is needed and the filter as it was).
// args->pass_bytes != 0: in passes of that many bytes (beast_in_passes), which gives the same.
int beast_in_decode_sequential(const struct mgpu_beast_in_args *args, const struct mgpu_raw_in_config *cfg, IcaoFilter &filter);

}  // namespace mgpu

extern "C" {
// The same for a caller without C++ (the tests, through ctypes): the filter as mgpu_raw_decode_host takes it (room for n_active + the
// stream's messages).  cfg->mode_ac is the handler's Modes.mode_ac; net_ingest is args->net_ingest.
int mgpu_beast_decode_host(const struct mgpu_beast_in_args *args, const struct mgpu_raw_in_config *cfg, struct mgpu_raw_in_filter *filter);
}
