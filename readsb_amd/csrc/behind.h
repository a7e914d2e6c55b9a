// behind.h — private to the library: the device state of what runs behind the message list (behind.cpp).  Only the synchronous calls
// on stream_aux touch it, never the pipeline's threads.  api.cpp creates it with the context and releases it in mgpu_destroy.
#pragma once
#include "ctx.h"

// Owning, grow-only device scratch.  A failed reservation leaves it empty with the context's error text set.
struct DevBuf {
    void *p = nullptr;
    uint64_t cap = 0;                                        // bytes
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void) hipFree(p);
        p = nullptr; cap = 0;
    }
    int reserve_exact(mgpu_ctx *c, uint64_t bytes) {
        if (bytes <= cap) return MGPU_OK;
        release();
        HIPCHK(c, hipMalloc(&p, bytes));
        cap = bytes;
        return MGPU_OK;
    }
    int reserve(mgpu_ctx *c, uint64_t bytes) {               // with slack: lists of slowly growing sizes do not reallocate every call
        const uint64_t slack = bytes / 4 + 1024;
        return bytes <= cap ? MGPU_OK : reserve_exact(c, bytes + slack < bytes ? bytes : bytes + slack);
    }
    template <class T> T *as() const { return (T *) p; }
};

struct Behind {
    // the host-array forms' staged inputs and results: the message list, its verdicts and receiver ids; the beast stream, the deferred list
    DevBuf d_beast_in, d_beast_verdict, d_beast_ids, d_beast_out, d_deferred;
    // beast encoder scratch: per message length | signal byte << 8; per workgroup frame bytes | deferred messages and their offsets
    // (two halves each); the totals {bytes, deferred, last id}; with receiver ids the per-workgroup summaries
    DevBuf d_beast_len, d_beast_blocks, d_beast_off, d_beast_total, d_beast_idw;
    // the text outputs (kernels/text.inc): per message a line's length; per workgroup bytes | deferred | skipped and the first two's offsets (three
    // runs each); the three totals; the host-array forms' positions and geom_delta values (the rest is staged where the encoder stages it)
    DevBuf d_text_len, d_text_blocks, d_text_off, d_text_total, d_text_pos, d_text_delta;
    DevBuf d_asx_ids, d_asx_baro_alt, d_asx_category;            // mgpu_asterix_encode_ex's three optional arrays
    // the message dump (kernels/dump.inc): per message a dump's length (32 bits; the workgroup scratch is the text outputs'); the host-array
    // form's five optional arrays
    DevBuf d_dump_len, d_dump_forward, d_dump_ids, d_dump_pos, d_dump_nic, d_dump_rc;
    DevBuf d_fields;                                         // the host-array forms' field records
    // UAT input (kernels/uat.inc): per lane of a tile a halfword; per tile five words and three offsets; the five totals; the deferred
    // lines' indices; the table of signal bytes, uploaded on first use; the host-array form's staged text and its results
    DevBuf d_uat_meta, d_uat_blocks, d_uat_off, d_uat_total, d_uat_deferred, d_uat_sig_table, d_uat_in, d_uat_out, d_uat_msgs, d_uat_sig, d_uat_line_of;
    // SBS input (kernels/sbs_in.inc): the UAT input's scratch layout in buffers of its own; the host-array form's staged text and its results
    DevBuf d_sbs_in_meta, d_sbs_in_blocks, d_sbs_in_off, d_sbs_in_total, d_sbs_in_deferred, d_sbs_in_text, d_sbs_in_recs, d_sbs_in_line_of;
    // Raw input (kernels/raw_in.inc): the UAT input's per-tile scratch in buffers of its own; per candidate the record, the signal, the
    // line, the class word and the new adds; per workgroup of candidates two words and two offsets; the counters, L* and two totals;
    // the first-adder table (64 MiB, allocated and set to all ones by the first call), the two generation bitmaps (2 MiB each, zero
    // outside a call) and the members lists scattered into them; the CRC byte table; the host-array form's staged text and results
    DevBuf d_raw_in_meta, d_raw_in_blocks, d_raw_in_off, d_raw_in_total, d_raw_in_cand_rec, d_raw_in_cand_sig, d_raw_in_cand_line, d_raw_in_cand_meta, d_raw_in_new_adds;
    DevBuf d_raw_in_cb, d_raw_in_co, d_raw_in_misc, d_raw_in_first, d_raw_in_gen, d_raw_in_members, d_raw_in_crc;
    DevBuf d_raw_in_text, d_raw_in_msgs, d_raw_in_line_of, d_raw_in_sig, d_raw_in_cls;
    // Beast input (kernels/beast_in.inc): the tiles' and the groups' exit maps, the entries, the chain's bitmap; per lane a halfword and
    // an id; per tile six words, two offsets, an id set, an id in force and a flag; the nine totals; per candidate the id in force (the
    // other candidate arrays and the filter's tables are the raw input's); the host-array form's staged stream and results
    DevBuf d_bin_maps, d_bin_gmaps, d_bin_entry, d_bin_marks, d_bin_meta, d_bin_lane_ids, d_bin_blocks, d_bin_off, d_bin_tile_id, d_bin_entry_id, d_bin_idflag, d_bin_total;
    DevBuf d_bin_cand_id, d_bin_data, d_bin_msgs, d_bin_ids, d_bin_sig, d_bin_frame_of, d_bin_cls, d_bin_frame_off;
    // ASTERIX input (kernels/asterix_in.inc): the tiles' and the groups' exit maps; the entries; three bitmaps per tile; per tile four
    // words and two offsets; the nine totals; the host-array form's staged stream and its results
    DevBuf d_ast_in_maps, d_ast_in_gmaps, d_ast_in_entry, d_ast_in_bits, d_ast_in_blocks, d_ast_in_off, d_ast_in_total, d_ast_in_data, d_ast_in_recs, d_ast_in_frame_of;
    DevBuf d_roll_tan;                                      // tables.h build_roll_tangent_table(), uploaded on first use
    // the first-stage tracking gate (kernels/gate.inc): the aircraft table (1 GiB, allocated and zeroed by the first call), its scratch,
    // the host-array forms' verdicts
    DevBuf d_gate_table, d_gate_scratch, d_gate_verdict;
    // CPR pairing + position decode (kernels/cpr.inc): the aircraft table (2 GiB, likewise), its scratch, the host-array forms' positions
    // and cases | results
    DevBuf d_cpr_table, d_cpr_scratch, d_cpr_out, d_cpr_cases;
    // the time merge (kernels/merge.inc): its scratch; the host-array form's merged records | permutation | ids | verdicts
    DevBuf d_merge_scratch, d_merge_out;
    int merge_passes = 0;                                    // digit passes of the last merge
};
