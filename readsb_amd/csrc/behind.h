// behind.h — private to the library: the device state of what runs behind the message list (behind_out.cpp: the outputs over the list;
// behind_in.cpp: the stream inputs).  Only the synchronous calls on stream_aux touch it, never the pipeline's threads: one call is live
// at a time, so scratch and staging belong to a ROLE — the staged list, the staged stream, the tile scratch — and every format that
// needs the role uses the same buffer.  What persists from call to call (the tables) is never shared.  api.cpp creates it with the
// context and releases it in mgpu_destroy.
#pragma once
#include "devbuf.h"

// The line inputs' scratch (UAT, SBS, raw: kernels.h UatScratch): per lane of a tile a halfword; per tile five words and three offsets;
// the totals; for the two that defer lines, the deferred lines' indices.
struct LineScratch {
    DevBuf meta, blocks, off, total, deferred;
    int reserve(mgpu_ctx *c, uint64_t nbytes, UatScratch *w) {
        const size_t nb = (size_t) (nbytes / kUatTile + 2);
        if (int rc = meta.reserve(c, nb * kBlock * sizeof(uint16_t))) return rc;
        if (int rc = blocks.reserve(c, 5 * nb * sizeof(uint32_t))) return rc;
        if (int rc = off.reserve(c, 3 * nb * sizeof(unsigned long long))) return rc;
        if (int rc = total.reserve_exact(c, 8 * sizeof(unsigned long long))) return rc;
        *w = {meta.as<uint16_t>(), blocks.as<uint32_t>(), off.as<unsigned long long>(), total.as<unsigned long long>(), nb};
        return MGPU_OK;
    }
    int reserve_deferred(mgpu_ctx *c, uint64_t room) { return deferred.reserve(c, (room + 64) * sizeof(unsigned long long)); }
};

// The beast input's scratch (kernels.h BeastInScratch): the tiles' and the groups' exit maps, the entries, the chain's bitmap; per lane
// a halfword and an id; per tile six words, two offsets, an id set, an id in force and a flag; the nine totals; per candidate the id in
// force (the other candidate arrays are FilterPasses').
struct BeastInBufs {
    DevBuf maps, gmaps, entry, marks, meta, lane_ids, blocks, off, tile_id, entry_id, idflag, total, cand_id;
    int reserve(mgpu_ctx *c, uint64_t nbytes, BeastInScratch *w) {
        const size_t tiles = beast_in_tiles(nbytes), groups = beast_in_groups(nbytes);
        if (int rc = maps.reserve(c, tiles * 64)) return rc;
        if (int rc = gmaps.reserve(c, groups * 64)) return rc;
        if (int rc = entry.reserve(c, (tiles + groups) * sizeof(uint32_t))) return rc;
        if (int rc = marks.reserve(c, tiles * kBlock * sizeof(uint32_t))) return rc;
        if (int rc = meta.reserve(c, tiles * kBlock * sizeof(uint16_t))) return rc;
        if (int rc = lane_ids.reserve(c, tiles * kBlock * sizeof(uint64_t))) return rc;
        if (int rc = blocks.reserve(c, 6 * tiles * sizeof(uint32_t))) return rc;
        if (int rc = off.reserve(c, 2 * tiles * sizeof(uint64_t))) return rc;
        if (int rc = tile_id.reserve(c, tiles * sizeof(uint64_t))) return rc;
        if (int rc = entry_id.reserve(c, tiles * sizeof(uint64_t))) return rc;
        if (int rc = idflag.reserve(c, tiles * sizeof(uint32_t))) return rc;
        if (int rc = total.reserve_exact(c, 16 * sizeof(unsigned long long))) return rc;
        if (int rc = cand_id.reserve(c, beast_in_max_msgs(nbytes) * sizeof(uint64_t))) return rc;
        *w = {maps.as<uint8_t>(), gmaps.as<uint8_t>(), entry.as<uint32_t>(), marks.as<uint32_t>(), meta.as<uint16_t>(), lane_ids.as<unsigned long long>(),
              blocks.as<uint32_t>(), off.as<unsigned long long>(), tile_id.as<unsigned long long>(), entry_id.as<unsigned long long>(), idflag.as<uint32_t>(),
              total.as<unsigned long long>()};
        return MGPU_OK;
    }
    // The Planefinder input's scratch (kernels.h PfInScratch) in the same buffers, by role — one call is live at a time: the tiles'
    // event words where the entries are, their state bytes where the maps are; per lane a halfword; per tile four counts and two
    // offsets; the totals (the candidate arrays are FilterPasses').
    int reserve_pf(mgpu_ctx *c, uint64_t nbytes, PfInScratch *w) {
        const size_t tiles = pf_in_tiles(nbytes) + 1;
        if (int rc = entry.reserve(c, 5 * tiles * sizeof(uint32_t))) return rc;
        if (int rc = maps.reserve(c, tiles)) return rc;
        if (int rc = meta.reserve(c, tiles * kBlock * sizeof(uint16_t))) return rc;
        if (int rc = blocks.reserve(c, 4 * tiles * sizeof(uint32_t))) return rc;
        if (int rc = off.reserve(c, 2 * tiles * sizeof(uint64_t))) return rc;
        if (int rc = total.reserve_exact(c, 16 * sizeof(unsigned long long))) return rc;
        *w = {entry.as<uint32_t>(), maps.as<uint8_t>(), meta.as<uint16_t>(), blocks.as<uint32_t>(), off.as<unsigned long long>(), total.as<unsigned long long>()};
        return MGPU_OK;
    }
};

// The ASTERIX input's scratch (kernels.h AstInScratch): the tiles' and the groups' exit maps; the entries; three bitmaps per tile; per
// tile four words and two offsets; the nine totals.
struct AstInBufs {
    DevBuf maps, gmaps, entry, bits, blocks, off, total;
    int reserve(mgpu_ctx *c, uint64_t nbytes, AstInScratch *w) {
        const size_t tiles = ast_in_tiles(nbytes), groups = ast_in_groups(nbytes);
        if (int rc = maps.reserve(c, (uint64_t) tiles * kAstTile * sizeof(uint16_t))) return rc;
        if (int rc = gmaps.reserve(c, (uint64_t) groups * kAstTile * sizeof(uint16_t))) return rc;
        if (int rc = entry.reserve(c, (tiles + groups) * sizeof(uint32_t))) return rc;
        if (int rc = bits.reserve(c, 3 * (uint64_t) tiles * kAstWords * sizeof(uint32_t))) return rc;
        if (int rc = blocks.reserve(c, 4 * tiles * sizeof(uint32_t))) return rc;
        if (int rc = off.reserve(c, 2 * tiles * sizeof(unsigned long long))) return rc;
        if (int rc = total.reserve_exact(c, 16 * sizeof(unsigned long long))) return rc;
        *w = {maps.as<uint16_t>(), gmaps.as<uint16_t>(), entry.as<uint32_t>(), bits.as<uint32_t>(), blocks.as<uint32_t>(), off.as<unsigned long long>(),
              total.as<unsigned long long>(), tiles};
        return MGPU_OK;
    }
};

// The filter passes of the raw and the beast input (kernels/raw_in.inc): per candidate the record, the signal, the line, the class
// word and the new adds; per workgroup of candidates two words and two offsets; the counters, L* and two totals; the members lists.
// PERSISTENT: the first-adder table (64 MiB, allocated and set to all ones by the first call), the two generation bitmaps (2 MiB each,
// zero outside a call) and the CRC byte table.
struct FilterPasses {
    DevBuf cand_rec, cand_sig, cand_line, cand_meta, new_adds, cb, co, misc, members;
    DevBuf first, gen, crc;
};

struct Behind {
    // ---- the outputs over the list ----
    // the host-array forms' staged list, its verdicts and field records; the stream an encoder wrote and its deferred list
    DevBuf d_list, d_list_verdict, d_fields, d_out, d_deferred;
    // their optional per-message arrays, by role: positions, 64-bit ids, a 32-bit word, a byte (and the dump's second byte)
    DevBuf d_opt_pos, d_opt_ids, d_opt_word, d_opt_byte, d_opt_byte2;
    // beast encoder scratch: per message length | signal byte << 8; per workgroup frame bytes | deferred messages and their offsets
    // (two halves each); the totals {bytes, deferred, last id}; with receiver ids the per-workgroup summaries
    DevBuf d_beast_len, d_beast_blocks, d_beast_off, d_beast_total, d_beast_idw;
    // the text outputs (kernels/text.inc), ASTERIX out and the dump: per message a line's length (16 bits; the dump's: 32); per workgroup
    // bytes | deferred | skipped and the first two's offsets (three runs each); the three totals
    DevBuf d_text_len, d_text_blocks, d_text_off, d_text_total;
    DevBuf d_roll_tan;                                      // PERSISTENT: tables.h build_roll_tangent_table(), uploaded on first use
    // the first-stage tracking gate (kernels/gate.inc): PERSISTENT the aircraft table (1 GiB, allocated and zeroed by the first call);
    // its scratch, the host-array forms' verdicts
    DevBuf d_gate_table, d_gate_scratch, d_gate_verdict;
    // CPR pairing + position decode (kernels/cpr.inc): PERSISTENT the aircraft table (2 GiB, likewise); its scratch, the host-array
    // forms' positions and cases | results
    DevBuf d_cpr_table, d_cpr_scratch, d_cpr_out, d_cpr_cases;
    // the time merge (kernels/merge.inc): its scratch; the host-array form's merged records | permutation | ids | verdicts
    DevBuf d_merge_scratch, d_merge_out;
    int merge_passes = 0;                                    // digit passes of the last merge

    // ---- the stream inputs ----
    LineScratch lines;
    BeastInBufs beast_in;                                    // (the Planefinder input frames in these too: reserve_pf)
    AstInBufs ast_in;
    FilterPasses filter;
    DevBuf d_uat_sig_table;                                  // PERSISTENT: the UAT input's table of signal bytes, uploaded on first use
    // the host forms' staged pass of the stream, and what a pass gives before it is copied out: per unit its line or frame index;
    // message records, their signal levels, a class byte per line or handler call (raw, beast, UAT's records); each format's own
    DevBuf d_stream, d_index_of, d_in_msgs, d_in_signal, d_in_class;
    DevBuf d_uat_out, d_uat_sig, d_sbs_in_recs, d_ast_in_recs, d_bin_ids, d_bin_frame_off;
};
