// behind_in.cpp — behind the message list, the stream inputs: UAT, SBS, raw, beast, Planefinder and ASTERIX, each as a `_device` entry over a stream
// in HBM and a host form that stages the stream in passes (stream_passes.h); the one host core of the three message inputs.
// (The outputs over the list: behind_out.cpp.)
#include "behind.h"

#include <cstring>

#include "uat_format.h"
#include "sbs_in_format.h"
#include "raw_in_format.h"
#include "beast_in_host.h"
#include "pf_in_host.h"
#include "asterix_in_format.h"

constexpr uint64_t kLineDefaultPass = 64ull << 20;           // bytes the UAT, SBS, raw, beast and Planefinder host forms stage per pass, pass_bytes == 0
constexpr uint64_t kAstInDefaultPass = 16ull << 20;          // ... and the ASTERIX host form

// The counts of a UAT or SBS call, or of one pass of it (stream_passes.h), in the order of UatScratch's totals: lines, bytes consumed,
// units (UAT: frames; SBS: records), deferred lines, rejects (UAT: short lines; SBS: invalid ones).  Nothing stops a text.
struct LineCounts {
    uint64_t lines = 0, consumed = 0, units = 0, deferred = 0, rejects = 0;
    bool stopped() const { return false; }
    void add(const LineCounts &n) { lines += n.lines; units += n.units; deferred += n.deferred; rejects += n.rejects; }
};

// Behind the launch of either: the five totals back as the counts of this text; the deferred lines' indices, as far as def_room
// reached, to the caller's HOST list.
static int line_counts_back(mgpu_ctx *c, const UatScratch &w, uint64_t def_room, uint64_t *deferred, LineCounts *n) {
    HIPCHK(c, hipGetLastError());
    unsigned long long total[5] = {0, 0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(total, w.total, sizeof total, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    *n = {total[0], total[1], total[2], total[3], total[4]};
    const uint64_t fetch = std::min<uint64_t>(total[3], def_room);
    if (fetch) HIPCHK(c, hipMemcpy(deferred, c->behind->lines.deferred.p, fetch * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return MGPU_OK;
}

extern "C" {

// ---- UAT input: uat2esnt over dump978 downlink lines (uat_format.h, kernels/uat.inc) ----

// a: text, out and the three per-frame arrays device pointers; a.deferred a HOST array.  The counts of this text; the deferred lines'
// indices (line_base added) to a.deferred[listed ..] as far as deferred_cap reaches.  Overflows are the caller's to judge.
static int uat_encode_dev(mgpu_ctx *c, const struct mgpu_uat_args &a, uint64_t line_base, uint64_t listed, LineCounts *n) {
    Behind &b = *c->behind;
    if (!b.d_uat_sig_table.p) {
        if (int rc = b.d_uat_sig_table.reserve_exact(c, kUatSigTable)) return rc;
        HIPCHK(c, hipMemcpy(b.d_uat_sig_table.p, uat_sig_table(), kUatSigTable, hipMemcpyHostToDevice));
    }
    const uint64_t def_room = std::min<uint64_t>(a.deferred_cap > listed ? a.deferred_cap - listed : 0, uat_max_deferred(a.nbytes));   // (no more than the text can defer)
    UatScratch w;
    if (int rc = b.lines.reserve(c, a.nbytes, &w)) return rc;
    if (int rc = b.lines.reserve_deferred(c, def_room)) return rc;
    const bool records = a.msgs || a.sig || a.line_of;
    const UatParams p = {a.text, a.nbytes, b.d_uat_sig_table.as<uint8_t>(), a.out, a.cap, a.msgs, a.sig, (unsigned long long *) a.line_of, records ? a.msgs_cap : 0,
                         b.lines.deferred.as<unsigned long long>(), def_room, line_base, a.now_ms};
    launch_uat_encode(p, w, c->stream_aux);
    return line_counts_back(c, w, def_room, a.deferred + listed, n);
}

static bool uat_args_ok(const struct mgpu_uat_args *a) {
    if (!a || a->size < sizeof(struct mgpu_uat_args) || !a->bytes || !a->consumed || !a->nlines || !a->nframes) return false;
    if (a->nbytes > kUatMaxBytes || a->cap > UINT64_MAX / 2) return false;
    if (a->nbytes && !a->text) return false;
    if ((a->cap && !a->out) || (a->deferred_cap && (!a->deferred || !a->ndeferred))) return false;
    if (a->nbytes && a->cap) {                                // out must not overlap text
        const uintptr_t i0 = (uintptr_t) a->text, i1 = i0 + a->nbytes, o0 = (uintptr_t) a->out, o1 = o0 + a->cap;
        if (i0 < o1 && o0 < i1) return false;
    }
    return true;
}

static void uat_report(const struct mgpu_uat_args *a, const LineCounts &n) {
    *a->bytes = n.units * kUatFrameText;
    *a->consumed = n.consumed;
    *a->nlines = n.lines;
    *a->nframes = n.units;
    if (a->nshort) *a->nshort = n.rejects;
    if (a->ndeferred) *a->ndeferred = n.deferred;
}

static int uat_verdict(mgpu_ctx *c, const struct mgpu_uat_args *a, const LineCounts &n) {
    if (n.units * kUatFrameText > a->cap) { c->err = "uat encode: output buffer too small"; return MGPU_E_OVERFLOW; }
    if ((a->msgs || a->sig || a->line_of) && n.units > a->msgs_cap) { c->err = "uat encode: more frames than the per-frame arrays hold"; return MGPU_E_OVERFLOW; }
    if (n.deferred > a->deferred_cap) { c->err = "uat encode: more deferred lines than the list holds"; return MGPU_E_OVERFLOW; }
    return MGPU_OK;
}

int mgpu_uat_encode_device(mgpu_ctx *c, const struct mgpu_uat_args *a) {
    if (!c || !uat_args_ok(a)) return MGPU_E_INVAL;
    LineCounts n;
    uat_report(a, n);
    if (a->nbytes == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = uat_encode_dev(c, *a, 0, 0, &n)) return rc;
    uat_report(a, n);
    return uat_verdict(c, a, n);
}

int mgpu_uat_encode(mgpu_ctx *c, const struct mgpu_uat_args *a) {
    if (!c || !uat_args_ok(a)) return MGPU_E_INVAL;
    LineCounts all;
    uat_report(a, all);
    if (a->nbytes == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    const bool records = a->msgs || a->sig || a->line_of;
    const int prc = stream_passes(a->nbytes, a->pass_bytes ? a->pass_bytes : kLineDefaultPass, true, all,
        [&](uint64_t at, uint64_t nb, bool, const LineCounts &so_far, LineCounts &n) -> int {
            // what this pass may write: what the caller's buffers still hold, and no more than nb bytes of text can give
            const uint64_t most = uat_max_frames(nb), done = so_far.units;
            const uint64_t out_room = a->cap > done * kUatFrameText ? std::min<uint64_t>(a->cap - done * kUatFrameText, most * kUatFrameText) : 0;
            const uint64_t rec_room = records && a->msgs_cap > done ? std::min<uint64_t>(a->msgs_cap - done, most) : 0;
            if (int rc = b.d_stream.reserve(c, nb + 64)) return rc;
            if (int rc = b.d_uat_out.reserve(c, out_room + 64)) return rc;
            struct mgpu_uat_args d = *a;
            d.text = b.d_stream.as<uint8_t>(); d.nbytes = nb;
            d.out = b.d_uat_out.as<uint8_t>(); d.cap = out_room;
            d.msgs = nullptr; d.sig = nullptr; d.line_of = nullptr; d.msgs_cap = rec_room;
            if (a->msgs) { if (int rc = b.d_in_msgs.reserve(c, (rec_room + 1) * sizeof(mgpu_msg))) return rc; d.msgs = b.d_in_msgs.as<mgpu_msg>(); }
            if (a->sig) { if (int rc = b.d_uat_sig.reserve(c, rec_room + 64)) return rc; d.sig = b.d_uat_sig.as<uint8_t>(); }
            if (a->line_of) { if (int rc = b.d_index_of.reserve(c, (rec_room + 1) * sizeof(uint64_t))) return rc; d.line_of = b.d_index_of.as<uint64_t>(); }
            HIPCHK(c, hipMemcpyAsync(b.d_stream.p, a->text + at, nb, hipMemcpyHostToDevice, c->stream_aux));
            if (int rc = uat_encode_dev(c, d, so_far.lines, std::min<uint64_t>(so_far.deferred, a->deferred_cap), &n)) return rc;
            // (the pass stored the bytes and records below its rooms only: the copies stay inside the caller's buffers; a pass that is
            // repeated consumed no line, so it has nothing to copy)
            const uint64_t nout = std::min<uint64_t>(n.units * kUatFrameText, out_room), nrec = std::min<uint64_t>(n.units, rec_room);
            if (nout) HIPCHK(c, hipMemcpy(a->out + done * kUatFrameText, d.out, nout, hipMemcpyDeviceToHost));
            if (nrec && a->msgs) HIPCHK(c, hipMemcpy(a->msgs + done, d.msgs, nrec * sizeof(mgpu_msg), hipMemcpyDeviceToHost));
            if (nrec && a->sig) HIPCHK(c, hipMemcpy(a->sig + done, d.sig, nrec, hipMemcpyDeviceToHost));
            if (nrec && a->line_of) HIPCHK(c, hipMemcpy(a->line_of + done, d.line_of, nrec * sizeof(uint64_t), hipMemcpyDeviceToHost));
            return MGPU_OK;
        },
        [] {});
    if (prc != MGPU_OK) return prc;
    uat_report(a, all);
    return uat_verdict(c, a, all);
}

// ---- SBS input: decodeSbsLine over BaseStation lines (sbs_in_format.h, kernels/sbs_in.inc) ----

// a: text, recs and line_of device pointers; a.deferred a HOST array.  The counts of this text; the deferred lines' indices (line_base
// added) to a.deferred[listed ..] as far as deferred_cap reaches.  Overflows are the caller's to judge.
static int sbs_decode_dev(mgpu_ctx *c, const struct mgpu_sbs_in_args &a, uint64_t line_base, uint64_t listed, LineCounts *n) {
    Behind &b = *c->behind;
    const uint64_t def_room = std::min<uint64_t>(a.deferred_cap > listed ? a.deferred_cap - listed : 0, sbs_in_max_recs(a.nbytes));   // (no more than the text can defer)
    UatScratch w;
    if (int rc = b.lines.reserve(c, a.nbytes, &w)) return rc;
    if (int rc = b.lines.reserve_deferred(c, def_room)) return rc;
    const SbsInParams p = {a.text, a.nbytes, a.recs, (unsigned long long *) a.line_of, a.recs ? a.recs_cap : 0, b.lines.deferred.as<unsigned long long>(), def_room,
                           line_base, a.now_ms, a.source};
    launch_sbs_decode(p, w, c->stream_aux);
    return line_counts_back(c, w, def_room, a.deferred + listed, n);
}

static bool sbs_in_args_ok(const struct mgpu_sbs_in_args *a) {
    if (!a || a->size < sizeof(struct mgpu_sbs_in_args) || !a->consumed || !a->nlines || !a->nrecs) return false;
    if (!sbs_in_source_ok(a->source) || a->nbytes > kUatMaxBytes || a->recs_cap > UINT64_MAX / sizeof(mgpu_sbs_rec)) return false;
    if (a->nbytes && !a->text) return false;
    if ((a->recs_cap && !a->recs) || (a->deferred_cap && (!a->deferred || !a->ndeferred))) return false;
    return true;
}

static void sbs_in_report(const struct mgpu_sbs_in_args *a, const LineCounts &n) {
    *a->consumed = n.consumed;
    *a->nlines = n.lines;
    *a->nrecs = n.units;
    if (a->ninvalid) *a->ninvalid = n.rejects;
    if (a->ndeferred) *a->ndeferred = n.deferred;
}

static int sbs_in_verdict(mgpu_ctx *c, const struct mgpu_sbs_in_args *a, const LineCounts &n) {
    if (n.units > a->recs_cap) { c->err = "sbs decode: more records than the array holds"; return MGPU_E_OVERFLOW; }
    if (n.deferred > a->deferred_cap) { c->err = "sbs decode: more deferred lines than the list holds"; return MGPU_E_OVERFLOW; }
    return MGPU_OK;
}

int mgpu_sbs_decode_device(mgpu_ctx *c, const struct mgpu_sbs_in_args *a) {
    if (!c || !sbs_in_args_ok(a)) return MGPU_E_INVAL;
    if (((uintptr_t) a->recs | (uintptr_t) a->line_of) & 7u) return MGPU_E_INVAL;
    LineCounts n;
    sbs_in_report(a, n);
    if (a->nbytes == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = sbs_decode_dev(c, *a, 0, 0, &n)) return rc;
    sbs_in_report(a, n);
    return sbs_in_verdict(c, a, n);
}

int mgpu_sbs_decode(mgpu_ctx *c, const struct mgpu_sbs_in_args *a) {
    if (!c || !sbs_in_args_ok(a)) return MGPU_E_INVAL;
    LineCounts all;
    sbs_in_report(a, all);
    if (a->nbytes == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    const int prc = stream_passes(a->nbytes, a->pass_bytes ? a->pass_bytes : kLineDefaultPass, true, all,
        [&](uint64_t at, uint64_t nb, bool, const LineCounts &so_far, LineCounts &n) -> int {
            // what this pass may write: what the caller's arrays still hold, and no more than nb bytes of text can give
            const uint64_t rec_room = a->recs_cap > so_far.units ? std::min<uint64_t>(a->recs_cap - so_far.units, sbs_in_max_recs(nb)) : 0;
            if (int rc = b.d_stream.reserve(c, nb + 64)) return rc;
            if (int rc = b.d_sbs_in_recs.reserve(c, (rec_room + 1) * sizeof(mgpu_sbs_rec))) return rc;
            struct mgpu_sbs_in_args d = *a;
            d.text = b.d_stream.as<uint8_t>(); d.nbytes = nb;
            d.recs = b.d_sbs_in_recs.as<mgpu_sbs_rec>(); d.recs_cap = rec_room;
            d.line_of = nullptr;
            if (a->line_of) { if (int rc = b.d_index_of.reserve(c, (rec_room + 1) * sizeof(uint64_t))) return rc; d.line_of = b.d_index_of.as<uint64_t>(); }
            HIPCHK(c, hipMemcpyAsync(b.d_stream.p, a->text + at, nb, hipMemcpyHostToDevice, c->stream_aux));
            if (int rc = sbs_decode_dev(c, d, so_far.lines, std::min<uint64_t>(so_far.deferred, a->deferred_cap), &n)) return rc;
            // (the pass stored the records below its room only: the copies stay inside the caller's arrays)
            const uint64_t nrec = std::min<uint64_t>(n.units, rec_room);
            if (nrec) HIPCHK(c, hipMemcpy(a->recs + so_far.units, d.recs, nrec * sizeof(mgpu_sbs_rec), hipMemcpyDeviceToHost));
            if (nrec && a->line_of) HIPCHK(c, hipMemcpy(a->line_of + so_far.units, d.line_of, nrec * sizeof(uint64_t), hipMemcpyDeviceToHost));
            return MGPU_OK;
        },
        [] {});
    if (prc != MGPU_OK) return prc;
    sbs_in_report(a, all);
    return sbs_in_verdict(c, a, all);
}

// ---- The message inputs: raw (AVR lines; raw_in_format.h, kernels/raw_in.inc), beast (a binary stream; beast_in_format.h,
// kernels/beast_in.inc) and Planefinder (a DLE-framed stream; pf_in_format.h, kernels/pf_in.inc).  Each frames its stream with a front
// of its own and ends in the same candidate arrays and filter passes, so a call is written once (msg_in_passes, msg_in_staged,
// msg_in_call) over a MsgInStretch (raw_in_host.h), and a format states only what is its own (RawIn, BeastIn, PfIn). ----

// The filter passes' side of a call (launch_raw_in_resolve): the candidate arrays and the tables reserved, the filter's generations
// scattered into their bitmaps, p's candidate, table and filter fields set.
struct FilterGens {
    uint32_t *d_members, *gen_active, *gen_inactive;
    uint32_t na, ni;
};
static int filter_passes_begin(mgpu_ctx *c, uint64_t cand_cap, RawInParams &p, FilterGens &r) {
    Behind &b = *c->behind;
    const uint64_t ncb = cand_cap / kBlock + 1;
    if (int rc = b.filter.cand_rec.reserve(c, cand_cap * sizeof(mgpu_msg))) return rc;
    if (int rc = b.filter.cand_sig.reserve(c, cand_cap * sizeof(double))) return rc;
    if (int rc = b.filter.cand_line.reserve(c, cand_cap * sizeof(uint32_t))) return rc;
    if (int rc = b.filter.cand_meta.reserve(c, cand_cap * sizeof(uint32_t))) return rc;
    if (int rc = b.filter.new_adds.reserve(c, cand_cap * sizeof(uint32_t))) return rc;
    if (int rc = b.filter.cb.reserve(c, 8 * ncb * sizeof(uint32_t))) return rc;
    if (int rc = b.filter.co.reserve(c, 2 * ncb * sizeof(unsigned long long))) return rc;
    if (int rc = b.filter.misc.reserve_exact(c, 16 * sizeof(unsigned long long))) return rc;
    if (!b.filter.first.p) {                                  // the tables, once: first[] all ones, the bitmaps zero, the CRC's bytes
        if (int rc = b.filter.first.reserve_exact(c, (uint64_t) sizeof(uint32_t) << 24)) return rc;
        HIPCHK(c, hipMemsetAsync(b.filter.first.p, 0xff, (size_t) sizeof(uint32_t) << 24, c->stream_aux));
    }
    if (!b.filter.gen.p) {
        if (int rc = b.filter.gen.reserve_exact(c, 2 * ((1u << 24) / 8))) return rc;
        HIPCHK(c, hipMemsetAsync(b.filter.gen.p, 0, 2 * ((1u << 24) / 8), c->stream_aux));
    }
    if (!b.filter.crc.p) {
        if (int rc = b.filter.crc.reserve_exact(c, 256 * sizeof(uint32_t))) return rc;
        HIPCHK(c, hipMemcpy(b.filter.crc.p, crc_tables().byte_table, 256 * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    // the filter's generations into their bitmaps
    IcaoFilter &flt = c->resolver.filter();
    const std::vector<uint32_t> &ma = flt.members(true), &mi = flt.members(false);
    r.na = (uint32_t) ma.size(); r.ni = (uint32_t) mi.size();
    if (int rc = b.filter.members.reserve(c, ((uint64_t) r.na + r.ni + 1) * sizeof(uint32_t))) return rc;
    r.d_members = b.filter.members.as<uint32_t>(); r.gen_active = b.filter.gen.as<uint32_t>(); r.gen_inactive = r.gen_active + (1u << 24) / 32;
    if (r.na) HIPCHK(c, hipMemcpyAsync(r.d_members, ma.data(), r.na * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream_aux));
    if (r.ni) HIPCHK(c, hipMemcpyAsync(r.d_members + r.na, mi.data(), r.ni * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream_aux));
    launch_raw_in_scatter(r.d_members, r.na, r.gen_active, 1, c->stream_aux);
    launch_raw_in_scatter(r.d_members + r.na, r.ni, r.gen_inactive, 1, c->stream_aux);
    // occupied > buckets / 3 makes the table grow (icao_filter.c:127); between calls occupied <= buckets / 3
    const uint64_t buckets = 1ull << flt.table_bits(), third = buckets / 3;
    const uint64_t kstar = flt.table_bits() >= 20 ? 0 : (flt.occupied() <= third ? third - flt.occupied() + 1 : 1);
    p.cfg = RawInConfig{c->cfg.nfix_crc, c->cfg.fixDF, (int32_t) c->cfg.mode_ac};
    p.tb = RawInTables{b.filter.crc.as<uint32_t>(), c->d_tab_long, c->d_tab_short, (uint32_t) c->n_long, (uint32_t) c->n_short};
    p.cand_rec = b.filter.cand_rec.as<mgpu_msg>(); p.cand_sig = b.filter.cand_sig.as<double>();
    p.cand_line = b.filter.cand_line.as<uint32_t>(); p.cand_meta = b.filter.cand_meta.as<uint32_t>(); p.cand_cap = cand_cap;
    p.gen_active = r.gen_active; p.gen_inactive = r.gen_inactive; p.first = b.filter.first.as<uint32_t>();
    p.new_adds = b.filter.new_adds.as<uint32_t>(); p.kstar = kstar;
    return MGPU_OK;
}

// The passes over ncand candidates, the bitmaps put back, the stream drained; misc[16] as launch_raw_in_resolve leaves it (zeros for no
// candidates); the new adds appended to *adds and moved into the context's filter.  ncls: bytes of p.line_class to zero first.
static int filter_passes_end(mgpu_ctx *c, const RawInParams &p, const FilterGens &r, uint64_t ncand, size_t ncls, unsigned long long *misc, std::vector<uint32_t> *adds) {
    Behind &b = *c->behind;
    memset(misc, 0, 16 * sizeof(unsigned long long));
    if (ncand) {
        unsigned long long *d_misc = b.filter.misc.as<unsigned long long>();
        HIPCHK(c, hipMemsetAsync(d_misc, 0, 16 * sizeof(unsigned long long), c->stream_aux));
        HIPCHK(c, hipMemsetAsync(d_misc + 8, 0xff, sizeof(unsigned long long), c->stream_aux));
        if (ncls) HIPCHK(c, hipMemsetAsync(p.line_class, 0, ncls, c->stream_aux));
        launch_raw_in_resolve(p, (uint32_t) ncand, b.filter.cb.as<uint32_t>(), b.filter.co.as<unsigned long long>(), d_misc, c->stream_aux);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(misc, d_misc, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream_aux));
    } else if (ncls) HIPCHK(c, hipMemsetAsync(p.line_class, 0, ncls, c->stream_aux));
    launch_raw_in_scatter(r.d_members, r.na, r.gen_active, 0, c->stream_aux);
    launch_raw_in_scatter(r.d_members + r.na, r.ni, r.gen_inactive, 0, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    if (misc[9]) {                                              // the new adds, in the reference's order, into the context's filter
        IcaoFilter &flt = c->resolver.filter();
        const size_t at = adds->size();
        adds->resize(at + misc[9]);
        HIPCHK(c, hipMemcpy(adds->data() + at, p.new_adds, misc[9] * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t k = at; k < adds->size(); ++k) flt.add((*adds)[k]);
    }
    return MGPU_OK;
}

// The generation bitmaps are zero and first[] is all ones OUTSIDE a call: a call that ends early (rc: a HIP error between the scatter-in
// and the passes that put them back) gives the tables up, and the next call allocates and initialises them again.
static int filter_tables_after(mgpu_ctx *c, int rc) {
    if (rc != MGPU_OK) {
        (void) hipStreamSynchronize(c->stream_aux);
        c->behind->filter.first.release();
        c->behind->filter.gen.release();
    }
    return rc;
}

// the pre-screen learns the addresses a call added to the filter, as mgpu_filter_add teaches it one (nothing is in flight behind the
// drain)
static int filter_publish_adds(mgpu_ctx *c, const std::vector<uint32_t> &adds) {
    if (adds.empty()) return MGPU_OK;
    Behind &b = *c->behind;
    if (int rc = b.filter.members.reserve(c, adds.size() * sizeof(uint32_t))) return rc;
    HIPCHK(c, hipMemcpyAsync(b.filter.members.p, adds.data(), adds.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream_aux));
    launch_raw_in_scatter(b.filter.members.as<uint32_t>(), (uint32_t) adds.size(), c->d_adder_bitmap, 1, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    return MGPU_OK;
}

}  // extern "C"

namespace {

// What a format states of its own:
//   Args, stretch(), report(): its public struct, onto a MsgInStretch and back from the counts (raw_in_host.h and its like);
//   args_ok(), aligned(): its MGPU_E_INVAL conditions, the latter the `_device` entry's;
//   max_cands(nb), max_units(nb): what nb bytes can give at the most; look(a, at, nb): what a pass stages behind its nb bytes;
//   Scratch, reserve(), front(): the scratch of its front and the launch (s: the stretch; p: the filter passes' side filled);
//   ntotal, cand_total: how many totals the front leaves, and which of them counts the candidates; total[0] counts the units;
//   counts(): what the totals say beyond the units, the messages and the seven counters all three share;
//   zero_class: only candidates store a class, so the array is zeroed first; tail_pass: stream_passes.h;
//   has_ids, has_off: it has receiver ids, unit offsets (the staging buffers a pass reserves);
//   overflow[]: its texts for more candidates than max_cands (cannot happen), more messages, more units than the arrays hold.
struct RawIn {
    using Args = struct mgpu_raw_in_args;
    using Scratch = UatScratch;
    static constexpr bool zero_class = true, tail_pass = true, has_ids = false, has_off = false;
    static constexpr int ntotal = 3, cand_total = 2;
    static constexpr const char *overflow[3] = {"raw decode: more candidates than the text can hold", "raw decode: more messages than the array holds",
                                                "raw decode: more lines than line_class holds"};
    static MsgInStretch stretch(const Args &a) { return raw_in_stretch(a); }
    static void report(const Args &a, const MsgInCounts &n) { raw_in_report(a, n); }
    static bool args_ok(const Args *a) {
        if (!a || a->size < sizeof(Args) || !a->consumed || !a->nlines || !a->nmsgs || !a->counters) return false;
        if (a->nbytes >= (1ull << 32) || a->msgs_cap > UINT64_MAX / sizeof(mgpu_msg)) return false;
        if (a->now_ms < 0 || a->now_ms >= 253402300800000ll) return false;
        if (a->nbytes && !a->text) return false;
        return !((a->msgs_cap && !a->msgs) || (a->line_class_cap && !a->line_class));
    }
    static bool aligned(const Args &a) { return !(((uintptr_t) a.msgs | (uintptr_t) a.line_of | (uintptr_t) a.signal_level) & 7u); }
    static uint64_t max_cands(uint64_t nb) { return raw_in_max_cands(nb); }
    static uint64_t max_units(uint64_t nb) { return nb; }
    static uint64_t look(const MsgInStretch &, uint64_t, uint64_t) { return 0; }
    static int reserve(mgpu_ctx *c, uint64_t nb, Scratch *w) { return c->behind->lines.reserve(c, nb, w); }
    static void front(mgpu_ctx *c, const MsgInStretch &, RawInParams &p, const Scratch &w) { launch_raw_in_front(p, w, c->stream_aux); }
    static void counts(const MsgInStretch &, const unsigned long long *total, MsgInCounts *n) { n->consumed = total[1]; }
};

struct BeastIn {
    using Args = struct mgpu_beast_in_args;
    using Scratch = BeastInScratch;
    // (every handler call's class is stored, by k_beast_in_classify or by the filter passes: nothing to zero)
    static constexpr bool zero_class = false, tail_pass = false, has_ids = true, has_off = true;
    static constexpr int ntotal = 9, cand_total = 1;
    static constexpr const char *overflow[3] = {"beast decode: more candidates than the stream can hold", "beast decode: more messages than the arrays hold",
                                                "beast decode: more handler calls than the frame arrays hold"};
    static MsgInStretch stretch(const Args &a) { return beast_in_stretch(a); }
    static void report(const Args &a, const MsgInCounts &n) { beast_in_report(a, n); }
    static bool args_ok(const Args *a) {
        if (!a || a->size < sizeof(Args) || !a->consumed || !a->nframes || !a->nmsgs || !a->stop || !a->stop_off || !a->receiver_id_out || !a->counters) return false;
        if (a->nbytes >= (1ull << 32) || a->msgs_cap > UINT64_MAX / sizeof(mgpu_msg) || a->frames_cap > UINT64_MAX / sizeof(uint64_t)) return false;
        if (a->now_ms < 0 || a->now_ms >= 253402300800000ll) return false;
        if (a->nbytes && !a->data) return false;
        return !((a->msgs_cap && (!a->msgs || !a->receiver_id)) || (a->frames_cap && !a->frame_class && !a->frame_off));
    }
    static bool aligned(const Args &a) {
        return !(((uintptr_t) a.msgs | (uintptr_t) a.receiver_id | (uintptr_t) a.frame_of | (uintptr_t) a.signal_level | (uintptr_t) a.frame_off) & 7u);
    }
    static uint64_t max_cands(uint64_t nb) { return beast_in_max_msgs(nb); }
    static uint64_t max_units(uint64_t nb) { return beast_in_max_frames(nb); }
    static uint64_t look(const MsgInStretch &, uint64_t, uint64_t) { return 0; }
    static int reserve(mgpu_ctx *c, uint64_t nb, Scratch *w) { return c->behind->beast_in.reserve(c, nb, w); }
    static void front(mgpu_ctx *c, const MsgInStretch &s, RawInParams &p, const Scratch &w) {
        p.cand_id = c->behind->beast_in.cand_id.as<unsigned long long>(); p.receiver_id = (unsigned long long *) s.ids;
        BeastInParams q;
        q.data = s.data; q.nbytes = s.nbytes; q.net_ingest = s.net_ingest ? 1u : 0u; q.cfg = p.cfg; q.receiver_id_in = s.receiver_id_in;
        q.cand_id = c->behind->beast_in.cand_id.as<unsigned long long>();
        q.frame_class = s.unit_class; q.frame_off = (unsigned long long *) s.unit_off; q.frames_cap = (s.unit_class || s.unit_off) ? s.units_cap : 0; q.off_base = s.off_base;
        launch_beast_in_front(q, p, w, c->stream_aux);
    }
    static void counts(const MsgInStretch &s, const unsigned long long *total, MsgInCounts *n) {
        n->id = total[8];
        uint64_t garbage = total[2];
        if (total[6] != ~0ull) {
            const uint64_t at = total[6] >> 8, delta = (total[6] >> 3) & 31u;
            n->stop = (total[6] & 7u) == BEAST_IN_STOP_SYNTH ? MGPU_BEAST_STOP_SYNTH : MGPU_BEAST_STOP_UUID;
            n->consumed = at + delta;
        } else {
            n->consumed = total[7];
            if (s.final && s.nbytes - n->consumed > kBeastInTail) {   // net_io.c:5010-5015
                garbage += s.nbytes - n->consumed;
                n->consumed = s.nbytes;
            }
        }
        n->stop_off = n->consumed;
        n->cn[1] += total[5];                                     // remote_received_modeac: the records, and the frames dropped with mode_ac off
        n->cn[7] = garbage; n->cn[8] = total[4]; n->cn[9] = total[3];
    }
};

struct PfIn {
    using Args = struct mgpu_pf_in_args;
    using Scratch = PfInScratch;
    // (every handler call's class is stored, by k_pf_in_classify or by the filter passes: nothing to zero)
    static constexpr bool zero_class = false, tail_pass = false, has_ids = false, has_off = true;
    static constexpr int ntotal = 6, cand_total = 1;
    static constexpr const char *overflow[3] = {"pf decode: more candidates than the stream can hold", "pf decode: more messages than the arrays hold",
                                                "pf decode: more handler calls than the frame arrays hold"};
    static MsgInStretch stretch(const Args &a) { return pf_in_stretch(a); }
    static void report(const Args &a, const MsgInCounts &n) { pf_in_report(a, n); }
    static bool args_ok(const Args *a) {
        if (!a || a->size < sizeof(Args) || !a->consumed || !a->nframes || !a->nmsgs || !a->counters) return false;
        if (a->nbytes + a->look >= (1ull << 32) || a->msgs_cap > UINT64_MAX / sizeof(mgpu_msg) || a->frames_cap > UINT64_MAX / sizeof(uint64_t)) return false;
        if (a->now_ms < 0 || a->now_ms >= 253402300800000ll) return false;
        if (a->nbytes && !a->data) return false;
        return !((a->msgs_cap && !a->msgs) || (a->frames_cap && !a->frame_class && !a->frame_off));
    }
    static bool aligned(const Args &a) { return !(((uintptr_t) a.msgs | (uintptr_t) a.frame_of | (uintptr_t) a.signal_level | (uintptr_t) a.frame_off) & 7u); }
    static uint64_t max_cands(uint64_t nb) { return pf_in_max_frames(nb); }
    static uint64_t max_units(uint64_t nb) { return pf_in_max_frames(nb); }
    // a pass frames nb bytes; the lookahead and the handler's reads may take kPfInReach more, which decide every frame that starts inside it
    static uint64_t look(const MsgInStretch &a, uint64_t at, uint64_t nb) { return pf_in_look(a.nbytes + a.look, at, nb); }
    static int reserve(mgpu_ctx *c, uint64_t nb, Scratch *w) { return c->behind->beast_in.reserve_pf(c, nb, w); }
    static void front(mgpu_ctx *c, const MsgInStretch &s, RawInParams &p, const Scratch &w) {
        PfInParams q;
        q.data = s.data; q.nbytes = s.nbytes; q.look = s.look; q.cfg = p.cfg;
        q.frame_class = s.unit_class; q.frame_off = (unsigned long long *) s.unit_off; q.frames_cap = (s.unit_class || s.unit_off) ? s.units_cap : 0; q.off_base = s.off_base;
        launch_pf_in_front(q, p, w, c->stream_aux);
    }
    static void counts(const MsgInStretch &, const unsigned long long *total, MsgInCounts *n) {
        n->consumed = total[4];
        n->cn[7] = total[2]; n->cn[8] = total[3];
    }
};

// The passes over one stretch on the device.  s: data and the arrays device pointers, the capacities what this stretch may store (the
// per-unit arrays indexed by this stretch's own units).  The counts of this stretch; the context's filter moved on by the stretch's
// new adds, which are appended to *adds (the caller publishes them to the pre-screen's bitmap, or puts the filter back).
template <class F>
static int msg_in_passes(mgpu_ctx *c, const MsgInStretch &s, MsgInCounts *n, std::vector<uint32_t> *adds) {
    const uint64_t cand_cap = F::max_cands(s.nbytes);
    typename F::Scratch w;
    if (int rc = F::reserve(c, s.nbytes, &w)) return rc;
    RawInParams p;
    FilterGens r;
    if (int rc = filter_passes_begin(c, cand_cap, p, r)) return rc;
    p.text = s.data; p.nbytes = s.nbytes; p.now_ms = s.now_ms;
    p.msgs = s.msgs; p.line_of = (unsigned long long *) s.index_of; p.signal_level = s.signal; p.msgs_cap = s.msgs ? s.msgs_cap : 0;
    p.line_class = s.unit_class; p.line_class_cap = s.unit_class ? s.units_cap : 0; p.line_base = s.unit_base;
    F::front(c, s, p, w);
    HIPCHK(c, hipGetLastError());
    unsigned long long total[F::ntotal] = {};
    HIPCHK(c, hipMemcpyAsync(total, w.total, sizeof total, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    unsigned long long misc[16];
    int rc = MGPU_OK;
    const size_t ncls = F::zero_class && p.line_class ? (size_t) std::min<uint64_t>(total[0], p.line_class_cap) : 0;   // "not a frame" is 0
    if (total[F::cand_total] > cand_cap) { c->err = F::overflow[0]; rc = MGPU_E_OVERFLOW; }
    if (int rc2 = filter_passes_end(c, p, r, rc ? 0 : total[F::cand_total], rc ? 0 : ncls, misc, adds)) return rc2;
    if (rc) return rc;
    n->units = total[0]; n->msgs = misc[10];
    n->cn[0] = misc[2] + misc[3] + misc[4] + misc[5] + misc[6];   // remote_received_modes: every Mode S unit that reached the decode
    for (int k = 1; k < 7; ++k) n->cn[k] = misc[k];
    F::counts(s, total, n);
    return MGPU_OK;
}

// The host form: a's arrays in host memory, the stream staged in passes (stream_passes.h) whose results go through the staging
// buffers; the filter, the receiver id and the remainder carried from pass to pass.  The counts of the stream in *all.
template <class F>
static int msg_in_staged(mgpu_ctx *c, const MsgInStretch &a, uint64_t pass_bytes, MsgInCounts *all, std::vector<uint32_t> *adds) {
    Behind &b = *c->behind;
    IcaoFilter &flt = c->resolver.filter();
    IcaoFilter::Snapshot pass_before;
    size_t adds_before = 0;
    const bool want_units = a.unit_class || a.unit_off;
    return stream_passes(a.nbytes, pass_bytes ? pass_bytes : kLineDefaultPass, F::tail_pass, *all,
        [&](uint64_t at, uint64_t nb, bool final, const MsgInCounts &so_far, MsgInCounts &n) -> int {
            // what this pass may write: what the caller's arrays still hold, and no more than nb bytes can give
            const uint64_t look = F::look(a, at, nb);
            const uint64_t msg_room = a.msgs_cap > so_far.msgs ? std::min<uint64_t>(a.msgs_cap - so_far.msgs, F::max_cands(nb)) : 0;
            const uint64_t unit_room = want_units && a.units_cap > so_far.units ? std::min<uint64_t>(a.units_cap - so_far.units, F::max_units(nb)) : 0;
            int rc;
            if ((rc = b.d_stream.reserve(c, nb + look + 64)) || (rc = b.d_in_msgs.reserve(c, (msg_room + 1) * sizeof(mgpu_msg))) ||
                (F::has_ids && (rc = b.d_bin_ids.reserve(c, (msg_room + 1) * sizeof(uint64_t)))) || (rc = b.d_index_of.reserve(c, (msg_room + 1) * sizeof(uint64_t))) ||
                (rc = b.d_in_signal.reserve(c, (msg_room + 1) * sizeof(double))) || (rc = b.d_in_class.reserve(c, unit_room + 1)) ||
                (F::has_off && (rc = b.d_bin_frame_off.reserve(c, (unit_room + 1) * sizeof(uint64_t))))) return rc;
            MsgInStretch d = a;
            d.data = b.d_stream.as<uint8_t>(); d.nbytes = nb; d.look = look; d.final = final; d.receiver_id_in = so_far.id;
            d.msgs = b.d_in_msgs.as<mgpu_msg>(); d.ids = F::has_ids ? b.d_bin_ids.as<uint64_t>() : nullptr; d.msgs_cap = msg_room;
            d.index_of = a.index_of ? b.d_index_of.as<uint64_t>() : nullptr;
            d.signal = a.signal ? b.d_in_signal.as<double>() : nullptr;
            d.unit_class = a.unit_class ? b.d_in_class.as<uint8_t>() : nullptr;
            d.unit_off = a.unit_off ? b.d_bin_frame_off.as<uint64_t>() : nullptr;
            d.units_cap = unit_room; d.unit_base = so_far.units; d.off_base = at;
            HIPCHK(c, hipMemcpyAsync(b.d_stream.p, a.data + at, nb + look, hipMemcpyHostToDevice, c->stream_aux));
            adds_before = adds->size();
            flt.snapshot(pass_before);
            if ((rc = filter_tables_after(c, msg_in_passes<F>(c, d, &n, adds)))) return rc;
            // (the pass stored below its rooms only: the copies stay inside the caller's arrays)
            const uint64_t nmsg = std::min<uint64_t>(n.msgs, msg_room), nunit = std::min<uint64_t>(n.units, unit_room);
            if (nmsg) HIPCHK(c, hipMemcpy(a.msgs + so_far.msgs, d.msgs, nmsg * sizeof(mgpu_msg), hipMemcpyDeviceToHost));
            if (nmsg && a.ids) HIPCHK(c, hipMemcpy(a.ids + so_far.msgs, d.ids, nmsg * sizeof(uint64_t), hipMemcpyDeviceToHost));
            if (nmsg && a.index_of) HIPCHK(c, hipMemcpy(a.index_of + so_far.msgs, d.index_of, nmsg * sizeof(uint64_t), hipMemcpyDeviceToHost));
            if (nmsg && a.signal) HIPCHK(c, hipMemcpy(a.signal + so_far.msgs, d.signal, nmsg * sizeof(double), hipMemcpyDeviceToHost));
            if (nunit && a.unit_class) HIPCHK(c, hipMemcpy(a.unit_class + so_far.units, d.unit_class, nunit, hipMemcpyDeviceToHost));
            if (nunit && a.unit_off) HIPCHK(c, hipMemcpy(a.unit_off + so_far.units, d.unit_off, nunit * sizeof(uint64_t), hipMemcpyDeviceToHost));
            return MGPU_OK;
        },
        [&] { flt.restore(pass_before); adds->resize(adds_before); });   // a larger pass, from the same filter
}

// A call of either form (staged: the host form).  An empty stream is answered before anything is drained.  Around the passes the
// filter's one snapshot: an error or an overflow puts the filter back where it stood and teaches the pre-screen nothing; otherwise
// the pre-screen learns the new addresses.
template <class F>
static int msg_in_call(mgpu_ctx *c, const typename F::Args *a, bool staged) {
    if (!c || !F::args_ok(a) || (!staged && !F::aligned(*a))) return MGPU_E_INVAL;
    const MsgInStretch s = F::stretch(*a);
    MsgInCounts n;
    n.id = s.receiver_id_in;
    F::report(*a, n);
    if (s.nbytes == 0) return MGPU_OK;
    { const int rc = drain(c); if (rc != MGPU_OK) return rc; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    IcaoFilter &flt = c->resolver.filter();
    IcaoFilter::Snapshot before;
    flt.snapshot(before);
    std::vector<uint32_t> adds;
    if (int rc = staged ? msg_in_staged<F>(c, s, a->pass_bytes, &n, &adds) : filter_tables_after(c, msg_in_passes<F>(c, s, &n, &adds))) { flt.restore(before); return rc; }
    F::report(*a, n);
    const int over = msg_in_overflow(s, n);
    if (!over) return filter_publish_adds(c, adds);
    flt.restore(before);
    c->err = F::overflow[over];
    return MGPU_E_OVERFLOW;
}

}  // namespace

extern "C" {

int mgpu_raw_decode_device(mgpu_ctx *c, const struct mgpu_raw_in_args *a) { return msg_in_call<RawIn>(c, a, false); }
int mgpu_raw_decode(mgpu_ctx *c, const struct mgpu_raw_in_args *a) { return msg_in_call<RawIn>(c, a, true); }
int mgpu_beast_decode_device(mgpu_ctx *c, const struct mgpu_beast_in_args *a) { return msg_in_call<BeastIn>(c, a, false); }
int mgpu_beast_decode(mgpu_ctx *c, const struct mgpu_beast_in_args *a) { return msg_in_call<BeastIn>(c, a, true); }
int mgpu_pf_decode_device(mgpu_ctx *c, const struct mgpu_pf_in_args *a) { return msg_in_call<PfIn>(c, a, false); }
int mgpu_pf_decode(mgpu_ctx *c, const struct mgpu_pf_in_args *a) { return msg_in_call<PfIn>(c, a, true); }

// ---- ASTERIX input: readAsterix + decodeAsterixMessage over a length-chained stream (asterix_in_format.h, kernels/asterix_in.inc) ----

struct AstInCounts {
    uint64_t frames = 0, recs = 0, other = 0, undefined = 0, consumed = 0;
    uint32_t stop = MGPU_AST_STOP_END;
    bool stopped() const { return stop != MGPU_AST_STOP_END; }   // for stream_passes: a closing frame ends the call where it stands
    void add(const AstInCounts &n) { frames += n.frames; recs += n.recs; other += n.other; undefined += n.undefined; stop = n.stop; }
};

// a: data, recs and frame_of device pointers; `look` bytes behind a.nbytes are the stream's too.  The counts of this stretch.
// Overflows are the caller's to judge.
static int asterix_decode_dev(mgpu_ctx *c, const struct mgpu_asterix_in_args &a, uint64_t look, uint64_t frame_base, AstInCounts *n) {
    AstInScratch w;
    if (int rc = c->behind->ast_in.reserve(c, a.nbytes, &w)) return rc;
    const AstInParams p = {a.data, a.nbytes, look, a.recs, (unsigned long long *) a.frame_of, a.recs ? a.recs_cap : 0, frame_base, a.now_ms, a.source};
    launch_asterix_decode(p, w, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    unsigned long long total[6] = {0, 0, 0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(total, w.total, sizeof total, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    n->frames = total[0]; n->recs = total[1]; n->other = total[2]; n->undefined = total[3]; n->consumed = total[4]; n->stop = (uint32_t) total[5];
    return MGPU_OK;
}

static bool asterix_in_args_ok(const struct mgpu_asterix_in_args *a) {
    if (!a || a->size < sizeof(struct mgpu_asterix_in_args) || !a->consumed || !a->nframes || !a->nrecs || !a->stop) return false;
    if (!ast_in_source_ok(a->source) || !ast_in_now_ok(a->now_ms) || a->nbytes > kAstMaxBytes || a->recs_cap > UINT64_MAX / sizeof(mgpu_asterix_rec)) return false;
    if (a->nbytes && !a->data) return false;
    if (a->recs_cap && !a->recs) return false;
    return true;
}

static void asterix_in_report(const struct mgpu_asterix_in_args *a, const AstInCounts &n) {
    *a->consumed = n.consumed;
    *a->nframes = n.frames;
    *a->nrecs = n.recs;
    *a->stop = n.stop;
    if (a->nother) *a->nother = n.other;
    if (a->nundefined) *a->nundefined = n.undefined;
}

static int asterix_in_verdict(mgpu_ctx *c, const struct mgpu_asterix_in_args *a, const AstInCounts &n) {
    if (n.recs > a->recs_cap) { c->err = "asterix decode: more records than the array holds"; return MGPU_E_OVERFLOW; }
    return MGPU_OK;
}

int mgpu_asterix_decode_device(mgpu_ctx *c, const struct mgpu_asterix_in_args *a) {
    if (!c || !asterix_in_args_ok(a)) return MGPU_E_INVAL;
    if (((uintptr_t) a->recs & 15u) || ((uintptr_t) a->frame_of & 7u)) return MGPU_E_INVAL;
    AstInCounts n;
    asterix_in_report(a, n);
    if (a->nbytes == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = asterix_decode_dev(c, *a, 0, 0, &n)) return rc;
    asterix_in_report(a, n);
    return asterix_in_verdict(c, a, n);
}

int mgpu_asterix_decode(mgpu_ctx *c, const struct mgpu_asterix_in_args *a) {
    if (!c || !asterix_in_args_ok(a)) return MGPU_E_INVAL;
    AstInCounts all;
    asterix_in_report(a, all);
    if (a->nbytes == 0) return MGPU_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    const int prc = stream_passes(a->nbytes, a->pass_bytes ? a->pass_bytes : kAstInDefaultPass, false, all,
        [&](uint64_t at, uint64_t nb, bool, const AstInCounts &so_far, AstInCounts &n) -> int {
            // a pass frames nb bytes; its items may read kAstInLook more, which decide every frame that starts inside the pass; the
            // unconsumed tail is the next pass's head, and a record longer than the pass is what makes it repeat
            const uint64_t look = std::min<uint64_t>(kAstInLook, a->nbytes - at - nb);
            const uint64_t rec_room = a->recs_cap > so_far.recs ? std::min<uint64_t>(a->recs_cap - so_far.recs, ast_in_max_recs(nb)) : 0;
            if (int rc = b.d_stream.reserve(c, nb + look + 64)) return rc;
            if (int rc = b.d_ast_in_recs.reserve(c, (rec_room + 1) * sizeof(mgpu_asterix_rec))) return rc;
            struct mgpu_asterix_in_args d = *a;
            d.data = b.d_stream.as<uint8_t>(); d.nbytes = nb;
            d.recs = b.d_ast_in_recs.as<mgpu_asterix_rec>(); d.recs_cap = rec_room;
            d.frame_of = nullptr;
            if (a->frame_of) { if (int rc = b.d_index_of.reserve(c, (rec_room + 1) * sizeof(uint64_t))) return rc; d.frame_of = b.d_index_of.as<uint64_t>(); }
            HIPCHK(c, hipMemcpyAsync(b.d_stream.p, a->data + at, nb + look, hipMemcpyHostToDevice, c->stream_aux));
            if (int rc = asterix_decode_dev(c, d, look, so_far.frames, &n)) return rc;
            // (the pass stored the records below its room only: the copies stay inside the caller's arrays)
            const uint64_t nrec = std::min<uint64_t>(n.recs, rec_room);
            if (nrec) HIPCHK(c, hipMemcpy(a->recs + so_far.recs, d.recs, nrec * sizeof(mgpu_asterix_rec), hipMemcpyDeviceToHost));
            if (nrec && a->frame_of) HIPCHK(c, hipMemcpy(a->frame_of + so_far.recs, d.frame_of, nrec * sizeof(uint64_t), hipMemcpyDeviceToHost));
            return MGPU_OK;
        },
        [] {});
    if (prc != MGPU_OK) return prc;
    asterix_in_report(a, all);
    return asterix_in_verdict(c, a, all);
}

}  // extern "C"
