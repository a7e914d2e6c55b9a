// behind_in.cpp — behind the message list, the stream inputs: UAT, SBS, raw, beast, Planefinder and ASTERIX, each as a `_device` entry over a stream
// in HBM and a host form that stages the stream in passes (stream_passes.h); the filter passes the raw and the beast input share.
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

// ---- Raw input: decodeHexMessage + the front of decodeModesMessage over AVR lines (raw_in_format.h, kernels/raw_in.inc) ----

struct RawInCounts {
    uint64_t lines = 0, consumed = 0, msgs = 0;
    uint64_t cn[7] = {0, 0, 0, 0, 0, 0, 0};
    bool stopped() const { return false; }                      // (for stream_passes, as LineCounts)
    void add(const RawInCounts &n) {
        lines += n.lines; msgs += n.msgs;
        for (int k = 0; k < 7; ++k) cn[k] += n.cn[k];
    }
};

// The filter passes' side of a call (launch_raw_in_resolve), shared with the beast input: the candidate arrays and the tables reserved,
// the filter's generations scattered into their bitmaps, p's candidate, table and filter fields set.
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

// a: text, msgs, line_of, signal_level, line_class device pointers, the capacities what this text may store (line_class indexed by
// this text's own lines).  The counts of this text; the context's filter moved on by the text's new adds, which are appended to
// *adds (the caller publishes them to the pre-screen's bitmap, or puts the filter back).
static int raw_decode_passes(mgpu_ctx *c, const struct mgpu_raw_in_args &a, uint64_t line_base, RawInCounts *n, std::vector<uint32_t> *adds) {
    Behind &b = *c->behind;
    const uint64_t cand_cap = raw_in_max_cands(a.nbytes);
    UatScratch w;
    if (int rc = b.lines.reserve(c, a.nbytes, &w)) return rc;
    RawInParams p;
    FilterGens r;
    if (int rc = filter_passes_begin(c, cand_cap, p, r)) return rc;
    p.text = a.text; p.nbytes = a.nbytes; p.now_ms = a.now_ms;
    p.msgs = a.msgs; p.line_of = (unsigned long long *) a.line_of; p.signal_level = a.signal_level; p.msgs_cap = a.msgs ? a.msgs_cap : 0;
    p.line_class = a.line_class; p.line_class_cap = a.line_class ? a.line_class_cap : 0; p.line_base = line_base;
    launch_raw_in_front(p, w, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    unsigned long long total[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(total, w.total, sizeof total, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    unsigned long long misc[16];
    int rc = MGPU_OK;
    const size_t ncls = p.line_class ? (size_t) std::min<uint64_t>(total[0], p.line_class_cap) : 0;   // "not a frame" is 0: only candidates store a class
    if (total[2] > cand_cap) { c->err = "raw decode: more candidates than the text can hold"; rc = MGPU_E_OVERFLOW; }   // (cannot happen: raw_in_max_cands)
    if (int rc2 = filter_passes_end(c, p, r, rc ? 0 : total[2], rc ? 0 : ncls, misc, adds)) return rc2;
    if (rc) return rc;
    n->lines = total[0]; n->consumed = total[1]; n->msgs = misc[10];
    for (int k = 1; k < 7; ++k) n->cn[k] = misc[k];
    n->cn[0] = misc[2] + misc[3] + misc[4] + misc[5] + misc[6];   // remote_received_modes: every Mode S line that reached the decode
    return MGPU_OK;
}

static int raw_decode_dev(mgpu_ctx *c, const struct mgpu_raw_in_args &a, uint64_t line_base, RawInCounts *n, std::vector<uint32_t> *adds) {
    return filter_tables_after(c, raw_decode_passes(c, a, line_base, n, adds));
}

static bool raw_in_args_ok(const struct mgpu_raw_in_args *a) {
    if (!a || a->size < sizeof(struct mgpu_raw_in_args) || !a->consumed || !a->nlines || !a->nmsgs || !a->counters) return false;
    if (a->nbytes >= (1ull << 32) || a->msgs_cap > UINT64_MAX / sizeof(mgpu_msg)) return false;
    if (a->now_ms < 0 || a->now_ms >= 253402300800000ll) return false;
    if (a->nbytes && !a->text) return false;
    if ((a->msgs_cap && !a->msgs) || (a->line_class_cap && !a->line_class)) return false;
    return true;
}

static void raw_in_report(const struct mgpu_raw_in_args *a, const RawInCounts &n) {
    *a->consumed = n.consumed;
    *a->nlines = n.lines;
    *a->nmsgs = n.msgs;
    struct mgpu_raw_in_counters &k = *a->counters;
    k.remote_received_modes = n.cn[0]; k.remote_received_modeac = n.cn[1]; k.remote_rejected_unknown_icao = n.cn[2]; k.remote_rejected_bad = n.cn[3];
    for (int i = 0; i < 3; ++i) k.remote_accepted[i] = n.cn[4 + i];
}

// the pre-screen learns the addresses a call added to the filter, as mgpu_filter_add teaches it one (nothing is in flight behind the
// drain); the raw input's and the beast input's
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

// the end of a call (overflow: its text, or null): on overflow the filter goes back to where it stood; otherwise the pre-screen learns
// the new addresses
static int filter_call_end(mgpu_ctx *c, const char *overflow, const IcaoFilter::Snapshot &before, const std::vector<uint32_t> &adds) {
    if (!overflow) return filter_publish_adds(c, adds);
    c->resolver.filter().restore(before);
    c->err = overflow;
    return MGPU_E_OVERFLOW;
}

static int raw_in_finish(mgpu_ctx *c, const struct mgpu_raw_in_args *a, const RawInCounts &n, const IcaoFilter::Snapshot &before, const std::vector<uint32_t> &adds) {
    const char *overflow = n.msgs > a->msgs_cap ? "raw decode: more messages than the array holds" :
                           a->line_class && n.lines > a->line_class_cap ? "raw decode: more lines than line_class holds" : nullptr;
    return filter_call_end(c, overflow, before, adds);
}

int mgpu_raw_decode_device(mgpu_ctx *c, const struct mgpu_raw_in_args *a) {
    if (!c || !raw_in_args_ok(a)) return MGPU_E_INVAL;
    if (((uintptr_t) a->msgs | (uintptr_t) a->line_of | (uintptr_t) a->signal_level) & 7u) return MGPU_E_INVAL;
    RawInCounts n;
    raw_in_report(a, n);
    if (a->nbytes == 0) return MGPU_OK;
    { const int rc = drain(c); if (rc != MGPU_OK) return rc; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    IcaoFilter::Snapshot before;
    c->resolver.filter().snapshot(before);
    std::vector<uint32_t> adds;
    if (int rc = raw_decode_dev(c, *a, 0, &n, &adds)) { c->resolver.filter().restore(before); return rc; }
    raw_in_report(a, n);
    return raw_in_finish(c, a, n, before, adds);
}

int mgpu_raw_decode(mgpu_ctx *c, const struct mgpu_raw_in_args *a) {
    if (!c || !raw_in_args_ok(a)) return MGPU_E_INVAL;
    RawInCounts all;
    raw_in_report(a, all);
    if (a->nbytes == 0) return MGPU_OK;
    { const int rc = drain(c); if (rc != MGPU_OK) return rc; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    IcaoFilter::Snapshot before, pass_before;
    c->resolver.filter().snapshot(before);
    std::vector<uint32_t> adds;
    size_t adds_before = 0;
    const int prc = stream_passes(a->nbytes, a->pass_bytes ? a->pass_bytes : kLineDefaultPass, true, all,
        [&](uint64_t at, uint64_t nb, bool final, const RawInCounts &so_far, RawInCounts &n) -> int {
            // what this pass may write: what the caller's arrays still hold, and no more than nb bytes of text can give
            const uint64_t msg_room = a->msgs_cap > so_far.msgs ? std::min<uint64_t>(a->msgs_cap - so_far.msgs, raw_in_max_cands(nb)) : 0;
            const uint64_t cls_room = a->line_class_cap > so_far.lines ? std::min<uint64_t>(a->line_class_cap - so_far.lines, nb) : 0;
            int rc;
            if ((rc = b.d_stream.reserve(c, nb + 64)) || (rc = b.d_in_msgs.reserve(c, (msg_room + 1) * sizeof(mgpu_msg))) ||
                (rc = b.d_index_of.reserve(c, (msg_room + 1) * sizeof(uint64_t))) || (rc = b.d_in_signal.reserve(c, (msg_room + 1) * sizeof(double))) ||
                (rc = b.d_in_class.reserve(c, cls_room + 1))) return rc;
            struct mgpu_raw_in_args d = *a;
            d.text = b.d_stream.as<uint8_t>(); d.nbytes = nb;
            d.msgs = b.d_in_msgs.as<mgpu_msg>(); d.msgs_cap = msg_room;
            d.line_of = a->line_of ? b.d_index_of.as<uint64_t>() : nullptr;
            d.signal_level = a->signal_level ? b.d_in_signal.as<double>() : nullptr;
            d.line_class = a->line_class ? b.d_in_class.as<uint8_t>() : nullptr; d.line_class_cap = cls_room;
            HIPCHK(c, hipMemcpyAsync(b.d_stream.p, a->text + at, nb, hipMemcpyHostToDevice, c->stream_aux));
            adds_before = adds.size();
            if (!final) c->resolver.filter().snapshot(pass_before);   // (only such a pass can be repeated)
            if ((rc = raw_decode_dev(c, d, so_far.lines, &n, &adds))) return rc;
            // (the pass stored below its rooms only: the copies stay inside the caller's arrays)
            const uint64_t nmsg = std::min<uint64_t>(n.msgs, msg_room), ncls = std::min<uint64_t>(n.lines, cls_room);
            if (nmsg) HIPCHK(c, hipMemcpy(a->msgs + so_far.msgs, d.msgs, nmsg * sizeof(mgpu_msg), hipMemcpyDeviceToHost));
            if (nmsg && a->line_of) HIPCHK(c, hipMemcpy(a->line_of + so_far.msgs, d.line_of, nmsg * sizeof(uint64_t), hipMemcpyDeviceToHost));
            if (nmsg && a->signal_level) HIPCHK(c, hipMemcpy(a->signal_level + so_far.msgs, d.signal_level, nmsg * sizeof(double), hipMemcpyDeviceToHost));
            if (ncls && a->line_class) HIPCHK(c, hipMemcpy(a->line_class + so_far.lines, d.line_class, ncls, hipMemcpyDeviceToHost));
            return MGPU_OK;
        },
        [&] { c->resolver.filter().restore(pass_before); adds.resize(adds_before); });   // a larger pass, from the same filter
    if (prc != MGPU_OK) { c->resolver.filter().restore(before); return prc; }
    raw_in_report(a, all);
    return raw_in_finish(c, a, all, before, adds);
}

// ---- Beast input: readBeast + decodeBinMessage over a binary stream (beast_in_format.h, kernels/beast_in.inc) ----

// a: data and the per-message / per-call arrays device pointers, the capacities what this stretch may store (frame_class and frame_off
// indexed by this stretch's own handler calls); frame_base and off_base are added to frame_of and frame_off.  final: the tail rule
// applies.  The counts of this stretch; the filter moved on as in raw_decode_passes.
static int beast_decode_passes(mgpu_ctx *c, const struct mgpu_beast_in_args &a, uint64_t frame_base, uint64_t off_base, bool final, BeastInCounts *n,
                               std::vector<uint32_t> *adds) {
    Behind &b = *c->behind;
    const uint64_t cand_cap = beast_in_max_msgs(a.nbytes);
    BeastInScratch w;
    if (int rc = b.beast_in.reserve(c, a.nbytes, &w)) return rc;
    RawInParams p;
    FilterGens r;
    if (int rc = filter_passes_begin(c, cand_cap, p, r)) return rc;
    p.text = a.data; p.nbytes = a.nbytes; p.now_ms = a.now_ms;
    p.msgs = a.msgs; p.line_of = (unsigned long long *) a.frame_of; p.signal_level = a.signal_level; p.msgs_cap = a.msgs ? a.msgs_cap : 0;
    p.line_class = a.frame_class; p.line_class_cap = a.frame_class ? a.frames_cap : 0; p.line_base = frame_base;
    p.cand_id = b.beast_in.cand_id.as<unsigned long long>(); p.receiver_id = (unsigned long long *) a.receiver_id;
    BeastInParams q;
    q.data = a.data; q.nbytes = a.nbytes; q.net_ingest = a.net_ingest ? 1u : 0u; q.cfg = p.cfg; q.receiver_id_in = a.receiver_id_in;
    q.cand_id = b.beast_in.cand_id.as<unsigned long long>();
    q.frame_class = a.frame_class; q.frame_off = (unsigned long long *) a.frame_off; q.frames_cap = (a.frame_class || a.frame_off) ? a.frames_cap : 0; q.off_base = off_base;
    launch_beast_in_front(q, p, w, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    unsigned long long total[9];
    HIPCHK(c, hipMemcpyAsync(total, w.total, sizeof total, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    unsigned long long misc[16];
    int rc = MGPU_OK;
    if (total[1] > cand_cap) { c->err = "beast decode: more candidates than the stream can hold"; rc = MGPU_E_OVERFLOW; }   // (cannot happen: beast_in_max_msgs)
    // (every handler call's class is stored, by k_beast_in_classify or by the filter passes: nothing to zero)
    if (int rc2 = filter_passes_end(c, p, r, rc ? 0 : total[1], 0, misc, adds)) return rc2;
    if (rc) return rc;
    n->frames = total[0]; n->msgs = misc[10]; n->id = total[8];
    uint64_t garbage = total[2];
    if (total[6] != ~0ull) {
        const uint64_t at = total[6] >> 8, delta = (total[6] >> 3) & 31u;
        n->stop = (total[6] & 7u) == BEAST_IN_STOP_SYNTH ? MGPU_BEAST_STOP_SYNTH : MGPU_BEAST_STOP_UUID;
        n->consumed = at + delta;
    } else {
        n->consumed = total[7];
        if (final && a.nbytes - n->consumed > kBeastInTail) {   // net_io.c:5010-5015
            garbage += a.nbytes - n->consumed;
            n->consumed = a.nbytes;
        }
    }
    n->stop_off = n->consumed;
    n->cn[0] = misc[2] + misc[3] + misc[4] + misc[5] + misc[6];   // remote_received_modes: every Mode S frame that reached the decode
    n->cn[1] = misc[1] + total[5];                              // remote_received_modeac: the records, and the frames dropped with mode_ac off
    for (int k = 2; k < 7; ++k) n->cn[k] = misc[k];
    n->cn[7] = garbage; n->cn[8] = total[4]; n->cn[9] = total[3];
    return MGPU_OK;
}

static int beast_decode_dev(mgpu_ctx *c, const struct mgpu_beast_in_args &a, uint64_t frame_base, uint64_t off_base, bool final, BeastInCounts *n, std::vector<uint32_t> *adds) {
    return filter_tables_after(c, beast_decode_passes(c, a, frame_base, off_base, final, n, adds));
}

static bool beast_in_args_ok(const struct mgpu_beast_in_args *a) {
    if (!a || a->size < sizeof(struct mgpu_beast_in_args) || !a->consumed || !a->nframes || !a->nmsgs || !a->stop || !a->stop_off || !a->receiver_id_out || !a->counters) return false;
    if (a->nbytes >= (1ull << 32) || a->msgs_cap > UINT64_MAX / sizeof(mgpu_msg) || a->frames_cap > UINT64_MAX / sizeof(uint64_t)) return false;
    if (a->now_ms < 0 || a->now_ms >= 253402300800000ll) return false;
    if (a->nbytes && !a->data) return false;
    if ((a->msgs_cap && (!a->msgs || !a->receiver_id)) || (a->frames_cap && !a->frame_class && !a->frame_off)) return false;
    return true;
}

static void beast_in_report(const struct mgpu_beast_in_args *a, const BeastInCounts &n) {
    *a->consumed = n.consumed; *a->nframes = n.frames; *a->nmsgs = n.msgs; *a->stop = n.stop; *a->stop_off = n.stop_off; *a->receiver_id_out = n.id;
    beast_in_counters_of(n, a->counters);
}

static int beast_in_finish(mgpu_ctx *c, const struct mgpu_beast_in_args *a, const BeastInCounts &n, const IcaoFilter::Snapshot &before, const std::vector<uint32_t> &adds) {
    const char *overflow = n.msgs > a->msgs_cap ? "beast decode: more messages than the arrays hold" :
                           (a->frame_class || a->frame_off) && n.frames > a->frames_cap ? "beast decode: more handler calls than the frame arrays hold" : nullptr;
    return filter_call_end(c, overflow, before, adds);
}

int mgpu_beast_decode_device(mgpu_ctx *c, const struct mgpu_beast_in_args *a) {
    if (!c || !beast_in_args_ok(a)) return MGPU_E_INVAL;
    if (((uintptr_t) a->msgs | (uintptr_t) a->receiver_id | (uintptr_t) a->frame_of | (uintptr_t) a->signal_level | (uintptr_t) a->frame_off) & 7u) return MGPU_E_INVAL;
    BeastInCounts n;
    n.id = a->receiver_id_in;
    beast_in_report(a, n);
    if (a->nbytes == 0) return MGPU_OK;
    { const int rc = drain(c); if (rc != MGPU_OK) return rc; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    IcaoFilter::Snapshot before;
    c->resolver.filter().snapshot(before);
    std::vector<uint32_t> adds;
    if (int rc = beast_decode_dev(c, *a, 0, 0, true, &n, &adds)) { c->resolver.filter().restore(before); return rc; }
    beast_in_report(a, n);
    return beast_in_finish(c, a, n, before, adds);
}

int mgpu_beast_decode(mgpu_ctx *c, const struct mgpu_beast_in_args *a) {
    if (!c || !beast_in_args_ok(a)) return MGPU_E_INVAL;
    BeastInCounts all;
    all.id = a->receiver_id_in;
    beast_in_report(a, all);
    if (a->nbytes == 0) return MGPU_OK;
    { const int rc = drain(c); if (rc != MGPU_OK) return rc; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    IcaoFilter::Snapshot before;
    c->resolver.filter().snapshot(before);
    std::vector<uint32_t> adds;
    const bool want_frames = a->frame_class || a->frame_off;
    size_t adds_before = 0;
    IcaoFilter::Snapshot pass_before;
    const int prc = stream_passes(a->nbytes, a->pass_bytes ? a->pass_bytes : kLineDefaultPass, false, all,
        [&](uint64_t at, uint64_t nb, bool final, const BeastInCounts &so_far, BeastInCounts &n) -> int {
            // what this pass may write: what the caller's arrays still hold, and no more than nb bytes can give
            const uint64_t msg_room = a->msgs_cap > so_far.msgs ? std::min<uint64_t>(a->msgs_cap - so_far.msgs, beast_in_max_msgs(nb)) : 0;
            const uint64_t frame_room = want_frames && a->frames_cap > so_far.frames ? std::min<uint64_t>(a->frames_cap - so_far.frames, beast_in_max_frames(nb)) : 0;
            int rc;
            if ((rc = b.d_stream.reserve(c, nb + 64)) || (rc = b.d_in_msgs.reserve(c, (msg_room + 1) * sizeof(mgpu_msg))) ||
                (rc = b.d_bin_ids.reserve(c, (msg_room + 1) * sizeof(uint64_t))) || (rc = b.d_index_of.reserve(c, (msg_room + 1) * sizeof(uint64_t))) ||
                (rc = b.d_in_signal.reserve(c, (msg_room + 1) * sizeof(double))) || (rc = b.d_in_class.reserve(c, frame_room + 1)) ||
                (rc = b.d_bin_frame_off.reserve(c, (frame_room + 1) * sizeof(uint64_t)))) return rc;
            struct mgpu_beast_in_args d = *a;
            d.data = b.d_stream.as<uint8_t>(); d.nbytes = nb; d.receiver_id_in = so_far.id;
            d.msgs = b.d_in_msgs.as<mgpu_msg>(); d.receiver_id = b.d_bin_ids.as<uint64_t>(); d.msgs_cap = msg_room;
            d.frame_of = a->frame_of ? b.d_index_of.as<uint64_t>() : nullptr;
            d.signal_level = a->signal_level ? b.d_in_signal.as<double>() : nullptr;
            d.frame_class = a->frame_class ? b.d_in_class.as<uint8_t>() : nullptr;
            d.frame_off = a->frame_off ? b.d_bin_frame_off.as<uint64_t>() : nullptr;
            d.frames_cap = frame_room;
            HIPCHK(c, hipMemcpyAsync(b.d_stream.p, a->data + at, nb, hipMemcpyHostToDevice, c->stream_aux));
            adds_before = adds.size();
            c->resolver.filter().snapshot(pass_before);
            if ((rc = beast_decode_dev(c, d, so_far.frames, at, final, &n, &adds))) return rc;
            // (the pass stored below its rooms only: the copies stay inside the caller's arrays)
            const uint64_t nmsg = std::min<uint64_t>(n.msgs, msg_room), nfr = std::min<uint64_t>(n.frames, frame_room);
            if (nmsg) HIPCHK(c, hipMemcpy(a->msgs + so_far.msgs, d.msgs, nmsg * sizeof(mgpu_msg), hipMemcpyDeviceToHost));
            if (nmsg) HIPCHK(c, hipMemcpy(a->receiver_id + so_far.msgs, d.receiver_id, nmsg * sizeof(uint64_t), hipMemcpyDeviceToHost));
            if (nmsg && a->frame_of) HIPCHK(c, hipMemcpy(a->frame_of + so_far.msgs, d.frame_of, nmsg * sizeof(uint64_t), hipMemcpyDeviceToHost));
            if (nmsg && a->signal_level) HIPCHK(c, hipMemcpy(a->signal_level + so_far.msgs, d.signal_level, nmsg * sizeof(double), hipMemcpyDeviceToHost));
            if (nfr && a->frame_class) HIPCHK(c, hipMemcpy(a->frame_class + so_far.frames, d.frame_class, nfr, hipMemcpyDeviceToHost));
            if (nfr && a->frame_off) HIPCHK(c, hipMemcpy(a->frame_off + so_far.frames, d.frame_off, nfr * sizeof(uint64_t), hipMemcpyDeviceToHost));
            return MGPU_OK;
        },
        [&] { c->resolver.filter().restore(pass_before); adds.resize(adds_before); });
    if (prc != MGPU_OK) { c->resolver.filter().restore(before); return prc; }
    beast_in_report(a, all);
    return beast_in_finish(c, a, all, before, adds);
}

// ---- Planefinder input: readPlanefinder + decodePfMessage over a DLE-framed stream (pf_in_format.h, kernels/pf_in.inc) ----

// a: data and the per-message / per-call arrays device pointers, the capacities what this stretch may store (frame_class and frame_off
// indexed by this stretch's own handler calls); a.nbytes are framed, `look` bytes behind them are the stream's too; frame_base and
// off_base are added to frame_of and frame_off.  The counts of this stretch; the filter moved on as in raw_decode_passes.
static int pf_decode_passes(mgpu_ctx *c, const struct mgpu_pf_in_args &a, uint64_t look, uint64_t frame_base, uint64_t off_base, PfInCounts *n, std::vector<uint32_t> *adds) {
    Behind &b = *c->behind;
    const uint64_t cand_cap = pf_in_max_frames(a.nbytes);
    PfInScratch w;
    if (int rc = b.beast_in.reserve_pf(c, a.nbytes, &w)) return rc;
    RawInParams p;
    FilterGens r;
    if (int rc = filter_passes_begin(c, cand_cap, p, r)) return rc;
    p.text = a.data; p.nbytes = a.nbytes; p.now_ms = a.now_ms;
    p.msgs = a.msgs; p.line_of = (unsigned long long *) a.frame_of; p.signal_level = a.signal_level; p.msgs_cap = a.msgs ? a.msgs_cap : 0;
    p.line_class = a.frame_class; p.line_class_cap = a.frame_class ? a.frames_cap : 0; p.line_base = frame_base;
    PfInParams q;
    q.data = a.data; q.nbytes = a.nbytes; q.look = look; q.cfg = p.cfg;
    q.frame_class = a.frame_class; q.frame_off = (unsigned long long *) a.frame_off; q.frames_cap = (a.frame_class || a.frame_off) ? a.frames_cap : 0; q.off_base = off_base;
    launch_pf_in_front(q, p, w, c->stream_aux);
    HIPCHK(c, hipGetLastError());
    unsigned long long total[6];
    HIPCHK(c, hipMemcpyAsync(total, w.total, sizeof total, hipMemcpyDeviceToHost, c->stream_aux));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    unsigned long long misc[16];
    int rc = MGPU_OK;
    if (total[1] > cand_cap) { c->err = "pf decode: more candidates than the stream can hold"; rc = MGPU_E_OVERFLOW; }   // (cannot happen: pf_in_max_frames)
    // (every handler call's class is stored, by k_pf_in_classify or by the filter passes: nothing to zero)
    if (int rc2 = filter_passes_end(c, p, r, rc ? 0 : total[1], 0, misc, adds)) return rc2;
    if (rc) return rc;
    n->frames = total[0]; n->msgs = misc[10]; n->consumed = total[4];
    n->cn[0] = misc[2] + misc[3] + misc[4] + misc[5] + misc[6];   // remote_received_modes: every Mode S frame that reached the decode
    for (int k = 1; k < 7; ++k) n->cn[k] = misc[k];
    n->cn[7] = total[2]; n->cn[8] = total[3];
    return MGPU_OK;
}

static int pf_decode_dev(mgpu_ctx *c, const struct mgpu_pf_in_args &a, uint64_t look, uint64_t frame_base, uint64_t off_base, PfInCounts *n, std::vector<uint32_t> *adds) {
    return filter_tables_after(c, pf_decode_passes(c, a, look, frame_base, off_base, n, adds));
}

static bool pf_in_args_ok(const struct mgpu_pf_in_args *a) {
    if (!a || a->size < sizeof(struct mgpu_pf_in_args) || !a->consumed || !a->nframes || !a->nmsgs || !a->counters) return false;
    if (a->nbytes + a->look >= (1ull << 32) || a->msgs_cap > UINT64_MAX / sizeof(mgpu_msg) || a->frames_cap > UINT64_MAX / sizeof(uint64_t)) return false;
    if (a->now_ms < 0 || a->now_ms >= 253402300800000ll) return false;
    if (a->nbytes && !a->data) return false;
    if ((a->msgs_cap && !a->msgs) || (a->frames_cap && !a->frame_class && !a->frame_off)) return false;
    return true;
}

static void pf_in_report(const struct mgpu_pf_in_args *a, const PfInCounts &n) {
    *a->consumed = n.consumed; *a->nframes = n.frames; *a->nmsgs = n.msgs;
    pf_in_counters_of(n, a->counters);
}

static int pf_in_finish(mgpu_ctx *c, const struct mgpu_pf_in_args *a, const PfInCounts &n, const IcaoFilter::Snapshot &before, const std::vector<uint32_t> &adds) {
    const char *overflow = n.msgs > a->msgs_cap ? "pf decode: more messages than the arrays hold" :
                           (a->frame_class || a->frame_off) && n.frames > a->frames_cap ? "pf decode: more handler calls than the frame arrays hold" : nullptr;
    return filter_call_end(c, overflow, before, adds);
}

int mgpu_pf_decode_device(mgpu_ctx *c, const struct mgpu_pf_in_args *a) {
    if (!c || !pf_in_args_ok(a)) return MGPU_E_INVAL;
    if (((uintptr_t) a->msgs | (uintptr_t) a->frame_of | (uintptr_t) a->signal_level | (uintptr_t) a->frame_off) & 7u) return MGPU_E_INVAL;
    PfInCounts n;
    pf_in_report(a, n);
    if (a->nbytes == 0) return MGPU_OK;
    { const int rc = drain(c); if (rc != MGPU_OK) return rc; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    IcaoFilter::Snapshot before;
    c->resolver.filter().snapshot(before);
    std::vector<uint32_t> adds;
    if (int rc = pf_decode_dev(c, *a, a->look, 0, 0, &n, &adds)) { c->resolver.filter().restore(before); return rc; }
    pf_in_report(a, n);
    return pf_in_finish(c, a, n, before, adds);
}

int mgpu_pf_decode(mgpu_ctx *c, const struct mgpu_pf_in_args *a) {
    if (!c || !pf_in_args_ok(a)) return MGPU_E_INVAL;
    PfInCounts all;
    pf_in_report(a, all);
    if (a->nbytes == 0) return MGPU_OK;
    { const int rc = drain(c); if (rc != MGPU_OK) return rc; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    Behind &b = *c->behind;
    IcaoFilter::Snapshot before;
    c->resolver.filter().snapshot(before);
    std::vector<uint32_t> adds;
    const bool want_frames = a->frame_class || a->frame_off;
    size_t adds_before = 0;
    IcaoFilter::Snapshot pass_before;
    const int prc = stream_passes(a->nbytes, a->pass_bytes ? a->pass_bytes : kLineDefaultPass, false, all,
        [&](uint64_t at, uint64_t nb, bool, const PfInCounts &so_far, PfInCounts &n) -> int {
            // a pass frames nb bytes; the lookahead and the handler's reads may take kPfInReach more, which decide every frame that starts
            // inside the pass; what the caller's arrays still hold, and no more than nb bytes can give
            const uint64_t look = pf_in_look(a->nbytes + a->look, at, nb);
            const uint64_t msg_room = a->msgs_cap > so_far.msgs ? std::min<uint64_t>(a->msgs_cap - so_far.msgs, pf_in_max_frames(nb)) : 0;
            const uint64_t frame_room = want_frames && a->frames_cap > so_far.frames ? std::min<uint64_t>(a->frames_cap - so_far.frames, pf_in_max_frames(nb)) : 0;
            int rc;
            if ((rc = b.d_stream.reserve(c, nb + look + 64)) || (rc = b.d_in_msgs.reserve(c, (msg_room + 1) * sizeof(mgpu_msg))) ||
                (rc = b.d_index_of.reserve(c, (msg_room + 1) * sizeof(uint64_t))) || (rc = b.d_in_signal.reserve(c, (msg_room + 1) * sizeof(double))) ||
                (rc = b.d_in_class.reserve(c, frame_room + 1)) || (rc = b.d_bin_frame_off.reserve(c, (frame_room + 1) * sizeof(uint64_t)))) return rc;
            struct mgpu_pf_in_args d = *a;
            d.data = b.d_stream.as<uint8_t>(); d.nbytes = nb;
            d.msgs = b.d_in_msgs.as<mgpu_msg>(); d.msgs_cap = msg_room;
            d.frame_of = a->frame_of ? b.d_index_of.as<uint64_t>() : nullptr;
            d.signal_level = a->signal_level ? b.d_in_signal.as<double>() : nullptr;
            d.frame_class = a->frame_class ? b.d_in_class.as<uint8_t>() : nullptr;
            d.frame_off = a->frame_off ? b.d_bin_frame_off.as<uint64_t>() : nullptr;
            d.frames_cap = frame_room;
            HIPCHK(c, hipMemcpyAsync(b.d_stream.p, a->data + at, nb + look, hipMemcpyHostToDevice, c->stream_aux));
            adds_before = adds.size();
            c->resolver.filter().snapshot(pass_before);
            if ((rc = pf_decode_dev(c, d, look, so_far.frames, at, &n, &adds))) return rc;
            // (the pass stored below its rooms only: the copies stay inside the caller's arrays)
            const uint64_t nmsg = std::min<uint64_t>(n.msgs, msg_room), nfr = std::min<uint64_t>(n.frames, frame_room);
            if (nmsg) HIPCHK(c, hipMemcpy(a->msgs + so_far.msgs, d.msgs, nmsg * sizeof(mgpu_msg), hipMemcpyDeviceToHost));
            if (nmsg && a->frame_of) HIPCHK(c, hipMemcpy(a->frame_of + so_far.msgs, d.frame_of, nmsg * sizeof(uint64_t), hipMemcpyDeviceToHost));
            if (nmsg && a->signal_level) HIPCHK(c, hipMemcpy(a->signal_level + so_far.msgs, d.signal_level, nmsg * sizeof(double), hipMemcpyDeviceToHost));
            if (nfr && a->frame_class) HIPCHK(c, hipMemcpy(a->frame_class + so_far.frames, d.frame_class, nfr, hipMemcpyDeviceToHost));
            if (nfr && a->frame_off) HIPCHK(c, hipMemcpy(a->frame_off + so_far.frames, d.frame_off, nfr * sizeof(uint64_t), hipMemcpyDeviceToHost));
            return MGPU_OK;
        },
        [&] { c->resolver.filter().restore(pass_before); adds.resize(adds_before); });
    if (prc != MGPU_OK) { c->resolver.filter().restore(before); return prc; }
    pf_in_report(a, all);
    return pf_in_finish(c, a, all, before, adds);
}

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
