// sbs_in_host.cpp — the SBS input parser (sbs_in_format.h) on the host: mgpu_sbs_parse_host / mgpu_sbs_parse_line_host, which settle
// the lines the device defers, every number outside the plain form resolved by the host's strtol and strtod as the reference's
// atoi, strtol and strtod calls do (net_io.c:3054-3115).  No HIP in this file: tests/host_stub/sbs_in_format_check.cpp compiles it
// with plain g++, under ASan and UBSan too.
#include <cstdlib>
#include <cstring>

#include "sbs_in_format.h"

namespace {
// a token is shorter than a line: NUL-terminated in a copy, as strsep leaves it in the reference's buffer
struct LibcResolve {
    bool integer(const uint8_t *t, uint32_t len, long long &v) const {
        char buf[kSbsInMaxLen + 1];
        memcpy(buf, t, len);
        buf[len] = 0;
        v = strtol(buf, nullptr, 10);                                 // (atoi is (int) strtol(s, NULL, 10))
        return true;
    }
    bool real(const uint8_t *t, uint32_t len, double &v) const {
        char buf[kSbsInMaxLen + 1];
        memcpy(buf, t, len);
        buf[len] = 0;
        v = strtod(buf, nullptr);
        return true;
    }
};
}  // namespace

extern "C" {

int mgpu_sbs_parse_line_host(const uint8_t *line, uint64_t len, uint32_t source, int64_t now_ms, struct mgpu_sbs_rec *rec) {
    if ((len && !line) || !rec || !sbs_in_source_ok(source)) return MGPU_E_INVAL;
    memset(rec, 0, sizeof *rec);
    mgpu_sbs_rec r;
    const int cls = sbs_in_line(line, (uint32_t) (len > kSbsInLook ? kSbsInLook : len), source, now_ms, LibcResolve{}, r);
    if (cls != SBS_IN_RECORD) return 0;
    *rec = r;
    return 1;
}

int mgpu_sbs_parse_host(const struct mgpu_sbs_in_args *a, uint64_t line_index, struct mgpu_sbs_rec *rec) {
    if (!a || a->size < sizeof(struct mgpu_sbs_in_args) || (a->nbytes && !a->text) || !rec) return MGPU_E_INVAL;
    const uint8_t *p = a->text, *end = a->text + a->nbytes;
    for (uint64_t k = 0;; ++k) {
        const uint8_t *q = p;
        while (q < end && *q != '\n' && *q != 0) ++q;
        if (q >= end) return MGPU_E_INVAL;                            // (bytes behind the last terminator are no line)
        if (k == line_index) return mgpu_sbs_parse_line_host(p, (uint64_t) (q - p), a->source, a->now_ms, rec);
        p = q + 1;
    }
}

}  // extern "C"
