// asterix_in_host.cpp — the ASTERIX input parser (asterix_in_format.h) on the host: mgpu_asterix_parse_host /
// mgpu_asterix_parse_record_host.  No HIP in this file: tests/host_stub/asterix_in_format_check.cpp compiles it with plain g++, under
// ASan and UBSan too.
#include <cstring>

#include "asterix_in_format.h"

extern "C" {

int mgpu_asterix_parse_record_host(const uint8_t *data, uint64_t nbytes, uint64_t offset, uint32_t source, int64_t now_ms, struct mgpu_asterix_rec *rec) {
    if (!data || offset >= nbytes || !rec || !ast_in_source_ok(source) || !ast_in_now_ok(now_ms)) return MGPU_E_INVAL;
    memset(rec, 0, sizeof *rec);
    mgpu_asterix_rec r;
    if (ast_in_record(AstBytes{data, nbytes}, offset, source, now_ms, r) != AST_IN_RECORD) return 0;
    *rec = r;
    return 1;
}

int mgpu_asterix_parse_host(const struct mgpu_asterix_in_args *a, uint64_t frame_index, struct mgpu_asterix_rec *rec) {
    if (!a || a->size < sizeof(struct mgpu_asterix_in_args) || (a->nbytes && !a->data) || !rec) return MGPU_E_INVAL;
    const AstBytes s = {a->data, a->nbytes};
    uint64_t at = 0;
    for (uint64_t k = 0;; ++k) {
        uint32_t len;
        if (ast_in_frame(s, at, len) != AST_IN_FRAME) return MGPU_E_INVAL;
        if (k == frame_index) return mgpu_asterix_parse_record_host(a->data, a->nbytes, at, a->source, a->now_ms, rec);
        mgpu_asterix_rec r;
        const int cls = ast_in_record(s, at, 0, 0, r);
        if (cls == AST_IN_CLOSED) return MGPU_E_INVAL;                // nothing behind it is framed
        at += len;
    }
}

}  // extern "C"
