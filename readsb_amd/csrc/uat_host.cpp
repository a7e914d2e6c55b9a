// uat_host.cpp — the UAT formatter (uat_format.h) on the host: mgpu_uat_format_host / mgpu_uat_format_line_host, which settle the
// lines the device defers with the host's sscanf and libm, and the one cached table of signal bytes (mgpu::uat_sig_table) that the
// host formatter reads and behind_in.cpp uploads for the device.  No HIP in this file:
// tests/host_stub/uat_format_check.cpp compiles it with plain g++, under ASan and UBSan too.
#include <cstring>
#include <vector>

#include "uat_format.h"

namespace mgpu {
// the one table of signal bytes, built on first use: the host formatter reads it here, behind_in.cpp uploads it for the device
const uint8_t *uat_sig_table() {
    static const std::vector<uint8_t> table = [] {
        std::vector<uint8_t> t(kUatSigTable);
        uat_build_sig_table(t.data());
        return t;
    }();
    return table.data();
}
}  // namespace mgpu
using mgpu::uat_sig_table;

namespace {
struct HostEmit {
    uint8_t *text;
    uint64_t cap, at;
    mgpu_msg *msgs;
    uint8_t *sig;
    int64_t now_ms;
    uint32_t n;
    struct Sink {
        HostEmit &e;
        void put(uint32_t c) { if (e.at < e.cap) e.text[e.at] = (uint8_t) c; ++e.at; }
    };
    void frame(uint32_t s, const UatFrame &fr) {
        Sink sink{*this};
        uat_put_frame(sink, s, fr);
        if (msgs && n < kUatMaxFrames) { memset(&msgs[n], 0, sizeof msgs[n]); uat_fill_msg(msgs[n], s, fr, now_ms); }
        if (sig) *sig = (uint8_t) s;
        ++n;
    }
};
}  // namespace

extern "C" {

int64_t mgpu_uat_format_line_host(const uint8_t *line, uint64_t len, int64_t now_ms, uint8_t *text, uint64_t cap, struct mgpu_msg *msgs, uint8_t *sig) {
    if ((len && !line) || (cap && !text)) return MGPU_E_INVAL;
    HostEmit e = {text, cap, 0, msgs, sig, now_ms, 0};
    uat_host_line(line, len, uat_sig_table(), e);
    return (int64_t) e.at;
}

int64_t mgpu_uat_format_host(const struct mgpu_uat_args *a, uint64_t line_index, uint8_t *text, uint64_t cap, struct mgpu_msg *msgs, uint8_t *sig) {
    if (!a || a->size < sizeof(struct mgpu_uat_args) || (a->nbytes && !a->text)) return MGPU_E_INVAL;
    const uint8_t *p = a->text, *end = a->text + a->nbytes;
    for (uint64_t k = 0;; ++k) {
        const uint8_t *nl = p < end ? (const uint8_t *) memchr(p, '\n', (size_t) (end - p)) : nullptr;
        if (!nl) return MGPU_E_INVAL;                                 // (bytes behind the last '\n' are no line)
        if (k == line_index) return mgpu_uat_format_line_host(p, (uint64_t) (nl - p), a->now_ms, text, cap, msgs, sig);
        p = nl + 1;
    }
}

}  // extern "C"
