// devbuf.h — private to the library: owning, grow-only device scratch (struct Behind in behind.h, struct Snip in snip.h).
#pragma once
#include "ctx.h"

// A failed reservation leaves it empty with the context's error text set.
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
