// snip.h — private to the library: the device state of mgpu_snip / mgpu_snip_device (snip.cpp).  Only those synchronous calls on
// stream_aux touch it.  api.cpp creates it with the context and releases it in mgpu_destroy.
#pragma once
#include "devbuf.h"

struct Snip {
    // the passes' scratch (kernels/snip.inc): the keep masks; per workgroup kept | last loud, and the first's offsets; the two totals
    DevBuf d_masks, d_blocks, d_off, d_total;
    DevBuf d_in, d_out;                                      // the host form's staged pass and what it keeps
};
