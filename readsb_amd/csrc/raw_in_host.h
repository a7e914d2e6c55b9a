// raw_in_host.h — private to the library and its check programs: the host side of the raw input (raw_in_host.cpp).  The sequential
// resolver below is NOT part of the installed C ABI (include/modes_gpu.h): it is the plain statement of the rule for the host-side
// checks and the tests, exported from the library only so that the tests reach it.
#pragma once
#include <cstdint>
#include <vector>

#include "icao_filter.h"
#include "raw_in_format.h"

namespace mgpu {

struct RawInHostTables {
    std::vector<uint64_t> tab_long, tab_short;
};
const RawInHostTables &raw_in_host_tables(int nfix_crc);     // the packed syndrome tables of an nfix_crc value, built once
RawInTables raw_in_tables_of(const RawInHostTables &t);

// Every terminated line of a HOST-memory text in order through the parser and decodeModesMessage's filter questions, against `filter`
// (icao_filter.h: the library's own model), which is moved on as the reference's would be; the outputs as mgpu_raw_decode gives them
// (capacities as there: MGPU_E_OVERFLOW with what is needed and the filter as it was).
int raw_in_decode_sequential(const struct mgpu_raw_in_args *args, const struct mgpu_raw_in_config *cfg, IcaoFilter &filter);

}  // namespace mgpu

extern "C" {
// The same for a caller without C++ (the tests, through ctypes): the filter given and returned as its two generations (addresses
// below 2^24; room for n_active + the text's lines and n_inactive entries), its occupied count and log2 of its table size.
struct mgpu_raw_in_filter {
    uint32_t *gen_active, *gen_inactive;
    uint64_t n_active, n_inactive;
    uint32_t occupied, table_bits;
};
int mgpu_raw_decode_host(const struct mgpu_raw_in_args *args, const struct mgpu_raw_in_config *cfg, struct mgpu_raw_in_filter *filter);
}
