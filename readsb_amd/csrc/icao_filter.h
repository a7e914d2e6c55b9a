// icao_filter.h — the ICAO address filter of the reference (icao_filter.c) as an exact model, free of the device headers: the ordered
// walk (resolve.h), the raw input's replay of the device's new adds (behind_in.cpp) and its sequential resolver and check programs
// (raw_in_host.cpp, tests/host_stub/raw_in_*_check.cpp, plain g++) all use this one.  Header only, so that each of them is one
// translation unit more and no more.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace mgpu {

// Exact model of icao_filter.c: two generations, `occupied`, table size.  Bucket placement never
// shows in results; membership, the occupied count and the grow/shrink thresholds do, because
// growing re-inserts only the active generation (icaoFilterResize, icao_filter.c:65-93).
class IcaoFilter {
  public:
    IcaoFilter();
    void init();                       // icaoFilterInit (:47-59)
    void add(uint32_t addr);           // icaoFilterAdd (:112-130)
    bool test(uint32_t addr) const {   // icaoFilterTest (:132-154)
        return addr < (1u << 24) ? (((bits_[0][addr >> 6] | bits_[1][addr >> 6]) >> (addr & 63)) & 1) : big_test(addr);
    }
    void expire();                     // icaoFilterExpire (:96-110)
    uint32_t occupied() const { return occupied_; }
    uint32_t table_bits() const { return filter_bits_; }

    // --- support for the speculative parallel walk (resolve.cpp: Resolver::spec_walk / commit_segment) ---
    struct Snapshot {
        std::vector<uint32_t> members[2], big[2];
        int active = 0;
        uint32_t occupied = 0, filter_bits = 8;
    };
    void snapshot(Snapshot &s) const;
    void restore(const Snapshot &s);
    int active_index() const { return active_; }
    void union_sorted(std::vector<uint32_t> &out) const;      // addresses < 2^24 in either generation, ascending
    const std::vector<uint32_t> &members(bool active) const { return members_[active ? active_ : active_ ^ 1]; }   // addresses < 2^24
    bool same_as(const IcaoFilter &o) const;                  // membership per generation, occupied, table size
    bool in_generation(uint32_t addr, bool active) const {    // addr < 2^24
        return (bits_[active ? active_ : active_ ^ 1][addr >> 6] >> (addr & 63)) & 1;
    }
    // addresses that leave the union (expire / resize) and addresses that enter it (first add)
    void track_changes(std::vector<uint32_t> *drops, std::vector<uint32_t> *news) { drops_ = drops; news_ = news; }

  private:
    void resize(uint32_t bits);
    bool big_test(uint32_t addr) const;
    void clear_gen(int g);
    std::vector<uint64_t> bits_[2];       // 2^24-bit membership bitmap per generation
    std::vector<uint32_t> members_[2];    // for O(members) clearing
    std::vector<uint32_t> big_[2];        // addresses >= 2^24 (only Modes.show_only's default)
    int active_ = 0;
    uint32_t occupied_ = 0, filter_bits_ = 8;
    std::vector<uint32_t> *drops_ = nullptr, *news_ = nullptr;
};

inline IcaoFilter::IcaoFilter() {
    for (int g = 0; g < 2; ++g) bits_[g].assign(1u << 18, 0);
    init();
}

inline void IcaoFilter::clear_gen(int g) {
    if (drops_)   // what leaves the union: members of this generation the other one does not hold
        for (uint32_t a : members_[g])
            if (!((bits_[g ^ 1][a >> 6] >> (a & 63)) & 1)) drops_->push_back(a);
    for (uint32_t a : members_[g]) bits_[g][a >> 6] = 0;
    members_[g].clear();
    big_[g].clear();
}

inline void IcaoFilter::init() {
    clear_gen(0);
    clear_gen(1);
    active_ = 0;
    occupied_ = 0;
    filter_bits_ = 8;
}

inline bool IcaoFilter::big_test(uint32_t addr) const {
    for (int g = 0; g < 2; ++g)
        if (std::find(big_[g].begin(), big_[g].end(), addr) != big_[g].end()) return true;
    return false;
}

inline void IcaoFilter::resize(uint32_t bits) {
    // two fresh tables; only the ACTIVE generation's entries are re-inserted
    filter_bits_ = bits;
    clear_gen(active_ ^ 1);
    occupied_ = (uint32_t) (members_[active_].size() + big_[active_].size());
}

inline void IcaoFilter::add(uint32_t addr) {
    bool inserted = false;
    if (addr < (1u << 24)) {
        uint64_t &w = bits_[active_][addr >> 6];
        const uint64_t bit = 1ull << (addr & 63);
        if (!(w & bit)) {
            w |= bit; members_[active_].push_back(addr); inserted = true;
            if (news_ && !((bits_[active_ ^ 1][addr >> 6] >> (addr & 63)) & 1)) news_->push_back(addr);
        }
    } else if (std::find(big_[active_].begin(), big_[active_].end(), addr) == big_[active_].end()) {
        big_[active_].push_back(addr);
        inserted = true;
    }
    if (inserted) ++occupied_;
    if (occupied_ > (1u << filter_bits_) / 3 && filter_bits_ < 20) resize(filter_bits_ + 1);
}

inline void IcaoFilter::expire() {
    if (occupied_ < (1u << filter_bits_) / 9 && filter_bits_ > 8) resize(filter_bits_ - 1);
    occupied_ = 0;
    clear_gen(active_ ^ 1);
    active_ ^= 1;
}

inline void IcaoFilter::snapshot(Snapshot &s) const {
    for (int g = 0; g < 2; ++g) { s.members[g] = members_[g]; s.big[g] = big_[g]; }
    s.active = active_; s.occupied = occupied_; s.filter_bits = filter_bits_;
}

inline void IcaoFilter::restore(const Snapshot &s) {
    std::vector<uint32_t> *keep = drops_;
    drops_ = nullptr;   // (news_ is only touched by add)
    for (int g = 0; g < 2; ++g) {
        clear_gen(g);
        for (uint32_t a : s.members[g]) bits_[g][a >> 6] |= 1ull << (a & 63);
        members_[g] = s.members[g];
        big_[g] = s.big[g];
    }
    active_ = s.active; occupied_ = s.occupied; filter_bits_ = s.filter_bits;
    drops_ = keep;
}

inline void IcaoFilter::union_sorted(std::vector<uint32_t> &out) const {
    out.clear();
    out.insert(out.end(), members_[0].begin(), members_[0].end());
    out.insert(out.end(), members_[1].begin(), members_[1].end());
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
}

inline bool IcaoFilter::same_as(const IcaoFilter &o) const {
    if (occupied_ != o.occupied_ || filter_bits_ != o.filter_bits_) return false;
    for (int g = 0; g < 2; ++g) {
        std::vector<uint32_t> x = members_[g ? active_ ^ 1 : active_], y = o.members_[g ? o.active_ ^ 1 : o.active_];
        std::vector<uint32_t> bx = big_[g ? active_ ^ 1 : active_], by = o.big_[g ? o.active_ ^ 1 : o.active_];
        std::sort(x.begin(), x.end()); std::sort(y.begin(), y.end());
        std::sort(bx.begin(), bx.end()); std::sort(by.begin(), by.end());
        if (x != y || bx != by) return false;
    }
    return true;
}

}  // namespace mgpu
