// lz4e_hostreg.h -- registry of host memory the caller registered with
// lz4e_register_host_memory (include/lz4e.h): an interval map from host
// address ranges to the device addresses hipHostGetDevicePointer gave for
// them.  The chunk pipeline hands the device only addresses that translate()
// returned, so this is the one place that decides what "inside a
// registration" means.  Plain C++ (no HIP): tests/test_hostreg.py builds it
// alone under ASan + UBSan.  Not thread safe: the owner locks.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <map>

namespace lz4e {

class HostRegistry {
  public:
    struct Range {
        uintptr_t base;
        size_t len;
        uint64_t dev;  // device address of base
    };
    static constexpr uint64_t kNotContained = ~uint64_t(0);

    // True when [base, base + len) shares a byte with a live registration.
    bool overlaps(uintptr_t base, size_t len) const {
        auto it = map_.upper_bound(base);  // first registration starting after base
        if (it != map_.end() && it->first - base < len) return true;
        if (it == map_.begin()) return false;
        --it;
        return base - it->second.base < it->second.len;
    }

    // Adds [base, base + len) -> dev_base.  Refused (false): an empty range,
    // one that wraps the address space, or one that overlaps a live
    // registration (adjacent ranges do not overlap).
    bool insert(uintptr_t base, size_t len, uint64_t dev_base) {
        if (len == 0 || len - 1 > UINTPTR_MAX - base || overlaps(base, len)) return false;
        map_[base] = Range{base, len, dev_base};
        return true;
    }

    // Removes the registration that starts exactly at base.
    bool erase(uintptr_t base) { return map_.erase(base) != 0; }

    // The registration that holds address p, or nullptr.  The pointer stays
    // valid until that registration is erased.
    const Range* find(uintptr_t p) const {
        auto it = map_.upper_bound(p);
        if (it == map_.begin()) return nullptr;
        --it;
        return p - it->second.base < it->second.len ? &it->second : nullptr;
    }

    // Device address of p when [p, p + len) lies wholly inside r, else
    // kNotContained.  len == 0: p itself must lie inside r.
    static uint64_t translate_in(const Range& r, uintptr_t p, size_t len) {
        if (p < r.base || p - r.base >= r.len) return kNotContained;
        const size_t off = p - r.base;
        if (len > r.len - off) return kNotContained;
        return r.dev + off;
    }

    // Device address of ptr when [ptr, ptr + len) lies wholly inside ONE
    // registration, else kNotContained: a range that starts in one
    // registration and ends outside it is not contained, also when the next
    // registration begins exactly where this one ends (two registrations
    // are two mappings; nothing says their device addresses are adjacent).
    uint64_t translate(const void* ptr, size_t len) const {
        const uintptr_t p = reinterpret_cast<uintptr_t>(ptr);
        const Range* r = find(p);
        return r ? translate_in(*r, p, len) : kNotContained;
    }

    bool empty() const { return map_.empty(); }
    size_t size() const { return map_.size(); }

  private:
    std::map<uintptr_t, Range> map_;
};

}  // namespace lz4e
