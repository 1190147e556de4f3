// lz4e_store_scratch.h -- how the packed store's read calls carve their one
// stream-ordered scratch allocation into arrays (lz4e_host.hip), stated once:
// the lane emulator (tools/emu) sizes its per-array allocations from the same
// layouts and checks them for overlap, alignment and bounds on the CPU.
// Plain C++: no HIP.  8-byte arrays come first, then 4-byte ones, then bytes,
// so every offset is a multiple of its array's element size.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace lz4e {

static_assert(sizeof(size_t) == 8, "the layouts hold byte counts of up to 2^63");

struct ScratchArray {
    size_t offset, bytes;
    template <class T>
    T* in(void* base) const {
        return reinterpret_cast<T*>(static_cast<uint8_t*>(base) + offset);
    }
};

// The next `count` elements of `elem` bytes at the running offset `o`.
inline ScratchArray scratch_take(size_t& o, size_t elem, uint64_t count) {
    const ScratchArray a{o, (size_t)(elem * count)};
    o += a.bytes;
    return a;
}

// The checksum's sizing hint where the caller has none: a workgroup per entry.
inline uint32_t crc_hint_or_default(uint32_t hint) { return hint ? hint : 256 * 64; }

// lz4e_unpack_verified_batch_dev, n entries, `words` partial checksum words.
struct VerifiedUnpackScratch {
    ScratchArray got, masked, partial, shown;
    size_t total;
    VerifiedUnpackScratch(uint32_t n, uint64_t words) {
        size_t o = 0;
        got = scratch_take(o, 4, n);
        masked = scratch_take(o, 4, n);
        partial = scratch_take(o, 4, words);
        shown = scratch_take(o, 1, n);
        total = o;
    }
};

// lz4e_unpack_range_batch_dev (verified == false: the arrays of the checksum
// and the election are empty) and lz4e_unpack_range_verified_batch_dev: nreq
// slots of roundup(max_end, 16) bytes, a multiple of 16 together, then the
// partial launch's descriptors and the verified read's columns.  max_end is at
// most 0x7FFFFFF0, so the slots stay under 2^63 bytes.
struct RangeScratch {
    size_t slot;
    ScratchArray slots, g_off, s_off, c_off, g_len, g_tgt, g_ret, c_len, got, owner, partial, shown;
    size_t total;
    RangeScratch(uint32_t nreq, uint32_t max_end, bool verified = false, uint32_t nentries = 0, uint64_t words = 0) {
        const uint64_t v = verified ? 1 : 0;
        size_t o = 0;
        slot = ((size_t)max_end + 15) & ~(size_t)15;
        slots = scratch_take(o, slot, nreq);
        g_off = scratch_take(o, 8, nreq);
        s_off = scratch_take(o, 8, nreq);
        c_off = scratch_take(o, 8, v * nreq);
        g_len = scratch_take(o, 4, nreq);
        g_tgt = scratch_take(o, 4, nreq);
        g_ret = scratch_take(o, 4, nreq);
        c_len = scratch_take(o, 4, v * nreq);
        got = scratch_take(o, 4, v * nreq);
        owner = scratch_take(o, 4, v * nentries);
        partial = scratch_take(o, 4, v * words);
        shown = scratch_take(o, 1, v * nentries);
        total = o + 16;  // spare bytes behind the last array, as these calls have always asked for
    }
};

}  // namespace lz4e
