// Lane emulator of the packed frame store's checksum kernels (debug/test
// tooling, tools/emu): compiles the unmodified csrc/lz4e_crc.hip as host C++
// and runs crc_team_kernel, crc_combine_kernel, unpack_verify_mask_kernel and
// unpack_verify_ret_kernel under the same emulated <hip/hip_runtime.h> as the
// other kernel files; csrc/lz4e_pack.hip is compiled in for the raw copy that
// runs between the two verify kernels (the decoders that run there too are
// emu_main's business: here their part is played by a stand-in that returns
// -1 for a masked length of 0 and a marker otherwise).  Stand-alone (its own
// main): built by EMU_CRC=1 build.sh, run by tests/test_emulator_crc.py under
// ASan + UBSan.  `emu_crc rangev` runs, in place of all that, the verified
// range read's composition (rangev_case: the four range_verify_* kernels of
// lz4e_crc.hip around launch_crc and lz4e_pack.hip's range_gather_kernel and
// range_deliver_kernel; tests/test_emulator_range_verified.py).
//
// The kernels read the CALLER's memory at byte granularity.  So every entry
// here is its own heap allocation that ends exactly at its last byte (ASan's
// redzone follows it), placed at a chosen alignment mod 16 (emu_harness.h, Buf).
// An entry that must not be read is an allocation of 0 bytes or an offset
// outside every allocation.  Expected values come from ref_crc below, a
// bitwise restatement of CRC-32C that shares nothing with the kernel's tables.
//
// crc_team_kernel fills a table in LDS behind a barrier and XORs across
// lanes, so it runs on the harness's pool of lane threads; the other kernels
// have neither, so their lanes run one after the other on the calling thread,
// and the pack scan kernels are not run here: the table next to main.
#include <algorithm>

#include "emu_harness.h"
#undef __shared__
#define __shared__ static

#include "lz4e_crc.hip"
#include "lz4e_pack.hip"

#include "lz4e.h"
#include "lz4e_store_scratch.h"

uint32_t g_rng = 2463534242u;
uint32_t rnd32() { return emu_lcg(g_rng) >> 8; }
uint8_t rnd() { return (uint8_t)rnd32(); }

namespace {

// CRC-32C bit by bit.
uint32_t ref_crc(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? 0x82F63B78u : 0u);
    }
    return c ^ 0xFFFFFFFFu;
}

constexpr uint32_t kHugeHint = 0x7E000000u;

// The carving lz4e_host.hip does (csrc/lz4e_store_scratch.h) on its own: every
// array holds its elements, lies inside [0, total) at a multiple of its
// element size and overlaps no other; `total` has not wrapped.
struct LArray {
    const char* name;
    lz4e::ScratchArray a;
    size_t elem;
    uint64_t count;
};
void layout_check(const char* what, const std::vector<LArray>& as, size_t total) {
    unsigned __int128 need = 0;
    for (size_t i = 0; i < as.size(); ++i) {
        const lz4e::ScratchArray& a = as[i].a;
        need += (unsigned __int128)as[i].elem * as[i].count;
        CHECK(a.bytes == (unsigned __int128)as[i].elem * as[i].count, "%s: %s holds %zu bytes", what, as[i].name, a.bytes);
        CHECK(a.offset + a.bytes >= a.offset && a.offset + a.bytes <= total, "%s: %s ends outside the allocation", what, as[i].name);
        CHECK(a.offset % as[i].elem == 0, "%s: %s at offset %zu", what, as[i].name, a.offset);
        for (size_t k = 0; k < i; ++k)
            CHECK(a.offset >= as[k].a.offset + as[k].a.bytes || as[k].a.offset >= a.offset + a.bytes || !a.bytes || !as[k].a.bytes,
                  "%s: %s overlaps %s", what, as[i].name, as[k].name);
    }
    CHECK(total >= need, "%s: a total of %zu bytes", what, total);
}
void layout_sweep() {
    for (uint32_t n : {0u, 1u, 2u, 3u, 255u, 256u, 257u})
        for (uint64_t words : {(uint64_t)0, (uint64_t)1, (uint64_t)5, (uint64_t)64 * n}) {
            const lz4e::VerifiedUnpackScratch U(n, words);
            layout_check("verified unpack", {{"got", U.got, 4, n}, {"masked", U.masked, 4, n}, {"partial", U.partial, 4, words}, {"shown", U.shown, 1, n}},
                         U.total);
            for (uint32_t ne : {0u, 1u, 7u, 300u})
                for (uint32_t max_end : {0u, 1u, 15u, 16u, 17u, 4097u, 0x7FFFFFF0u})
                    for (uint64_t v : {0u, 1u}) {
                        const lz4e::RangeScratch L(n, max_end, v != 0, ne, words);
                        const size_t slot = ((size_t)max_end + 15) / 16 * 16;
                        CHECK(L.slot == slot, "range read: a slot of %zu bytes for max_end %u", L.slot, max_end);
                        layout_check(v ? "verified range read" : "range read",
                                     {{"slots", L.slots, 16, (uint64_t)n * (slot / 16)}, {"g_off", L.g_off, 8, n}, {"s_off", L.s_off, 8, n},
                                      {"c_off", L.c_off, 8, v * n}, {"g_len", L.g_len, 4, n}, {"g_tgt", L.g_tgt, 4, n}, {"g_ret", L.g_ret, 4, n},
                                      {"c_len", L.c_len, 4, v * n}, {"got", L.got, 4, v * n}, {"owner", L.owner, 4, v * ne},
                                      {"partial", L.partial, 4, v * words}, {"shown", L.shown, 1, v * ne}},
                                     L.total);
                    }
        }
}

// launch_crc with the scratch lz4e_host.hip would take from the pool: an
// exact-size allocation, so a partial written outside it is a report.
void run_crc(const lz4e::CrcBatch& a, const char* what) {
    const uint64_t words = lz4e::crc_partial_words(a.max_len, a.nblocks);
    Buf partial(0, 4 * (size_t)words);
    partial.fill(kFill);
    CHECK(lz4e::launch_crc(a, words ? partial.as<uint32_t>() : nullptr, nullptr) == hipSuccess, "%s: launch", what);
}

struct CEntry {
    int32_t len;  // <= 0: an allocation of 0 bytes
    uint32_t align;
};

// lz4e_crc32c_batch_dev's kernels on entries that are allocations of their
// own, once per hint; every column must equal the bitwise restatement.
void crc_case(const char* what, const std::vector<CEntry>& es, const std::vector<uint32_t>& hints) {
    const uint32_t n = (uint32_t)es.size();
    std::vector<BufP> bufs;
    std::vector<uint32_t> want(n);
    for (uint32_t i = 0; i < n; ++i) {
        bufs.emplace_back(new Buf(es[i].align, es[i].len > 0 ? (size_t)es[i].len : 0));
        bufs[i]->fill_random();
        want[i] = ref_crc(bufs[i]->p, bufs[i]->n);
    }
    const uint8_t* data = lowest(bufs);
    Buf off(0, 8 * (size_t)n), len(0, 4 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        off.as<uint64_t>()[i] = (uint64_t)(bufs[i]->p - data);
        len.as<int32_t>()[i] = es[i].len;
    }
    for (uint32_t hint : hints) {
        Buf crc(0, 4 * (size_t)n);
        crc.fill(kFill);
        const lz4e::CrcBatch a{data, off.as<uint64_t>(), nullptr, nullptr, nullptr, len.as<int32_t>(),
                               crc.as<uint32_t>(), n, hint};
        run_crc(a, what);
        for (uint32_t i = 0; i < n; ++i)
            CHECK(crc.as<uint32_t>()[i] == want[i], "%s: hint %u (team shift %u), entry %u of %u (len %d at %u mod 16): %08x, expected %08x",
                  what, hint, lz4e::crc_team_shift(hint, n), i, n, es[i].len, es[i].align, crc.as<uint32_t>()[i], want[i]);
    }
    for (uint32_t i = 0; i < n; ++i) CHECK(bufs[i]->canary_ok(), "%s: canary of entry %u", what, i);
}

// The same bytes between different neighbours, inside one allocation each.
void context_case(uint32_t body_len, uint32_t hint) {
    std::vector<uint8_t> body(body_len);
    for (auto& b : body) b = rnd();
    const uint32_t want = ref_crc(body.data(), body_len);
    const uint32_t before[4] = {0, 1, 37, 4096}, after[4] = {0, 64, 5, 1};
    std::vector<BufP> bufs;
    Buf off(0, 8 * 4), len(0, 4 * 4), crc(0, 4 * 4);
    for (uint32_t k = 0; k < 4; ++k) {
        bufs.emplace_back(new Buf(k * 5, before[k] + body_len + after[k]));
        bufs[k]->fill_random();
        memcpy(bufs[k]->p + before[k], body.data(), body_len);
    }
    const uint8_t* data = lowest(bufs);
    for (uint32_t k = 0; k < 4; ++k) {
        off.as<uint64_t>()[k] = (uint64_t)(bufs[k]->p + before[k] - data);
        len.as<int32_t>()[k] = (int32_t)body_len;
    }
    crc.fill(kFill);
    const lz4e::CrcBatch a{data, off.as<uint64_t>(), nullptr, nullptr, nullptr, len.as<int32_t>(), crc.as<uint32_t>(), 4, hint};
    run_crc(a, "context");
    for (uint32_t k = 0; k < 4; ++k)
        CHECK(crc.as<uint32_t>()[k] == want, "context: %u bytes after %u and before %u others: %08x, expected %08x", body_len,
              before[k], after[k], crc.as<uint32_t>()[k], want);
}

struct PEntry {
    uint8_t kind;
    uint32_t len, frame_align, src_align;
};

// lz4e_pack_crc_batch_dev's launch: what an entry's kind does not read is 0 bytes long.
void pack_crc_case(const char* what, const std::vector<PEntry>& es, const std::vector<uint32_t>& hints) {
    const uint32_t n = (uint32_t)es.size();
    std::vector<BufP> slots, srcs;
    std::vector<uint32_t> want(n);
    for (uint32_t i = 0; i < n; ++i) {
        const bool frame = es[i].kind == LZ4E_PACK_FRAME;
        slots.emplace_back(new Buf(es[i].frame_align, frame ? es[i].len : 0));
        srcs.emplace_back(new Buf(es[i].src_align, frame ? 0 : es[i].len));
        slots[i]->fill_random();
        srcs[i]->fill_random();
        want[i] = frame ? ref_crc(slots[i]->p, es[i].len) : ref_crc(srcs[i]->p, es[i].len);
    }
    const uint8_t* frames = lowest(slots);
    const uint8_t* src = lowest(srcs);
    Buf fr_off(0, 8 * (size_t)n), src_off(0, 8 * (size_t)n), pk_len(0, 4 * (size_t)n), pk_kind(0, n);
    for (uint32_t i = 0; i < n; ++i) {
        fr_off.as<uint64_t>()[i] = (uint64_t)(slots[i]->p - frames);
        src_off.as<uint64_t>()[i] = (uint64_t)(srcs[i]->p - src);
        pk_len.as<int32_t>()[i] = (int32_t)es[i].len;
        pk_kind.as<uint8_t>()[i] = es[i].kind;
    }
    for (uint32_t hint : hints) {
        Buf crc(0, 4 * (size_t)n);
        crc.fill(kFill);
        const lz4e::CrcBatch a{frames, fr_off.as<uint64_t>(), src, src_off.as<uint64_t>(), pk_kind.as<uint8_t>(),
                               pk_len.as<int32_t>(), crc.as<uint32_t>(), n, hint};
        run_crc(a, what);
        for (uint32_t i = 0; i < n; ++i)
            CHECK(crc.as<uint32_t>()[i] == want[i], "%s: hint %u, entry %u (kind %u, len %u): %08x, expected %08x", what, hint, i,
                  es[i].kind, es[i].len, crc.as<uint32_t>()[i], want[i]);
    }
    bool canaries = true;
    for (uint32_t i = 0; i < n; ++i) canaries &= slots[i]->canary_ok() && srcs[i]->canary_ok();
    CHECK(canaries, "%s: canary", what);
}

struct VEntry {
    uint8_t kind;
    int32_t len, cap;
    bool good_crc;
    bool outside;  // pk_off points outside every allocation
};
constexpr int32_t kDecoded = 424242;  // the stand-in decoder's ret for an entry it was shown

// lz4e_unpack_verified_batch_dev's composition on an image of the given
// entries (align 1): checksum, mask, stand-in decoders, raw copy, ret.
void verify_case(const char* what, const std::vector<VEntry>& es, uint32_t packed_align, uint32_t hint) {
    const uint32_t n = (uint32_t)es.size();
    const lz4e::VerifiedUnpackScratch L(n, lz4e::crc_partial_words(hint, n));  // (partial: run_crc's)
    Buf pk_off(0, 8 * ((size_t)n + 1)), pk_len(0, 4 * (size_t)n), pk_kind(0, n), pk_crc(0, 4 * (size_t)n),
        dst_off(0, 8 * (size_t)n), dst_cap(0, 4 * (size_t)n), ret(0, 4 * (size_t)n), masked(0, L.masked.bytes),
        got(0, L.got.bytes), shown(0, L.shown.bytes);
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        pk_off.as<uint64_t>()[i] = es[i].outside ? ((uint64_t)1 << 46) + i : at;
        if (!es[i].outside) at += (uint64_t)(es[i].len > 0 ? es[i].len : 0);
        pk_len.as<int32_t>()[i] = es[i].len;
        pk_kind.as<uint8_t>()[i] = es[i].kind;
        dst_cap.as<int32_t>()[i] = es[i].cap;
    }
    pk_off.as<uint64_t>()[n] = at;
    Buf packed(packed_align, at);
    packed.fill_random();
    for (uint32_t i = 0; i < n; ++i) {
        const bool readable = !es[i].outside && es[i].len >= 0;
        const uint32_t c = readable ? ref_crc(packed.p + pk_off.as<uint64_t>()[i], (size_t)es[i].len) : 0x1234567u;
        pk_crc.as<uint32_t>()[i] = es[i].good_crc ? c : c ^ (1u << (i % 32));
    }
    std::vector<BufP> dsts;
    for (uint32_t i = 0; i < n; ++i) {
        dsts.emplace_back(new Buf(i * 3, es[i].cap > 0 ? (size_t)es[i].cap : 0));
        dsts[i]->fill(kFill);
    }
    uint8_t* dst = const_cast<uint8_t*>(lowest(dsts));
    for (uint32_t i = 0; i < n; ++i) dst_off.as<uint64_t>()[i] = (uint64_t)(dsts[i]->p - dst);
    got.fill(kFill);
    masked.fill(kFill);
    shown.fill(kFill);
    const lz4e::CrcBatch c{packed.p, pk_off.as<uint64_t>(), packed.p, pk_off.as<uint64_t>(), pk_kind.as<uint8_t>(),
                           pk_len.as<int32_t>(), got.as<uint32_t>(), n, hint};
    run_crc(c, what);
    CHECK(lz4e::launch_unpack_verify_mask(pk_len.as<int32_t>(), pk_kind.as<uint8_t>(), pk_crc.as<uint32_t>(),
                                          got.as<uint32_t>(), n, masked.as<int32_t>(), shown.as<uint8_t>(),
                                          nullptr) == hipSuccess,
          "%s: mask launch", what);
    for (uint32_t i = 0; i < n; ++i)  // the decoders: -1 for srcSize 0 before they read or write anything
        ret.as<int32_t>()[i] = masked.as<int32_t>()[i] == 0 ? -1 : kDecoded;
    const lz4e::UnpackRawBatch r{packed.p, pk_off.as<uint64_t>(), pk_len.as<int32_t>(), shown.as<uint8_t>(), dst,
                                 dst_off.as<uint64_t>(), dst_cap.as<int32_t>(), ret.as<int32_t>(), n, hint};
    CHECK(lz4e::launch_unpack_raw(r, nullptr) == hipSuccess, "%s: raw launch", what);
    CHECK(lz4e::launch_unpack_verify_ret(shown.as<uint8_t>(), n, ret.as<int32_t>(), nullptr) == hipSuccess, "%s: ret launch",
          what);
    for (uint32_t i = 0; i < n; ++i) {
        const VEntry& e = es[i];
        const int32_t m = masked.as<int32_t>()[i], rr = ret.as<int32_t>()[i];
        const bool valid = (e.kind == LZ4E_PACK_FRAME || e.kind == LZ4E_PACK_RAW) && e.len >= 0;
        if (!valid) {
            CHECK(rr == -1 && m == 0 && dsts[i]->all(kFill), "%s: invalid entry %u (kind %u, len %d): ret %d, masked %d", what, i,
                  e.kind, e.len, rr, m);
        } else if (!e.good_crc) {
            CHECK(rr == LZ4E_UNPACK_BAD_CRC && m == 0 && dsts[i]->all(kFill), "%s: entry %u with a wrong checksum (kind %u, len %d, cap %d): ret %d, masked %d",
                  what, i, e.kind, e.len, e.cap, rr, m);
        } else if (e.kind == LZ4E_PACK_FRAME) {
            CHECK(m == e.len && rr == (e.len ? kDecoded : -1) && dsts[i]->all(kFill), "%s: clean frame entry %u (len %d): ret %d, masked %d",
                  what, i, e.len, rr, m);
        } else if (e.len <= e.cap) {
            bool good = rr == e.len && m == 0 && (e.len == 0 || memcmp(dsts[i]->p, packed.p + pk_off.as<uint64_t>()[i], (size_t)e.len) == 0);
            for (size_t k = (size_t)e.len; k < dsts[i]->n; ++k) good &= dsts[i]->p[k] == kFill;
            CHECK(good, "%s: clean raw entry %u (len %d, cap %d): ret %d", what, i, e.len, e.cap, rr);
        } else {
            CHECK(rr == -1 && m == 0 && dsts[i]->all(kFill), "%s: raw entry %u over capacity (len %d, cap %d): ret %d", what, i, e.len,
                  e.cap, rr);
        }
        CHECK(dsts[i]->canary_ok(), "%s: bytes before destination %u written", what, i);
    }
    CHECK(packed.canary_ok(), "%s: packed canary", what);
}

const int32_t kLens[] = {0, 1, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 511, 512, 4096, 4097, 70000};
constexpr uint32_t kSmallLens = 13;  // 0 ... 65

// ---- the verified range read (`emu_crc rangev`) ----
enum Damage { kClean, kWrongCrc, kFlipFirst, kFlipLast };
struct REntry {
    uint8_t kind;
    int32_t len;
    Damage damage;
    bool outside;  // pk_off points outside every allocation: the entry must not be read
};
struct RReq {
    uint32_t sel;
    int32_t lo, len;
};

// lz4e_unpack_range_verified_batch_dev's composition, launch for launch as
// lz4e_host.hip issues it, once per hint.  Every entry is an allocation of its
// own (exactly pk_len bytes), every scratch array one of exactly the size
// lz4e_store_scratch.h states, every destination one of exactly the bytes its request must
// get.  The decoders' part is played by a stand-in that takes a frame's bytes
// for its data: -1 for a length of 0 before it reads or writes anything, else
// the first min(length, target) bytes into the request's slot.  Expected
// values: ref_crc and the plain loop below.
void rangev_case(const char* what, const std::vector<REntry>& es, const std::vector<RReq>& rq, bool null_sel,
                 uint32_t max_end, const std::vector<uint32_t>& hints) {
    const uint32_t n = (uint32_t)es.size(), m = (uint32_t)rq.size();
    std::vector<BufP> ents;
    for (uint32_t i = 0; i < n; ++i) {
        ents.emplace_back(new Buf(i * 7 + 1, !es[i].outside && es[i].len > 0 ? (size_t)es[i].len : 0));
        ents[i]->fill_random();
    }
    const uint8_t* packed = lowest(ents);
    Buf pk_off(0, 8 * ((size_t)n + 1)), pk_len(0, 4 * (size_t)n), pk_kind(0, n), pk_crc(0, 4 * (size_t)n);
    std::vector<bool> damaged(n);
    for (uint32_t i = 0; i < n; ++i) {
        const REntry& e = es[i];
        pk_off.as<uint64_t>()[i] = e.outside ? ((uint64_t)1 << 46) + i : (uint64_t)(ents[i]->p - packed);
        pk_len.as<int32_t>()[i] = e.len;
        pk_kind.as<uint8_t>()[i] = e.kind;
        uint32_t c = e.outside ? 0x1234567u : ref_crc(ents[i]->p, ents[i]->n);
        damaged[i] = e.damage != kClean;
        if (e.damage == kWrongCrc || ents[i]->n == 0) {
            if (damaged[i]) c ^= 1u << (i % 32);
        } else if (e.damage == kFlipFirst) {
            ents[i]->p[0] ^= 0x01;
        } else if (e.damage == kFlipLast) {
            ents[i]->p[ents[i]->n - 1] ^= 0x80;
        }
        pk_crc.as<uint32_t>()[i] = c;
    }
    pk_off.as<uint64_t>()[n] = 0;
    // the requests and what each must get
    Buf sel(0, 4 * (size_t)m), lo(0, 4 * (size_t)m), len(0, 4 * (size_t)m);
    std::vector<int32_t> want(m);
    std::vector<int64_t> count(m);  // bytes delivered; -1: rule 1, -2: rule 2, -3: rule 3
    std::vector<bool> wanted(n);
    for (uint32_t j = 0; j < m; ++j) {
        const RReq& q = rq[j];
        if (null_sel && q.sel != j) abort();
        sel.as<uint32_t>()[j] = q.sel;
        lo.as<int32_t>()[j] = q.lo;
        len.as<int32_t>()[j] = q.len;
        const bool valid = q.sel < n && q.lo >= 0 && q.len >= 0 &&
                           (es[q.sel].kind == LZ4E_PACK_FRAME || es[q.sel].kind == LZ4E_PACK_RAW) && es[q.sel].len >= 0;
        if (!valid) {
            want[j] = -1, count[j] = -1;
        } else if (q.len == 0) {
            want[j] = 0, count[j] = -2;
        } else {
            const REntry& e = es[q.sel];
            if (e.outside) abort();  // a mistake in the case: this request reads the entry
            wanted[q.sel] = true;
            const uint64_t end = std::min<uint64_t>((uint64_t)q.lo + (uint64_t)q.len, max_end);
            const int64_t d = (int64_t)std::min<uint64_t>((uint64_t)e.len, end);
            const int64_t cnt = e.kind == LZ4E_PACK_FRAME && e.len == 0 ? -1 : d > q.lo ? d - q.lo : 0;
            if (damaged[q.sel]) want[j] = LZ4E_UNPACK_BAD_CRC, count[j] = -3;
            else want[j] = (int32_t)cnt, count[j] = cnt < 0 ? 0 : cnt;
        }
    }
    uint32_t nwanted = 0;
    for (uint32_t i = 0; i < n; ++i) nwanted += wanted[i];
    const uint64_t slot = lz4e::RangeScratch(m, max_end).slot;
    for (uint32_t hint : hints) {
        std::vector<BufP> dsts;
        for (uint32_t j = 0; j < m; ++j) {
            // a refused request's slot is what a plain read might have written
            const size_t sz = count[j] >= 0 ? (size_t)count[j] : (size_t)std::min<int64_t>(std::max(rq[j].len, 0), 512);
            dsts.emplace_back(new Buf(j * 3 + 2, sz));
            dsts[j]->fill(kFill);
        }
        uint8_t* dst = const_cast<uint8_t*>(lowest(dsts));
        Buf dst_off(0, 8 * (size_t)m), ret(0, 4 * (size_t)m);
        for (uint32_t j = 0; j < m; ++j) dst_off.as<uint64_t>()[j] = (uint64_t)(dsts[j]->p - dst);
        const uint64_t words = lz4e::crc_partial_words(hint, m);
        const lz4e::RangeScratch L(m, max_end, true, n, words);
        Buf slots(0, L.slots.bytes), g_off(0, L.g_off.bytes), s_off(0, L.s_off.bytes), c_off(0, L.c_off.bytes),
            g_len(0, L.g_len.bytes), g_tgt(0, L.g_tgt.bytes), g_ret(0, L.g_ret.bytes), c_len(0, L.c_len.bytes),
            got(0, L.got.bytes), owner(0, L.owner.bytes), partial(0, L.partial.bytes), shown(0, L.shown.bytes);
        for (Buf* b : {&ret, &slots, &g_off, &s_off, &c_off, &g_len, &g_tgt, &g_ret, &c_len, &got, &owner, &partial, &shown})
            b->fill(kFill);
        const uint32_t* selp = null_sel ? nullptr : sel.as<uint32_t>();
        const lz4e::RangeVerifyBatch v{pk_off.as<uint64_t>(), pk_len.as<int32_t>(), pk_kind.as<uint8_t>(),
                                       pk_crc.as<uint32_t>(), n, selp, lo.as<int32_t>(), len.as<int32_t>(),
                                       ret.as<int32_t>(), m, owner.as<uint32_t>(), shown.as<uint8_t>(),
                                       c_off.as<uint64_t>(), c_len.as<int32_t>(), got.as<uint32_t>()};
        const lz4e::CrcBatch c{packed, c_off.as<uint64_t>(), nullptr, nullptr, nullptr, c_len.as<int32_t>(),
                               got.as<uint32_t>(), m, hint};
        const lz4e::RangeBatch r{packed, pk_off.as<uint64_t>(), pk_len.as<int32_t>(), shown.as<uint8_t>(), n, selp,
                                 lo.as<int32_t>(), len.as<int32_t>(), dst, dst_off.as<uint64_t>(), ret.as<int32_t>(), m,
                                 max_end, slot, slots.p, g_off.as<uint64_t>(), g_len.as<int32_t>(), g_tgt.as<int32_t>(),
                                 s_off.as<uint64_t>(), g_ret.as<int32_t>()};
        CHECK(lz4e::launch_range_verify_init(v, nullptr) == hipSuccess, "%s: init launch", what);
        CHECK(lz4e::launch_range_verify_elect(v, nullptr) == hipSuccess, "%s: elect launch", what);
        CHECK(lz4e::launch_crc(c, words ? partial.as<uint32_t>() : nullptr, nullptr) == hipSuccess, "%s: crc launch", what);
        CHECK(lz4e::launch_range_verify_verdict(v, nullptr) == hipSuccess, "%s: verdict launch", what);
        CHECK(lz4e::launch_range_gather(r, nullptr) == hipSuccess, "%s: gather launch", what);
        for (uint32_t j = 0; j < m; ++j) {  // the decoders
            const int32_t fl = g_len.as<int32_t>()[j], tgt = g_tgt.as<int32_t>()[j];
            if (fl == 0) {
                g_ret.as<int32_t>()[j] = -1;
                continue;
            }
            const int32_t d = fl < tgt ? fl : tgt;
            memcpy(slots.p + s_off.as<uint64_t>()[j], packed + g_off.as<uint64_t>()[j], (size_t)d);
            g_ret.as<int32_t>()[j] = d;
        }
        CHECK(lz4e::launch_range_deliver(r, nullptr) == hipSuccess, "%s: deliver launch", what);
        CHECK(lz4e::launch_range_verify_ret(v, nullptr) == hipSuccess, "%s: ret launch", what);
        // once per entry: one owner per wanted entry describes it to the checksum, nobody else describes anything
        uint32_t nowners = 0;
        for (uint32_t j = 0; j < m; ++j) {
            const bool owns = count[j] != -1 && count[j] != -2 && owner.as<uint32_t>()[rq[j].sel] == j;
            nowners += owns;
            const int32_t cl = c_len.as<int32_t>()[j];
            CHECK(cl == (owns ? es[rq[j].sel].len : 0), "%s: hint %u, request %u describes %d bytes to the checksum", what, hint,
                  j, cl);
        }
        CHECK(nowners == nwanted, "%s: hint %u: %u owners for %u wanted entries", what, hint, nowners, nwanted);
        for (uint32_t j = 0; j < m; ++j) {
            const int32_t rr = ret.as<int32_t>()[j];
            bool good = rr == want[j];
            if (count[j] > 0) good &= memcmp(dsts[j]->p, ents[rq[j].sel]->p + rq[j].lo, (size_t)count[j]) == 0;
            else good &= dsts[j]->all(kFill);
            CHECK(good, "%s: hint %u, request %u of %u (entry %u, lo %d, len %d; kind %u, len %d, damage %d): ret %d, expected %d%s",
                  what, hint, j, m, rq[j].sel, rq[j].lo, rq[j].len, rq[j].sel < n ? es[rq[j].sel].kind : 999,
                  rq[j].sel < n ? es[rq[j].sel].len : -999, rq[j].sel < n ? (int)es[rq[j].sel].damage : -1, rr, want[j],
                  rr == want[j] ? ", wrong bytes" : "");
            CHECK(dsts[j]->canary_ok(), "%s: bytes before destination %u written", what, j);
        }
    }
    for (uint32_t i = 0; i < n; ++i) CHECK(ents[i]->canary_ok(), "%s: canary of entry %u", what, i);
}

std::vector<RReq> shuffled(std::vector<RReq> rq) {
    for (size_t k = rq.size(); k > 1; --k) std::swap(rq[k - 1], rq[rnd32() % k]);
    return rq;
}

int rangev_main() {
    layout_sweep();
    const int32_t lens[] = {0, 1, 15, 16, 17, 300, 4097, 70000};
    // ---- every length, frame and raw, clean and damaged in each way; entries nobody reads and entries
    //      no one may read; three hints on the same batch ----
    {
        std::vector<REntry> es;
        uint32_t k = 0;
        for (int32_t l : lens)
            for (uint8_t kind : {LZ4E_PACK_FRAME, LZ4E_PACK_RAW}) {
                es.push_back({kind, l, kClean, false});
                es.push_back({kind, l, l == 0 ? kWrongCrc : (Damage)(kWrongCrc + k++ % 3), false});
            }
        const uint32_t named = (uint32_t)es.size();
        es.push_back({LZ4E_PACK_FRAME, 4097, kClean, true});     // named by nobody
        es.push_back({LZ4E_PACK_RAW, 300, kWrongCrc, true});     // named by len == 0 requests only
        es.push_back({2, 300, kClean, true});                    // unknown kinds and negative lengths
        es.push_back({255, 17, kWrongCrc, true});
        es.push_back({LZ4E_PACK_RAW, -5, kClean, true});
        es.push_back({LZ4E_PACK_FRAME, -70000, kWrongCrc, true});
        // `all`: five ranges of every named entry; `one`: one of the five, a different one from entry to entry
        std::vector<RReq> all, one;
        for (uint32_t e = 0; e < named; ++e) {
            const int32_t l = es[e].len;
            const RReq five[5] = {{e, 0, l + 1}, {e, l / 2, 4096}, {e, 0, 0}, {e, l, 5}, {e, l > 0 ? l - 1 : 0, 1}};
            for (const RReq& q : five) all.push_back(q);
            one.push_back(five[(e / 4) % 2]);
        }
        for (std::vector<RReq>* rq : {&all, &one}) {
            for (uint32_t e = named + 1; e < es.size(); ++e) {
                rq->push_back({e, 0, 0});
                rq->push_back({e, 7, 0});
                if (e > named + 1) rq->push_back({e, 0, 16});
            }
            rq->push_back({3, -1, 16});  // invalid requests on a damaged entry, and past the index
            rq->push_back({3, 1, -16});
            rq->push_back({(uint32_t)es.size(), 0, 16});
            rq->push_back({0xFFFFFFFFu, 0, 0});
        }
        // (the last hint puts 64 workgroups on every request, so that batch has one request per entry)
        rangev_case("lengths", es, shuffled(one), false, 70001 + 4096, {1u, 70000u, kHugeHint});
        rangev_case("ranges", es, shuffled(all), false, 70001 + 4096, {4096u});
        // the same with a max_end that clamps the long requests
        rangev_case("clamped", es, shuffled(all), false, 4000, {0u});
    }
    // ---- 1, 2, 17 and 300 requests on one entry, interleaved with as many on a damaged one ----
    for (uint32_t k : {1u, 2u, 17u, 300u}) {
        const std::vector<REntry> es = {{LZ4E_PACK_FRAME, 4097, kClean, false},
                                        {LZ4E_PACK_RAW, 300, kFlipLast, false},
                                        {LZ4E_PACK_RAW, 17, kClean, false},
                                        {LZ4E_PACK_FRAME, 512, kFlipFirst, false}};
        std::vector<RReq> rq;
        for (uint32_t i = 0; i < k; ++i) {
            rq.push_back({0, (int32_t)(13 * i), (int32_t)(40 + i)});
            rq.push_back({1, (int32_t)i, i % 3 ? 64 : 0});  // every third of them reads nothing: 0, not BAD_CRC
            if (i % 5 == 0) rq.push_back({2, (int32_t)(i % 20), 9});
            if (i % 7 == 0) rq.push_back({3, 0, (int32_t)(1 + i)});
        }
        // (two workgroups to a request where the batch is small enough for the emulator)
        rangev_case("fan-in", es, rq, false, 4200, k <= 17 ? std::vector<uint32_t>{4096u, 64u << 9} : std::vector<uint32_t>{4096u});
    }
    // ---- index sizes around a workgroup, null sel and a given one with repeats ----
    for (uint32_t n : {1u, 255u, 256u, 257u})
        for (int mode = 0; mode < 3; ++mode) {
            std::vector<REntry> es;
            const uint32_t m = mode == 1 && n > 1 ? n - 1 : n;  // mode 1: the last entry is named by nobody
            for (uint32_t i = 0; i < n; ++i) {
                const int32_t l = (int32_t)(rnd32() % 41);
                const uint8_t kind = (i & 1) ? LZ4E_PACK_RAW : LZ4E_PACK_FRAME;
                if (i >= m || i % 11 == 10) es.push_back({i % 22 == 10 ? (uint8_t)2 : kind, i % 3 ? l : -l - 1, kClean, true});
                else es.push_back({kind, l, i % 5 == 4 ? (l && (i & 8) ? kFlipFirst : kWrongCrc) : kClean, false});
            }
            std::vector<RReq> rq;
            for (uint32_t j = 0; j < m; ++j) {
                uint32_t e = mode == 2 ? rnd32() % n : j;
                const bool readable = !es[e].outside;
                rq.push_back({e, (int32_t)(rnd32() % 8), readable ? (int32_t)(rnd32() % 48) : 0});
            }
            if (n > 1 && mode == 1) es[n - 1] = {LZ4E_PACK_RAW, 33, kWrongCrc, true};
            rangev_case(mode == 2 ? "index sizes, sel" : "index sizes, null sel", es, rq, mode != 2, 64,
                        n == 257 && mode == 0 ? std::vector<uint32_t>{1u, 64u << 9} : std::vector<uint32_t>{1u});
        }
    // ---- no request at all: nothing is launched ----
    {
        const uint64_t before = g_groups_run;
        rangev_case("no request", {{LZ4E_PACK_RAW, 300, kWrongCrc, true}}, {}, false, 64, {0u, 70000u});
        rangev_case("no request, no entry", {}, {}, true, 0, {1u});
        CHECK(g_groups_run == before, "no request: the checksum kernel ran");
    }
    fprintf(stderr, "emu_crc rangev: %llu workgroups of crc_team_kernel\n", (unsigned long long)g_groups_run);
    return emu_finish("emu_crc rangev");
}

}  // namespace

// No default: lz4e_pack.hip's other kernels (the pack scan among them) are not run here.
const EmuKernelMode emu_modes[] = {
    {"crc_team_kernel", kEmuPool},                {"crc_combine_kernel", kEmuSerial},
    {"unpack_verify_mask_kernel", kEmuSerial},    {"unpack_verify_ret_kernel", kEmuSerial},
    {"range_verify_init_kernel", kEmuSerial},     {"range_verify_elect_kernel", kEmuSerial},
    {"range_verify_verdict_kernel", kEmuSerial},  {"range_verify_ret_kernel", kEmuSerial},
    {"unpack_raw_kernel", kEmuSerial},            {"range_gather_kernel", kEmuSerial},
    {"range_deliver_kernel", kEmuSerial},         {nullptr, kEmuNone}};

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "rangev") == 0) return rangev_main();
    layout_sweep();
    {  // the restatement itself
        const uint8_t nine[] = {'1', '2', '3', '4', '5', '6', '7', '8', '9'};
        uint8_t z[32] = {0};
        CHECK(ref_crc(nine, 9) == 0xE3069283u && ref_crc(z, 32) == 0x8A9136AAu && ref_crc(z, 0) == 0, "ref_crc");
    }
    // ---- every length, three hints on the same batch ----
    {
        std::vector<CEntry> es;
        uint32_t k = 0;
        for (int32_t len : kLens) es.push_back({len, (5 * k++ + 3) & 15});
        es.push_back({-7, 0});  // a negative length reads nothing
        crc_case("lengths", es, {1u, 70000u, kHugeHint});
    }
    // ---- every start residue for the lengths up to 65; the last hint splits them over workgroups ----
    {
        std::vector<CEntry> es;
        for (uint32_t li = 0; li < kSmallLens; ++li)
            for (uint32_t a = 0; a < 16; ++a) es.push_back({kLens[li], a});
        crc_case("residues", es, {1u, 65u, 4096u, 64u << 9});
    }
    // ---- every team size: one byte under, at and over one vector per thread, the hint's 64 bytes per
    //      thread, a wave's 64 threads busy and a workgroup's 256 ----
    for (uint32_t shift = 4; shift <= 14; ++shift) {
        const uint32_t nt = 1u << shift, hint = 64u << shift;
        if (lz4e::crc_team_shift(hint, 1) != shift) {
            CHECK(false, "team shift %u is not what hint %u picks", shift, hint);
            continue;
        }
        std::vector<CEntry> es;
        uint32_t k = shift;
        for (uint32_t at : {16 * nt, 64 * nt, 16u * 64, 64u * 64, 16u * 256, 64u * 256, 80u * 256})
            for (int32_t d = -1; d <= 1; ++d)
                if (at <= 64 * nt) es.push_back({(int32_t)at + d, (7 * k++) & 15});
        crc_case("team sizes", es, {hint});
    }
    // ---- the same bytes with different neighbours ----
    context_case(1000, 1000);
    context_case(33, 1);
    context_case(5000, 64u << 10);
    // ---- entry counts: none, one, around a workgroup's 16, 4, 2 and 1 entries ----
    for (uint32_t hint : {1u, 64u << 6, 64u << 7, 64u << 8, 64u << 9})
        for (uint32_t n : {0u, 1u, 2u, 3u, 4u, 5u, 15u, 16u, 17u, 33u}) {
            std::vector<CEntry> es;
            for (uint32_t i = 0; i < n; ++i) es.push_back({(int32_t)(rnd32() % 41), rnd32() & 15});
            crc_case("counts", es, {hint});
        }
    // ---- pack_crc: frame and raw entries; the other side of each is 0 bytes long ----
    {
        std::vector<PEntry> es;
        uint32_t k = 0;
        for (int32_t len : kLens) {
            if (len) es.push_back({LZ4E_PACK_FRAME, (uint32_t)len, (k * 3 + 1) & 15, (k * 7) & 15});
            es.push_back({LZ4E_PACK_RAW, (uint32_t)len, (k * 5) & 15, (k * 11 + 5) & 15});
            ++k;
        }
        pack_crc_case("pack_crc", es, {1u, 70000u, 64u << 9});
    }
    // ---- verified unpack: mask, raw copy and ret ----
    for (uint32_t hint : {4096u, 64u << 9}) {
        std::vector<VEntry> es;
        for (int32_t len : {0, 1, 17, 512, 4097}) {
            es.push_back({LZ4E_PACK_FRAME, len, len + 40, true, false});   // clean
            es.push_back({LZ4E_PACK_RAW, len, len, true, false});
            es.push_back({LZ4E_PACK_FRAME, len, len + 40, false, false});  // a wrong pk_crc
            es.push_back({LZ4E_PACK_RAW, len, len + 9, false, false});
            es.push_back({LZ4E_PACK_RAW, len + 1, len, true, false});      // over capacity, good and bad checksum
            es.push_back({LZ4E_PACK_RAW, len + 1, len, false, false});
            es.push_back({2, len, len + 40, true, true});                  // unknown kinds and a negative length:
            es.push_back({255, len, len, false, true});                    // the offset points nowhere
            es.push_back({LZ4E_PACK_RAW, -5 - len, 64, true, true});
            es.push_back({LZ4E_PACK_FRAME, -1 - len, 64, false, true});
        }
        verify_case("verify", es, hint == 4096u ? 0 : 11, hint);
    }
    verify_case("verify, no entry", {}, 0, 4096);
    fprintf(stderr, "emu_crc: %llu workgroups of crc_team_kernel\n", (unsigned long long)g_groups_run);
    return emu_finish("emu_crc");
}
