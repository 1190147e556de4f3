// Lane emulator of the packed frame store's kernels (debug/test tooling,
// tools/emu): compiles the unmodified csrc/lz4e_pack.hip as host C++ and runs
// the four pack kernels, unpack_mask_kernel and unpack_raw_kernel lane by
// lane, under the same emulated <hip/hip_runtime.h> as the other
// kernel files (the decoders that run between the two unpack kernels are
// emu_main's business).  Stand-alone (its own main): built by
// EMU_PACK=1 build.sh, run by tests/test_emulator_pack.py under ASan + UBSan.
// `emu_pack range` runs the range read's two kernels instead
// (range_gather_kernel, range_deliver_kernel; tests/test_emulator_partial.py):
// the partial launch between them is played by the program, which fills the
// scratch slots and the decode values itself.
//
// The kernels work on the CALLER's memory at byte granularity.  So every
// frame slot, every source block, `packed`, every unpack destination and
// every index array here is its own heap allocation that ends exactly at the
// last byte the contract allows (ASan's redzone follows it), placed at a
// chosen alignment mod 16 with a poisoned prefix and a canary (emu_harness.h,
// Buf).  A frame entry's source and a raw entry's frame slot are allocations
// of 0 bytes: reading them at all is a report.
//
// The scan kernels use cross-lane operations and workgroup barriers, so they
// run on the harness's pool of lane threads (the one-wave scan of the tile
// sums on 64 of them); the copy, mask and raw-copy kernels and the range
// read's two have neither, so their lanes run one after the other on the
// calling thread: the table next to main.
#include "emu_harness.h"
#undef __shared__
#define __shared__ static

#include "lz4e_pack.hip"

#include "lz4e.h"
#include "lz4e_store_scratch.h"

uint32_t g_rng = 2463534242u;
uint32_t rnd32() { return emu_lcg(g_rng) >> 8; }
uint8_t rnd() { return (uint8_t)rnd32(); }

namespace {

struct Entry {
    uint32_t src_len;
    int32_t ret;
    uint32_t src_align, frame_align;
};
Entry frame_of(uint32_t len, uint32_t sa = 0, uint32_t fa = 0) {  // len >= 1
    return Entry{len + 1 + rnd32() % 7, (int32_t)len, sa, fa};
}
Entry raw_of(uint32_t len, uint32_t sa = 0, uint32_t fa = 0) {
    // a failed compress, a frame as large as the input, a larger one, a negative ret
    const int32_t rets[4] = {0, (int32_t)len, (int32_t)len + 5, -3};
    return Entry{len, rets[rnd32() % 4], sa, fa};
}

enum Cap { kCapExact, kCapOneShort, kCapZero };

// One lz4e_pack_batch_dev against its restatement in plain C.
void pack_case(const char* what, const std::vector<Entry>& es, uint32_t align, uint32_t packed_align, Cap cap) {
    const uint32_t n = (uint32_t)es.size();
    // ---- the restatement ----
    std::vector<uint64_t> want_off(n + 1);
    std::vector<int32_t> want_len(n);
    std::vector<uint8_t> want_kind(n);
    uint64_t at = 0;
    uint32_t max_len = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const bool frame = es[i].ret > 0 && (uint32_t)es[i].ret < es[i].src_len;
        want_kind[i] = frame ? LZ4E_PACK_FRAME : LZ4E_PACK_RAW;
        want_len[i] = frame ? es[i].ret : (int32_t)es[i].src_len;
        want_off[i] = at;
        at += ((uint64_t)want_len[i] + align - 1) / align * align;
        if (es[i].src_len > max_len) max_len = es[i].src_len;
    }
    want_off[n] = at;
    const uint64_t total = at;
    // ---- the batch: what an entry's kind does not read is 0 bytes long ----
    std::vector<BufP> slots, srcs;
    for (uint32_t i = 0; i < n; ++i) {
        const bool frame = want_kind[i] == LZ4E_PACK_FRAME;
        slots.emplace_back(new Buf(es[i].frame_align, frame ? (size_t)es[i].ret : 0));
        srcs.emplace_back(new Buf(es[i].src_align, frame ? 0 : es[i].src_len));
        slots[i]->fill_random();
        srcs[i]->fill_random();
    }
    const uint8_t* frames = lowest(slots);
    const uint8_t* src = lowest(srcs);
    Buf fr_off(0, 8 * (size_t)n), src_off(0, 8 * (size_t)n), ret(0, 4 * (size_t)n), src_len(0, 4 * (size_t)n);
    Buf pk_off(0, 8 * ((size_t)n + 1)), pk_len(0, 4 * (size_t)n), pk_kind(0, n);
    for (uint32_t i = 0; i < n; ++i) {
        fr_off.as<uint64_t>()[i] = (uint64_t)(slots[i]->p - frames);
        src_off.as<uint64_t>()[i] = (uint64_t)(srcs[i]->p - src);
        ret.as<int32_t>()[i] = es[i].ret;
        src_len.as<uint32_t>()[i] = es[i].src_len;
    }
    pk_off.fill(kFill);
    pk_len.fill(kFill);
    pk_kind.fill(kFill);
    std::vector<uint8_t> image(total, 0);
    for (uint32_t i = 0; i < n; ++i)
        if (want_len[i])
            memcpy(image.data() + want_off[i], want_kind[i] == LZ4E_PACK_FRAME ? slots[i]->p : srcs[i]->p,
                   (size_t)want_len[i]);
    const uint64_t packed_cap = cap == kCapExact ? total : (cap == kCapOneShort && total ? total - 1 : 0);
    const bool fits = total <= packed_cap;
    Buf packed(packed_align, packed_cap);
    packed.fill(kFill);
    // ---- the kernels ----
    const lz4e::PackBatch a{frames, fr_off.as<uint64_t>(), ret.as<int32_t>(), src, src_off.as<uint64_t>(),
                            src_len.as<uint32_t>(), packed.p, packed_cap, align, pk_off.as<uint64_t>(),
                            pk_len.as<int32_t>(), pk_kind.as<uint8_t>(), n, max_len};
    CHECK(lz4e::launch_pack(a, nullptr) == hipSuccess, "%s: launch", what);
    bool index_ok = memcmp(pk_off.p, want_off.data(), pk_off.n) == 0;
    if (n) index_ok &= memcmp(pk_len.p, want_len.data(), pk_len.n) == 0 && memcmp(pk_kind.p, want_kind.data(), n) == 0;
    CHECK(index_ok, "%s: index (n %u, align %u)", what, n, align);
    if (fits)
        CHECK(total == 0 || memcmp(packed.p, image.data(), total) == 0, "%s: image (n %u, align %u, packed at %u mod 16)",
              what, n, align, packed_align);
    else
        CHECK(packed.all(kFill), "%s: packed written although %llu > cap %llu", what, (unsigned long long)total,
              (unsigned long long)packed_cap);
    bool canaries = packed.canary_ok();
    for (uint32_t i = 0; i < n; ++i) canaries &= slots[i]->canary_ok() && srcs[i]->canary_ok();
    CHECK(canaries, "%s: canary (n %u)", what, n);
}

struct UEntry {
    uint8_t kind;
    int32_t len, cap;
    uint32_t dst_align;
};

// unpack_mask_kernel and unpack_raw_kernel on an image of the given entries
// (align 1), `packed` at packed_align mod 16.
void unpack_case(const char* what, const std::vector<UEntry>& es, uint32_t packed_align) {
    const uint32_t n = (uint32_t)es.size();
    constexpr int32_t kUntouched = -7777;
    Buf pk_off(0, 8 * ((size_t)n + 1)), pk_len(0, 4 * (size_t)n), pk_kind(0, n), dst_off(0, 8 * (size_t)n),
        dst_cap(0, 4 * (size_t)n), ret(0, 4 * (size_t)n), masked(0, 4 * (size_t)n);
    uint64_t at = 0;
    uint32_t max_cap = 0;
    for (uint32_t i = 0; i < n; ++i) {
        pk_off.as<uint64_t>()[i] = at;
        at += (uint64_t)(es[i].len > 0 ? es[i].len : 0);
        pk_len.as<int32_t>()[i] = es[i].len;
        pk_kind.as<uint8_t>()[i] = es[i].kind;
        dst_cap.as<int32_t>()[i] = es[i].cap;
        ret.as<int32_t>()[i] = kUntouched;
        if (es[i].cap > 0 && (uint32_t)es[i].cap > max_cap) max_cap = (uint32_t)es[i].cap;
    }
    pk_off.as<uint64_t>()[n] = at;
    Buf packed(packed_align, at);
    packed.fill_random();
    std::vector<BufP> dsts;
    for (uint32_t i = 0; i < n; ++i) {
        dsts.emplace_back(new Buf(es[i].dst_align, es[i].cap > 0 ? (size_t)es[i].cap : 0));
        dsts[i]->fill(kFill);
    }
    uint8_t* dst = const_cast<uint8_t*>(lowest(dsts));
    for (uint32_t i = 0; i < n; ++i) dst_off.as<uint64_t>()[i] = (uint64_t)(dsts[i]->p - dst);
    masked.fill(kFill);
    CHECK(lz4e::launch_unpack_mask(pk_len.as<int32_t>(), pk_kind.as<uint8_t>(), n, masked.as<int32_t>(), nullptr) ==
              hipSuccess,
          "%s: mask launch", what);
    const lz4e::UnpackRawBatch a{packed.p, pk_off.as<uint64_t>(), pk_len.as<int32_t>(), pk_kind.as<uint8_t>(), dst,
                                 dst_off.as<uint64_t>(), dst_cap.as<int32_t>(), ret.as<int32_t>(), n, max_cap};
    CHECK(lz4e::launch_unpack_raw(a, nullptr) == hipSuccess, "%s: raw launch", what);
    for (uint32_t i = 0; i < n; ++i) {
        const UEntry& e = es[i];
        const int32_t m = masked.as<int32_t>()[i], r = ret.as<int32_t>()[i];
        CHECK(m == (e.kind == LZ4E_PACK_FRAME ? e.len : 0), "%s: masked[%u] = %d (kind %u, len %d)", what, i, m, e.kind,
              e.len);
        const uint8_t* from = packed.p + pk_off.as<uint64_t>()[i];
        if (e.kind == LZ4E_PACK_FRAME) {  // the decoders' entry: the raw kernel leaves it alone
            CHECK(r == kUntouched && dsts[i]->all(kFill), "%s: frame entry %u touched (ret %d)", what, i, r);
        } else if (e.kind == LZ4E_PACK_RAW && e.len >= 0 && e.len <= e.cap) {
            bool good = r == e.len && (e.len == 0 || memcmp(dsts[i]->p, from, (size_t)e.len) == 0);
            for (size_t k = (size_t)e.len; k < dsts[i]->n; ++k) good &= dsts[i]->p[k] == kFill;
            CHECK(good, "%s: raw entry %u (len %d, cap %d, dst at %u mod 16): ret %d", what, i, e.len, e.cap,
                  e.dst_align, r);
        } else {
            CHECK(r == -1 && dsts[i]->all(kFill), "%s: entry %u (kind %u, len %d, cap %d) must fail untouched: ret %d",
                  what, i, e.kind, e.len, e.cap, r);
        }
        CHECK(dsts[i]->canary_ok(), "%s: bytes before destination %u written", what, i);
    }
    CHECK(packed.canary_ok(), "%s: packed canary", what);
}

struct RReq {
    uint32_t sel;
    int32_t lo, len;
    uint32_t dst_align;
    int32_t decoded;  // frame entries: what the partial decode returns for the target (kAsTarget: min(data, target))
};
constexpr int32_t kAsTarget = 0x7FFFFFFF;

// range_gather_kernel and range_deliver_kernel on an image of the given
// entries (UEntry::cap: the bytes a frame entry decodes to).  Every
// destination is an allocation of exactly the bytes the request must get.
void range_case(const char* what, const std::vector<UEntry>& es, const std::vector<RReq>& rq, bool with_sel,
                uint32_t packed_align) {
    const uint32_t n = (uint32_t)es.size(), m = (uint32_t)rq.size();
    constexpr int32_t kUntouched = -7777;
    Buf pk_off(0, 8 * ((size_t)n + 1)), pk_len(0, 4 * (size_t)n), pk_kind(0, n);
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        pk_off.as<uint64_t>()[i] = at;
        at += (uint64_t)(es[i].len > 0 ? es[i].len : 0);
        pk_len.as<int32_t>()[i] = es[i].len;
        pk_kind.as<uint8_t>()[i] = es[i].kind;
    }
    pk_off.as<uint64_t>()[n] = at;
    Buf packed(packed_align, at);
    packed.fill_random();
    uint32_t max_end = 0;
    for (const RReq& q : rq)
        if (q.lo >= 0 && q.len >= 0 && (uint32_t)q.lo + (uint32_t)q.len > max_end) max_end = (uint32_t)q.lo + (uint32_t)q.len;
    const lz4e::RangeScratch L(m, max_end);  // lz4e_unpack_range_batch_dev's arrays, an allocation each
    const uint64_t slot = L.slot;
    Buf sel(0, 4 * (size_t)m), lo(0, 4 * (size_t)m), len(0, 4 * (size_t)m), dst_off(0, 8 * (size_t)m), ret(0, 4 * (size_t)m);
    Buf g_off(0, L.g_off.bytes), s_off(0, L.s_off.bytes), g_len(0, L.g_len.bytes), g_tgt(0, L.g_tgt.bytes),
        g_ret(0, L.g_ret.bytes), scratch(0, L.slots.bytes);
    scratch.fill_random();
    // ---- the restatement ----
    std::vector<int32_t> want(m);
    std::vector<const uint8_t*> from(m, nullptr);
    for (uint32_t j = 0; j < m; ++j) {
        const RReq& q = rq[j];
        const uint32_t e = with_sel ? q.sel : j;
        sel.as<uint32_t>()[j] = q.sel;
        lo.as<int32_t>()[j] = q.lo;
        len.as<int32_t>()[j] = q.len;
        ret.as<int32_t>()[j] = kUntouched;
        g_ret.as<int32_t>()[j] = kUntouched;
        const bool valid = e < n && q.lo >= 0 && q.len >= 0 && (es[e].kind == LZ4E_PACK_FRAME || es[e].kind == LZ4E_PACK_RAW) &&
                           es[e].len >= 0;
        if (!valid) {
            want[j] = -1;
        } else if (q.len == 0) {
            want[j] = 0;
        } else {
            const int32_t end = q.lo + q.len;
            int32_t d;
            if (es[e].kind == LZ4E_PACK_FRAME) {
                d = q.decoded == kAsTarget ? (es[e].cap < end ? es[e].cap : end) : q.decoded;
                g_ret.as<int32_t>()[j] = d;  // the partial launch's value
                from[j] = scratch.p + j * slot;
            } else {
                d = es[e].len < end ? es[e].len : end;
                from[j] = packed.p + pk_off.as<uint64_t>()[e];
            }
            want[j] = d < 0 ? d : (d > q.lo ? d - q.lo : 0);
        }
    }
    std::vector<BufP> dsts;
    for (uint32_t j = 0; j < m; ++j) {
        dsts.emplace_back(new Buf(rq[j].dst_align, want[j] > 0 ? (size_t)want[j] : 0));
        dsts[j]->fill(kFill);
    }
    uint8_t* dst = m ? const_cast<uint8_t*>(lowest(dsts)) : nullptr;
    for (uint32_t j = 0; j < m; ++j) dst_off.as<uint64_t>()[j] = (uint64_t)(dsts[j]->p - dst);
    // ---- the kernels ----
    const lz4e::RangeBatch a{packed.p, pk_off.as<uint64_t>(), pk_len.as<int32_t>(), pk_kind.as<uint8_t>(), n,
                             with_sel ? sel.as<uint32_t>() : nullptr, lo.as<int32_t>(), len.as<int32_t>(), dst,
                             dst_off.as<uint64_t>(), ret.as<int32_t>(), m, max_end, slot, scratch.p,
                             g_off.as<uint64_t>(), g_len.as<int32_t>(), g_tgt.as<int32_t>(), s_off.as<uint64_t>(),
                             g_ret.as<int32_t>()};
    CHECK(lz4e::launch_range_gather(a, nullptr) == hipSuccess, "%s: gather launch", what);
    for (uint32_t j = 0; j < m; ++j) {
        const uint32_t e = with_sel ? rq[j].sel : j;
        const bool dec = want[j] != -1 && rq[j].len > 0 && e < n && es[e].kind == LZ4E_PACK_FRAME;
        CHECK(g_off.as<uint64_t>()[j] == (dec ? pk_off.as<uint64_t>()[e] : 0) &&
                  g_len.as<int32_t>()[j] == (dec ? es[e].len : 0) &&
                  g_tgt.as<int32_t>()[j] == (dec ? rq[j].lo + rq[j].len : 0) && s_off.as<uint64_t>()[j] == j * slot,
              "%s: descriptors of request %u", what, j);
    }
    CHECK(lz4e::launch_range_deliver(a, nullptr) == hipSuccess, "%s: deliver launch", what);
    for (uint32_t j = 0; j < m; ++j) {
        const int32_t r = ret.as<int32_t>()[j];
        bool good = r == want[j];
        if (good && r > 0) good = memcmp(dsts[j]->p, from[j] + rq[j].lo, (size_t)r) == 0;
        CHECK(good, "%s: request %u (sel %u, lo %d, len %d, dst at %u mod 16): ret %d, want %d", what, j, rq[j].sel,
              rq[j].lo, rq[j].len, rq[j].dst_align, r, want[j]);
        CHECK(dsts[j]->canary_ok(), "%s: bytes before destination %u written", what, j);
    }
    CHECK(packed.canary_ok(), "%s: packed canary", what);
}

int range_main() {
    // entries: a frame of 300 bytes that decodes to 1000, a raw entry of 777 bytes, an empty raw entry, an
    // unknown kind, a negative length, a frame that decodes to 40 bytes
    const std::vector<UEntry> es = {{LZ4E_PACK_FRAME, 300, 1000, 0}, {LZ4E_PACK_RAW, 777, 0, 0}, {LZ4E_PACK_RAW, 0, 0, 0},
                                    {7, 50, 50, 0},                   {LZ4E_PACK_RAW, -4, 0, 0},  {LZ4E_PACK_FRAME, 33, 40, 0}};
    for (uint32_t pa : {0u, 5u, 11u}) {
        // lo and len at every residue pair mod 16, one entry of each kind, destinations at every residue
        for (uint32_t e : {0u, 1u}) {
            std::vector<RReq> rq;
            for (int32_t lo = 0; lo < 16; ++lo)
                for (int32_t ln = 0; ln < 16; ++ln) {
                    rq.push_back({e, lo + 16 * (ln & 3), ln, (uint32_t)(lo * 5 + ln) & 15, kAsTarget});
                    rq.push_back({e, lo, ln + 16 * (1 + (lo & 7)), (uint32_t)(lo + 3 * ln) & 15, kAsTarget});
                }
            range_case("residues", es, rq, true, pa);
        }
        // around the entry's end, past it, errors of the decode, invalid requests, repeated and permuted sel
        std::vector<RReq> rq;
        for (uint32_t e : {0u, 1u, 5u}) {
            const int32_t n = es[e].kind == LZ4E_PACK_FRAME ? es[e].cap : es[e].len;
            for (int32_t lo : {0, 1, n / 2, n - 1, n, n + 5})
                for (int32_t ln : {0, 1, 17, n, n + 9}) rq.push_back({e, lo, ln, (uint32_t)(lo + ln) & 15, kAsTarget});
        }
        rq.push_back({0, 10, 100, 3, -57});            // a damaged frame: the decode's error code
        rq.push_back({0, 900, 200, 3, 950});           // a decode that ends before the target
        rq.push_back({0, 990, 10, 3, 500});            // ... and before lo
        for (uint32_t e : {2u, 3u, 4u, 6u, 0xFFFFFFFFu}) rq.push_back({e, 0, 16, 1, kAsTarget});
        rq.push_back({1, -1, 16, 1, kAsTarget});
        rq.push_back({1, 3, -16, 1, kAsTarget});
        rq.push_back({3, 0, 0, 1, kAsTarget});         // invalid comes before empty
        range_case("edges", es, rq, true, pa);
        std::vector<RReq> id;                          // sel == NULL: request j reads entry j
        for (uint32_t j = 0; j < 8; ++j) id.push_back({99, (int32_t)j, 20, j, kAsTarget});
        range_case("null sel", es, id, false, pa);
    }
    range_case("no request", es, {}, true, 0);
    return emu_finish("emu_pack range");
}

const uint32_t kLens[] = {0, 1, 15, 16, 17, 31, 33, 511, 512, 4096, 4097, 70000};
constexpr uint32_t kSmallLens = 7;  // 0 ... 33

Entry entry_of(uint32_t len, bool frame, uint32_t sa, uint32_t fa) {
    return frame && len ? frame_of(len, sa, fa) : raw_of(len, sa, fa);
}

}  // namespace

const EmuKernelMode emu_modes[] = {{"pack_tile_sum_kernel", kEmuPool},   {"pack_tile_scan_kernel", kEmuPool},
                                   {"pack_index_kernel", kEmuPool},      {"pack_copy_kernel", kEmuSerial},
                                   {"unpack_mask_kernel", kEmuSerial},   {"unpack_raw_kernel", kEmuSerial},
                                   {"range_gather_kernel", kEmuSerial}, {"range_deliver_kernel", kEmuSerial},
                                   {nullptr, kEmuNone}};

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "range")) return range_main();
    const uint32_t T = lz4e::kPackTile;
    // ---- pack: every source residue against every packed residue, lengths up to 33 ----
    // align 1; ahead of each entry a raw filler whose length puts it at the wanted residue
    for (uint32_t li = 0; li < kSmallLens; ++li)
        for (uint32_t frame = 0; frame < 2; ++frame) {
            std::vector<Entry> es;
            uint64_t at = 0;
            for (uint32_t sa = 0; sa < 16; ++sa)
                for (uint32_t da = 0; da < 16; ++da) {
                    const uint32_t fill = (uint32_t)((da + 16 - at % 16) % 16);
                    if (fill) es.push_back(raw_of(fill, (sa * 7 + da) & 15, da));
                    es.push_back(entry_of(kLens[li], frame != 0, sa, sa));
                    at += fill + kLens[li];
                }
            pack_case("residues", es, 1, 0, kCapExact);
            pack_case("residues", es, 1, 5 + li, kCapExact);
        }
    // ---- every length, all-raw / all-frame / alternating, every align, three capacities ----
    for (uint32_t align : {1u, 16u, 512u, 4096u})
        for (uint32_t mix = 0; mix < 3; ++mix)
            for (Cap cap : {kCapExact, kCapOneShort, kCapZero}) {
                std::vector<Entry> es;
                uint32_t k = 0;
                for (uint32_t len : kLens) {
                    const bool frame = mix == 1 || (mix == 2 && (k & 1));
                    es.push_back(entry_of(len, frame, (k * 3 + align) & 15, (k * 11 + 5) & 15));
                    ++k;
                }
                pack_case(mix == 0 ? "all raw" : mix == 1 ? "all frame" : "alternating", es, align, (align + mix) & 15, cap);
            }
    // ---- the scan: block counts around the tile, and one that takes the tile-sum workgroup round twice ----
    for (uint32_t n : {0u, 1u, T - 1, T, T + 1, 2 * T + 1, T * 64 + 1})
        for (uint32_t align : {1u, 512u}) {
            if (n > 2 * T + 1 && align != 1) continue;
            std::vector<Entry> es;
            for (uint32_t i = 0; i < n; ++i) es.push_back(entry_of(rnd32() % 4, (i & 1) != 0, i & 15, (i >> 4) & 15));
            pack_case("scan", es, align, n & 15, kCapExact);
            if (n <= 2 * T + 1) pack_case("scan, no room", es, align, 0, n & 1 ? kCapOneShort : kCapZero);
        }
    // ---- unpack: mask and raw copy ----
    for (uint32_t da = 0; da < 16; ++da) {
        std::vector<UEntry> es;
        uint32_t k = 0;
        for (uint32_t len : kLens) {
            const int32_t L = (int32_t)len;
            es.push_back({LZ4E_PACK_RAW, L, L, (da + k) & 15});        // fits exactly
            es.push_back({LZ4E_PACK_RAW, L, L + 9, (da * 3 + k) & 15});  // room to spare
            es.push_back({LZ4E_PACK_RAW, L, L - 1, da});               // one byte short (len 0: cap -1)
            es.push_back({LZ4E_PACK_RAW, L, 0, da});                   // no room (len 0: an empty copy)
            es.push_back({LZ4E_PACK_FRAME, L, L + 40, da});            // the decoders' entry
            es.push_back({2, L, L + 40, da});                          // an unknown kind
            es.push_back({255, L, L, da});
            ++k;
        }
        es.push_back({LZ4E_PACK_RAW, -5, 64, da});  // a corrupt index
        unpack_case("unpack", es, da);
    }
    for (uint32_t pa = 0; pa < 16; ++pa)  // every packed residue against every destination residue
        for (uint32_t li = 1; li < kSmallLens; ++li) {
            std::vector<UEntry> es;
            for (uint32_t k = 0; k < 16; ++k) es.push_back({LZ4E_PACK_RAW, (int32_t)kLens[li], (int32_t)kLens[li], k});
            unpack_case("unpack residues", es, pa);
        }
    unpack_case("unpack, no entry", {}, 0);
    return emu_finish("emu_pack");
}
