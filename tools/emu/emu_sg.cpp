// Lane emulator of the zero-copy scatter-gather kernels (debug/test tooling,
// tools/emu): compiles the unmodified csrc/lz4e_sg.hip as host C++ and runs
// sg_gather_kernel and sg_deliver_kernel lane by lane, under the same
// emulated <hip/hip_runtime.h> as the other kernel files.  Stand-alone (its own main): built by EMU_SG=1 build.sh, run
// by tests/test_emulator_sg.py under ASan + UBSan.
//
// The kernels work on the CALLER's memory and must not touch a byte outside
// [src, src + n) or [dst, dst + n).  So every source segment and every
// destination here is its own heap allocation that ends exactly at the
// buffer's last byte (ASan's redzone follows it: one byte of over-read or
// over-write is a report), at a chosen alignment mod 16 with a poisoned
// prefix and a canary that is checked after the run (emu_harness.h, Buf).
//
// The two kernels have no barrier and no cross-lane operation, so a
// workgroup's lanes run one after the other on the calling thread (the
// harness, its Buf and its kernel modes: emu_harness.h).
#include "emu_harness.h"

#include "lz4e_sg.hip"

#include "lz4e.h"

uint32_t g_rng = 12345;
uint8_t rnd() { return (uint8_t)(emu_lcg(g_rng) >> 24); }

namespace {

// The host gather the staged path uses (csrc/lz4e_host.hip, sg_gather), restated.
void sg_gather_ref(const struct bio_vec* bv, const struct bvec_iter& it, uint8_t* to, uint32_t len) {
    uint32_t idx = it.bi_idx, done = it.bi_bvec_done;
    while (len) {
        uint32_t take = bv[idx].bv_len - done < len ? bv[idx].bv_len - done : len;
        memcpy(to, reinterpret_cast<const uint8_t*>(bv[idx].bv_page) + bv[idx].bv_offset + done, take);
        to += take;
        len -= take;
        done = 0;
        idx++;
    }
}

// One request: segments of the given lengths at the given source alignments,
// gathered by the kernel into an exact-size destination at dst_align.  The
// iterator starts `start_done` bytes into segment `start_idx`.
void gather_case(const std::vector<uint32_t>& lens, const std::vector<uint32_t>& aligns, uint32_t dst_align,
                 uint32_t start_idx = 0, uint32_t start_done = 0) {
    const size_t S = lens.size();
    std::vector<Buf*> seg;
    std::vector<struct bio_vec> bv(S ? S : 1);
    uint32_t total = 0;
    for (size_t i = 0; i < S; ++i) {
        seg.push_back(new Buf(aligns[i], lens[i]));
        seg[i]->fill_random();
        bv[i].bv_page = reinterpret_cast<struct page*>(seg[i]->p);
        bv[i].bv_len = lens[i];
        bv[i].bv_offset = 0;
        if (i >= start_idx) total += lens[i];
    }
    total -= S ? start_done : 0;
    struct bvec_iter it = {0, total, start_idx, start_done};
    std::vector<uint8_t> want(total);
    sg_gather_ref(bv.data(), it, want.data(), total);
    // descriptors as the pipeline builds them (csrc/lz4e_host.hip, plan_zero_copy)
    std::vector<lz4e::SgGatherDesc> gd;
    {
        uint32_t idx = start_idx, done = start_done, left = total;
        uint64_t at = 0;
        while (left) {
            const uint32_t take = bv[idx].bv_len - done < left ? bv[idx].bv_len - done : left;
            const uint64_t src = reinterpret_cast<uint64_t>(bv[idx].bv_page) + bv[idx].bv_offset + done;
            for (uint32_t p = 0; p < take; p += lz4e::kSgPiece)
                gd.push_back({src + p, at + p, take - p < lz4e::kSgPiece ? take - p : lz4e::kSgPiece, 0});
            at += take;
            left -= take;
            done = 0;
            idx++;
        }
    }
    Buf dst(dst_align, total);
    dst.fill(0x5A);
    // the descriptor list is an exact-size allocation too
    Buf dl(0, gd.size() * sizeof(lz4e::SgGatherDesc));
    if (!gd.empty()) memcpy(dl.p, gd.data(), dl.n);
    const hipError_t e = lz4e::launch_sg_gather(reinterpret_cast<const lz4e::SgGatherDesc*>(dl.p),
                                                (uint32_t)gd.size(), dst.p, nullptr);
    CHECK(e == hipSuccess, "gather launch");
    CHECK(total == 0 || memcmp(dst.p, want.data(), total) == 0, "gather: %zu segments (first %u B), dst align %u",
          S, S ? lens[0] : 0, dst_align);
    CHECK(dst.canary_ok(), "gather: bytes before the destination written (dst align %u)", dst_align);
    for (Buf* b : seg) {
        CHECK(b->canary_ok(), "gather: source canary");
        delete b;
    }
}

struct DeliverCase {
    uint32_t len;        // request size
    int32_t ret, dret;   // the round trip's values
    bool want_frame;
    int32_t frame_cap;
    uint32_t src_align, frame_align, data_align;
    bool frame_last;  // slot layout [out | frame] (else [frame | out]): the last part ends its block
};

void deliver_case(const DeliverCase& c) {
    const uint32_t fbytes = c.ret > 0 ? (uint32_t)c.ret : 0;
    // the slot's data buffer holds the frame and the decoded output
    Buf slot(c.src_align, (size_t)fbytes + c.len);
    slot.fill_random();
    const uint64_t fr_off = c.frame_last ? c.len : 0, out_off = c.frame_last ? 0 : fbytes;
    Buf frame(c.frame_align, c.want_frame ? (size_t)(c.frame_cap > 0 ? c.frame_cap : 0) : 0);
    Buf data(c.data_align, c.len);
    frame.fill(0x5A);
    data.fill(0x5A);
    const bool ok = c.ret > 0 && c.dret == (int32_t)c.len && (!c.want_frame || c.frame_cap >= c.ret);
    // entry 1 of a two-entry batch (entry 0's values would deliver nothing)
    const uint64_t fr[2] = {0, fr_off}, out[2] = {0, out_off};
    const uint32_t in_len[2] = {7, c.len};
    const int32_t ret[2] = {0, c.ret}, dret[2] = {-1, c.dret};
    Buf dl(0, sizeof(lz4e::SgDeliverDesc));
    const lz4e::SgDeliverDesc d{c.want_frame ? reinterpret_cast<uint64_t>(frame.p) : 0,
                                reinterpret_cast<uint64_t>(data.p), 1, c.frame_cap};
    memcpy(dl.p, &d, sizeof d);
    const lz4e::SgDeliverBatch a{reinterpret_cast<const lz4e::SgDeliverDesc*>(dl.p), 1, slot.p, fr, out,
                                 in_len, ret, dret, c.len};
    CHECK(lz4e::launch_sg_deliver(a, nullptr) == hipSuccess, "deliver launch");
    bool good = true;
    if (ok) {
        good &= memcmp(data.p, slot.p + out_off, c.len) == 0;
        if (c.want_frame) {
            good &= memcmp(frame.p, slot.p + fr_off, fbytes) == 0;
            for (size_t i = fbytes; i < frame.n; ++i) good &= frame.p[i] == 0x5A;
        }
    } else {  // a failing request: nothing written
        for (size_t i = 0; i < data.n; ++i) good &= data.p[i] == 0x5A;
        for (size_t i = 0; i < frame.n; ++i) good &= frame.p[i] == 0x5A;
    }
    CHECK(good, "deliver: len %u ret %d dret %d frame %d cap %d aligns %u/%u/%u", c.len, c.ret, c.dret,
          (int)c.want_frame, c.frame_cap, c.src_align, c.frame_align, c.data_align);
    CHECK(frame.canary_ok() && data.canary_ok() && slot.canary_ok(), "deliver: canary (len %u)", c.len);
}

}  // namespace

const EmuKernelMode emu_modes[] = {{"sg_gather_kernel", kEmuSerial}, {"sg_deliver_kernel", kEmuSerial}, {nullptr, kEmuNone}};

int main() {
    const uint32_t small[] = {1, 15, 16, 17, 31, 33}, large[] = {511, 512, 4096, 4097};
    // ---- gather ----
    // every source alignment against every destination alignment, lengths up to 33
    for (uint32_t len : small)
        for (uint32_t sa = 0; sa < 16; ++sa)
            for (uint32_t da = 0; da < 16; ++da) gather_case({len}, {sa}, da);
    for (uint32_t len : large)
        for (uint32_t k = 0; k < 16; ++k) gather_case({len}, {k}, (k * 7 + 3) & 15);
    // all ten lengths as one request's segments: every segment after the
    // first lands at whatever alignment the ones before leave
    for (uint32_t da = 0; da < 16; ++da)
        gather_case({1, 15, 16, 17, 31, 33, 511, 512, 4096, 4097}, {3, 0, 9, 15, 1, 8, 5, 0, 7, 13}, da);
    // a segment longer than one descriptor's piece, the iterator starting inside segment 1
    gather_case({100, 40000, 17}, {1, 6, 11}, 5);
    gather_case({100, 40000, 17}, {1, 6, 11}, 0, 1, 33);
    gather_case({4096, 4096}, {0, 0}, 0, 0, 4095);
    // 256 segments of 16 B, and an empty request
    gather_case(std::vector<uint32_t>(256, 16), std::vector<uint32_t>(256, 4), 0);
    {
        std::vector<uint32_t> al(256);
        for (uint32_t i = 0; i < 256; ++i) al[i] = i * 5 & 15;
        gather_case(std::vector<uint32_t>(256, 16), al, 9);
    }
    gather_case({}, {}, 0);
    gather_case({}, {}, 7);
    // ---- deliver ----
    for (uint32_t len : small)
        for (uint32_t sa = 0; sa < 16; ++sa)
            for (uint32_t da = 0; da < 16; ++da) {
                const int32_t ret = (int32_t)small[(len + sa) % 6];
                deliver_case({len, ret, (int32_t)len, true, ret + 3, sa, da, (da + 5) & 15, (sa & 1) != 0});
            }
    for (uint32_t len : large)
        for (uint32_t k = 0; k < 16; ++k) {
            const int32_t ret = (int32_t)(len / 2 + k);
            deliver_case({len, ret, (int32_t)len, true, ret, k, (k * 3 + 1) & 15, (k * 11 + 6) & 15, (k & 1) != 0});
        }
    for (uint32_t k = 0; k < 16; ++k)
        for (uint32_t len : {17u, 4097u, 40000u}) {
            const int32_t ret = (int32_t)len / 3 + 1, il = (int32_t)len;
            const uint32_t fa = (k + 9) & 15, da = (k * 5 + 2) & 15;
            deliver_case({len, ret, il, true, ret + 100, k, fa, da, false});  // success
            deliver_case({len, ret, il, false, 0, k, fa, da, true});          // success, no frame wanted
            deliver_case({len, 0, il, true, ret + 100, k, fa, da, false});    // compress failed
            deliver_case({len, -5, il, true, ret + 100, k, fa, da, false});
            deliver_case({len, ret, il - 1, true, ret + 100, k, fa, da, true});   // dret != len
            deliver_case({len, ret, -3, false, 0, k, fa, da, false});
            deliver_case({len, ret, il, true, ret, k, fa, da, true});        // frame_cap == ret
            deliver_case({len, ret, il, true, ret - 1, k, fa, da, false});   // frame_cap == ret - 1
            deliver_case({len, ret, il, true, 0, k, fa, da, true});          // frame_cap == 0
        }
    deliver_case({0, 1, 0, true, 1, 0, 3, 7, false});  // an empty request: a 1-byte frame, no data
    return emu_finish("emu_sg");
}
