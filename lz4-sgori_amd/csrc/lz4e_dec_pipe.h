// lz4e_dec_pipe.h -- the pipelined decoder's device code: one block per
// 4-wave workgroup (included by lz4e_decompress.hip alone;
// decompress_pipe_kernel is there).
//
// The one-wave decoder runs the parse and the copies of each batch one
// after the other, and a block's time is the sum of both over its ~150
// batches; with ~3 blocks per SIMD the kernel time is the slowest block's
// chain.  Here the parse and the copies of different batches overlap:
//
//  * wave 0 parses (parse_batch: the reference's exact checks, so the return
//    value is decided here) and publishes each batch -- per-lane sequence
//    records plus its output range [lo, hi) -- in a ring of record slots;
//  * waves 1..3 (copier c = wave - 1) copy batches j = c, c+3, c+6, ... so
//    three batches are in flight at once.  A fast batch (at most kPipeOut
//    output bytes) is assembled in an LDS span; every output byte is a
//    literal (from the compressed input in HBM), a match byte whose source
//    lies before the far line F (final in HBM: loaded), one whose source lies
//    in the batch itself (internal pointer) or one whose source lies in the
//    spans of batches j-1 / j-2, still in LDS (cross pointer).  Match byte t
//    of a sequence copies output byte x - off, also inside a self-overlapping
//    match, so the pointers are linear in t.  Internal pointers resolve by
//    pointer jumping (a chain of depth d in log2 d rounds) in parallel with
//    the other copiers; only the gather of the cross bytes waits for batches
//    j-1 and j-2, and that is one LDS round trip, so the batches' serial
//    chain is short.  The span then leaves in 16-byte stores.  A scalar-path
//    batch (long runs, block ends) copies in HBM once every earlier batch is
//    stored.
//
// Progress flags (LDS, workgroup-scope acquire/release): `resolved` counts
// the batches whose bytes are final (in order), `stored` is the output
// prefix known to be in HBM (each batch's stores waited for with
// s_waitcnt vmcnt(0) before it moves, in order).  Far loads wait for
// stored >= F.  Measured against per-copier flags (batches finishing out of
// order, "all batches <= k" read off three flags): the in-order counters
// poll one word instead of three and were 10 % faster on silesia64k.  Every
// wait is bounded (watchdog).
#pragma once

#include "lz4e_dec_copy.h"
#include "lz4e_results.h"

namespace lz4e {

namespace {

// Waves per workgroup (parser + copiers) and the workgroups per CU asked of
// the compiler (24 waves: 76 VGPRs and 19 KiB of LDS each): 2, 3 and 5 waves
// and 5, 7 and 8 workgroups measured slower or spilled
// (profiles/r06/pipe_waves_occupancy.log).
constexpr uint32_t kPipeWaves = 4;
constexpr uint32_t kPipeMinWg = 6;
constexpr uint32_t kCopiers = kPipeWaves - 1;
// Record slots between the parser and the copiers (how far the parser may
// run ahead of the slowest copier): 6, 8 and 12 measured 0.874 / 0.882 /
// 0.902 ms against 0.878-0.883 ms for 4 on silesia64k
// (profiles/r05/pipe_recs/).
constexpr uint32_t kPipeRecs = 4;
constexpr uint32_t kPipeSpans = kCopiers + 2;  // see copy_fast's slot safety
constexpr int32_t kPipeOut = 1024;                   // output bytes per fast batch
constexpr uint32_t kPipeSpan = kPipeOut + 16 + 48;   // its span (16-B aligned start)
constexpr uint16_t kCross = 0x8000;  // jump entry: 0x8000 | (source - F)
enum : int32_t { kKindFast = 0, kKindHbm = 1 };
// record header: sequences, kind, output range, far line F, the starts of
// batches j-1 and j-2
enum { kHdrN, kHdrKind, kHdrLo, kHdrHi, kHdrF, kHdrLo1, kHdrLo2, kHdrWords = 8 };

struct PipeLds {
    uint32_t ring[(kRing + kRingPad) / 4];     // parser input ring
    int32_t rec[kPipeRecs][5][kWave];          // ls, L, op, off, M per sequence
    int32_t hdr[kPipeRecs][kHdrWords];
    uint8_t span[kPipeSpans][kPipeSpan];
    uint16_t jump[kCopiers][kPipeSpan];
    uint8_t sink[kCopiers][kSink];
    int32_t pub[kPipeRecs], con[kPipeRecs];    // record slot published / consumed (batch index)
    int32_t resolved;                          // batches whose bytes are final, in order
    int32_t stored;                            // output prefix known to be in HBM
    int32_t nb_total;                          // batches, once the parser is done
    int32_t abort;                             // a wait timed out (watchdog): every wave leaves
    int32_t beat;                              // heartbeat of a long in-HBM copy (watchdog)
    int32_t result;                            // the parse's return value (decided by wave 0)
    uint32_t spin_max;                         // the watchdog's limit for this block (see below)
};

// Watchdog of the waits: a wait that sees the counters it watches stand
// still for S.spin_max sleeps in a row means a broken invariant; the block
// then fails (ret = kPipeAbort = LZ4E_DECODE_ABORTED, include/lz4e.h: the
// host entry points report it through lz4e_last_error) instead of hanging.
// The bound, from the frame's own worst case ("Watchdog"):
// between two moves of a watched counter a valid frame's decode does one
// of (a) a batch's parse and copies (<= 64 sequences, <= 1 KiB of output:
// tens of k cycles), (b) a scalar sequence's copy in HBM, which bumps
// `beat` every round trip, or (c) the parser's vector scan of one length-
// extension run, 256 bytes per ~1-2 k-cycle step and no counter moved:
// at most srcSize / 256 steps.  A sleep is >= 128 cycles (s_sleep 2), so
// spin_max = kSpinMax (2^23 sleeps, ~0.45 s at 2.4 GHz, for (a) and
// anything the hardware adds) + srcSize >> kSpinBytesShift sleeps (64 per
// 256 bytes: 4-8x the scan's worst case) can only fire on a broken
// invariant.  Progress resets the count.  LZ4E_SPIN_MAX / _BYTES_SHIFT
// override the terms (the emulator's watchdog test builds a limit of one
// sleep and no per-byte term).
#ifndef LZ4E_SPIN_MAX
#define LZ4E_SPIN_MAX (1u << 23)
#endif
#ifndef LZ4E_SPIN_BYTES_SHIFT
#define LZ4E_SPIN_BYTES_SHIFT 2
#endif
constexpr uint32_t kSpinMax = LZ4E_SPIN_MAX;
constexpr uint32_t kSpinBytesShift = LZ4E_SPIN_BYTES_SHIFT;
constexpr int32_t kPipeAbort = kDecodeAborted;  // lz4e_results.h

LZ4E_DEV int32_t lds_acquire(int32_t* p) {
    return (int32_t)uni((uint32_t)__hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
}
// Called by every lane of the wave: the wave's earlier LDS / global
// accesses have all been issued before it (lockstep).
LZ4E_DEV void lds_release(int32_t* p, int32_t v) {
    lockstep();
    __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// u16 x 4 at a jump-table index (unaligned forms for the pointer runs).
typedef uint64_t __attribute__((aligned(2), may_alias)) u64a2;
typedef __attribute__((address_space(3))) u64a2 lu64a2;
typedef __attribute__((address_space(3), may_alias)) uint64_t lu64;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3), may_alias)) u32x4 lu128;
LZ4E_DEV int32_t wave_min_i32(int32_t v) {
    const int32_t e = wave_excl_min(v);
    const int32_t m = e < v ? e : v;
    return (int32_t)lane_val((uint32_t)m, kWave - 1);
}

// Cycle counters of the stamped build, per block (u64 x 20): parser parse,
// parser waits, copier other work, copier waits for records, for far loads,
// for batch j-1 (resolved), for the in-order store flag, batches; copier
// phases: loads + span setup, internal rounds, cross gather, store pass,
// store completion; internal rounds, batches with internal pointers; copier
// pointer entries; parser phases: window, table composition, follow, fields;
// the block's shader cycles and 100 MHz ticks (wave 0, start to end).
enum { kStParse, kStPWait, kStWork, kStRec, kStFar, kStPrev, kStStore, kStBatches, kStLoads,
       kStRounds, kStGather, kStSpass, kStVm, kStNRounds, kStNInt, kStPtrs,
       kStPWin, kStPComp, kStPFollow, kStPFields, kStT, kStR, kStSlots };
// The accumulators live in LDS (a row per wave), so that the stamped build
// has the register allocation of the real one.
struct PipeStamps {
    uint64_t* acc = nullptr;  // LDS row of this wave (stamped build)
    uint64_t t = 0;
    LZ4E_DEV void lap(bool on, int k) {
        if (!on) return;
        const uint64_t now = clock64();
        if (lane_id() == 0) acc[k] += now - t;
        t = now;
    }
    LZ4E_DEV void bump(bool on, int k) {
        if (on && lane_id() == 0) acc[k]++;
    }
};

// Waits until ready(); false when the watchdog fired (here or in another
// wave).  watch() is the LDS counter the wait depends on: the watchdog
// counts sleeps since it last moved.
template <class SL, class F, class W>
LZ4E_DEV bool wait_for(SL& S, F ready, W watch) {
    int32_t last = watch();
    for (uint32_t k = 0; !ready(); ++k) {
        const int32_t now = watch();
        if (now != last) {
            last = now;
            k = 0;
        }
        if (k >= S.spin_max || lds_acquire(&S.abort)) {
            lds_release(&S.abort, 1);
            return false;
        }
        __builtin_amdgcn_s_sleep(2);
    }
    return true;
}

template <bool kStamps, class F, class W>
LZ4E_DEV bool spin(PipeLds& S, F ready, W watch, PipeStamps& st, int k) {
    st.lap(kStamps, kStWork);
    const bool ok = wait_for(S, ready, watch);
    st.lap(kStamps, k);
    return ok;
}

// A fast batch j (see above).  Slot safety with K copiers in round robin
// and K + 2 spans: span slot j % (K+2) last held batch j-K-2, read by
// batches j-K-1 and j-K (cross gathers) and by its own store pass; j-K was
// this wave's previous batch, j-K-1's gather happened before `resolved`
// reached j-K (this wave waited for that), and j-K-2 was stored before this
// wave's batch j-K could be.
template <bool kStamps>
LZ4E_DEV bool copy_fast(PipeLds& S, uint32_t c, int32_t j, const Batch& b, const int32_t* hdr,
                        const uint8_t* in, int32_t srcSize, uint8_t* gout, uint32_t lane,
                        PipeStamps& st) {
    const int32_t lo = hdr[kHdrLo], hi = hdr[kHdrHi], F = hdr[kHdrF];
    const int32_t a0 = lo & ~15;
    const int32_t s0 = lo - a0, s1 = hi - a0;  // span indices of [lo, hi)
    lu8* span = (lu8*)S.span[(uint32_t)j % kPipeSpans];
    lu16* jt = (lu16*)S.jump[c];
    lu8* sink = (lu8*)S.sink[c] + 4 * lane;
    const bool valid = lane < b.n;
    const int32_t ms = b.op + b.L, ss = ms - b.off;
    // Match byte t of a sequence copies output byte ss + t; bytes [0, nf)
    // come from before F (HBM).
    int32_t nf = 0;
    if (valid && b.off != 0 && ss < F) nf = b.M < F - ss ? b.M : F - ss;
    if (ballot(nf > 0) &&
        !spin<kStamps>(S, [&] { return lds_acquire(&S.stored) >= F; },
                       [&] { return lds_acquire(&S.stored) + lds_acquire(&S.beat); }, st, kStFar))
        return false;
    // loads first (far source bytes, the literal run), consumed below
    uint4 h0 = make_uint4(0, 0, 0, 0), h1 = h0, lv = h0;
    if (nf > 0) {
        h0 = ldg16(gout + ss);
        if (nf > 16) h1 = ldg16(gout + ss + 16);
    }
    const bool lfast = valid && b.L > 0 && b.ls + 16 <= srcSize;
    if (lfast) lv = ldg16(in + b.ls);
    // every byte of [lo, hi) final until shown otherwise: 4 entries per
    // 8-byte store (the row is 16-byte aligned; entries outside [lo, hi) are
    // never read as pointers -- `entry` masks them)
    for (int32_t g = (s0 & ~3) + 4 * (int32_t)lane; g < s1; g += 4 * (int32_t)kWave)
        *(lu64*)(jt + g) = ~0ull;
    wave_fence();
    // match bytes [nf, M): a cross pointer below lo, else an internal one
    const bool ptrs = valid && b.off != 0 && nf < b.M;
    if (ptrs) {
        lu16* e = jt + (ms - a0);
#pragma clang loop unroll(disable) vectorize(disable)
        for (int32_t t = nf; t < b.M; ++t) {
            const int32_t y = ss + t;
            e[t] = (uint16_t)(y < lo ? (int32_t)kCross + (y - F) : y - a0);
        }
    }
    const bool has_cross = ptrs && ss + nf < lo;
    const bool has_int = ptrs && ss + b.M > lo;
    // rounds and gather start at the first pointer byte
    const int32_t i0 = (int32_t)uni((uint32_t)wave_min_i32(ptrs ? ms + nf - a0 : s1));
    st.lap(kStamps, kStPtrs);
    // the loaded bytes into the span
    if (valid && b.L > 0) {
        if (lfast) {
            static_assert(kFastLitMax <= 16, "one put16 carries a fast literal run");
            put16(span + (b.op - a0), lv, b.L < 16 ? (uint32_t)b.L : 16u, sink);
        } else {
#pragma clang loop unroll(disable) vectorize(disable)
            for (int32_t t = 0; t < b.L; ++t) span[b.op - a0 + t] = in[b.ls + t];
        }
    }
    if (nf > 0) {
        static_assert(kFastMatchMax <= 32, "h0 and h1 carry a fast match's whole head");
        put16(span + (ms - a0), h0, nf < 16 ? nf : 16, sink);
        if (nf > 16) put16(span + (ms - a0) + 16, h1, nf < 32 ? nf - 16 : 16, sink);
    }
    if (valid && b.off == 0)  // offset 0 writes zeros (:313, 407-415)
#pragma clang loop unroll(disable) vectorize(disable)
        for (int32_t t = 0; t < b.M; ++t) span[ms - a0 + t] = 0;
    wave_fence();
    st.lap(kStamps, kStLoads);
    // internal pointers: pointer jumping until each byte is final or cross.
    // Lane l owns the 8 span bytes / jump entries at g = b0 + 8l (+ 512k):
    // one 16-byte entry read and one 8-byte span read per group, the 8
    // dependent entry reads and byte reads independent of each other, and
    // one write back of each (positions outside [i0, s1) keep their values).
    const int32_t b0 = i0 & ~7;
    auto entry = [&](const u32x4& jv, int q, int32_t g) -> uint32_t {
        const uint32_t e = (jv[q >> 1] >> (16 * (q & 1))) & 0xFFFFu;
        return (g + q >= i0 && g + q < s1) ? e : kFinal;
    };
    if (ballot(has_int)) {
        st.bump(kStamps, kStNInt);
        for (;;) {
            st.bump(kStamps, kStNRounds);
            bool more = false;
            for (int32_t g = b0 + 8 * (int32_t)lane; g < s1; g += 8 * (int32_t)kWave) {
                u32x4 jv = *(const lu128*)(jt + g);
                uint64_t sp = *(const lu64*)(span + g);
                uint32_t v[8], w[8], sb[8];
                bool anyp = false;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    v[q] = entry(jv, q, g);
                    anyp |= v[q] < kCross;
                }
                if (!anyp) continue;  // (exec mask: only lanes with pointers read)
                // unconditional reads (index 0 when unused): no branches
                // between them, so all eight are in flight together
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const uint32_t x = jt[v[q] < kCross ? v[q] : 0u];
                    w[q] = v[q] < kCross ? x : kFinal;
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) sb[q] = span[v[q] < kCross ? v[q] : 0u];
                bool any = false;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const bool ptr = v[q] < kCross, fin = w[q] == kFinal;
                    any |= ptr;
                    more |= ptr && w[q] < kCross;
                    const uint32_t sh = 16 * (q & 1);
                    const uint32_t cur = (jv[q >> 1] >> sh) & 0xFFFFu;
                    const uint32_t ne = ptr ? w[q] : cur;
                    jv[q >> 1] = (jv[q >> 1] & ~(0xFFFFu << sh)) | (ne << sh);
                    const uint64_t bm = 0xFFull << (8 * q);
                    sp = (ptr && fin) ? ((sp & ~bm) | ((uint64_t)(sb[q] & 0xFFu) << (8 * q))) : sp;
                }
                if (any) {
                    *(lu64*)(span + g) = sp;
                    *(lu128*)(jt + g) = jv;
                }
            }
            wave_fence();
            if (!ballot(more)) break;
        }
    }
    st.lap(kStamps, kStRounds);
    // cross bytes: batches j-1 and j-2 are final once `resolved` reaches j
    if (!spin<kStamps>(S, [&] { return lds_acquire(&S.resolved) >= j; },
                       [&] { return lds_acquire(&S.resolved) + lds_acquire(&S.beat); }, st, kStPrev))
        return false;
    if (ballot(has_cross)) {
        const int32_t lo1 = hdr[kHdrLo1], lo2 = hdr[kHdrLo2];
        const lu8* p1 = (const lu8*)S.span[(uint32_t)(j + kPipeSpans - 1) % kPipeSpans] - (lo1 & ~15);
        const lu8* p2 = (const lu8*)S.span[(uint32_t)(j + kPipeSpans - 2) % kPipeSpans] - (lo2 & ~15);
        for (int32_t g = b0 + 8 * (int32_t)lane; g < s1; g += 8 * (int32_t)kWave) {
            const u32x4 jv = *(const lu128*)(jt + g);
            uint64_t sp = *(const lu64*)(span + g);
            uint32_t x[8];
            bool any = false;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const uint32_t v = entry(jv, q, g);
                any |= v != kFinal && v >= kCross;
            }
            if (!any) continue;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const uint32_t v = entry(jv, q, g);
                const bool cr = v != kFinal && v >= kCross;
                const int32_t y = cr ? F + (int32_t)(v - kCross) : lo1;
                x[q] = y >= lo1 ? p1[y] : p2[y];  // unconditional (p1[lo1] when unused)
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const uint32_t v = entry(jv, q, g);
                const bool cr = v != kFinal && v >= kCross;
                any |= cr;
                const uint64_t bm = 0xFFull << (8 * q);
                sp = cr ? ((sp & ~bm) | ((uint64_t)(x[q] & 0xFFu) << (8 * q))) : sp;
            }
            if (any) *(lu64*)(span + g) = sp;
        }
        wave_fence();
    }
    lds_release(&S.resolved, j + 1);
    st.lap(kStamps, kStGather);
    // store pass: 16-byte HBM chunks of [lo, hi); partial end chunks by bytes
    const int32_t nch = (hi - a0 + 15) >> 4;
    for (int32_t i = (int32_t)lane; i < nch; i += kWave) {
        const int32_t c0 = a0 + 16 * i;
        const lu8* sc = span + 16 * i;
        if (c0 >= lo && c0 + 16 <= hi) {
            const u32x4 v = *(const lu128*)sc;
            stg16(gout + c0, make_uint4(v.x, v.y, v.z, v.w));
        } else {
#pragma clang loop unroll(disable) vectorize(disable)
            for (int32_t x = c0 > lo ? c0 : lo; x < c0 + 16 && x < hi; ++x)
                *(gu8*)(gout + x) = sc[x - c0];
        }
    }
    st.lap(kStamps, kStSpass);
    if (!spin<kStamps>(S, [&] { return lds_acquire(&S.stored) >= lo; },
                       [&] { return lds_acquire(&S.stored) + lds_acquire(&S.beat); }, st, kStStore))
        return false;
    stores_done();
    lds_release(&S.stored, hi);
    st.lap(kStamps, kStVm);
    return true;
}

}  // namespace

}  // namespace lz4e
