// lz4e_decompress.hip -- gfx950 LZ4E safe block decoders.
//
// Restates /root/reference/lz4e/lz4e_decompress.c:62-469
// (LZ4E_decompress_generic, instance endOnInputSize + decode_full_block +
// noDict).  The batch decoders share one parse (parse_batch, lz4e_dec_parse.h)
// and the copy primitives of lz4e_dec_copy.h, and differ in how the copies of
// a batch are scheduled; the group decoder runs the scalar loop per group of
// 8 lanes.  pick_decoder below chooses one per launch ("Auto
// mode").
//
//  * decompress_kernel, one wave per block (this file): the wave parses a
//    batch, then copies it -- fast batches assembled in a small LDS span
//    (literals from a 1 KiB LDS ring that mirrors the compressed segments
//    the parse loaded, match sources before the batch from HBM, in-batch
//    dependencies in rounds or by pointer jumping over the span's bytes) and
//    written with one pass of 16-byte stores; scalar-path batches (long
//    runs, block ends) copy in HBM.  LDS per block: ring 1 KiB + mirror
//    128 B + store sink 256 B + span 2,112 B + jump table 4,224 B = 7,744 B.
//    Its LDS form (blocks of <= kSmallOut bytes) stages the whole input and
//    assembles the whole output in LDS.
//  * decompress_pipe_kernel, one 4-wave workgroup per block: lz4e_dec_pipe.h.
//  * decompress_group_kernel, one block per group of 8 lanes, handing blocks
//    of short sequences to decompress_resume_kernel: lz4e_dec_group.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "lz4e_device.h"
#include "lz4e_gpu.h"
#include "lz4e_order.h"
#include "lz4e_dec_parse.h"
#include "lz4e_dec_copy.h"
#include "lz4e_dec_group.h"
#include "lz4e_dec_pipe.h"

namespace lz4e {

namespace {

// ---------------------------------------------------------------- one wave per block

// LDS per block besides the input ring and the store sink: the span buffer
// of a fast batch and its jump table.
constexpr uint32_t kSpan = kWave * (uint32_t)kFastSeqMax + 16 + 48;  // a fast batch's output, 16-B aligned start
constexpr uint32_t kJump = 2 * kSpan;                                // u16 per span byte (chain resolution)
// The LDS form's fast batches (the span is the LDS output itself).
constexpr int32_t kSmallBatchOut = 1024;                    // fast-batch output cap there
constexpr uint32_t kSmallJump = 2 * (kSmallBatchOut + 64);  // its jump table

// The one-wave decoder reads length-extension runs with the byte loop: the
// vector scan's 2 more VGPRs would cost it a wave per SIMD, and its <= 16 KiB
// blocks hold short runs.  The CPU lane emulator's test build turns the scan
// on (-DLZ4E_ONEWAVE_VEC_EXT=true) so that it runs under ASan against the
// oracle (tests/test_emulator.py).
#ifndef LZ4E_ONEWAVE_VEC_EXT
#define LZ4E_ONEWAVE_VEC_EXT false
#endif
constexpr bool kOneWaveVecExt = LZ4E_ONEWAVE_VEC_EXT;

// Small blocks in LDS: a block of at most kSmallOut output bytes without a
// dictionary (4 KiB blocks, the drop-in single calls) can keep its whole
// output in LDS: a scalar-path sequence (long literal runs and matches, as
// in fio-style data) then copies LDS to LDS at LDS latency instead of a
// store, a load that waits behind it and another store in HBM per sequence,
// and the block leaves in one pass of 16-byte stores at the end.

// Whole-wave copy of n (<= 1024 per call of a round) bytes of a literal run
// from the input ring (block bytes [p, p + n) held by it): 16 bytes per lane,
// ring offsets wrap through the mirror.
LZ4E_DEV void wave_lit_ring(lu8* dst, const InWindow& w, int32_t p, int32_t n, lu8* sink,
                            uint32_t lane) {
    for (int32_t k = 16 * (int32_t)lane; k < n; k += 16 * (int32_t)kWave)
        piece16(dst + k, w.at(p + k), (uint32_t)(n - k < 16 ? n - k : 16), sink);
}

// Whole-wave copy of n (<= kSmallOut) literal bytes from HBM into LDS: every
// load before the first store (one round trip); loads never read at or past
// srcSize.
LZ4E_DEV void wave_lit_hbm(lu8* dst, const uint8_t* in, int32_t p, int32_t n, int32_t srcSize,
                           lu8* sink, uint32_t lane) {
    constexpr int kR = (kSmallOut + 16 * kWave - 1) / (16 * kWave);
    uint4 v[kR];
#pragma unroll
    for (int j = 0; j < kR; ++j) {
        const int32_t k = 16 * ((int32_t)lane + j * (int32_t)kWave);
        v[j] = (k < n && p + k + 16 <= srcSize) ? ldg16(in + p + k) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < kR; ++j) {
        const int32_t k = 16 * ((int32_t)lane + j * (int32_t)kWave);
        if (k >= n) continue;
        const int32_t c = n - k < 16 ? n - k : 16;
        if (p + k + 16 <= srcSize) put16(dst + k, v[j], (uint32_t)c, sink);
        else
            for (int32_t t = 0; t < c; ++t) dst[k + t] = in[p + k + t];
    }
}

// Whole-wave match copy inside LDS: out[op + t] = out[op + t - off] for t in
// [0, len), any overlap (offset 0: zeros).  Round r copies [t, t + c) from D
// bytes back, D a multiple of off with c <= D <= t + off, so every source
// byte is final before the round; D doubles while 2D <= t (a run of period
// 1 takes ~log2(len) rounds).  The loop is wave-uniform.
LZ4E_DEV void wave_match_lds(lu8* out, int32_t op, uint32_t off, int32_t len, lu8* sink,
                             uint32_t lane) {
    if (off == 0) {
        for (int32_t k = 16 * (int32_t)lane; k < len; k += 16 * (int32_t)kWave)
            put16(out + op + k, make_uint4(0, 0, 0, 0), (uint32_t)(len - k < 16 ? len - k : 16), sink);
        return;
    }
    if (off < 16) {
        // short periods from registers (see wave_match): one LDS read of the
        // final period, then every chunk without waiting on earlier ones
        const lu8* pp = out + op - (int32_t)off;
        const uint4 pv = make_uint4(ld4(pp), ld4(pp + 4), ld4(pp + 8), ld4(pp + 12));
        const uint32_t step = (16u * kWave) % off;
        uint32_t ph = (16u * lane) % off;
        for (int32_t k = 16 * (int32_t)lane; k < len; k += 16 * (int32_t)kWave) {
            uint32_t w[4] = {0, 0, 0, 0}, j = ph;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                w[q >> 2] |= pat_byte(pv, j) << (8 * (q & 3));
                j = j + 1 == off ? 0 : j + 1;
            }
            put16(out + op + k, make_uint4(w[0], w[1], w[2], w[3]), (uint32_t)(len - k < 16 ? len - k : 16), sink);
            ph += step;
            ph = ph >= off ? ph - off : ph;
        }
        return;
    }
    int32_t t = 0, D = (int32_t)off;
    while (t < len) {
        int32_t c = len - t < D ? len - t : D;
        c = c < 16 * (int32_t)kWave ? c : 16 * (int32_t)kWave;
        lu8* d = out + op + t;
        const int32_t k = 16 * (int32_t)lane;
        if (k < c) piece16(d + k, d + k - D, (uint32_t)(c - k < 16 ? c - k : 16), sink);
        lockstep();  // the next round reads these bytes
        t += c;
        while (2 * D <= t) D *= 2;
    }
}

// Copies of a scalar-path batch (one sequence, any length) into the LDS
// output: the literal run from the input ring when it holds it, else from
// HBM, then the match.
LZ4E_DEV void copy_scalar_lds(const Batch& b, const InWindow& win, const uint8_t* in,
                              int32_t srcSize, lu8* obuf, lu8* sink, uint32_t lane) {
    const int32_t L = lane_val((uint32_t)b.L, 0), op = lane_val((uint32_t)b.op, 0);
    const int32_t ls = lane_val((uint32_t)b.ls, 0);
    const int32_t M = lane_val((uint32_t)b.M, 0), off = lane_val((uint32_t)b.off, 0);
    if (L > 0) {
        if (win.holds(ls, L) && (win.lb || L <= 16 * (int32_t)kWave))
            wave_lit_ring(obuf + op, win, ls, L, sink, lane);
        else wave_lit_hbm(obuf + op, in, ls, L, srcSize, sink, lane);
        lockstep();
    }
    if (M > 0) wave_match_lds(obuf, op + L, (uint32_t)off, M, sink, lane);
}

// The LDS output [0, n) to HBM in 16-byte stores (the partial end chunk by
// bytes: nothing past n is written).
LZ4E_DEV void flush_lds(uint8_t* gout, const lu8* obuf, int32_t n, uint32_t lane) {
    for (int32_t c0 = 16 * (int32_t)lane; c0 < n; c0 += 16 * (int32_t)kWave) {
        const lu8* sc = obuf + c0;
        if (c0 + 16 <= n) stg16(gout + c0, make_uint4(ld4(sc), ld4(sc + 4), ld4(sc + 8), ld4(sc + 12)));
        else
            for (int32_t x = c0; x < n; ++x) *(gu8*)(gout + x) = sc[x - c0];
    }
}

struct WaveStamps {
    uint64_t t = 0, acc[4] = {0, 0, 0, 0}, batches = 0, rounds = 0;
};

// Decode one block into HBM on one wave.  LDS: the input ring, the store
// sink, the span buffer of the fast batches and its jump table.  kLdsOut:
// the whole output is assembled in obuf (kSmallBuf bytes; outSize <=
// kSmallOut, no dictionary) and stored at the end; a fast batch's span is
// then obuf itself.  kPartial: outSize is the target of a partial decode
// (parse_batch); the copies are the same, a cut match may be 1..3 bytes.
template <bool kStamps, bool kLdsOut = false, bool kPartial = false>
LZ4E_DEV void decode_block(const uint8_t* in, int32_t srcSize, uint8_t* gout, int32_t outSize,
                           int32_t* ret_slot, uint64_t* dbg, uint32_t lane, lu8* span_buf,
                           lu32* ring, lu16* jump, int32_t dict, lu8* sinkb, lu8* obuf = nullptr,
                           lu8* lin = nullptr, int32_t ip0 = 0, int32_t op0 = 0) {
    WaveStamps st;
    [[maybe_unused]] uint64_t t_start = 0, r_start = 0;
    if constexpr (kStamps) {
        t_start = clock64();
        r_start = realtime64();
    }
    auto lap = [&](int ph) {
        if constexpr (kStamps) {
            const uint64_t now = clock64();
            st.acc[ph] += now - st.t;
            st.t = now;
        }
    };
    if constexpr (kStamps) st.t = clock64();
    lu8* sink = sinkb + 4 * lane;
    Parse P;
    P.init(in, srcSize, outSize, ring, lane, dict, lin, ip0, op0);

    for (;;) {
        Batch b;
        const ParseResult pr = parse_batch<kOneWaveVecExt, kPartial>(
            P, b, lane, kLdsOut ? kSmallBatchOut : (int32_t)kWave * kFastSeqMax);
        if (pr == kParseFail) {
            if (lane == 0) *ret_slot = -P.ip - 1;
            break;
        }
        lap(0);
        if constexpr (kStamps) st.batches++;
        const bool valid = lane < b.n;
        const int32_t op = P.op;  // end of the batch's output
        if (pr == kParsedFast) {
            // ---------------- span-staged copies (fast batches) -------------
            // The batch's output [lo, op) (<= 64 x kFastSeqMax bytes) is
            // assembled in LDS: literals from the ring; the part of a match
            // source that lies before lo from HBM (final: written by earlier
            // batches); the rest in LDS dependency rounds.  Then one store pass.
            const int32_t lo = lane_val((uint32_t)b.op, 0);
            const int32_t a0 = lo & ~15;  // span index of position x: x - a0
            lu8* span = kLdsOut ? obuf + a0 : span_buf;
            const int32_t ms = b.op + b.L, ss = ms - b.off;
            int32_t n0 = 0;
            uint4 h0 = make_uint4(0, 0, 0, 0), h1 = h0;
            // fast path: lo <= oend - kFastSeqMax, so [ss, ss + 32) is in the block
            if (valid && ss < lo) {
                n0 = b.M < lo - ss ? b.M : lo - ss;
                if constexpr (!kLdsOut) {
                    h0 = ldg16(gout + ss);
                    if (n0 > 16) h1 = ldg16(gout + ss + 16);
                }
            }
            if (valid && b.L > 0) {
                const lu8* rs = P.win.in_ring(b.ls, b.L);
                if (rs) lane_copy(span + (b.op - a0), rs, b.L, sink);
                else lane_copy64(span + (b.op - a0), in + b.ls, b.L, in + srcSize);
            }
            if constexpr (kLdsOut) {
                // the source bytes before lo are final in obuf (and end before ms)
                if (n0 > 0) lane_copy(span + (ms - a0), obuf + ss, n0, sink);
            } else if (n0 > 0) {
                put16(span + (ms - a0), h0, n0 < 16 ? n0 : 16, sink);
                if (n0 > 16) put16(span + (ms - a0) + 16, h1, n0 < 32 ? n0 - 16 : 16, sink);
                // Dead: n0 <= kFastMatchMax = 18, so h0 and h1 carry the whole
                // head.  The loop stays: without it the one-wave kernel ran
                // 5 % slower on silesia64k (1.229 -> 1.289 ms).
                for (int32_t t = 32; t < n0; t += 16)
                    put16(span + (ms - a0) + t, ldg16(gout + ss + t), n0 - t < 16 ? n0 - t : 16, sink);
            }
            lap(1);
            const int32_t ms2 = ms + n0, m2 = b.M - n0, me = ms + b.M;
            const int32_t ss2 = ss + n0;
            const int32_t need = me - b.off < ms2 ? me - b.off : ms2;  // source part before own output
            uint64_t pending = ballot(valid && m2 > 0);
            while (pending) {
                // ready when [ss2, need) overlaps no earlier pending output
                const bool mine = (pending >> lane) & 1;
                const int32_t mn = wave_excl_min(mine ? ms2 : INT32_MAX);
                const int32_t mx = wave_excl_max(mine ? me : INT32_MIN);
                const bool ready = mine && (need <= mn || ss2 >= mx);
                const uint64_t rm = ballot(ready);
                const uint32_t np = popc64(pending);
                if ((rm == (pending & (0 - pending)) && np > 1) || (np >= 4 && 4 * popc64(rm) <= np)) {
                    // Dependency chains (few of the pending matches are
                    // ready): resolve every pending byte by pointer jumping.
                    const int32_t s0 = (int32_t)lane_val((uint32_t)ms2, ctz64(pending)) - a0;
                    const uint32_t nr = resolve_chains(span, jump, lo - a0, op - a0, s0, mine,
                                                       ms2 - a0, m2, b.off, lane);
                    if constexpr (kStamps) st.rounds += nr;
                    break;
                }
                if (ready) {
                    if (b.off != 0) lane_match(span + (ms2 - a0), (uint32_t)b.off, m2, sink);
                    else lane_zero(span + (ms2 - a0), m2, sink);
                }
                pending &= ~rm;
                if constexpr (kStamps) st.rounds++;
            }
            lap(2);
            lockstep();  // the last round's span bytes, read by other lanes
            // store pass: 16-byte HBM chunks of [lo, op); partial end chunks by bytes
            const int32_t nch = kLdsOut ? 0 : (op - a0 + 15) >> 4;
            for (int32_t i = (int32_t)lane; i < nch; i += kWave) {
                const int32_t c0 = a0 + 16 * i;
                const lu8* sc = span + 16 * i;
                if (c0 >= lo && c0 + 16 <= op) {
                    stg16(gout + c0, make_uint4(ld4(sc), ld4(sc + 4), ld4(sc + 8), ld4(sc + 12)));
                } else {
                    for (int32_t x = c0 > lo ? c0 : lo; x < c0 + 16 && x < op; ++x)
                        *(gu8*)(gout + x) = sc[x - c0];
                }
            }
            lap(3);
        } else {
            // ---------------- in-HBM copies (scalar-path batches) -----------
            if constexpr (kLdsOut) {
                copy_scalar_lds(b, P.win, in, srcSize, obuf, sink, lane);
                lockstep();  // later batches read these bytes
            } else {
                copy_scalar_hbm(b, in, srcSize, gout, outSize, lane);
            }
            lap(2);
        }
        if (P.done) {
            if (lane == 0) *ret_slot = P.op;
            break;
        }
    }
    // (a failed block leaves the output its completed batches wrote, as the
    // HBM form does)
    if constexpr (kLdsOut) flush_lds(gout, obuf, P.op, lane);
    if constexpr (kStamps) {
        if (lane == 0 && dbg) {
            dbg[0] = st.acc[0];
            dbg[1] = st.acc[1];
            dbg[2] = st.acc[2];
            dbg[3] = st.batches;
            dbg[4] = st.rounds;
            dbg[5] = st.acc[3];
            dbg[6] = clock64() - t_start;     // the block's shader cycles
            dbg[7] = realtime64() - r_start;  // and its 100 MHz ticks (its clock)
        }
    }
}

// ---------------------------------------------------------------- kernels

// Dictionary bytes of block b: the dict_len[b] bytes before its output;
// anything from 64 KiB on behaves alike (no offset reaches further, and the
// reference's checkOffset is off, :93).
LZ4E_DEV int32_t dict_of(const int32_t* dict_len, uint32_t b) {
    if (!dict_len) return 0;
    const int32_t d = dict_len[b];
    return d <= 0 ? 0 : (d > 65536 ? 65536 : d);
}

// The reference's special cases (lz4e_decompress.c:113-120); true when the
// block is fully handled.
LZ4E_DEV bool special_case(const uint8_t* in, int32_t srcSize, int32_t outSize, int32_t* ret_slot,
                           uint32_t lane) {
    if (outSize == 0) {
        if (lane == 0) *ret_slot = (srcSize == 1 && in[0] == 0) ? 0 : -1;
        return true;
    }
    if (srcSize == 0) {
        if (lane == 0) *ret_slot = -1;
        return true;
    }
    if (srcSize < 0) {  // token read, then every path fails at ip == 1
        if (lane == 0) *ret_slot = -2;
        return true;
    }
    return false;
}

// kSmall: the LDS-output form for blocks of at most kSmallOut bytes without
// a dictionary (other blocks of the launch take the HBM form).  kPartial:
// dst_cap[b] is block b's target size.
template <bool kStamps, bool kSmall = false, bool kPartial = false>
__global__ __launch_bounds__(64) void decompress_kernel(const uint8_t* __restrict__ src,
                                                        const uint64_t* __restrict__ src_off,
                                                        const int32_t* __restrict__ src_len,
                                                        uint8_t* dst,
                                                        const uint64_t* __restrict__ dst_off,
                                                        const int32_t* __restrict__ dst_cap,
                                                        int32_t* __restrict__ ret, uint32_t nblocks,
                                                        uint64_t* __restrict__ dbg,
                                                        const int32_t* __restrict__ dict_len) {
    const uint32_t b = blockIdx.x;
    if (b >= nblocks) return;
    const uint32_t lane = lane_id();
    const int32_t srcSize = src_len[b];
    const int32_t outSize = dst_cap[b];
    const uint8_t* in = src + src_off[b];
    uint8_t* out = dst + dst_off[b];
    uint64_t* d = kStamps && dbg ? dbg + 8 * (size_t)b : nullptr;
    if (special_case(in, srcSize, outSize, ret + b, lane)) return;
    // LDS: [input ring + mirror] [store sink] [span] [jump table]; small
    // blocks: [store sink] [output] [jump table] [input]
    constexpr uint32_t kWaveLds = kRing + kRingPad + kSink + kSpan + kJump;
    // (+ 256 B after the staged input: the fast path's window probe reads up
    // to ~258 bytes past ip, beyond any byte it uses; 12 032 B, still 13 per CU)
    constexpr uint32_t kSmallLds = kSink + kSmallBuf + kSmallJump + kSmallBuf + 256;
    __shared__ __attribute__((aligned(16))) uint8_t smem[kSmall && kSmallLds > kWaveLds ? kSmallLds : kWaveLds];
    const int32_t dict = dict_of(dict_len, b);
    if (kSmall && dict == 0 && outSize <= kSmallOut && srcSize <= kSmallOut) {
        lu8* obuf = (lu8*)(smem + kSink);
        decode_block<kStamps, true, kPartial>(in, srcSize, out, outSize, ret + b, d, lane, obuf, nullptr,
                                    (lu16*)(obuf + kSmallBuf), 0, (lu8*)smem, obuf,
                                    obuf + kSmallBuf + kSmallJump);
    } else {
        lu8* sinkb = (lu8*)(smem + kRing + kRingPad);
        decode_block<kStamps, false, kPartial>(in, srcSize, out, outSize, ret + b, d, lane, sinkb + kSink,
                                               (lu32*)smem, (lu16*)(sinkb + kSink + kSpan), dict, sinkb);
    }
}

// The block-per-group decoder (see group_decode): block b on group
// b % (kGroupWg / kGroup) of workgroup b / (kGroupWg / kGroup).
// (6 waves per SIMD asked of the compiler: 80 VGPRs instead of 82, one wave
// more per SIMD; fio4k 0.84 -> 0.80 ms; 8 spills and is slower)
__global__ __launch_bounds__(kGroupWg, 6) void decompress_group_kernel(
    const uint8_t* __restrict__ src, const uint64_t* __restrict__ src_off,
    const int32_t* __restrict__ src_len, uint8_t* dst, const uint64_t* __restrict__ dst_off,
    const int32_t* __restrict__ dst_cap, int32_t* __restrict__ ret, uint32_t nblocks,
    const int32_t* __restrict__ dict_len, uint32_t* __restrict__ handover) {
    const uint32_t tid = threadIdx.x, s = tid % kGroup, lane = lane_id();
    const uint32_t b = blockIdx.x * (kGroupWg / kGroup) + tid / kGroup;
    // (no lane leaves early: the hand-over below is a whole-wave step)
    bool act = b < nblocks;
    int32_t r = 0, ip = 0, op = 0;
    if (act) {
        const int32_t srcSize = src_len[b], outSize = dst_cap[b];
        const uint8_t* in = src + src_off[b];
        if (special_case(in, srcSize, outSize, ret + b, s)) act = false;
        else r = group_decode(in, srcSize, dst + dst_off[b], outSize, dict_of(dict_len, b), handover != nullptr,
                              &ip, &op, s);
    }
    // hand-over list entries from each group's lane 0, one atomic per wave
    const bool ho = act && r == kLaneHandOver;
    const uint64_t m = ballot(ho && s == 0);
    if (m) {
        const uint32_t lead = ctz64(m);
        uint32_t base = 0;
        if (lane == lead) base = atomicAdd(handover, popc64(m));
        base = shfl(base, lead);
        if (ho && s == 0) {
            const uint32_t k = base + popc64(m & ((1ull << lane) - 1));
            handover[1 + 3 * k] = b;
            handover[2 + 3 * k] = (uint32_t)ip;
            handover[3 + 3 * k] = (uint32_t)op;
        }
    }
    if (act && !ho && s == 0) ret[b] = r;
}

// The blocks the group decoder handed over, one wave each from their
// sequence boundary on (decode_block's HBM form; the output before it is in
// HBM): workgroup i takes entry i, those past the count leave at once (as
// balanced as the one-wave kernel itself; a fixed grid striding over the
// list measured 1.31 vs 1.12 ms when every block was handed over).
template <bool kStamps>
__global__ __launch_bounds__(64) void decompress_resume_kernel(
    const uint8_t* __restrict__ src, const uint64_t* __restrict__ src_off,
    const int32_t* __restrict__ src_len, uint8_t* dst, const uint64_t* __restrict__ dst_off,
    const int32_t* __restrict__ dst_cap, int32_t* __restrict__ ret, const uint32_t* __restrict__ handover,
    uint64_t* __restrict__ dbg, const int32_t* __restrict__ dict_len) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[kRing + kRingPad + kSink + kSpan + kJump];
    const uint32_t lane = lane_id();
    const uint32_t cnt = handover[0];
    for (uint32_t i = blockIdx.x; i < cnt; i += gridDim.x) {  // (one pass: grid = every block)
        const uint32_t b = handover[1 + 3 * i];
        const int32_t ip0 = (int32_t)handover[2 + 3 * i], op0 = (int32_t)handover[3 + 3 * i];
        uint64_t* d = kStamps && dbg ? dbg + 8 * (size_t)b : nullptr;
        lu8* sinkb = (lu8*)(smem + kRing + kRingPad);
        decode_block<kStamps>(src + src_off[b], src_len[b], dst + dst_off[b], dst_cap[b], ret + b, d, lane,
                              sinkb + kSink, (lu32*)smem, (lu16*)(sinkb + kSink + kSpan), dict_of(dict_len, b),
                              sinkb, nullptr, nullptr, ip0, op0);
        lockstep();  // the next block reuses the LDS
    }
}

// The pipelined decoder (lz4e_dec_pipe.h): wave 0 parses, waves 1..3 copy.
// kPartial (compile time: the kernel sits at its register cap): dst_cap[b]
// is block b's target size; only the parser differs.
template <bool kStamps, bool kPartial = false>
__global__ __launch_bounds__(kPipeWaves * kWave, kPipeMinWg) void decompress_pipe_kernel(
    const uint8_t* __restrict__ src, const uint64_t* __restrict__ src_off,
    const int32_t* __restrict__ src_len, uint8_t* dst, const uint64_t* __restrict__ dst_off,
    const int32_t* __restrict__ dst_cap, int32_t* __restrict__ ret, uint32_t nblocks,
    uint64_t* __restrict__ dbg, const int32_t* __restrict__ dict_len,
    const uint32_t* __restrict__ order) {
    __shared__ __attribute__((aligned(16))) PipeLds S;
    if (blockIdx.x >= nblocks) return;
    const uint32_t b = order ? order[blockIdx.x] : blockIdx.x;
    const uint32_t tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const int32_t srcSize = src_len[b];
    const int32_t outSize = dst_cap[b];
    const uint8_t* in = src + src_off[b];
    uint8_t* gout = dst + dst_off[b];
    if (special_case(in, srcSize, outSize, ret + b, tid)) return;
    if (tid < kPipeRecs) {
        S.pub[tid] = -1;
        S.con[tid] = (int32_t)tid - (int32_t)kPipeRecs;
    }
    if (tid == 0) {
        S.nb_total = INT32_MAX;
        S.resolved = 0;
        S.stored = 0;
        S.abort = 0;
        S.beat = 0;
        S.result = kPipeAbort;
        S.spin_max = kSpinMax + (kSpinBytesShift < 31 ? (uint32_t)srcSize >> kSpinBytesShift : 0u);
    }
    __syncthreads();
    PipeStamps st;
    __shared__ uint64_t st_rows[kStamps ? kPipeWaves * kStSlots : 1];
    [[maybe_unused]] uint64_t t_start = 0, r_start = 0;
    if (kStamps) {
        st.acc = st_rows + wave * kStSlots;
        if (lane < kStSlots) st.acc[lane] = 0;
        st.t = clock64();
        t_start = st.t;
        r_start = realtime64();
    }

    if (wave == 0) {
        // ---------------- parser ----------------
        // (the critical path of the block: first in issue arbitration)
        __builtin_amdgcn_s_setprio(3);
        Parse P;
        P.init(in, srcSize, outSize, (lu32*)S.ring, lane, dict_of(dict_len, b));
        int32_t j = 0, lo1 = 0, lo2 = 0, hi1 = 0, hi2 = 0;
        bool hbm1 = false, hbm2 = false;
        for (;;) {
            Batch bt;
            const int32_t lo = P.op;
            const ParseResult pr = parse_batch<true, kPartial>(P, bt, lane, kPipeOut, [&](int k) {
                if (kStamps) st.lap(true, kStPWin + k);
            });
            st.lap(kStamps, kStParse);
            if (pr == kParseFail) {
                if (lane == 0) S.result = -P.ip - 1;
                break;
            }
            // far line: sources before it are read from HBM (see copy_fast)
            int32_t F = j >= 2 ? lo2 : 0;
            if (j >= 2 && hbm2) F = F > hi2 ? F : hi2;
            if (j >= 1 && hbm1) F = F > hi1 ? F : hi1;
            const uint32_t slot = (uint32_t)j % kPipeRecs;
            if (!wait_for(S, [&] { return lds_acquire(&S.con[slot]) == j - (int32_t)kPipeRecs; },
                          [&] { return lds_acquire(&S.beat) + lds_acquire(&S.con[slot]); })) {
                lds_release(&S.abort, 1);
                break;
            }
            st.lap(kStamps, kStPWait);
            S.rec[slot][0][lane] = bt.ls;
            S.rec[slot][1][lane] = bt.L;
            S.rec[slot][2][lane] = bt.op;
            S.rec[slot][3][lane] = bt.off;
            S.rec[slot][4][lane] = bt.M;
            if (lane < kHdrWords) {
                const int32_t h[kHdrWords] = {(int32_t)bt.n, pr == kParsedScalar ? kKindHbm : kKindFast,
                                              lo, P.op, F, lo1, lo2, 0};
                int32_t v = 0;
#pragma unroll
                for (uint32_t q = 0; q < kHdrWords; ++q) v = lane == q ? h[q] : v;
                S.hdr[slot][lane] = v;
            }
            lds_release(&S.pub[slot], j);
            lo2 = lo1;
            hi2 = hi1;
            hbm2 = hbm1;
            lo1 = lo;
            hi1 = P.op;
            hbm1 = pr == kParsedScalar;
            j++;
            if (P.done) {
                if (lane == 0) S.result = P.op;
                break;
            }
        }
        lds_release(&S.nb_total, j);
        st.lap(kStamps, kStParse);
    } else {
        // ---------------- copiers ----------------
        const uint32_t c = wave - 1;
        for (int32_t j = (int32_t)c;; j += kCopiers) {
            const uint32_t slot = (uint32_t)j % kPipeRecs;
            st.lap(kStamps, kStWork);
            const bool ok = wait_for(
                S, [&] { return lds_acquire(&S.pub[slot]) == j || lds_acquire(&S.nb_total) <= j; },
                [&] { return lds_acquire(&S.beat) + lds_acquire(&S.pub[slot]); });
            st.lap(kStamps, kStRec);
            if (!ok) {
                lds_release(&S.abort, 1);
                break;
            }
            if (lds_acquire(&S.pub[slot]) != j) break;  // the parser ended before batch j
            Batch bt;
            bt.ls = S.rec[slot][0][lane];
            bt.L = S.rec[slot][1][lane];
            bt.op = S.rec[slot][2][lane];
            bt.off = S.rec[slot][3][lane];
            bt.M = S.rec[slot][4][lane];
            int32_t hdr[kHdrWords];
#pragma unroll
            for (uint32_t q = 0; q < kHdrWords; ++q) hdr[q] = (int32_t)uni((uint32_t)S.hdr[slot][q]);
            bt.n = (uint32_t)hdr[kHdrN];
            lds_release(&S.con[slot], j);
            st.bump(kStamps, kStBatches);
            if (hdr[kHdrKind] == kKindHbm) {
                // every earlier batch in HBM, then in place
                if (!spin<kStamps>(S, [&] { return lds_acquire(&S.stored) >= hdr[kHdrLo]; },
                                   [&] { return lds_acquire(&S.stored) + lds_acquire(&S.beat); }, st, kStStore)) {
                    lds_release(&S.abort, 1);
                    break;
                }
                copy_scalar_hbm<4>(bt, in, srcSize, gout, outSize, lane, [&] {
                    // (called in lane-divergent loops: lane 0 alone, no ordering)
                    if (lane == 0)
                        __hip_atomic_fetch_add(&S.beat, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                });
                stores_done();
                lds_release(&S.resolved, j + 1);
                lds_release(&S.stored, hdr[kHdrHi]);
                st.lap(kStamps, kStVm);
            } else if (!copy_fast<kStamps>(S, c, j, bt, hdr, in, srcSize, gout, lane, st)) {
                lds_release(&S.abort, 1);
                break;
            }
        }
    }
    // Every wave has left its loop (each wait is bounded by the watchdog):
    // the block's value is the parse's unless a wave gave up, which fails
    // the whole block -- the parser may finish its parse without ever
    // waiting, so only here are all waves' outcomes known.
    __syncthreads();
    if (tid == 0) ret[b] = __hip_atomic_load(&S.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
                               ? kPipeAbort
                               : S.result;
    if constexpr (kStamps) {
        if (lane == 0 && wave == 0) {
            st.acc[kStT] = clock64() - t_start;     // the block's shader cycles
            st.acc[kStR] = realtime64() - r_start;  // and its 100 MHz ticks (its clock)
        }
        if (lane == 0 && dbg) {
            uint64_t* d = dbg + kStSlots * (size_t)b;
            for (int k = 0; k < kStSlots; ++k)
                if (st.acc[k]) atomicAdd((unsigned long long*)(d + k), (unsigned long long)st.acc[k]);
        }
    }
}

// ---------------------------------------------------------------- the decoder choice

// Blocks whose capacity lies in [kPipeMinCap, kPipeMaxCap) take the
// pipelined decoder.  Small blocks parse in a few batches, and one wave each
// keeps more of them resident.  Large blocks (256 KiB: ~560 batches each)
// decode faster one wave per block as well: 20 resident blocks per CU
// against 6 four-wave ones, so a 3 815-block batch runs in one round of
// workgroups instead of 2.5 (text256k decompress-only 4.33 -> 3.04 ms,
// profiles/r04/decmodes.txt); at 64 KiB the pipelined decoder's per-block
// speed wins (silesia64k 0.85 vs 1.20 ms).
constexpr uint32_t kPipeMinCap = 16384;
constexpr uint32_t kPipeMaxCap = 131072;
// Batches that leave most of the pipelined decoder's round of workgroups
// (kOrderMin) unused are latency-bound whatever the block size: the pipelined
// decoder overlaps a block's parse with its copies (drop-in single call,
// 4 KiB text: 71 us p50 against 82 us for the LDS form and 92 us one-wave,
// tools/single_call_trace.py; 1 024 4 KiB Silesia-proxy blocks 0.085 ms
// against 0.101 / 0.102, fio 0.036 / 0.034 / 0.035; at 3 072 blocks the LDS
// form wins, 0.115 against 0.162 ms; tools/decmodes.py).
constexpr uint32_t kLatencyMaxBlocks = 1024;
// Batches of at least this many blocks of <= kSmallOut bytes take the group
// decoder (blocks that open with a short sequence go straight on to the
// one-wave decoder).  Fio-style blocks (tools/decmodes.py, group vs one-wave
// vs LDS form): 4 096 blocks 0.080 / 0.055 / 0.067 ms, 16 384 0.093 / 0.170 /
// 0.189, 65 536 0.279 / 0.717 / 0.693, 262 144 0.89 / 2.76 / 2.69; 4 KiB
// Silesia-proxy blocks, all handed over: 65 536 1.215 / 1.131 / 1.316
// (profiles/r05/group_decoder/).
constexpr uint32_t kGroupMinBlocks = 16384;
// Batches of small blocks that fit one round of the LDS form's workgroups
// (11.8 KiB of LDS: 13 per CU) take that form: no HBM round trip inside a
// block's decode (drop-in single call, 4 KiB text: 89 -> 79 us p50); with
// more rounds the one-wave form's 20 workgroups per CU win (65 536 4 KiB
// Silesia-proxy blocks: 1.13 vs 1.30 ms).
constexpr uint32_t kSmallMaxBlocks = 256 * 13;

// Auto mode: the decoder for a batch of nblocks blocks whose capacities are
// at most max_cap (0: unknown), in the order of DESIGN.md §3.2.
constexpr uint32_t pick_decoder(uint32_t max_cap, uint32_t nblocks) {
    if (max_cap == 0 || (max_cap >= kPipeMinCap && max_cap < kPipeMaxCap)) return kDecPipe;
    if (nblocks <= kLatencyMaxBlocks) return kDecPipe;
    const bool small = max_cap <= (uint32_t)kSmallOut;
    if (small && nblocks >= kGroupMinBlocks) return kDecGroup;
    if (small && nblocks <= kSmallMaxBlocks) return kDecSmall;
    return kDecWave;
}
// Both sides of every threshold.
static_assert(pick_decoder(0, 1) == kDecPipe && pick_decoder(0, 100000) == kDecPipe);
static_assert(pick_decoder(16384, 5000) == kDecPipe && pick_decoder(131071, 5000) == kDecPipe);
static_assert(pick_decoder(16383, 5000) == kDecWave && pick_decoder(131072, 5000) == kDecWave);
static_assert(pick_decoder(4608, 16384) == kDecGroup && pick_decoder(4608, 16383) == kDecWave);
static_assert(pick_decoder(4609, 16384) == kDecWave);
static_assert(pick_decoder(4608, 1024) == kDecPipe && pick_decoder(4608, 1025) == kDecSmall);
static_assert(pick_decoder(4608, 3328) == kDecSmall && pick_decoder(4608, 3329) == kDecWave);
static_assert(pick_decoder(4609, 1024) == kDecPipe && pick_decoder(4609, 1025) == kDecWave);
static_assert(pick_decoder(300000, 1024) == kDecPipe && pick_decoder(300000, 1025) == kDecWave);

// Launch order of the pipelined decoder when the batch takes more than one
// round of workgroups (lz4e_order.h): a block's decode time grows with its
// sequence count, estimated by its compressed size; frames within 1/16 of
// their capacity (stored / incompressible data: a few long literal runs) are
// the lightest.
constexpr uint32_t kOrderMin = 256 * kPipeMinWg;  // one round: 256 CUs x 6 resident pipelined workgroups
static_assert(kOrderMin == 1536);
struct DecodeWeight {
    const int32_t* src_len;
    const int32_t* dst_cap;
    LZ4E_DEV uint32_t operator()(uint32_t b) const {
        const int64_t c = src_len[b], cap = dst_cap[b];
        if (cap <= 0 || c >= cap - cap / 16) return kOrderBuckets - 1;
        const int64_t q = c <= 0 ? 0 : c * (kOrderBuckets - 1) / cap;  // < 63
        return (uint32_t)(kOrderBuckets - 2 - (q < kOrderBuckets - 2 ? q : kOrderBuckets - 2));
    }
};

// kPartial: a partial launch (DecompressBatch::partial, no dictionary):
// the same choice with the group decoder, which has no partial form,
// replaced by the one-wave decoder (LZ4E_DECOMPRESS_MODE=g: auto).
template <bool kStamps, bool kPartial = false>
hipError_t launch_impl(const DecompressBatch& a, hipStream_t stream, uint64_t* dbg) {
    if (a.nblocks == 0) return hipSuccess;
    if constexpr (kPartial) {
        if (a.dict_len || a.mode == kDecGroupNoBail) return hipErrorInvalidValue;
    }
    // LZ4E_DECOMPRESS_MODE=w|p|s|g (one-wave, pipelined, LDS form, group)
    // overrides auto mode for A/B experiments; any other value is auto.
    static const char* env = getenv("LZ4E_DECOMPRESS_MODE");
    uint32_t mode = a.mode;
    if (mode == kDecAuto && env)
        mode = env[0] == 'w'   ? kDecWave
               : env[0] == 'p' ? kDecPipe
               : env[0] == 's' ? kDecSmall
               : env[0] == 'g' ? (kPartial ? kDecAuto : kDecGroup)
                               : kDecAuto;
    if (mode == kDecAuto) mode = pick_decoder(a.max_cap, a.nblocks);
    if (kPartial && mode == kDecGroup) mode = kDecWave;
    if (mode == kDecPipe) {
        const int om = launch_order_mode(false);
        uint32_t* order = nullptr;
        if ((om == kOrderAlways || (om == kOrderAuto && a.nblocks > kOrderMin)) &&
            hipMallocAsync((void**)&order, sizeof(uint32_t) * a.nblocks, stream) == hipSuccess) {
            hipLaunchKernelGGL((order_kernel<DecodeWeight>), dim3(1), dim3(kOrderThreads), 0, stream,
                               DecodeWeight{a.src_len, a.dst_cap}, a.nblocks, order);
        } else {
            (void)hipGetLastError();  // a failed pool allocation only costs the ordering
            order = nullptr;
        }
        hipLaunchKernelGGL((decompress_pipe_kernel<kStamps, kPartial>), dim3(a.nblocks), dim3(kPipeWaves * kWave),
                           0, stream, a.src, a.src_off, a.src_len, a.dst, a.dst_off, a.dst_cap, a.ret,
                           a.nblocks, dbg, a.dict_len, (const uint32_t*)order);
        const hipError_t err = hipGetLastError();
        if (order) (void)hipFreeAsync(order, stream);
        return err;
    }
    if (!kPartial && (mode == kDecGroup || mode == kDecGroupNoBail)) {
        // hand-over list (count + 3 words per block); without it (or in the
        // no-hand-over test mode) every group decodes its block to the end
        uint32_t* ho = nullptr;
        if (mode == kDecGroup && (hipMallocAsync((void**)&ho, 4 + 12 * (size_t)a.nblocks, stream) != hipSuccess ||
                                  hipMemsetAsync(ho, 0, 4, stream) != hipSuccess)) {
            (void)hipGetLastError();
            if (ho) (void)hipFreeAsync(ho, stream);
            ho = nullptr;
        }
        hipLaunchKernelGGL(decompress_group_kernel, dim3((a.nblocks + kGroupWg / kGroup - 1) / (kGroupWg / kGroup)),
                           dim3(kGroupWg), 0, stream, a.src, a.src_off, a.src_len, a.dst, a.dst_off, a.dst_cap,
                           a.ret, a.nblocks, a.dict_len, ho);
        hipError_t err = hipGetLastError();
        if (ho) {
            if (err == hipSuccess) {
                hipLaunchKernelGGL((decompress_resume_kernel<kStamps>), dim3(a.nblocks), dim3(kWave), 0, stream, a.src,
                                   a.src_off, a.src_len, a.dst, a.dst_off, a.dst_cap, a.ret, ho, dbg,
                                   a.dict_len);
                err = hipGetLastError();
            }
            (void)hipFreeAsync(ho, stream);
        }
        return err;
    }
    if (mode == kDecSmall)
        hipLaunchKernelGGL((decompress_kernel<kStamps, true, kPartial>), dim3(a.nblocks), dim3(kWave), 0, stream,
                           a.src, a.src_off, a.src_len, a.dst, a.dst_off, a.dst_cap, a.ret, a.nblocks,
                           dbg, a.dict_len);
    else
        hipLaunchKernelGGL((decompress_kernel<kStamps, false, kPartial>), dim3(a.nblocks), dim3(kWave), 0, stream,
                           a.src, a.src_off, a.src_len, a.dst, a.dst_off, a.dst_cap, a.ret, a.nblocks,
                           dbg, a.dict_len);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_decompress(const DecompressBatch& a, hipStream_t stream) {
    return a.partial ? launch_impl<false, true>(a, stream, nullptr) : launch_impl<false>(a, stream, nullptr);
}

// (the stamped build has no partial form)
hipError_t launch_decompress_stamped(const DecompressBatch& a, hipStream_t stream, uint64_t* dbg) {
    return a.partial ? hipErrorInvalidValue : launch_impl<true>(a, stream, dbg);
}

}  // namespace lz4e
