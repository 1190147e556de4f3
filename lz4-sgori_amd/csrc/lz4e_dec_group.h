// lz4e_dec_group.h -- the block-per-group decoder's device code (included by
// lz4e_decompress.hip alone; decompress_group_kernel is there).
//
// Large batches of small blocks whose sequences are long (fio-style 4 KiB
// buffers: ~14 sequences of ~300 bytes) leave the one-wave decoder parsing
// one scalar sequence at a time with the other 63 lanes idle: ~24 k issue
// cycles per block (tools/wavestamps.py).  Here a group of kGroup lanes
// decodes a block of its own (64 / kGroup blocks per wave): the reference's
// scalar loop (lz4e_decompress.c:123-446, the same checks in the same order
// as parse_batch's exact path, so values and error codes are the
// reference's), run by every lane of the group, with each literal run and
// match copied by the whole group, up to 256 bytes per round.  Round 4's
// version ran one block per lane with 16-byte copies per lane (fio4k 1.39
// ms).
#pragma once

#include "lz4e_dec_copy.h"

namespace lz4e {

namespace {

typedef __attribute__((address_space(1))) const uint8_t gcu8;
LZ4E_DEV uint32_t ldb(const uint8_t* p, int32_t i) { return ((gcu8*)p)[i]; }
// Global-address-space stores of the group decoder (flat ones would also
// count on lgkmcnt and make every wait a wait for both counters).
typedef __attribute__((address_space(1))) uint64_t gu64w;
typedef __attribute__((address_space(1))) uint16_t gu16w;
LZ4E_DEV void gst_tail(uint8_t* p, uint4 c, uint32_t n) {
    uint64_t lo = ((uint64_t)c.y << 32) | c.x, hi = ((uint64_t)c.w << 32) | c.z;
    if (n & 8) {
        *(gu32w*)p = (uint32_t)lo;
        *(gu32w*)(p + 4) = (uint32_t)(lo >> 32);
        p += 8;
        lo = hi;
        hi = 0;
    }
    if (n & 4) {
        *(gu32w*)p = (uint32_t)lo;
        p += 4;
        lo = (lo >> 32) | (hi << 32);
    }
    if (n & 2) {
        *(gu16w*)p = (uint16_t)lo;
        p += 2;
        lo >>= 16;
    }
    if (n & 1) *(gu8*)p = (uint8_t)lo;
}

// A lane's 16-byte window of its input (token, extension and offset bytes
// mostly come from one load): bytes [base, base + 16) in w.
struct LaneIn {
    const uint8_t* in;
    int32_t n, base;
    uint4 w;
    LZ4E_DEV void fill(int32_t p) {
        base = p;
        if (p + 16 <= n) {
            w = ldg16(in + p);
        } else {
            uint32_t x[4] = {0, 0, 0, 0};
#pragma unroll
            for (int32_t k = 0; k < 16; ++k)
                if (p + k < n) x[k >> 2] |= ldb(in, p + k) << (8 * (k & 3));
            w = make_uint4(x[0], x[1], x[2], x[3]);
        }
    }
    // byte p (< n)
    LZ4E_DEV uint32_t byte(int32_t p) {
        if ((uint32_t)(p - base) >= 16) fill(p);
        return pat_byte(w, (uint32_t)(p - base));
    }
};

// A group whose block turns out to hold short sequences (fewer than
// kLaneBailBytes output bytes per sequence over the last kLaneBailSeqs
// sequences: text, tables) hands the block over at a sequence boundary --
// such a block would hold its wave for milliseconds: group_decode returns
// kLaneHandOver with (*ip_out, *op_out), and the one-wave decoder resumes
// there (a group pays a few round trips per sequence, which only long
// sequences amortise).  The thresholds are round 5's; DESIGN.md §3.2 gives
// what the hand-over costs text-like blocks.
constexpr int32_t kLaneHandOver = INT32_MIN;
constexpr int32_t kLaneBailSeqs = 4;
constexpr int32_t kLaneBailBytes = 64;
constexpr uint32_t kLaneFirstLit = 200;  // (fio-style: 256)

// Lanes per block: groups of 8 take 0.88-0.89 ms on fio4k against 1.10 /
// 0.91 / 0.94 / 1.42 ms for 2 / 4 / 16 / 32 (profiles/r05/group_decoder/).
constexpr uint32_t kGroup = 8;
// Threads per workgroup: one wave is fastest, fio4k 0.836 ms against 0.850 /
// 0.892 / 0.988 / 1.012 ms for 128 / 256 / 512 / 1024 threads
// (profiles/r05/group_decoder/wg/).
constexpr uint32_t kGroupWg = 64;
// A round moves up to 256 bytes of a block: kPer 16-byte chunks per lane,
// contiguous per block, every load of the round issued before its first
// store (loads and stores share one in-order counter, so a load after a
// store waits for the store).  The group's lanes run the same scalar parse
// (their input window loads are one address per group).  In the copies
// below s is the lane's index in its group; dst and src are the group's.
constexpr int32_t kRound = 256;
constexpr uint32_t kPer = kRound / (16 * kGroup);
static_assert(kPer * 16 * kGroup == kRound && kGroupWg % kGroup == 0 && kWave % kGroup == 0,
              "a round is whole 16-byte chunks per lane, a wave whole groups");

// 16 bytes at p (n of them wanted), byte by byte where a 16-byte load
// would reach lim.
LZ4E_DEV uint4 ld16_lim(const uint8_t* p, uint32_t n, const uint8_t* lim) {
    if (p + 16 <= lim) return ldg16(p);
    uint32_t x[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < n; ++k) x[k >> 2] |= ldb(p, (int32_t)k) << (8 * (k & 3));
    return make_uint4(x[0], x[1], x[2], x[3]);
}
LZ4E_DEV void st16_n(uint8_t* p, uint4 v, uint32_t n) {
    if (n == 16) stg16(p, v);
    else gst_tail(p, v, n);
}

// Literal run: dst[t] = src[t] for t in [0, len), src a different buffer;
// loads never read at or past lim.
LZ4E_DEV void group_copy(uint8_t* dst, const uint8_t* src, int32_t len, const uint8_t* lim, uint32_t s) {
    for (int32_t t0 = 0; t0 < len; t0 += kRound) {
        uint4 v[kPer];
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) {
            const int32_t q = t0 + 16 * (int32_t)(s + kGroup * i);
            if (q < len) v[i] = ld16_lim(src + q, (uint32_t)(len - q < 16 ? len - q : 16), lim);
        }
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) {
            const int32_t q = t0 + 16 * (int32_t)(s + kGroup * i);
            if (q < len) st16_n(dst + q, v[i], (uint32_t)(len - q < 16 ? len - q : 16));
        }
    }
}

// 16 bytes of the period p (off < 16 bytes, pattern byte j = p's byte j)
// starting at phase j0.
LZ4E_DEV uint4 period16(uint4 p, uint32_t off, uint32_t j0) {
    uint32_t w[4] = {0, 0, 0, 0};
    uint32_t j = j0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        w[k >> 2] |= pat_byte(p, j) << (8 * (k & 3));
        j = (j + 1 == off) ? 0 : j + 1;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// Match: dst[t] = dst[t - off] for t in [0, len), any overlap (offset 0:
// zeros).  Periods below 16: every lane builds its 16-byte pieces from the
// period in registers (one pass); otherwise pieces [t, t + c) from D bytes
// back, D a multiple of off with c <= D <= t (doubling, up to 256 bytes a
// piece), so every source byte is written before its piece is read (same-wave
// stores and loads to one address are ordered; group_fence keeps the compiler
// from moving the loads up).  Loads never read at or past lim.
LZ4E_DEV void group_match(uint8_t* dst, uint32_t off, int32_t len, const uint8_t* lim, uint32_t s) {
    if (off == 0 || off < 16) {
        uint4 p = make_uint4(0, 0, 0, 0);
        if (off != 0) {
            if (dst - off + 16 <= lim) {
                p = ldg16(dst - off);
            } else {
                uint32_t x[4] = {0, 0, 0, 0};
                for (uint32_t k = 0; k < off; ++k) x[k >> 2] |= ldb(dst, (int32_t)k - (int32_t)off) << (8 * (k & 3));
                p = make_uint4(x[0], x[1], x[2], x[3]);
            }
        }
        for (int32_t t = 16 * (int32_t)s; t < len; t += 16 * (int32_t)kGroup) {
            const uint32_t n = (uint32_t)(len - t < 16 ? len - t : 16);
            const uint4 v = off == 0 ? make_uint4(0, 0, 0, 0) : period16(p, off, (uint32_t)t % off);
            st16_n(dst + t, v, n);
        }
        return;
    }
    uint32_t D = off;
    for (int32_t t = 0; t < len;) {
        int32_t c = len - t < (int32_t)D ? len - t : (int32_t)D;
        c = c < kRound ? c : kRound;
        uint4 v[kPer];
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) {
            const int32_t q = 16 * (int32_t)(s + kGroup * i);
            if (q < c) v[i] = ld16_lim(dst + t + q - (int32_t)D, (uint32_t)(c - q < 16 ? c - q : 16), lim);
        }
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) {
            const int32_t q = 16 * (int32_t)(s + kGroup * i);
            if (q < c) st16_n(dst + t + q, v[i], (uint32_t)(c - q < 16 ? c - q : 16));
        }
        group_fence(kGroup);
        t += c;
        while (2 * D <= (uint32_t)t) D *= 2;
    }
}

// One block on one group: the return value of LZ4E_decompress_safe (D
// dictionary bytes before out), or kLaneHandOver with (*ip_out, *op_out).
LZ4E_DEV int32_t group_decode(const uint8_t* in, int32_t srcSize, uint8_t* out, int32_t outSize,
                              int32_t D, bool may_bail, int32_t* ip_out, int32_t* op_out, uint32_t s) {
    const int32_t iend = srcSize, oend = outSize;
    const int32_t shortiend = iend - kFastLitMax - 2;              // :100-101
    const int32_t shortoend = oend - kFastLitMax - kFastMatchMax;  // :102-103
    const uint8_t* ilim = in + srcSize;
    const uint8_t* olim = out + outSize;
    int32_t ip = 0, op = 0;
    LaneIn I;
    I.in = in;
    I.n = srcSize;
    I.fill(0);
    if (may_bail) {
        // a block that opens with a short literal run is most likely one of
        // short sequences: straight to the one-wave decoder (nor does one
        // whose first match is short: both must be long)
        const uint32_t t0 = I.byte(0);
        const uint32_t l0 = (t0 >> 4) == 15 && srcSize > 1 ? 15 + I.byte(1) : t0 >> 4;
        const int32_t q = 2 + (int32_t)l0 + 2;  // the first match's extension byte
        const bool long_m = l0 >= kLaneFirstLit && (t0 & 15) == 15 && q < srcSize && I.byte(q) >= 64 - 19;
        if (!long_m) {
            *ip_out = 0;
            *op_out = 0;
            return kLaneHandOver;
        }
    }
    int32_t op_chk = 0;  // output position at the last check
    for (int32_t nseq = 0;; ++nseq) {
        if (may_bail && nseq >= kLaneBailSeqs && nseq % kLaneBailSeqs == 0) {
            if (op - op_chk >= kLaneBailBytes * kLaneBailSeqs) {
                op_chk = op;
            } else {
                *ip_out = ip;
                *op_out = op;
                return kLaneHandOver;
            }
        }
        const uint32_t token = I.byte(ip);
        ip++;
        uint32_t length = token >> 4;  // saturates at kSat
        int32_t offset;
        if (length != 15 && ip < shortiend && op <= shortoend) {
            // two-stage shortcut (:150-191)
            if (length) group_copy(out + op, in + ip, (int32_t)length, ilim, s);
            op += (int32_t)length;
            ip += (int32_t)length;
            offset = (int32_t)(I.byte(ip) | (I.byte(ip + 1) << 8));
            ip += 2;
            length = token & 15;
            if (length != 15 && offset >= 8 && op >= offset) {
                group_fence(kGroup);
                group_match(out + op, (uint32_t)offset, (int32_t)length + 4, olim, s);
                group_fence(kGroup);
                op += (int32_t)length + 4;
                continue;
            }
        } else {
            if (length == 15) {  // :194-220
                if (ip >= iend - 15) break;
                uint32_t sb;
                do {
                    sb = I.byte(ip);
                    ip++;
                    length = length + sb > kSat ? kSat : length + sb;
                } while (ip < iend - 15 && sb == 255);
            }
            const uint32_t cpy = (uint32_t)op + length;  // :223-288
            const uint32_t iln = (uint32_t)ip + length;
            if (ugt(cpy, oend - 12) || ugt(iln, iend - 8)) {
                if (iln != (uint32_t)iend || ugt(cpy, oend)) break;
                group_copy(out + op, in + ip, (int32_t)length, ilim, s);  // final literal run
                return (int32_t)cpy;
            }
            if ((uint32_t)(ip + (int32_t)length - I.base) + 2 > 16) I.fill(ip + (int32_t)length);
            group_copy(out + op, in + ip, (int32_t)length, ilim, s);
            ip += (int32_t)length;
            op = (int32_t)cpy;
            offset = (int32_t)(I.byte(ip) | (I.byte(ip + 1) << 8));  // :291-296
            ip += 2;
            length = token & 15;
        }
        // _copy_match (:298-336, :422-431)
        if (op - offset + D < 0) break;
        if (length == 15) {
            uint32_t sb;
            bool bad = false;
            do {
                sb = I.byte(ip);
                ip++;
                if (ip > iend - 5) {
                    bad = true;
                    break;
                }
                length = length + sb > kSat ? kSat : length + sb;
            } while (sb == 255);
            if (bad) break;
        }
        if (ugt((uint32_t)op + length + 4, oend - 5)) break;
        group_fence(kGroup);  // the literal run's stores before the match's loads
        group_match(out + op, (uint32_t)offset, (int32_t)length + 4, olim, s);
        group_fence(kGroup);
        op += (int32_t)length + 4;
    }
    return -ip - 1;
}

}  // namespace

}  // namespace lz4e
