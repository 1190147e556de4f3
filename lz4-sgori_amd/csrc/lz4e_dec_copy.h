// lz4e_dec_copy.h -- the copy primitives the batch decoders share (included
// by lz4e_decompress.hip alone): HBM and LDS copies per lane and per wave,
// the pointer-jumping chain resolution, and a scalar-path batch's copies in
// HBM.
//
// Overlapping matches follow LZ semantics out[op + t] = out[op - off + t]
// byte by byte; offset 0 writes zeros, which is what the reference's
// LZ4_write32(op, offset) + overlap copy produce (lz4e_decompress.c:313,
// 407-415).  Same-wave stores and loads to one global address are ordered by
// the hardware (one vector L1 per CU), and wavefront-scope fences keep the
// compiler from moving a phase's loads above the previous phase's stores.
#pragma once

#include "lz4e_dec_parse.h"

namespace lz4e {

namespace {

constexpr int32_t kLongPiece = 64;  // longer literal runs / matches go to the whole wave
constexpr uint32_t kSink = 4 * kWave;  // LDS: a dword per lane for unwanted stores
constexpr uint16_t kFinal = 0xFFFF;    // jump entry of a byte whose value is final

// ---------------------------------------------------------------- HBM copies

LZ4E_DEV uint4 ld16(const uint8_t* p) { return *reinterpret_cast<const uint4*>(p); }
// Global-address-space forms (flat accesses would also count on lgkmcnt,
// coupling them to every LDS wait).
typedef __attribute__((address_space(1))) uint8_t gu8;
typedef __attribute__((address_space(1))) uint32_t gu32w;
LZ4E_DEV uint4 ldg16(const uint8_t* p) {
    const gu32w* q = (const gu32w*)p;
    return make_uint4(q[0], q[1], q[2], q[3]);
}
LZ4E_DEV void stg16(uint8_t* p, uint4 v) {
    gu32w* q = (gu32w*)p;
    q[0] = v.x;
    q[1] = v.y;
    q[2] = v.z;
    q[3] = v.w;
}
LZ4E_DEV void st16(uint8_t* p, uint4 v) { *reinterpret_cast<uint4*>(p) = v; }

// Exact store of n (< 16) bytes of chunk c at p: 8/4/2/1-byte pieces.
LZ4E_DEV void st_tail(uint8_t* p, uint4 c, uint32_t n) {
    uint64_t lo = ((uint64_t)c.y << 32) | c.x, hi = ((uint64_t)c.w << 32) | c.z;
    if (n & 8) {
        *reinterpret_cast<uint64_t*>(p) = lo;
        p += 8;
        lo = hi;
        hi = 0;
    }
    if (n & 4) {
        *reinterpret_cast<uint32_t*>(p) = (uint32_t)lo;
        p += 4;
        lo = (lo >> 32) | (hi << 32);
    }
    if (n & 2) {
        *reinterpret_cast<uint16_t*>(p) = (uint16_t)lo;
        p += 2;
        lo >>= 16;
    }
    if (n & 1) *p = (uint8_t)lo;
}

// Per-lane copy of len (1..64) bytes, src entirely before dst or in another
// buffer: every load is issued before the first store (one round trip).
// Loads never read at or past lim (byte path near the end of a buffer).
LZ4E_DEV void lane_copy64(uint8_t* dst, const uint8_t* src, int32_t len, const uint8_t* lim) {
    const uint32_t nch = ((uint32_t)len + 15) >> 4;
    if (src + 16 * nch > lim) {
        for (int32_t t = 0; t < len; ++t) dst[t] = src[t];
        return;
    }
    const uint4 c0 = ld16(src);
    uint4 c1 = c0, c2 = c0, c3 = c0;
    if (nch > 1) c1 = ld16(src + 16);
    if (nch > 2) c2 = ld16(src + 32);
    if (nch > 3) c3 = ld16(src + 48);
    const uint32_t full = (uint32_t)len >> 4, tail = (uint32_t)len & 15;
    if (full > 0) st16(dst, c0);
    if (full > 1) st16(dst + 16, c1);
    if (full > 2) st16(dst + 32, c2);
    if (full > 3) st16(dst + 48, c3);
    if (tail) {
        const uint4 ct = full == 0 ? c0 : full == 1 ? c1 : full == 2 ? c2 : c3;
        st_tail(dst + 16 * full, ct, tail);
    }
}

// Byte j (< 16) of a 16-byte register pattern.
LZ4E_DEV uint32_t pat_byte(uint4 p, uint32_t j) {
    const uint32_t w = j < 8 ? (j < 4 ? p.x : p.y) : (j < 12 ? p.z : p.w);
    return (w >> ((j & 3) * 8)) & 0xFFu;
}

// Per-lane match copy of len (1..64) bytes at dst with offset off; the bytes
// before dst are final.
LZ4E_DEV void lane_match(uint8_t* dst, uint32_t off, int32_t len, const uint8_t* lim) {
    if ((int32_t)off >= len) {
        lane_copy64(dst, dst - off, len, lim);  // no self-overlap
        return;
    }
    if (off >= 16) {
        // self-overlap with a period >= 16: the first period, then chunks
        // copied from the start, each at most as long as what is written
        lane_copy64(dst, dst - off, (int32_t)off, lim);
        for (int32_t t = (int32_t)off; t < len;) {
            const int32_t c = len - t < t ? len - t : t;
            lane_copy64(dst + t, dst, c, lim);
            t += c;
        }
        return;
    }
    if (off == 0) {
        for (int32_t t = 0; t < len; ++t) dst[t] = 0;
        return;
    }
    // 1 <= off < 16: repeat the final period [dst-off, dst) 4 bytes at a time
    // (the 16-byte load may cover bytes at/after dst: never used)
    if (dst - off + 16 > lim) {
        for (int32_t t = 0; t < len; ++t) dst[t] = dst[t - (int32_t)off];
        return;
    }
    const uint4 p = ld16(dst - off);
    uint32_t j = 0;
    int32_t t = 0;
    for (; t + 4 <= len; t += 4) {
        uint32_t w = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            w |= pat_byte(p, j) << (8 * i);
            j = (j + 1 == off) ? 0 : j + 1;
        }
        *reinterpret_cast<uint32_t*>(dst + t) = w;
    }
    for (; t < len; ++t) {
        dst[t] = (uint8_t)pat_byte(p, j);
        j = (j + 1 == off) ? 0 : j + 1;
    }
}

// Progress signal of a long copy (the pipelined decoder's watchdog
// heartbeat, see wait_for); the one-wave decoder passes none.
struct NoBeat {
    LZ4E_DEV void operator()() const {}
};

// Whole-wave copy of len literal bytes (non-overlapping), 16 B per lane.
// With kU > 1 long runs move kU KiB per HBM round trip: a wave's loads wait
// behind its earlier stores (one in-order vmcnt), so 1 KiB steps hold an
// incompressible block's copy at one round trip per KiB.  (The pipelined
// decoder uses 4; the one-wave decoder keeps 1: 16 more VGPRs would cost it
// a wave per SIMD.)
template <int kU = 1, class Beat = NoBeat>
LZ4E_DEV void wave_copy(uint8_t* dst, const uint8_t* src, int32_t len, uint32_t lane,
                        Beat beat = Beat()) {
    constexpr int32_t kStep = 16 * kWave;
    int32_t k = 16 * (int32_t)lane;
    if constexpr (kU > 1) {
        for (; k + (kU - 1) * kStep + 16 <= len; k += kU * kStep) {
            uint4 v[kU];
#pragma unroll
            for (int j = 0; j < kU; ++j) v[j] = *reinterpret_cast<const uint4*>(src + k + j * kStep);
#pragma unroll
            for (int j = 0; j < kU; ++j) *reinterpret_cast<uint4*>(dst + k + j * kStep) = v[j];
            beat();
        }
    }
    for (; k + 16 <= len; k += 16 * kWave)
        *reinterpret_cast<uint4*>(dst + k) = *reinterpret_cast<const uint4*>(src + k);
    for (int32_t t = (len & ~15) + lane; t < len; t += kWave) dst[t] = src[t];
}

// Whole-wave match copy: out[op + t] = out[op - off + t mod off].
template <class Beat = NoBeat>
LZ4E_DEV void wave_match(uint8_t* out, int32_t op, uint32_t off, int32_t len, uint32_t lane,
                         Beat beat = Beat()) {
    if (off == 0) {
        for (int32_t t = lane; t < len; t += kWave) out[op + t] = 0;
        return;
    }
    const int32_t src = op - (int32_t)off;  // signed: a dictionary source lies before out
    if (off >= 16 * kWave) {
        // each 1 KiB step reads bytes written before the step
        for (int32_t k0 = 0; k0 < len; k0 += 16 * kWave) {
            const int32_t k = k0 + 16 * (int32_t)lane;
            if (k + 16 <= len) {
                *reinterpret_cast<uint4*>(out + op + k) =
                    *reinterpret_cast<const uint4*>(out + src + k);
            } else {
                for (int32_t t = k; t < len && t < k + 16; ++t) out[op + t] = out[src + t];
            }
            wave_fence();
            beat();
        }
        return;
    }
    // off < 1024: period P = off * ceil(1024 / off) >= 1024; the first P bytes
    // come from the final period [op-off, op), the rest from P bytes back.
    // (Measured against 16-byte chunks built in registers from the period
    // and against offset-doubling rounds: both slower on fio4k, 2.73 ->
    // 3.15 / 4.91 ms one-wave: the byte loop's loads all read the final
    // period and issue together.)
    const int32_t P = (int32_t)off * ((16 * kWave + off - 1) / off);
    const int32_t head = len < P ? len : P;
    for (int32_t t = lane; t < head; t += kWave) out[op + t] = out[src + (int32_t)(t % off)];
    wave_fence();
    for (int32_t k0 = P; k0 < len; k0 += 16 * kWave) {
        const int32_t k = k0 + 16 * (int32_t)lane;
        if (k + 16 <= len) {
            *reinterpret_cast<uint4*>(out + op + k) =
                *reinterpret_cast<const uint4*>(out + op + k - P);
        } else {
            for (int32_t t = k; t < len && t < k + 16; ++t) out[op + t] = out[op + t - P];
        }
        wave_fence();
        beat();
    }
}

// ---------------------------------------------------------------- LDS copies
// Unaligned dword LDS accesses (gfx950 DS unaligned mode).  Sources may be
// read up to 3 bytes past their end: the output block is followed by the
// ring, and ring reads start below kRing with the kRingPad mirror after it.

// One piece of at most 16 bytes, src + n <= dst or another buffer: four
// dword loads, then the stores, branch-free: a store whose bytes are not
// all wanted goes to the lane's own dword of the sink instead.
LZ4E_DEV void piece16(lu8* dst, const lu8* src, uint32_t n, lu8* sink) {
    const uint32_t w0 = ld4(src), w1 = ld4(src + 4), w2 = ld4(src + 8), w3 = ld4(src + 12);
    st4(n >= 4 ? dst : sink, w0);
    st4(n >= 8 ? dst + 4 : sink, w1);
    st4(n >= 12 ? dst + 8 : sink, w2);
    st4(n >= 16 ? dst + 12 : sink, w3);
    const uint32_t k = n & 12u, r = n & 3u;
    const uint32_t wt = k == 0 ? w0 : (k == 4 ? w1 : (k == 8 ? w2 : w3));
    *(r > 0 ? dst + k : sink) = (uint8_t)wt;
    *(r > 1 ? dst + k + 1 : sink) = (uint8_t)(wt >> 8);
    *(r > 2 ? dst + k + 2 : sink) = (uint8_t)(wt >> 16);
}

// The store half of piece16: n (<= 16) bytes of v at dst.
LZ4E_DEV void put16(lu8* dst, uint4 v, uint32_t n, lu8* sink) {
    st4(n >= 4 ? dst : sink, v.x);
    st4(n >= 8 ? dst + 4 : sink, v.y);
    st4(n >= 12 ? dst + 8 : sink, v.z);
    st4(n >= 16 ? dst + 12 : sink, v.w);
    const uint32_t k = n & 12u, r = n & 3u;
    const uint32_t wt = k == 0 ? v.x : (k == 4 ? v.y : (k == 8 ? v.z : v.w));
    *(r > 0 ? dst + k : sink) = (uint8_t)wt;
    *(r > 1 ? dst + k + 1 : sink) = (uint8_t)(wt >> 8);
    *(r > 2 ? dst + k + 2 : sink) = (uint8_t)(wt >> 16);
}

// len zero bytes (offset-0 matches: the reference writes zeros).
LZ4E_DEV void lane_zero(lu8* dst, int32_t len, lu8* sink) {
    for (int32_t t = 0; t < len; t += 16)
        put16(dst + t, make_uint4(0, 0, 0, 0), (uint32_t)(len - t < 16 ? len - t : 16), sink);
}

// Chains of dependent matches (a match whose source is the output of an
// earlier, still pending one) by pointer jumping over span bytes: every byte
// of a pending match points at the byte it copies (x - off), every other byte
// of [lo_i, hi_i) is final; each whole-wave round either copies a byte whose
// target is final or jumps it to its target's target, so a chain of depth d
// takes about log2(d) rounds.  Targets lie at or after lo_i (the parts before
// the batch were copied from HBM first).  Returns the number of rounds.
LZ4E_DEV uint32_t resolve_chains(lu8* span, lu16* jump, int32_t lo_i, int32_t hi_i, int32_t s0,
                                 bool mine, int32_t ms, int32_t m, int32_t off, uint32_t lane) {
    for (int32_t i = lo_i + (int32_t)lane; i < hi_i; i += kWave) jump[i] = kFinal;
    wave_fence();
    if (mine) {
        for (int32_t t = 0; t < m; ++t) {
            if (off != 0) jump[ms + t] = (uint16_t)(ms + t - off);
            else span[ms + t] = 0;  // offset 0: zeros, final
        }
    }
    wave_fence();
    uint32_t rounds = 0;
    for (;;) {
        bool more = false;
        for (int32_t i = s0 + (int32_t)lane; i < hi_i; i += kWave) {
            const uint32_t y = jump[i];
            if (y != kFinal) {
                const uint32_t z = jump[y];
                if (z == kFinal) {
                    span[i] = span[y];
                    jump[i] = kFinal;
                } else {
                    jump[i] = (uint16_t)z;
                    more = true;
                }
            }
        }
        wave_fence();
        rounds++;
        if (!ballot(more)) break;
    }
    return rounds;
}

// Per-lane copy of len bytes, non-overlapping, in 16-byte pieces.
LZ4E_DEV void lane_copy(lu8* dst, const lu8* src, int32_t len, lu8* sink) {
    for (int32_t t = 0; t < len; t += 16) {
        const int32_t c = len - t < 16 ? len - t : 16;
        piece16(dst + t, src + t, (uint32_t)c, sink);
    }
}

// Per-lane match copy of len bytes at dst with offset off >= 1 (any
// overlap), in pieces whose source is already final: piece [t, t + c) comes
// from D bytes back, D a multiple of off with c <= D <= t (first piece: D =
// off, from before dst); D doubles while 2D <= t.
LZ4E_DEV void lane_match(lu8* dst, uint32_t off, int32_t len, lu8* sink) {
    int32_t t = 0, D = (int32_t)off;
    while (t < len) {
        int32_t c = len - t < 16 ? len - t : 16;
        c = c < D ? c : D;
        piece16(dst + t, dst + t - D, (uint32_t)c, sink);
        t += c;
        if (2 * D <= t) D *= 2;
    }
}

// Per-lane copy of len (1..64) bytes from HBM into LDS (loads never read
// at or past lim).
LZ4E_DEV void lane_copy64(lu8* dst, const uint8_t* src, int32_t len, const uint8_t* lim) {
    const uint32_t nch = ((uint32_t)len + 15) >> 4;
    if (src + 16 * nch > lim) {
        for (int32_t t = 0; t < len; ++t) dst[t] = src[t];
        return;
    }
    uint4 c[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) c[i] = i < nch ? ld16(src + 16 * i) : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t w[4] = {c[i].x, c[i].y, c[i].z, c[i].w};
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t k = 16 * i + 4 * j;
            if (k + 4 <= (uint32_t)len) {
                st4(dst + k, w[j]);
            } else if (k < (uint32_t)len) {
                for (uint32_t q = 0; k + q < (uint32_t)len; ++q) dst[k + q] = (uint8_t)(w[j] >> (8 * q));
            }
        }
    }
}

// ---------------------------------------------------------------- batch copies

// Copies of a scalar-path batch (one sequence, any length) in HBM: the
// literal run, then the match; same-wave stores and loads to one global
// address are ordered by the hardware (one vector L1 per CU) and the
// wavefront fences keep the compiler from moving loads above the stores.
template <int kU = 1, class Beat = NoBeat>
LZ4E_DEV void copy_scalar_hbm(const Batch& b, const uint8_t* in, int32_t srcSize, uint8_t* gout,
                              int32_t outSize, uint32_t lane, Beat beat = Beat()) {
    const int32_t L = lane_val((uint32_t)b.L, 0), op = lane_val((uint32_t)b.op, 0);
    const int32_t ls = lane_val((uint32_t)b.ls, 0);
    const int32_t M = lane_val((uint32_t)b.M, 0), off = lane_val((uint32_t)b.off, 0);
    wave_fence();
    if (L > 0 && L <= kLongPiece) {
        if (lane == 0) lane_copy64(gout + op, in + ls, L, in + srcSize);
    } else if (L > kLongPiece) {
        wave_copy<kU>(gout + op, in + ls, L, lane, beat);
    }
    wave_fence();
    const int32_t ms = op + L;
    if (M > 0 && M <= kLongPiece) {
        if (lane == 0) lane_match(gout + ms, (uint32_t)off, M, gout + outSize);
    } else if (M > kLongPiece) {
        wave_match(gout, ms, (uint32_t)off, M, lane, beat);
    }
    wave_fence();
}

}  // namespace

}  // namespace lz4e
