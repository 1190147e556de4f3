// lz4e_dec_parse.h -- the parse every batch decoder shares (included by
// lz4e_decompress.hip alone): LDS access types, the input window, the parse
// state and parse_batch.
//
// Parse, in batches of up to 64 sequences: the token stream is walked
// wave-uniformly with the reference's exact sequence of bound checks --
// including the two-stage 16/18-byte shortcut, whose entry conditions change
// which malformed inputs are rejected and where -- so the return value,
// including the error code -(ip - src) - 1, is the reference's.  A fast batch
// (no extension bytes, far from both block ends) is found by pointer doubling
// over a 256-byte window of the token stream; anything else is one sequence on
// the exact scalar path.  Sequence k of a batch is recorded in lane k (literal
// source, literal length, output position, offset, match length).
#pragma once

#include "lz4e_device.h"

namespace lz4e {

namespace {

// LDS of the parse: the input ring (+ mirror).
constexpr uint32_t kRing = 1024;                    // 4 segments of 256 B
constexpr uint32_t kRingPad = 128;                  // mirror of ring bytes [0, 128)
// Small blocks (decode_block's LDS form): output and input both staged in
// LDS, at most kSmallOut bytes each, kSmallBuf bytes of LDS each.
constexpr int32_t kSmallOut = 4608;  // 4 KiB blocks and their 4 KiB + 32 capacities
constexpr uint32_t kSmallBuf = kSmallOut + 64;

// LDS access types.  Every wider type may alias every other (may_alias):
// the decoders read LDS bytes through whichever width suits the step, so no
// access order may rest on type-based alias analysis.
typedef __attribute__((address_space(3))) uint8_t lu8;
typedef __attribute__((address_space(3), may_alias)) uint32_t lu32;
typedef __attribute__((address_space(3), may_alias)) uint16_t lu16;
typedef uint32_t __attribute__((aligned(1), may_alias)) u32a1;
typedef __attribute__((address_space(3))) u32a1 lu32a1;

LZ4E_DEV uint32_t ld4(const lu8* p) { return *(const lu32a1*)p; }
LZ4E_DEV void st4(lu8* p, uint32_t v) { *(lu32a1*)p = v; }

// Two 256-byte windows of the compressed block, A = segment seg and B =
// segment seg + 1, where segment s is block bytes [256 s - shift, +256)
// (shift = the block's offset inside its first aligned word), plus C =
// segment seg + 2 loaded ahead.  Word loads are clamped to the block.  With
// a ring, every segment is written to LDS slot s & 3 when it becomes B.
struct InWindow {
    gcu32* w;        // word-aligned base of the block
    int32_t shift;   // byte offset of the block inside w[0]
    int32_t last;    // last word index that belongs to the block
    uint32_t lane;
    int32_t seg;     // segment of window A
    int32_t base;    // block position of window A byte 0 (256 seg - shift)
    int32_t ring_lo; // lowest block position held by the ring
    uint32_t a, b, c;  // this lane's dword of A, B and C
    lu32* ring;      // kRing + kRingPad bytes of LDS
    // Small blocks: the whole block staged in LDS (words 0..last, 64 bytes of
    // slack after), read instead of HBM and instead of the ring; nullptr:
    // HBM + ring.
    const lu8* lb = nullptr;

    LZ4E_DEV uint32_t load(int32_t wi) const {
        wi = wi < 0 ? 0 : wi;
        wi = wi < last ? wi : last;
        return lb ? ((const lu32*)lb)[wi] : w[wi];
    }
    LZ4E_DEV void put_ring(int32_t s, uint32_t v) const {
        if (lb) return;
        const uint32_t slot = (uint32_t)s & 3;
        ring[slot * 64 + lane] = v;
        if (slot == 0 && lane < kRingPad / 4) ring[kRing / 4 + lane] = v;
    }
    LZ4E_DEV void reload(int32_t p) {
        seg = (p + shift) >> 8;
        base = seg * 256 - shift;
        a = load(seg * 64 + (int32_t)lane);
        b = load(seg * 64 + 64 + (int32_t)lane);
        c = load(seg * 64 + 128 + (int32_t)lane);
        put_ring(seg, a);
        put_ring(seg + 1, b);
        ring_lo = base;
        lockstep();  // other lanes read the ring next
    }
    LZ4E_DEV void slide() {
        a = b;
        b = c;
        seg++;
        base += 256;
        put_ring(seg + 1, b);
        c = load(seg * 64 + 128 + (int32_t)lane);
        const int32_t lo = base - 512;  // segments seg-2 .. seg+1 stay in the ring
        ring_lo = ring_lo > lo ? ring_lo : lo;
        lockstep();  // other lanes read the ring next
    }
    // Byte p of the block (reloads when p is outside [base, base + 512)).
    LZ4E_DEV uint32_t byte(int32_t p) {
        uint32_t r = (uint32_t)(p - base);
        if (r >= 512) {
            if (r < 768) slide();
            else reload(p);
            r = (uint32_t)(p - base);
        }
        const uint32_t w = r < 256 ? lane_val(a, r >> 2) : lane_val(b, (r - 256) >> 2);
        return (w >> ((r & 3) * 8)) & 0xFFu;
    }
    // Length-extension scan, 256 bytes per step: the first block position
    // q >= p0 whose byte is not 255 or that is >= plim (the reference reads
    // such runs one byte at a time, lz4e_decompress.c:201-206, 319-326; a
    // byte at a time cost one v_readlane round trip each).  Bytes past the
    // block read as the clamped last word, never past q's decision: q <= plim
    // and plim lies inside the block.
    LZ4E_DEV int32_t ext_stop(int32_t p0, int32_t plim) {
        for (int32_t p = p0;;) {
            follow(p);  // p in window A = [base, base + 256)
            const int32_t pa = base + 4 * (int32_t)lane;
            uint32_t m = 0;
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t) {
                const int32_t q = pa + (int32_t)t;
                const bool stop = q >= p && (((a >> (8 * t)) & 0xFFu) != 0xFFu || q >= plim);
                m |= (stop ? 1u : 0u) << t;
            }
            const uint64_t bm = ballot(m != 0);
            if (bm) {
                const uint32_t l = ctz64(bm);
                return base + 4 * (int32_t)l + (int32_t)__builtin_ctz(lane_val(m, l));
            }
            p = base + 256;
        }
    }
    // Byte at window offset r (< 512), no range check.
    LZ4E_DEV uint32_t ubyte(uint32_t r) const {
        const uint32_t w = r < 256 ? lane_val(a, r >> 2) : lane_val(b, (r - 256) >> 2);
        return (w >> ((r & 3) * 8)) & 0xFFu;
    }
    // Little-endian 16 bits at window offset r (r + 2 <= 512), no range check.
    LZ4E_DEV uint32_t ule16(uint32_t r) const { return ubyte(r) | (ubyte(r + 1) << 8); }
    // Keep the parse position inside window A.
    LZ4E_DEV void follow(int32_t p) {
        const uint32_t r = (uint32_t)(p - base);
        if (r >= 256 && r < 512) slide();
        else if (r >= 512) reload(p);
    }
    // Little-endian 32 / 16 bits at block position p from the ring
    // (p in [ring_lo, base + 512 - 4 / 2)).
    LZ4E_DEV uint32_t rd4(int32_t p) const { return ld4(at(p)); }
    // LDS address of block byte p (held: see holds); 16 bytes readable from it.
    LZ4E_DEV const lu8* at(int32_t p) const {
        if (lb) return lb + (uint32_t)(p + shift);
        return reinterpret_cast<const lu8*>(ring) + ((uint32_t)(p + shift) & (kRing - 1));
    }
    LZ4E_DEV uint32_t rd16(int32_t p) const { return rd4(p) & 0xFFFFu; }
    // Block bytes [p, p + n) all held by the ring (at ring offsets that may
    // wrap: see wave_lit_ring).
    LZ4E_DEV bool holds(int32_t p, int32_t n) const {
        return lb || (p >= ring_lo && p + n <= base + 512);
    }
    // The ring copy of block bytes [p, p + n), or nullptr when not all held.
    LZ4E_DEV const lu8* in_ring(int32_t p, int32_t n) const {
        if (lb) return lb + (uint32_t)(p + shift);
        if (p < ring_lo || p + n > base + 512) return nullptr;
        const uint32_t i = (uint32_t)(p + shift) & (kRing - 1);
        // contiguous through the mirror, reads of up to 3 bytes past included
        if (i + (uint32_t)n + 3 > kRing + kRingPad) return nullptr;
        return reinterpret_cast<const lu8*>(ring) + i;
    }
};

// a > b for an unsigned a < 2^32 and a signed b (the reference compares
// pointers; b = end - k may lie before the buffer).
LZ4E_DEV bool ugt(uint32_t a, int32_t b) { return b < 0 || a > (uint32_t)b; }

constexpr uint32_t kSat = 0x7FFFFFFFu;  // length saturation: keeps every bound check's outcome

// ---------------------------------------------------------------- parse helpers

// Byte x (< 256) of a 256-byte table held one dword per lane (ds_bpermute).
LZ4E_DEV uint32_t table_at(uint32_t tab, uint32_t x) {
    return (shfl_addr(tab, x & 0xFCu) >> ((x & 3) * 8)) & 0xFFu;
}

// The composed table B[A[p]] for this lane's 4 positions p: four gathers of
// the source dwords (byte address = index & ~3), the wanted bytes picked and
// packed by two v_perm_b32.
LZ4E_DEV uint32_t table_compose(uint32_t A, uint32_t B) {
    const uint32_t a = A & 0xFCFCFCFCu;
    const uint32_t g0 = shfl_addr(B, a & 0xFFu), g1 = shfl_addr(B, (a >> 8) & 0xFFu);
    const uint32_t g2 = shfl_addr(B, (a >> 16) & 0xFFu), g3 = shfl_addr(B, a >> 24);
    const uint32_t s = A & 0x03030303u;
    const uint32_t r01 = perm_bytes(g1, g0, (s & 0xFFFFu) + 0x0C0C0400u);
    const uint32_t r23 = perm_bytes(g3, g2, (s >> 16) + 0x0C0C0400u);
    return r01 | (r23 << 16);
}

// ---------------------------------------------------------------- the parse

// A fast-path sequence has no extension byte: both token nibbles are below
// 15, so its literal run is 0..kFastLitMax bytes and its match 4..kFastMatchMax
// (the lengths of the reference's two-stage shortcut, :150-191).  The
// pipelined decoder's copy_fast relies on both bounds (static_asserts at its
// copy sites); tests/frame_synth.py plants sequences at them (FAST_LIT_MAX,
// FAST_MATCH_MAX).
constexpr int32_t kFastLitMax = 14;
constexpr int32_t kFastMatchMax = 18;
constexpr int32_t kFastSeqMax = kFastLitMax + kFastMatchMax;  // output bytes per fast sequence

// Parse state of one block: wave-uniform scalars plus the input window.
struct Parse {
    InWindow win;
    int32_t iend, oend, shortiend, shortoend;
    int32_t ip, op;
    int32_t D;  // dictionary bytes before the output (<= 65536; 0: noDict)
    bool done;  // the final literal run has been parsed

    // lin (small blocks, srcSize <= kSmallOut): stage the whole block into
    // these kSmallBuf bytes of LDS first, one round trip for all its loads.
    // (ip0, op0): resume at a sequence boundary (the group decoder's hand-over)
    LZ4E_DEV void init(const uint8_t* in, int32_t srcSize, int32_t outSize, lu32* ring,
                       uint32_t lane, int32_t dict = 0, lu8* lin = nullptr, int32_t ip0 = 0,
                       int32_t op0 = 0) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(in);
        win.shift = (int32_t)(a & 3);
        win.w = (gcu32*)(a - win.shift);
        win.last = (srcSize + win.shift - 1) >> 2;
        win.lane = lane;
        win.ring = ring;
        win.lb = nullptr;
        if (lin) {
            constexpr int kR = (kSmallOut + 4 + 16 * kWave - 1) / (16 * kWave);
            uint32_t v[kR][4];
#pragma unroll
            for (int r = 0; r < kR; ++r)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int32_t wi = 4 * ((int32_t)lane + r * (int32_t)kWave) + q;
                    v[r][q] = win.w[wi < win.last ? wi : win.last];
                }
#pragma unroll
            for (int r = 0; r < kR; ++r) {
                const int32_t wi = 4 * ((int32_t)lane + r * (int32_t)kWave);
                if (wi <= win.last) {
                    lu32* d = (lu32*)lin + wi;
                    d[0] = v[r][0];
                    d[1] = v[r][1];
                    d[2] = v[r][2];
                    d[3] = v[r][3];
                }
            }
            lockstep();  // every lane reads the staged words next
            win.lb = lin;
        }
        win.reload(ip0);
        iend = srcSize;
        oend = outSize;
        shortiend = iend - kFastLitMax - 2;              // :100-101
        shortoend = oend - kFastLitMax - kFastMatchMax;  // :102-103
        ip = ip0;
        op = op0;
        D = dict;
        done = false;
    }
};

// One parsed batch: lane k < n holds sequence k (literal source, literal
// length, output position, offset, match length; the final literal run has
// match length 0).
struct Batch {
    int32_t ls = 0, L = 0, op = 0, off = 0, M = 0;
    uint32_t n = 0;
};

enum ParseResult { kParsedFast, kParsedScalar, kParseFail };

struct NoLap {
    LZ4E_DEV void operator()(int) const {}
};

// Window offset (from ip) of the token after the token t at offset p, for
// the fast path: 255 when the sequence has an extension byte (a nibble of
// 15) and so cannot be on the fast path.
LZ4E_DEV uint32_t fast_next(uint32_t t, uint32_t p) {
    const uint32_t Lt = t >> 4, Mt = t & 15;
    return (Lt != 15 && Mt != 15) ? p + Lt + 3 : 255u;
}

// The next batch of the token stream, with every bound check of the
// reference in its order (lz4e_decompress.c:123-446).  kParsedFast: up to 64
// sequences without extension bytes, far from both block ends (each literal
// run 0..kFastLitMax, match 4..kFastMatchMax, so at most kFastSeqMax = 32
// output bytes per sequence); kParsedScalar: one sequence of any length;
// kParseFail: malformed input or too small a capacity, the return value is
// -(P.ip) - 1.  A fast batch's output is at most cap_out (>= kFastSeqMax)
// bytes.
// kVecExt: length-extension runs by 256-byte vector scans (the pipelined
// decoder; the one-wave decoder keeps the byte loop, see kOneWaveVecExt).
// kPartial: the reference's partial_decode instance (oend = the target size;
// include/lz4e.h, LZ4E_decompress_safe_partial).  Its branches (:229-246,
// 281, 388-405) all lie on the scalar path -- the shortcut needs
// op <= oend - 32 -- and each of its exits sets P.done; the value is P.op.
template <bool kVecExt = false, bool kPartial = false, class Lap = NoLap>
LZ4E_DEV ParseResult parse_batch(Parse& P, Batch& b, uint32_t lane,
                                 int32_t cap_out = (int32_t)kWave * kFastSeqMax, Lap lap = Lap()) {
    const int32_t iend = P.iend, oend = P.oend;
    int32_t ip = P.ip, op = P.op;
    InWindow& win = P.win;

    // Fast path: a run of tokens with no length-extension bytes, far from
    // both block ends, where the reference takes its two-stage shortcut
    // (:150-191).  The token chain inside the 256-byte window at ip is found
    // by pointer doubling: jump tables J_{2^i} (window offset -> offset 2^i
    // tokens on, 255 = chain end; one byte per position, lane l holding
    // positions 4l..4l+3) are composed with ds_bpermute gathers, then lane k
    // follows the bits of k to token k.  Every field and check is then
    // evaluated per lane.
    // (iend - 18: the shortcut's entry ip + 1 < shortiend for the token at ip)
    bool fast = ip <= iend - 18 && op <= oend - kFastSeqMax;
    uint32_t wv = 0;
    if (fast) {
        win.follow(ip);
        wv = win.rd4(ip + 4 * (int32_t)lane);
        // A batch that starts at a token the fast path cannot take -- every
        // such token ends the fast batch before it -- is the scalar path's:
        // lane 0's token would fail `cand` below, so no tables are composed.
        fast = fast_next(lane_val(wv, 0) & 0xFFu, 0) <= 254;
    }
    if (fast) {
        const int32_t r0 = ip - win.base;                  // < 256
        const int32_t rin = iend - 18 - win.base;          // last token offset on the fast path
        const int32_t jlim = (rin < 494 ? rin : 494) - r0;  // (offset bytes stay in A+B)
        uint32_t J[6];
        {
            uint32_t j1 = 0;
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t t = (wv >> (8 * q)) & 0xFFu, p = 4 * lane + q;
                const uint32_t n = fast_next(t, p);
                const bool go = (int32_t)p <= jlim && n <= 254;
                j1 |= (go ? n : 255u) << (8 * q);
            }
            J[0] = j1;
        }
        lap(0);
#pragma unroll
        for (int i = 1; i < 6; ++i) J[i] = table_compose(J[i - 1], J[i - 1]);
        lap(1);
        uint32_t x = 0;  // lane k: window offset of token k (255: past the chain)
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const uint32_t y = table_at(J[i], x);
            x = (lane >> i) & 1 ? y : x;
        }
        lap(2);
        const uint32_t t = table_at(wv, x);  // token byte
        const int32_t Lt = (int32_t)(t >> 4), Mt = (int32_t)(t & 15);
        const int32_t L = Lt, M = Mt + 4, lp = ip + (int32_t)x + 1;  // literal start
        const bool cand = x != 255 && Lt != 15 && Mt != 15 && (int32_t)x <= jlim;
        const int32_t off = cand ? (int32_t)win.rd16(lp + L) : 0;
        const int32_t nxt = lp + L + 2;
        const int32_t size = cand ? L + M : 0;
        const int32_t incl = (int32_t)wave_incl_add((uint32_t)size);
        const int32_t o_k = op + incl - size;
        const int32_t m_k = o_k + L;
        // the reference's checks on this path: shortcut entry (op <= oend-32,
        // input side guaranteed by jlim), match inside the block (:299-302),
        // and for offsets < 8 the _copy_match end check (:422-431); a source
        // in the dictionary takes _copy_match: offset inside dictionary +
        // block (:299-302), then the extDict end check (:341-346).
        // Partial: _copy_match has no end check (:388-405), but a match of
        // an offset < 8 that ends at oend ends the decode there (:402-403):
        // that sequence is the scalar path's.
        const bool end_ok = kPartial ? m_k + M < oend : m_k + M <= oend - 5;
        const bool ok = cand && o_k <= oend - kFastSeqMax && incl <= cap_out &&
                        (m_k >= off ? (off >= 8 || end_ok) : (m_k - off + P.D >= 0 && end_ok));
        const uint64_t okm = ballot(ok);
        const uint32_t nf = (~okm) ? ctz64(~okm) : kWave;  // first failing lane
        if (nf > 0) {
            b.ls = lp;
            b.L = L;
            b.op = o_k;
            b.off = off;
            b.M = M;
            b.n = nf;
            P.op = op + lane_val((uint32_t)incl, nf - 1);
            P.ip = lane_val((uint32_t)nxt, nf - 1);  // the token after the last one
            lap(3);
            return kParsedFast;
        }
    }

    // Exact scalar path (extension bytes, block ends, anything the fast path
    // declined): one sequence.
    win.follow(ip);  // ip now in window A: bytes up to ip + 256 are readable unchecked
    const uint32_t r0 = (uint32_t)(ip - win.base);
    const uint32_t token = win.ubyte(r0);
    ip++;
    uint32_t length = token >> 4;  // saturates at kSat
    int32_t offset = 0, lit_ip, lit_op;
    uint32_t L;

    if (length != 15 && ip < P.shortiend && op <= P.shortoend) {
        // Two-stage shortcut (:150-191): literals 0..14 fit, offset read.
        lit_ip = ip;
        lit_op = op;
        L = length;
        offset = (int32_t)win.ule16(r0 + 1 + length);
        op += (int32_t)length;
        ip += (int32_t)length + 2;
        length = token & 15;
        if (length != 15 && offset >= 8 && op >= offset) {
            // 18-byte shortcut copy: match length 4..18, no checks left
            length += 4;
            goto record;
        }
        goto copy_match_checks;
    }
    if (length == 15) {  // :194-220
        if (ip >= iend - 15) goto fail;
        if constexpr (kVecExt) {
            // bytes ip .. q: 255 each, then s; the loop goes on while the
            // next position is below iend - 15
            const int32_t q = win.ext_stop(ip, iend - 16);
            const uint64_t sum = (uint64_t)length + 255ull * (uint64_t)(q - ip) + win.byte(q);
            length = sum > kSat ? kSat : (uint32_t)sum;
            ip = q + 1;
        } else {
            uint32_t s;
            do {
                s = win.byte(ip);
                ip++;
                length = length + s > kSat ? kSat : length + s;
            } while (ip < iend - 15 && s == 255);
        }
    }
    {
        const uint32_t cpy = (uint32_t)op + length;  // :223-288
        const uint32_t iln = (uint32_t)ip + length;
        lit_ip = ip;
        lit_op = op;
        L = length;
        if (ugt(cpy, oend - 12) || ugt(iln, iend - 8)) {
            if constexpr (kPartial) {
                // :229-246: the run is cut at oend, and must lie in the input
                if (ugt(cpy, oend)) L = length = (uint32_t)(oend - op);
                if (ugt((uint32_t)ip + length, iend)) goto fail;
                ip += (int32_t)length;
                op += (int32_t)length;
                // :281: the end, unless output and an offset's input remain
                if (op == oend || ip >= iend - 2) {
                    length = 0;
                    P.done = true;
                    goto record;
                }
            } else {
                if (iln != (uint32_t)iend || ugt(cpy, oend)) goto fail;
                ip += (int32_t)length;
                op += (int32_t)length;
                length = 0;
                P.done = true;  // final literal run: no match
                goto record;
            }
        } else {
            ip += (int32_t)length;
            op = (int32_t)cpy;
        }
    }
    offset = (int32_t)(win.byte(ip) | (win.byte(ip + 1) << 8));  // :291-296
    ip += 2;
    length = token & 15;

copy_match_checks:
    // _copy_match (:298-336, :422-431); with a dictionary the source may lie
    // up to D bytes before the output (:299-302, checkOffset)
    if (op - offset + P.D < 0) goto fail;
    if (length == 15) {
        // bytes ip .. q: 255 each, then s; reading a byte at or past
        // iend - 5 fails (ip > iend - 5 after the read)
        if constexpr (kVecExt) {
            const int32_t q = win.ext_stop(ip, iend - 5);
            if (q + 1 > iend - 5) {
                ip = q + 1;
                goto fail;
            }
            const uint64_t sum = (uint64_t)length + 255ull * (uint64_t)(q - ip) + win.byte(q);
            length = sum > kSat ? kSat : (uint32_t)sum;
            ip = q + 1;
        } else {
            uint32_t s;
            do {
                s = win.byte(ip);
                ip++;
                if (ip > iend - 5) goto fail;
                length = length + s > kSat ? kSat : length + s;
            } while (s == 255);
        }
    }
    if constexpr (kPartial) {
        // :388-405: a match that ends past oend - 12 is cut at oend (to 1
        // byte or more: a match is only reached with op < oend) and ends the
        // decode when it reaches oend; the last-literals rule (:425-431) is
        // not checked
        length += 4;
        if (ugt((uint32_t)op + length, oend - 12)) {
            const uint32_t room = (uint32_t)(oend - op);
            length = length < room ? length : room;
            P.done = length == room;
        }
    } else {
        if (ugt((uint32_t)op + length + 4, oend - 5)) goto fail;
        length += 4;
    }

record:
    {
        const bool me = lane == 0;
        b.ls = me ? lit_ip : 0;
        b.L = me ? (int32_t)L : 0;
        b.op = me ? lit_op : 0;
        b.off = me ? offset : 0;
        b.M = me ? (int32_t)length : 0;
        b.n = 1;
    }
    P.op = op + (int32_t)length;
    P.ip = ip;
    return kParsedScalar;
fail:
    P.ip = ip;
    return kParseFail;
}

}  // namespace

}  // namespace lz4e
