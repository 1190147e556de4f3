// lz4e_crc.hip -- the packed frame store's checksum (gfx950): CRC-32C
// (Castagnoli: reflected, polynomial 0x1EDC6F41, initial value and final xor
// 0xFFFFFFFF) of every entry of a batch, for the four entry points of
// include/lz4e.h that need it: lz4e_crc32c_batch_dev, lz4e_pack_crc_batch_dev,
// lz4e_unpack_verified_batch_dev and lz4e_unpack_range_verified_batch_dev.
// One kernel serves all four; only where an entry's bytes come from differs
// (CrcBatch, lz4e_gpu.h).
//
// The state register is kept reflected: bit 31 is x^0 and "times x" is
// (b >> 1) ^ (b & 1 ? 0x82F63B78 : 0).  Feeding n zero bytes to a state is a
// multiplication by x^(8n) mod P, hence
//     state(A || B) = state(A) * x^(8 |B|)  ^  state0(B)
// with state0 started from 0: the checksum is linear over GF(2), so a team of
// threads shares an entry.  Thread t of the team of nt = 1 << team_shift
// threads sums the contiguous piece [t * piece, (t + 1) * piece) of the entry
// (piece = ceil(len / nt) rounded up to 16 bytes, from the entry's OWN length:
// the sizing hint max_len only picks nt, so no result depends on it), the
// thread with the first byte from 0xFFFFFFFF and every other from 0, advances
// its state by the bytes that follow its piece, and the team XORs the results.
//
//   summing   slice-by-4: 16-byte loads, per 32-bit word four look-ups in a
//             4 KiB table set in LDS; the < 16 bytes at the end of a piece go
//             byte by byte.  (The alternative that was measured, table-free
//             shifts, is in DESIGN.md 9.)
//   advance   x^(8n) = A0[n & 255] * A1[n >> 8 & 255] * A2[n >> 16 & 255] *
//             A3[n >> 24], Aj[d] = x^(8 d 256^j): one 32-step shift/xor
//             multiply mod P per non-zero byte of n, at most four, two for
//             any entry below 64 KiB.
//   team      XOR butterfly inside the wave (ds_bpermute), the workgroup's
//             waves through LDS; a team larger than the workgroup leaves one
//             partial per workgroup in scratch and crc_combine_kernel, the
//             next launch, XORs them: kernel boundaries are the only ordering
//             between workgroups (no atomics, no flags, no waiting).
//
// Both tables are generated at compile time (make_crc_tables).
//
// The kernel reads the CALLER's memory: no load touches a byte outside
// [p, p + len).  Unaligned 16-byte loads are legal on gfx950; every one lies
// wholly inside its thread's piece.  An entry with len <= 0, or (when kinds
// are given) with a kind that is neither frame nor raw, is not read at all.
//
// unpack_verify_mask_kernel and unpack_verify_ret_kernel wrap the unchanged
// lz4e_unpack_batch_dev composition (lz4e_pack.hip): the first hides every
// entry that is invalid or whose checksum differs from the decoders and from
// the raw copy, the second writes their ret.  The four range_verify_* kernels
// wrap the unchanged lz4e_unpack_range_batch_dev composition in the same way
// for lz4e_unpack_range_verified_batch_dev (lz4e_gpu.h, RangeVerifyBatch): an
// entry is summed once per call, by the one request elected for it.
//
// Kernels and launches only (no other runtime call), so that tools/emu
// compiles this file as host C++ (tools/emu/emu_crc.cpp,
// tests/test_emulator_crc.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4e_gpu.h"
#include "lz4e_range.h"
#include "lz4e_wave.h"

namespace lz4e {
namespace {

constexpr uint32_t kCrcThreads = 256;
constexpr uint32_t kCrcPoly = 0x82F63B78u;  // 0x1EDC6F41 reflected
constexpr uint32_t kCrcOne = 0x80000000u;   // x^0

constexpr uint32_t crc_times_x(uint32_t b) { return (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u); }

// a * b mod P, both reflected: b's bit 31 - i is the coefficient of x^i.
constexpr uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < 32; ++i) {
        r ^= (b & (kCrcOne >> i)) ? a : 0u;
        a = crc_times_x(a);
    }
    return r;
}

struct CrcTables {
    // slice[k][v]: the state after the byte v and k zero bytes, from state 0
    uint32_t slice[4][256];
    // pow[j][d] = x^(8 d 256^j)
    uint32_t pow[4][256];
};
constexpr CrcTables make_crc_tables() {
    CrcTables t{};
    for (uint32_t v = 0; v < 256; ++v) {
        uint32_t c = v;
        for (int k = 0; k < 8; ++k) c = crc_times_x(c);
        t.slice[0][v] = c;
    }
    for (uint32_t k = 1; k < 4; ++k)
        for (uint32_t v = 0; v < 256; ++v) {
            const uint32_t c = t.slice[k - 1][v];
            t.slice[k][v] = (c >> 8) ^ t.slice[0][c & 0xFFu];
        }
    uint32_t step = kCrcOne;  // x^(8 256^j)
    for (int k = 0; k < 8; ++k) step = crc_times_x(step);
    for (uint32_t j = 0; j < 4; ++j) {
        t.pow[j][0] = kCrcOne;
        for (uint32_t d = 1; d < 256; ++d) t.pow[j][d] = crc_mul(t.pow[j][d - 1], step);
        step = crc_mul(t.pow[j][255], step);
    }
    return t;
}
__device__ const CrcTables kCrcTables = make_crc_tables();
constexpr CrcTables kCrcCheck = make_crc_tables();
static_assert(kCrcCheck.pow[0][1] == 0x00800000u && kCrcCheck.pow[0][2] == 0x00008000u &&
                  kCrcCheck.pow[0][4] == kCrcPoly,
              "x^8, x^16, x^32 mod P");
static_assert(kCrcCheck.slice[0][1] == 0xF26B8303u && kCrcCheck.slice[0][255] == 0xAD7D5351u,
              "the byte table's first and last entry (RFC 3720's polynomial)");

typedef uint32_t crc_v4 __attribute__((ext_vector_type(4)));

// tab: the slice tables in LDS, slice[k][v] at tab[256 k + v].
LZ4E_DEV uint32_t crc_word(const uint32_t* tab, uint32_t state, uint32_t w) {
    state ^= w;
    return tab[768 + (state & 0xFFu)] ^ tab[512 + ((state >> 8) & 0xFFu)] ^ tab[256 + ((state >> 16) & 0xFFu)] ^
           tab[state >> 24];
}

// The state after the n bytes at p.  Loads: 16 bytes at p + 16 k while they
// lie wholly inside [p, p + n), then single bytes.
LZ4E_DEV uint32_t crc_piece(const uint32_t* tab, uint32_t state, const uint8_t* p, uint64_t n) {
    const uint64_t nvec = n >> 4;
    for (uint64_t k = 0; k < nvec; ++k) {
        crc_v4 v;
        __builtin_memcpy(&v, p + (k << 4), 16);
        state = crc_word(tab, state, v.x);
        state = crc_word(tab, state, v.y);
        state = crc_word(tab, state, v.z);
        state = crc_word(tab, state, v.w);
    }
    for (uint64_t k = nvec << 4; k < n; ++k) state = tab[(state ^ p[k]) & 0xFFu] ^ (state >> 8);
    return state;
}

// state * x^(8 n): the state after n more zero bytes.
LZ4E_DEV uint32_t crc_advance(uint32_t state, uint32_t n) {
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t d = (n >> (8 * j)) & 0xFFu;
        if (d) state = crc_mul(state, kCrcTables.pow[j][d]);
    }
    return state;
}

// Entry i's bytes: none when it is not to be read.
struct CrcEntry {
    const uint8_t* p;
    uint32_t len;
};
LZ4E_DEV CrcEntry crc_entry(const CrcBatch& a, uint64_t i) {
    const int32_t len = a.len[i];
    if (len <= 0) return CrcEntry{nullptr, 0};
    if (a.kind == nullptr) return CrcEntry{a.data + a.off[i], (uint32_t)len};
    const uint32_t kind = a.kind[i];
    if (kind == kPackFrame) return CrcEntry{a.data + a.off[i], (uint32_t)len};
    if (kind == kPackRaw) return CrcEntry{a.raw + a.raw_off[i], (uint32_t)len};
    return CrcEntry{nullptr, 0};
}

// Entry g >> team_shift is the work of the 1 << team_shift consecutive
// threads of the launch that share it (pack_copy_kernel's scheme).  Every
// thread runs to the end: the team's XOR is cross-lane and the workgroup's
// goes through barriers.  out: crc[] for a team inside a workgroup, else the
// workgroup's partial at out[blockIdx.x].
__global__ __launch_bounds__(256) void crc_team_kernel(CrcBatch a, uint32_t team_shift, uint32_t* __restrict__ out) {
    __shared__ uint32_t tab[1024];
    __shared__ uint32_t wave_x[kCrcThreads / kWave];
    {
        const uint32_t* flat = &kCrcTables.slice[0][0];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) tab[4 * threadIdx.x + k] = flat[4 * threadIdx.x + k];
    }
    block_sync();
    const uint64_t g = (uint64_t)blockIdx.x * kCrcThreads + threadIdx.x;
    const uint64_t i = g >> team_shift;
    const uint32_t nt = 1u << team_shift, t = (uint32_t)g & (nt - 1);
    CrcEntry e{nullptr, 0};
    if (i < a.nblocks) e = crc_entry(a, i);
    uint32_t x = 0;
    if (e.len) {
        uint64_t piece = ((uint64_t)e.len + nt - 1) >> team_shift;
        piece = (piece + 15) & ~(uint64_t)15;
        const uint64_t lo = (uint64_t)t * piece;
        if (lo < e.len) {  // thread 0 always: it holds the first byte
            const uint64_t hi = lo + piece < e.len ? lo + piece : e.len;
            x = crc_piece(tab, t == 0 ? 0xFFFFFFFFu : 0u, e.p + lo, hi - lo);
            x = crc_advance(x, (uint32_t)(e.len - hi));
        }
    }
    // the team's lanes of this wave
    const uint32_t lane = threadIdx.x % kWave;
    for (uint32_t d = 1; d < nt && d < kWave; d <<= 1) x ^= shfl(x, lane ^ d);
    const bool owner = t == 0 && i < a.nblocks;
    if (nt <= kWave) {
        if (owner) out[i] = e.len ? ~x : 0u;
        return;
    }
    if (lane == 0) wave_x[threadIdx.x / kWave] = x;
    block_sync();
    if (nt == 2 * kWave) {
        if (owner) out[i] = e.len ? ~(wave_x[threadIdx.x / kWave] ^ wave_x[threadIdx.x / kWave + 1]) : 0u;
        return;
    }
    if (threadIdx.x != 0) return;
    x = wave_x[0] ^ wave_x[1] ^ wave_x[2] ^ wave_x[3];
    if (nt == kCrcThreads) {
        if (owner) out[i] = e.len ? ~x : 0u;
    } else {
        out[blockIdx.x] = x;  // a team of several workgroups: i < nblocks (the grid is whole teams)
    }
}

// One thread per entry: the XOR of its 1 << wg_shift partials.
__global__ __launch_bounds__(256) void crc_combine_kernel(const uint32_t* __restrict__ partial,
                                                          const int32_t* __restrict__ len,
                                                          const uint8_t* __restrict__ kind, uint32_t nblocks,
                                                          uint32_t wg_shift, uint32_t* __restrict__ crc) {
    const uint64_t i = (uint64_t)blockIdx.x * kCrcThreads + threadIdx.x;
    if (i >= nblocks) return;
    uint32_t x = 0;
    for (uint32_t k = 0; k < (1u << wg_shift); ++k) x ^= partial[(i << wg_shift) + k];
    const bool read = len[i] > 0 && (kind == nullptr || kind[i] == kPackFrame || kind[i] == kPackRaw);
    crc[i] = read ? ~x : 0u;
}

// masked[i]: the length the decoders see; shown[i]: the kind the raw copy
// sees.  An entry that is invalid (rule 1 of lz4e_unpack_verified_batch_dev)
// or fails its checksum (rule 2) has length 0 for the decoders, which then
// return before they read or write anything, and a kind the raw copy refuses.
__global__ __launch_bounds__(256) void unpack_verify_mask_kernel(const int32_t* __restrict__ pk_len,
                                                                 const uint8_t* __restrict__ pk_kind,
                                                                 const uint32_t* __restrict__ pk_crc,
                                                                 const uint32_t* __restrict__ got, uint32_t nblocks,
                                                                 int32_t* __restrict__ masked,
                                                                 uint8_t* __restrict__ shown) {
    const uint64_t i = (uint64_t)blockIdx.x * kCrcThreads + threadIdx.x;
    if (i >= nblocks) return;
    const uint32_t kind = pk_kind[i];
    const int32_t len = pk_len[i];
    uint32_t show = kind;
    if ((kind != kPackFrame && kind != kPackRaw) || len < 0) show = kVerifyInvalid;
    else if (got[i] != pk_crc[i]) show = kVerifyBadCrc;
    masked[i] = show == kPackFrame ? len : 0;
    shown[i] = (uint8_t)show;
}

// Behind the decoders and the raw copy, which both left -1 there.
__global__ __launch_bounds__(256) void unpack_verify_ret_kernel(const uint8_t* __restrict__ shown, uint32_t nblocks,
                                                                int32_t* __restrict__ ret) {
    const uint64_t i = (uint64_t)blockIdx.x * kCrcThreads + threadIdx.x;
    if (i >= nblocks) return;
    const uint32_t show = shown[i];
    if (show == kVerifyBadCrc) ret[i] = kUnpackBadCrc;
    else if (show == kVerifyInvalid) ret[i] = -1;
}

// The verified range read's four kernels (lz4e_gpu.h, RangeVerifyBatch), a
// thread per request each.  A request's validity is range_req's on the REAL
// kind column, the plain range read's own test.
__global__ __launch_bounds__(256) void range_verify_init_kernel(const uint8_t* __restrict__ pk_kind,
                                                                uint32_t nentries, const uint32_t* __restrict__ sel,
                                                                uint32_t nreq, uint32_t* __restrict__ owner,
                                                                uint8_t* __restrict__ shown) {
    const uint64_t j = (uint64_t)blockIdx.x * kCrcThreads + threadIdx.x;
    if (j >= nreq) return;
    const uint32_t e = sel ? sel[j] : (uint32_t)j;
    if (e >= nentries) return;
    // (requests that share an entry all store the same two values)
    owner[e] = kNoOwner;
    shown[e] = pk_kind[e];
}

__global__ __launch_bounds__(256) void range_verify_elect_kernel(
    const uint64_t* __restrict__ pk_off, const int32_t* __restrict__ pk_len, const uint8_t* __restrict__ pk_kind,
    uint32_t nentries, const uint32_t* __restrict__ sel, const int32_t* __restrict__ lo,
    const int32_t* __restrict__ len, uint32_t nreq, uint32_t* __restrict__ owner, uint64_t* __restrict__ c_off,
    int32_t* __restrict__ c_len) {
    const uint64_t j = (uint64_t)blockIdx.x * kCrcThreads + threadIdx.x;
    if (j >= nreq) return;
    const RangeReq q = range_req(sel, lo, len, pk_len, pk_kind, nentries, j);
    bool won = false;
    if (q.valid && len[j] > 0) won = atomicCAS(&owner[q.entry], kNoOwner, (uint32_t)j) == kNoOwner;
    c_off[j] = won ? pk_off[q.entry] : 0;
    c_len[j] = won ? pk_len[q.entry] : 0;
}

__global__ __launch_bounds__(256) void range_verify_verdict_kernel(
    const int32_t* __restrict__ pk_len, const uint8_t* __restrict__ pk_kind, const uint32_t* __restrict__ pk_crc,
    uint32_t nentries, const uint32_t* __restrict__ sel, const int32_t* __restrict__ lo,
    const int32_t* __restrict__ len, uint32_t nreq, const uint32_t* __restrict__ owner,
    const uint32_t* __restrict__ got, uint8_t* __restrict__ shown) {
    const uint64_t j = (uint64_t)blockIdx.x * kCrcThreads + threadIdx.x;
    if (j >= nreq) return;
    const RangeReq q = range_req(sel, lo, len, pk_len, pk_kind, nentries, j);
    // (only a request that wanted its entry was ever made its owner)
    if (q.valid && owner[q.entry] == (uint32_t)j && got[j] != pk_crc[q.entry]) shown[q.entry] = (uint8_t)kVerifyBadCrc;
}

// Behind range_deliver_kernel, which saw `shown` and left -1 for every request
// on a marked entry.
__global__ __launch_bounds__(256) void range_verify_ret_kernel(
    const int32_t* __restrict__ pk_len, const uint8_t* __restrict__ pk_kind, uint32_t nentries,
    const uint32_t* __restrict__ sel, const int32_t* __restrict__ lo, const int32_t* __restrict__ len,
    uint32_t nreq, const uint8_t* __restrict__ shown, int32_t* __restrict__ ret) {
    const uint64_t j = (uint64_t)blockIdx.x * kCrcThreads + threadIdx.x;
    if (j >= nreq) return;
    const RangeReq q = range_req(sel, lo, len, pk_len, pk_kind, nentries, j);
    if (!q.valid) return;
    if (len[j] == 0) ret[j] = 0;
    else if (shown[q.entry] == kVerifyBadCrc) ret[j] = kUnpackBadCrc;
}

dim3 per_entry_grid(uint32_t nblocks) { return dim3((uint32_t)(((uint64_t)nblocks + kCrcThreads - 1) / kCrcThreads)); }

}  // namespace

// Threads per entry as pack_copy_kernel's: about 64 bytes for each of the
// largest entry, a power of two from 16 to 16384.  A team is split over
// several workgroups only while the launch stays within 2^20 of them (their
// partials are 4 MiB of scratch; past that the batch fills the chip anyway).
uint32_t crc_team_shift(uint32_t max_len, uint32_t nblocks) {
    uint32_t shift = 4;
    while (shift < 14 && ((uint64_t)64 << shift) < max_len) ++shift;
    while (shift > 8 && (((uint64_t)nblocks << shift) / kCrcThreads) > (1u << 20)) --shift;
    while (shift > 4 && (((uint64_t)nblocks << shift) + kCrcThreads - 1) / kCrcThreads > 0x7FFFFFFFull) --shift;
    return shift;
}

uint64_t crc_partial_words(uint32_t max_len, uint32_t nblocks) {
    const uint32_t shift = crc_team_shift(max_len, nblocks);
    return shift > 8 ? ((uint64_t)nblocks << (shift - 8)) : 0;
}

hipError_t launch_crc(const CrcBatch& a, uint32_t* partial, hipStream_t stream) {
    if (a.nblocks == 0) return hipSuccess;
    const uint32_t shift = crc_team_shift(a.max_len, a.nblocks);
    const dim3 grid((uint32_t)((((uint64_t)a.nblocks << shift) + kCrcThreads - 1) / kCrcThreads));
    if (shift <= 8) {
        hipLaunchKernelGGL(crc_team_kernel, grid, dim3(kCrcThreads), 0, stream, a, shift, a.crc);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(crc_team_kernel, grid, dim3(kCrcThreads), 0, stream, a, shift, partial);
    hipLaunchKernelGGL(crc_combine_kernel, per_entry_grid(a.nblocks), dim3(kCrcThreads), 0, stream,
                       (const uint32_t*)partial, a.len, a.kind, a.nblocks, shift - 8, a.crc);
    return hipGetLastError();
}

hipError_t launch_unpack_verify_mask(const int32_t* pk_len, const uint8_t* pk_kind, const uint32_t* pk_crc,
                                     const uint32_t* got, uint32_t nblocks, int32_t* masked, uint8_t* shown,
                                     hipStream_t stream) {
    if (nblocks == 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_verify_mask_kernel, per_entry_grid(nblocks), dim3(kCrcThreads), 0, stream, pk_len,
                       pk_kind, pk_crc, got, nblocks, masked, shown);
    return hipGetLastError();
}

hipError_t launch_unpack_verify_ret(const uint8_t* shown, uint32_t nblocks, int32_t* ret, hipStream_t stream) {
    if (nblocks == 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_verify_ret_kernel, per_entry_grid(nblocks), dim3(kCrcThreads), 0, stream, shown,
                       nblocks, ret);
    return hipGetLastError();
}

hipError_t launch_range_verify_init(const RangeVerifyBatch& a, hipStream_t stream) {
    if (a.nreq == 0) return hipSuccess;
    hipLaunchKernelGGL(range_verify_init_kernel, per_entry_grid(a.nreq), dim3(kCrcThreads), 0, stream, a.pk_kind,
                       a.nentries, a.sel, a.nreq, a.owner, a.shown);
    return hipGetLastError();
}

hipError_t launch_range_verify_elect(const RangeVerifyBatch& a, hipStream_t stream) {
    if (a.nreq == 0) return hipSuccess;
    hipLaunchKernelGGL(range_verify_elect_kernel, per_entry_grid(a.nreq), dim3(kCrcThreads), 0, stream, a.pk_off,
                       a.pk_len, a.pk_kind, a.nentries, a.sel, a.lo, a.len, a.nreq, a.owner, a.c_off, a.c_len);
    return hipGetLastError();
}

hipError_t launch_range_verify_verdict(const RangeVerifyBatch& a, hipStream_t stream) {
    if (a.nreq == 0) return hipSuccess;
    hipLaunchKernelGGL(range_verify_verdict_kernel, per_entry_grid(a.nreq), dim3(kCrcThreads), 0, stream, a.pk_len,
                       a.pk_kind, a.pk_crc, a.nentries, a.sel, a.lo, a.len, a.nreq, (const uint32_t*)a.owner,
                       (const uint32_t*)a.got, a.shown);
    return hipGetLastError();
}

hipError_t launch_range_verify_ret(const RangeVerifyBatch& a, hipStream_t stream) {
    if (a.nreq == 0) return hipSuccess;
    hipLaunchKernelGGL(range_verify_ret_kernel, per_entry_grid(a.nreq), dim3(kCrcThreads), 0, stream, a.pk_len,
                       a.pk_kind, a.nentries, a.sel, a.lo, a.len, a.nreq, (const uint8_t*)a.shown, a.ret);
    return hipGetLastError();
}

}  // namespace lz4e
