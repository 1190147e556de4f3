// lz4e_pack.hip -- the packed frame store's kernels (gfx950): the slots of a
// compress launch compacted into one dense image with an index, blocks that
// did not shrink stored raw (include/lz4e.h, lz4e_pack_batch_dev), and the way
// back (lz4e_unpack_batch_dev).
//
// Pack is four launches on the caller's stream; the kernel boundaries are the
// only ordering between workgroups (no kernel waits on another workgroup, no
// flag, no atomics):
//
//   pack_tile_sum_kernel   one workgroup per tile of kPackTile blocks: each
//                          thread decides its block's kind and length, the
//                          tile's padded sizes are summed (64-bit) and the sum
//                          is parked in pk_off[first block of the tile] -- a
//                          slot the index owns anyway, so pack needs no scratch.
//   pack_tile_scan_kernel  ONE workgroup of one wave: exclusive scan of the
//                          parked sums in place, 64 per round, a 64-bit carry
//                          between rounds; pk_off[nblocks] = the stored size.
//   pack_index_kernel      per tile again: exclusive scan of the padded sizes
//                          plus the tile's base -> pk_off, pk_len, pk_kind.
//   pack_copy_kernel       the gather.  A team of 16 ... 16384 threads per
//                          entry (a power of two picked from max_len: about
//                          64 bytes per thread of the largest entry, so 4 KiB
//                          blocks take a wave each, four to a workgroup, and a
//                          256 KiB block sixteen workgroups) copies the frame
//                          or the raw input with sg_copy and zeroes the
//                          padding.  Its first act is the overflow test, read
//                          from pk_off[nblocks]: a uniform early return.
//
// Unpack runs the unchanged decoders between two small kernels:
// unpack_mask_kernel writes the frame entries' lengths (0 for every other
// kind: each decoder returns -1 for srcSize 0 before it reads or writes
// anything), unpack_raw_kernel copies the raw entries behind the decoders and
// sets ret of everything that is not a frame.
//
// These kernels read and write the CALLER's memory at byte granularity, so
// every copy is sg_copy (lz4e_copy.h): nothing outside [src, src + n) and
// [dst, dst + n) is touched.
//
// Kernels and launches only (no other runtime call), so that tools/emu
// compiles this file as host C++ (tools/emu/emu_pack.cpp,
// tests/test_emulator_pack.py: every buffer an exact-size heap allocation
// under ASan).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4e_copy.h"
#include "lz4e_gpu.h"
#include "lz4e_range.h"
#include "lz4e_wave.h"

namespace lz4e {
namespace {

constexpr uint32_t kPackThreads = 256;
static_assert(kPackTile == kPackThreads, "one block per thread of a scan tile");

// Inclusive prefix sum over the wave of 64-bit values (the batch's total stays
// far below 2^63): three 21-bit limbs, each a 32-bit DPP scan that cannot
// overflow (64 x 2^21 = 2^27).
LZ4E_DEV uint64_t wave_incl_add64(uint64_t v) {
    constexpr uint64_t m = (1u << 21) - 1;
    const uint64_t a = wave_incl_add((uint32_t)(v & m));
    const uint64_t b = wave_incl_add((uint32_t)((v >> 21) & m));
    const uint64_t c = wave_incl_add((uint32_t)(v >> 42));
    return a + (b << 21) + (c << 42);
}

// Inclusive prefix sum of v over the workgroup's kPackThreads threads, the
// workgroup's sum in *total.  wsum: LDS, one word per wave.  Called by every
// thread (wave-uniform and workgroup-uniform control flow).
LZ4E_DEV uint64_t block_incl_add64(uint64_t v, uint64_t* wsum, uint64_t* total) {
    const uint32_t w = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const uint64_t x = wave_incl_add64(v);
    if (lane == kWave - 1) wsum[w] = x;
    block_sync();
    uint64_t base = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPackThreads / kWave; ++k) {
        const uint64_t s = wsum[k];
        base += k < w ? s : 0;
        all += s;
    }
    block_sync();  // wsum is written again by the caller's next round
    *total = all;
    return x + base;
}

// Block i's entry: a frame when the compress succeeded and the frame is
// smaller than the input, else the input itself.
struct PackEntry {
    uint32_t len, kind;
};
LZ4E_DEV PackEntry pack_entry(const int32_t* ret, const uint32_t* src_len, uint32_t i) {
    const int32_t r = ret[i];
    const uint32_t n = src_len[i];
    const bool frame = r > 0 && (uint32_t)r < n;
    return PackEntry{frame ? (uint32_t)r : n, frame ? kPackFrame : kPackRaw};
}
LZ4E_DEV uint64_t pack_padded(uint32_t len, uint32_t align) {
    return ((uint64_t)len + (align - 1)) & ~(uint64_t)(align - 1);
}

__global__ __launch_bounds__(256) void pack_tile_sum_kernel(const int32_t* __restrict__ ret,
                                                            const uint32_t* __restrict__ src_len,
                                                            uint32_t align, uint32_t nblocks,
                                                            uint64_t* __restrict__ pk_off) {
    __shared__ uint64_t wsum[kPackThreads / kWave];
    const uint64_t first = (uint64_t)blockIdx.x * kPackTile;
    const uint64_t i = first + threadIdx.x;
    const uint64_t v = i < nblocks ? pack_padded(pack_entry(ret, src_len, (uint32_t)i).len, align) : 0;
    uint64_t total;
    (void)block_incl_add64(v, wsum, &total);
    if (threadIdx.x == 0) pk_off[first] = total;  // first < nblocks: the grid has no empty tile
}

// One wave: its rounds need neither LDS nor a barrier.
__global__ __launch_bounds__(64) void pack_tile_scan_kernel(uint64_t* __restrict__ pk_off, uint32_t nblocks,
                                                            uint32_t ntiles) {
    uint64_t carry = 0;
    for (uint32_t base = 0; base < ntiles; base += kWave) {
        const uint32_t k = base + threadIdx.x;
        const uint64_t slot = (uint64_t)k * kPackTile;  // the tile's first block
        const uint64_t v = k < ntiles ? pk_off[slot] : 0;
        const uint64_t incl = wave_incl_add64(v);
        if (k < ntiles) pk_off[slot] = carry + incl - v;
        // the round's sum: the last lane's inclusive value, in two halves
        carry += ((uint64_t)lane_val((uint32_t)(incl >> 32), kWave - 1) << 32) | lane_val((uint32_t)incl, kWave - 1);
    }
    if (threadIdx.x == 0) pk_off[nblocks] = carry;
}

__global__ __launch_bounds__(256) void pack_index_kernel(const int32_t* __restrict__ ret,
                                                         const uint32_t* __restrict__ src_len,
                                                         uint32_t align, uint32_t nblocks,
                                                         uint64_t* pk_off, int32_t* __restrict__ pk_len,
                                                         uint8_t* __restrict__ pk_kind) {
    __shared__ uint64_t wsum[kPackThreads / kWave];
    const uint64_t first = (uint64_t)blockIdx.x * kPackTile;
    const uint64_t i = first + threadIdx.x;
    const bool have = i < nblocks;
    // every thread reads the tile's base before the scan's barrier; its slot
    // is rewritten (with the same value) only after it
    const uint64_t tile_base = pk_off[first];
    PackEntry e{0, kPackRaw};
    if (have) e = pack_entry(ret, src_len, (uint32_t)i);
    const uint64_t v = have ? pack_padded(e.len, align) : 0;
    uint64_t total;
    const uint64_t incl = block_incl_add64(v, wsum, &total);
    if (have) {
        pk_off[i] = tile_base + incl - v;
        pk_len[i] = (int32_t)e.len;
        pk_kind[i] = (uint8_t)e.kind;
    }
}

// Entry g >> team_shift is the work of the 1 << team_shift consecutive
// threads of the launch that share it.
__global__ __launch_bounds__(256) void pack_copy_kernel(
    const uint8_t* __restrict__ frames, const uint64_t* __restrict__ fr_off,
    const uint8_t* __restrict__ src, const uint64_t* __restrict__ src_off, uint8_t* __restrict__ packed,
    uint64_t packed_cap, const uint64_t* __restrict__ pk_off, const int32_t* __restrict__ pk_len,
    const uint8_t* __restrict__ pk_kind, uint32_t nblocks, uint32_t team_shift) {
    if (pk_off[nblocks] > packed_cap) return;  // all or nothing (uniform)
    const uint64_t g = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x;
    const uint64_t i = g >> team_shift;
    if (i >= nblocks) return;
    const uint32_t nt = 1u << team_shift, t = (uint32_t)g & (nt - 1);
    const uint64_t at = pk_off[i], end = pk_off[i + 1];
    const uint64_t len = (uint32_t)pk_len[i];
    const uint8_t* from = pk_kind[i] == kPackFrame ? frames + fr_off[i] : src + src_off[i];
    sg_copy(packed + at, from, len, t, nt);
    sg_zero(packed + at + len, end - at - len, t, nt);
}

__global__ __launch_bounds__(256) void unpack_mask_kernel(const int32_t* __restrict__ pk_len,
                                                          const uint8_t* __restrict__ pk_kind,
                                                          uint32_t nblocks, int32_t* __restrict__ masked) {
    const uint64_t i = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x;
    if (i < nblocks) masked[i] = pk_kind[i] == kPackFrame ? pk_len[i] : 0;
}

// Teams as in pack_copy_kernel.  A frame entry is the decoders' business.
__global__ __launch_bounds__(256) void unpack_raw_kernel(
    const uint8_t* __restrict__ packed, const uint64_t* __restrict__ pk_off,
    const int32_t* __restrict__ pk_len, const uint8_t* __restrict__ pk_kind, uint8_t* __restrict__ dst,
    const uint64_t* __restrict__ dst_off, const int32_t* __restrict__ dst_cap, int32_t* __restrict__ ret,
    uint32_t nblocks, uint32_t team_shift) {
    const uint64_t g = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x;
    const uint64_t i = g >> team_shift;
    if (i >= nblocks) return;
    const uint32_t kind = pk_kind[i];
    if (kind == kPackFrame) return;
    const uint32_t nt = 1u << team_shift, t = (uint32_t)g & (nt - 1);
    const int32_t len = pk_len[i];
    const bool ok = kind == kPackRaw && len >= 0 && len <= dst_cap[i];
    if (t == 0) ret[i] = ok ? len : -1;
    if (ok) sg_copy(dst + dst_off[i], packed + pk_off[i], (uint32_t)len, t, nt);
}

// Range read (lz4e_unpack_range_batch_dev), in front of the partial launch:
// request j's frame as the decoders see it.  A request the decoders must not
// touch -- not a frame entry, invalid, or empty -- gets length 0 and target 0:
// each decoder returns for it before it reads or writes anything.  The
// target is clamped to max_end, the size of a request's scratch slot.
// (RangeReq / range_req, a request's validity: lz4e_range.h.)
LZ4E_DEV int32_t range_end(const int32_t* lo, const int32_t* len, uint32_t max_end, uint64_t j) {
    const uint64_t end = (uint64_t)(uint32_t)lo[j] + (uint32_t)len[j];
    return (int32_t)(end < max_end ? end : max_end);
}

__global__ __launch_bounds__(256) void range_gather_kernel(
    const uint64_t* __restrict__ pk_off, const int32_t* __restrict__ pk_len, const uint8_t* __restrict__ pk_kind,
    uint32_t nentries, const uint32_t* __restrict__ sel, const int32_t* __restrict__ lo,
    const int32_t* __restrict__ len, uint32_t nreq, uint32_t max_end, uint64_t slot, uint64_t* __restrict__ g_off,
    int32_t* __restrict__ g_len, int32_t* __restrict__ g_tgt, uint64_t* __restrict__ s_off) {
    const uint64_t j = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x;
    if (j >= nreq) return;
    const RangeReq q = range_req(sel, lo, len, pk_len, pk_kind, nentries, j);
    const bool dec = q.valid && pk_kind[q.entry] == kPackFrame && len[j] > 0;
    g_off[j] = dec ? pk_off[q.entry] : 0;
    g_len[j] = dec ? pk_len[q.entry] : 0;
    g_tgt[j] = dec ? range_end(lo, len, max_end, j) : 0;
    s_off[j] = j * slot;
}

// Behind the partial launch, teams as in pack_copy_kernel: the wanted bytes
// of each request from its scratch slot (frame entries) or straight from the
// image (raw entries), and ret.
__global__ __launch_bounds__(256) void range_deliver_kernel(
    const uint8_t* __restrict__ packed, const uint64_t* __restrict__ pk_off, const int32_t* __restrict__ pk_len,
    const uint8_t* __restrict__ pk_kind, uint32_t nentries, const uint32_t* __restrict__ sel,
    const int32_t* __restrict__ lo, const int32_t* __restrict__ len, uint8_t* __restrict__ dst,
    const uint64_t* __restrict__ dst_off, int32_t* __restrict__ ret, uint32_t nreq, uint32_t max_end,
    const uint8_t* __restrict__ scratch, uint64_t slot, const int32_t* __restrict__ g_ret, uint32_t team_shift) {
    const uint64_t g = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x;
    const uint64_t j = g >> team_shift;
    if (j >= nreq) return;
    const uint32_t nt = 1u << team_shift, t = (uint32_t)g & (nt - 1);
    const RangeReq q = range_req(sel, lo, len, pk_len, pk_kind, nentries, j);
    if (!q.valid || len[j] == 0) {
        if (t == 0) ret[j] = q.valid ? 0 : -1;
        return;
    }
    const int32_t end = range_end(lo, len, max_end, j);
    const uint8_t* from;
    int32_t d;
    if (pk_kind[q.entry] == kPackFrame) {
        d = g_ret[j];  // the partial decode with target `end`
        from = scratch + j * slot;
    } else {
        d = pk_len[q.entry] < end ? pk_len[q.entry] : end;
        from = packed + pk_off[q.entry];
    }
    if (d < 0) {
        if (t == 0) ret[j] = d;
        return;
    }
    const int32_t cnt = d > lo[j] ? d - lo[j] : 0;
    if (t == 0) ret[j] = cnt;
    sg_copy(dst + dst_off[j], from + lo[j], (uint64_t)cnt, t, nt);
}

// Threads per entry: about 64 bytes for each of the largest entry, a power
// of two from 16 (a quarter wave: tiny entries, many to a workgroup) to 16384
// (64 workgroups on one entry); fewer where the grid would pass 2^31 - 1.
uint32_t team_shift_for(uint32_t max_len, uint32_t nblocks) {
    uint32_t shift = 4;
    while (shift < 14 && ((uint64_t)64 << shift) < max_len) ++shift;
    while (shift > 4 && (((uint64_t)nblocks << shift) + kPackThreads - 1) / kPackThreads > 0x7FFFFFFFull) --shift;
    return shift;
}
dim3 team_grid(uint32_t nblocks, uint32_t shift) {
    return dim3((uint32_t)((((uint64_t)nblocks << shift) + kPackThreads - 1) / kPackThreads));
}

}  // namespace

hipError_t launch_pack(const PackBatch& a, hipStream_t stream) {
    const uint32_t ntiles = (uint32_t)(((uint64_t)a.nblocks + kPackTile - 1) / kPackTile);
    const dim3 block(kPackThreads);
    if (ntiles)
        hipLaunchKernelGGL(pack_tile_sum_kernel, dim3(ntiles), block, 0, stream, a.ret, a.src_len, a.align,
                           a.nblocks, a.pk_off);
    // (with no block at all this launch alone runs: pk_off[0] = 0)
    hipLaunchKernelGGL(pack_tile_scan_kernel, dim3(1), dim3(kWave), 0, stream, a.pk_off, a.nblocks, ntiles);
    if (ntiles == 0) return hipGetLastError();
    hipLaunchKernelGGL(pack_index_kernel, dim3(ntiles), block, 0, stream, a.ret, a.src_len, a.align, a.nblocks,
                       a.pk_off, a.pk_len, a.pk_kind);
    const uint32_t shift = team_shift_for(a.max_len, a.nblocks);
    hipLaunchKernelGGL(pack_copy_kernel, team_grid(a.nblocks, shift), block, 0, stream, a.frames, a.fr_off, a.src,
                       a.src_off, a.packed, a.packed_cap, (const uint64_t*)a.pk_off, (const int32_t*)a.pk_len,
                       (const uint8_t*)a.pk_kind, a.nblocks, shift);
    return hipGetLastError();
}

hipError_t launch_unpack_mask(const int32_t* pk_len, const uint8_t* pk_kind, uint32_t nblocks, int32_t* masked,
                              hipStream_t stream) {
    if (nblocks == 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_mask_kernel, team_grid(nblocks, 0), dim3(kPackThreads), 0,
                       stream, pk_len, pk_kind, nblocks, masked);
    return hipGetLastError();
}

hipError_t launch_unpack_raw(const UnpackRawBatch& a, hipStream_t stream) {
    if (a.nblocks == 0) return hipSuccess;
    // capacity unknown: a workgroup per entry
    const uint32_t shift = a.max_cap ? team_shift_for(a.max_cap, a.nblocks) : team_shift_for(256 * 64, a.nblocks);
    hipLaunchKernelGGL(unpack_raw_kernel, team_grid(a.nblocks, shift), dim3(kPackThreads), 0, stream, a.packed,
                       a.pk_off, a.pk_len, a.pk_kind, a.dst, a.dst_off, a.dst_cap, a.ret, a.nblocks, shift);
    return hipGetLastError();
}

hipError_t launch_range_gather(const RangeBatch& a, hipStream_t stream) {
    if (a.nreq == 0) return hipSuccess;
    hipLaunchKernelGGL(range_gather_kernel, team_grid(a.nreq, 0), dim3(kPackThreads), 0, stream, a.pk_off, a.pk_len,
                       a.pk_kind, a.nentries, a.sel, a.lo, a.len, a.nreq, a.max_end, a.slot, a.g_off, a.g_len,
                       a.g_tgt, a.s_off);
    return hipGetLastError();
}

hipError_t launch_range_deliver(const RangeBatch& a, hipStream_t stream) {
    if (a.nreq == 0) return hipSuccess;
    const uint32_t shift = team_shift_for(a.max_end, a.nreq);
    hipLaunchKernelGGL(range_deliver_kernel, team_grid(a.nreq, shift), dim3(kPackThreads), 0, stream, a.packed,
                       a.pk_off, a.pk_len, a.pk_kind, a.nentries, a.sel, a.lo, a.len, a.dst, a.dst_off, a.ret,
                       a.nreq, a.max_end, (const uint8_t*)a.scratch, a.slot, (const int32_t*)a.g_ret, shift);
    return hipGetLastError();
}

}  // namespace lz4e
