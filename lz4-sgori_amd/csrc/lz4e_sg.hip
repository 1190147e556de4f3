// lz4e_sg.hip -- the chunk pipeline's zero-copy kernels (gfx950): the device
// itself reads a request's scatter-gather segments out of registered host
// memory and writes its results back there, over PCIe, where the staged path
// bounces both through pinned staging with host memcpy.
//
//   sg_gather_kernel   one workgroup per descriptor {source device address,
//                      destination offset in the slot's HBM data buffer,
//                      length}: the segment lands where the staged path's H2D
//                      copy would have put it, so launch_compress and
//                      launch_decompress run on that buffer unchanged.
//   sg_deliver_kernel  per request, chunk_finish's decision on the device
//                      (lz4e_host.hip): nothing is written unless the round
//                      trip succeeded and the frame fits; then ret frame
//                      bytes go to `frame` and len bytes to `data`.
//
// Both run on the CALLER's memory, so unlike copy_flat_kernel /
// copy_blocks_kernel (which round up to 16 B inside staging they own) the
// one copy routine (lz4e_copy.h) obeys a hard rule: no load and no store touches a
// byte outside [src, src + n) or [dst, dst + n).  The next byte may be
// someone else's data or an unmapped page.
//
// Kernels and launches only (no other runtime call), so that tools/emu
// compiles this file as host C++ like the other two kernel files
// (tools/emu/emu_sg.cpp, tests/test_emulator_sg.py: every buffer an
// exact-size heap allocation under ASan).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4e_copy.h"
#include "lz4e_gpu.h"

namespace lz4e {
namespace {

constexpr uint32_t kSgThreads = 256;

// sg_copy, the one copy routine of both kernels, lives in lz4e_copy.h (shared
// with the packed frame store, lz4e_pack.hip).

__global__ __launch_bounds__(256) void sg_gather_kernel(const SgGatherDesc* __restrict__ desc,
                                                        uint32_t ndesc, uint8_t* __restrict__ data) {
    const uint32_t d = blockIdx.x;
    if (d >= ndesc) return;
    const SgGatherDesc q = desc[d];
    sg_copy(data + q.dst_off, reinterpret_cast<const uint8_t*>(q.src), q.len, threadIdx.x, kSgThreads);
}

// `parts` workgroups per descriptor share its two copies.
__global__ __launch_bounds__(256) void sg_deliver_kernel(const SgDeliverDesc* __restrict__ desc,
                                                         uint32_t ndesc, uint32_t parts,
                                                         const uint8_t* __restrict__ data,
                                                         const uint64_t* __restrict__ fr_off,
                                                         const uint64_t* __restrict__ out_off,
                                                         const uint32_t* __restrict__ in_len,
                                                         const int32_t* __restrict__ ret,
                                                         const int32_t* __restrict__ dret) {
    const uint32_t d = blockIdx.x / parts, part = blockIdx.x % parts;
    if (d >= ndesc) return;
    const SgDeliverDesc q = desc[d];
    const uint32_t j = q.entry;
    const int32_t r = ret[j];
    const uint32_t len = in_len[j];
    if (r <= 0 || dret[j] != (int32_t)len) return;  // -EIO: nothing reaches the caller
    if (q.frame && q.frame_cap < r) return;         // -ENOSPC: neither frame nor data
    const uint32_t t = part * kSgThreads + threadIdx.x, nt = parts * kSgThreads;
    if (q.frame) sg_copy(reinterpret_cast<uint8_t*>(q.frame), data + fr_off[j], (uint32_t)r, t, nt);
    sg_copy(reinterpret_cast<uint8_t*>(q.data), data + out_off[j], len, t, nt);
}

}  // namespace

hipError_t launch_sg_gather(const SgGatherDesc* desc, uint32_t ndesc, uint8_t* data, hipStream_t stream) {
    if (ndesc == 0) return hipSuccess;
    hipLaunchKernelGGL(sg_gather_kernel, dim3(ndesc), dim3(kSgThreads), 0, stream, desc, ndesc, data);
    return hipGetLastError();
}

hipError_t launch_sg_deliver(const SgDeliverBatch& a, hipStream_t stream) {
    if (a.ndesc == 0) return hipSuccess;
    // one workgroup per kSgPiece bytes of the largest request, as in the gather
    uint32_t parts = (a.max_len + kSgPiece - 1) / kSgPiece;
    parts = parts < 1 ? 1 : (parts > 64 ? 64 : parts);
    while (parts > 1 && (uint64_t)a.ndesc * parts > 0x7FFFFFFFull) parts /= 2;  // grid limit
    hipLaunchKernelGGL(sg_deliver_kernel, dim3(a.ndesc * parts), dim3(kSgThreads), 0, stream, a.desc,
                       a.ndesc, parts, a.data, a.fr_off, a.out_off, a.in_len, a.ret, a.dret);
    return hipGetLastError();
}

}  // namespace lz4e
