// lz4e_copy.h -- the byte-exact cooperative copy (and fill) of the kernels
// that work on the CALLER's memory: the zero-copy scatter-gather kernels
// (lz4e_sg.hip) and the packed frame store (lz4e_pack.hip).  The one hard
// rule of both routines: no load and no store touches a byte outside
// [src, src + n) or [dst, dst + n).  The next byte may be someone else's data
// or an unmapped page.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lz4e {
namespace {

typedef uint32_t sg_v4 __attribute__((ext_vector_type(4)));

// Copies n bytes from src to dst as thread t of nt cooperating threads.
// src and dst have arbitrary, different byte alignment.  The body is 16-B
// stores aligned on dst fed by unaligned 16-B loads (global loads need no
// alignment on gfx950), consecutive threads on consecutive vectors; the
// < 16 bytes before dst's first 16-B boundary and the < 16 after its last
// whole vector go byte by byte.  Every access lies inside [src, src + n) /
// [dst, dst + n): the vectors cover [head, head + 16 nvec) with
// head + 16 nvec <= n.
__device__ __forceinline__ void sg_copy(uint8_t* dst, const uint8_t* src, uint64_t n, uint32_t t,
                                        uint32_t nt) {
    const uint64_t to_boundary = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
    const uint64_t head = to_boundary < n ? to_boundary : n;
    const uint64_t nvec = (n - head) >> 4;
    const uint64_t tail = head + (nvec << 4);
    for (uint64_t i = t; i < nvec; i += nt) {
        sg_v4 v;
        __builtin_memcpy(&v, src + head + (i << 4), 16);
        *reinterpret_cast<sg_v4*>(dst + head + (i << 4)) = v;
    }
    for (uint64_t i = t; i < head; i += nt) dst[i] = src[i];
    for (uint64_t i = tail + t; i < n; i += nt) dst[i] = src[i];
}

// Zeroes the n bytes at dst as thread t of nt cooperating threads: sg_copy's
// split of [dst, dst + n) (bytes up to dst's first 16-B boundary, aligned
// 16-B stores, bytes after the last whole vector) with nothing to load.
__device__ __forceinline__ void sg_zero(uint8_t* dst, uint64_t n, uint32_t t, uint32_t nt) {
    const uint64_t to_boundary = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
    const uint64_t head = to_boundary < n ? to_boundary : n;
    const uint64_t nvec = (n - head) >> 4;
    const uint64_t tail = head + (nvec << 4);
    const sg_v4 z = {0u, 0u, 0u, 0u};
    for (uint64_t i = t; i < nvec; i += nt) *reinterpret_cast<sg_v4*>(dst + head + (i << 4)) = z;
    for (uint64_t i = t; i < head; i += nt) dst[i] = 0;
    for (uint64_t i = tail + t; i < n; i += nt) dst[i] = 0;
}

}  // namespace
}  // namespace lz4e
