"""lz4e_amd -- Python view of the MI355X-native LZ4E scatter-gather codec.

The product is the C-ABI library ``liblz4e_amd.so`` (include/lz4e.h): HIP
kernels for gfx950 plus a host shim.  This module only binds it with ctypes
so that tests and the benchmark can drive the same entry points a C caller
(the lz4e_bdev chunk layer, lz4e_bdev/lz4e_chunk.c:139-159) would use:

* :func:`compress_default`   -- ``LZ4E_compress_default`` (bio_vec in/out)
* :func:`decompress_safe`    -- ``LZ4E_decompress_safe``
* :func:`compress_sg_batch`  -- many SG requests, one launch
* :func:`compress_batch_dev` / :func:`decompress_batch_dev` -- device-resident
  batches on torch CUDA(HIP) tensors (the throughput path)

There is no CPU fallback: importing works without a GPU (so host-side
helpers and symbol checks can run anywhere), but every codec call fails
loudly (:class:`GpuUnavailable`) when the library cannot reach a gfx950.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

__all__ = [
    "PAGE_SIZE", "BIO_MAX_VECS", "LZ4E_MEM_COMPRESS", "LZ4E_MAX_INPUT_SIZE",
    "BYU16", "BYU32", "BYU64", "compress_bound", "BioVec", "BvecIter",
    "SgRequest", "SgList", "make_sg", "lib", "gpu_available", "table_type",
    "compress_default", "decompress_safe", "compress_sg_batch",
    "decompress_batch", "compress_batch_dev", "decompress_batch_dev",
    "GpuUnavailable", "LIB_PATH", "EXPORTED_SYMBOLS", "HostArena", "GuardReport",
    "register_host_memory", "unregister_host_memory", "zero_copy_requests",
    "pack_batch_dev", "unpack_batch_dev", "PACK_FRAME", "PACK_RAW",
    "crc32c_batch_dev", "pack_crc_batch_dev", "unpack_verified_batch_dev", "UNPACK_BAD_CRC",
    "decompress_safe_partial", "decompress_partial_batch", "decompress_partial_batch_dev",
    "unpack_range_batch_dev", "unpack_range_verified_batch_dev",
]

PAGE_SIZE = 4096
BIO_MAX_VECS = 256
LZ4E_MEM_COMPRESS = 17440
LZ4E_MAX_INPUT_SIZE = 0x7E000000
BYU16, BYU32, BYU64 = 1, 3, 7

LIB_PATH = os.environ.get("LZ4E_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "liblz4e_amd.so")

# Every function include/lz4e.h declares.
EXPORTED_SYMBOLS = (
    "LZ4E_compress_default", "LZ4E_decompress_safe", "lz4e_sg_table_type",
    "lz4e_last_error", "lz4e_gpu_available", "lz4e_compress_sg_batch",
    "lz4e_decompress_batch", "lz4e_compress_batch_dev", "lz4e_decompress_batch_dev",
    "lz4e_decompress_batch_dev2",
    "lz4e_chunk_write_batch", "lz4e_decompress_safe_sg", "lz4e_decompress_sg_batch",
    "LZ4E_compress_usingDict", "LZ4E_decompress_safe_usingDict", "lz4e_compress_sg_batch_dict",
    "lz4e_decompress_batch_dict", "lz4e_compress_batch_dev_dict", "lz4e_decompress_batch_dev_dict",
    "lz4e_register_host_memory", "lz4e_unregister_host_memory",
    "lz4e_pack_batch_dev", "lz4e_unpack_batch_dev",
    "lz4e_crc32c_batch_dev", "lz4e_pack_crc_batch_dev", "lz4e_unpack_verified_batch_dev",
    "LZ4E_decompress_safe_partial", "lz4e_decompress_partial_batch", "lz4e_decompress_partial_batch_dev",
    "lz4e_unpack_range_batch_dev", "lz4e_unpack_range_verified_batch_dev",
)


class GpuUnavailable(RuntimeError):
    """The library could not reach a gfx950 device (no fallback exists)."""


def compress_bound(n: int) -> int:
    """LZ4E_COMPRESSBOUND (lz4e/include/lz4e.h:25-28)."""
    return 0 if n > LZ4E_MAX_INPUT_SIZE else n + n // 255 + 16


class BioVec(ctypes.Structure):
    _fields_ = [("bv_page", ctypes.c_void_p), ("bv_len", ctypes.c_uint),
                ("bv_offset", ctypes.c_uint)]


class BvecIter(ctypes.Structure):
    _fields_ = [("bi_sector", ctypes.c_uint64), ("bi_size", ctypes.c_uint),
                ("bi_idx", ctypes.c_uint), ("bi_bvec_done", ctypes.c_uint)]

    def as_tuple(self) -> Tuple[int, int, int]:
        return (self.bi_size, self.bi_idx, self.bi_bvec_done)


class SgRequest(ctypes.Structure):
    _fields_ = [("src", ctypes.POINTER(BioVec)), ("dst", ctypes.POINTER(BioVec)),
                ("srcIter", ctypes.POINTER(BvecIter)), ("dstIter", ctypes.POINTER(BvecIter)),
                ("ret", ctypes.c_int)]


class ChunkRequest(ctypes.Structure):
    """struct lz4e_chunk_request (include/lz4e.h)."""
    _fields_ = [("src", ctypes.POINTER(BioVec)), ("srcIter", ctypes.POINTER(BvecIter)),
                ("data", ctypes.c_void_p), ("frame", ctypes.c_void_p), ("frame_cap", ctypes.c_int),
                ("comp_size", ctypes.c_int), ("status", ctypes.c_int)]


class ChunkStats(ctypes.Structure):
    """struct lz4e_chunk_stats (include/lz4e.h)."""
    _fields_ = [("reqs_total", ctypes.c_uint64), ("reqs_failed", ctypes.c_uint64),
                ("vec_count", ctypes.c_uint64), ("data_in_bytes", ctypes.c_uint64),
                ("frame_bytes", ctypes.c_uint64)]


EIO, ENOSPC = 5, 28

_lib: Optional[ctypes.CDLL] = None


def lib() -> ctypes.CDLL:
    """Load liblz4e_amd.so (raises ImportError if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} missing: build it with `make -C lz4-sgori_amd` "
                          "(or __graft_entry__.build())")
    # One HIP runtime per process: torch wheels bundle their own
    # libamdhip64.so.7 (same soname as /opt/rocm's).  Whichever loads first is
    # shared by both, and torch only initialises on its own copy, so when
    # torch is installed it is imported before the library is loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    P, U32, I32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    L.LZ4E_compress_default.argtypes = [ctypes.POINTER(BioVec), ctypes.POINTER(BioVec),
                                        ctypes.POINTER(BvecIter), ctypes.POINTER(BvecIter), P]
    L.LZ4E_compress_default.restype = I32
    L.LZ4E_decompress_safe.argtypes = [P, P, I32, I32]
    L.LZ4E_decompress_safe.restype = I32
    L.lz4e_sg_table_type.argtypes = [ctypes.POINTER(BioVec), ctypes.POINTER(BvecIter)]
    L.lz4e_sg_table_type.restype = I32
    L.lz4e_last_error.argtypes = []
    L.lz4e_last_error.restype = ctypes.c_char_p
    L.lz4e_gpu_available.argtypes = []
    L.lz4e_gpu_available.restype = I32
    L.lz4e_compress_sg_batch.argtypes = [ctypes.POINTER(SgRequest), I32]
    L.lz4e_compress_sg_batch.restype = I32
    L.lz4e_decompress_batch.argtypes = [P, P, P, P, P, I32]
    L.lz4e_decompress_batch.restype = I32
    L.lz4e_compress_batch_dev.argtypes = [P, P, P, P, P, P, P, P, P, U32, U32, P]
    L.lz4e_compress_batch_dev.restype = I32
    L.lz4e_decompress_batch_dev.argtypes = [P, P, P, P, P, P, P, U32, P]
    L.lz4e_decompress_batch_dev.restype = I32
    L.lz4e_decompress_batch_dev2.argtypes = [P, P, P, P, P, P, P, U32, U32, P]
    L.lz4e_decompress_batch_dev2.restype = I32
    L.lz4e_chunk_write_batch.argtypes = [ctypes.POINTER(ChunkRequest), I32, ctypes.POINTER(ChunkStats)]
    L.lz4e_chunk_write_batch.restype = I32
    L.lz4e_decompress_safe_sg.argtypes = [P, ctypes.POINTER(BioVec), ctypes.POINTER(BvecIter), I32]
    L.lz4e_decompress_safe_sg.restype = I32
    L.lz4e_decompress_sg_batch.argtypes = [P, P, P, P, P, I32]
    L.lz4e_decompress_sg_batch.restype = I32
    L.LZ4E_compress_usingDict.argtypes = [ctypes.POINTER(BioVec), ctypes.POINTER(BioVec),
                                          ctypes.POINTER(BvecIter), ctypes.POINTER(BvecIter), P, P, I32]
    L.LZ4E_compress_usingDict.restype = I32
    L.LZ4E_decompress_safe_usingDict.argtypes = [P, P, I32, I32, P, I32]
    L.LZ4E_decompress_safe_usingDict.restype = I32
    L.lz4e_compress_sg_batch_dict.argtypes = [ctypes.POINTER(SgRequest), I32, P, P]
    L.lz4e_compress_sg_batch_dict.restype = I32
    L.lz4e_decompress_batch_dict.argtypes = [P, P, P, P, P, P, P, I32]
    L.lz4e_decompress_batch_dict.restype = I32
    L.lz4e_compress_batch_dev_dict.argtypes = [P, P, P, P, P, P, P, P, P, U32, U32, P, P]
    L.lz4e_compress_batch_dev_dict.restype = I32
    L.lz4e_decompress_batch_dev_dict.argtypes = [P, P, P, P, P, P, P, U32, U32, P, P]
    L.lz4e_decompress_batch_dev_dict.restype = I32
    # (LZ4E_LIB may name an older build for an A/B run, tools/e2e.py: it
    # lacks these three, and using them then fails with AttributeError)
    if hasattr(L, "lz4e_register_host_memory"):
        L.lz4e_register_host_memory.argtypes = [P, ctypes.c_size_t]
        L.lz4e_register_host_memory.restype = I32
        L.lz4e_unregister_host_memory.argtypes = [P]
        L.lz4e_unregister_host_memory.restype = I32
        L.lz4e_debug_chunk_zero_copy_requests.argtypes = []
        L.lz4e_debug_chunk_zero_copy_requests.restype = ctypes.c_uint64
    if hasattr(L, "lz4e_pack_batch_dev"):
        L.lz4e_pack_batch_dev.argtypes = [P] * 7 + [ctypes.c_uint64, U32, P, P, P, U32, U32, P]
        L.lz4e_pack_batch_dev.restype = I32
        L.lz4e_unpack_batch_dev.argtypes = [P] * 8 + [U32, U32, P]
        L.lz4e_unpack_batch_dev.restype = I32
    if hasattr(L, "lz4e_crc32c_batch_dev"):
        L.lz4e_crc32c_batch_dev.argtypes = [P] * 4 + [U32, U32, P]
        L.lz4e_crc32c_batch_dev.restype = I32
        L.lz4e_pack_crc_batch_dev.argtypes = [P] * 7 + [U32, U32, P]
        L.lz4e_pack_crc_batch_dev.restype = I32
        L.lz4e_unpack_verified_batch_dev.argtypes = [P] * 9 + [U32, U32, P]
        L.lz4e_unpack_verified_batch_dev.restype = I32
    if hasattr(L, "lz4e_decompress_partial_batch_dev"):
        L.LZ4E_decompress_safe_partial.argtypes = [P, P, I32, I32, I32]
        L.LZ4E_decompress_safe_partial.restype = I32
        L.lz4e_decompress_partial_batch.argtypes = [P, P, P, P, P, I32]
        L.lz4e_decompress_partial_batch.restype = I32
        L.lz4e_decompress_partial_batch_dev.argtypes = [P, P, P, P, P, P, P, U32, U32, P]
        L.lz4e_decompress_partial_batch_dev.restype = I32
        L.lz4e_debug_decompress_partial.argtypes = [P, P, P, P, P, P, P, U32, U32, P, U32]
        L.lz4e_debug_decompress_partial.restype = I32
        L.lz4e_unpack_range_batch_dev.argtypes = [P] * 4 + [U32] + [P] * 6 + [U32, U32, P]
        L.lz4e_unpack_range_batch_dev.restype = I32
    if hasattr(L, "lz4e_unpack_range_verified_batch_dev"):
        L.lz4e_unpack_range_verified_batch_dev.argtypes = [P] * 5 + [U32] + [P] * 6 + [U32, U32, U32, P]
        L.lz4e_unpack_range_verified_batch_dev.restype = I32
    _lib = L
    return L


def last_error() -> str:
    return lib().lz4e_last_error().decode()


def gpu_available() -> bool:
    return bool(lib().lz4e_gpu_available())


def _require_gpu() -> None:
    if not gpu_available():
        raise GpuUnavailable(last_error() or "lz4e: no usable gfx950 device")


# ---------------------------------------------------------------------------
# Scatter-gather buffers (userspace bio_vec lists backed by page-aligned memory)
# ---------------------------------------------------------------------------

@dataclass
class SgList:
    """A bio_vec list over page-aligned host memory plus an iterator into it."""
    backing: np.ndarray
    bvecs: ctypes.Array
    it: BvecIter
    seg_addr: List[int] = field(default_factory=list)

    @property
    def nseg(self) -> int:
        return len(self.bvecs)

    def read(self) -> bytes:
        """Bytes covered by the iterator (gathered)."""
        out = bytearray()
        size, idx, done = self.it.bi_size, self.it.bi_idx, self.it.bi_bvec_done
        while size:
            b = self.bvecs[idx]
            take = min(b.bv_len - done, size)
            out += ctypes.string_at(b.bv_page + b.bv_offset + done, take)
            size -= take
            done = 0
            idx += 1
        return bytes(out)

    def read_prefix(self, n: int) -> bytes:
        """First n bytes from the ORIGINAL start (segment order)."""
        out = bytearray()
        for b in self.bvecs:
            if len(out) >= n:
                break
            out += ctypes.string_at(b.bv_page + b.bv_offset, b.bv_len)
        return bytes(out[:n])


EINVAL, ENOENT = 22, 2


def register_host_memory(addr: int, nbytes: int) -> int:
    """lz4e_register_host_memory: 0, -22 (bad argument) or -1 (no GPU / HIP refused)."""
    return lib().lz4e_register_host_memory(addr, nbytes)


def unregister_host_memory(addr: int) -> int:
    """lz4e_unregister_host_memory: 0, -2 (not a registration's base) or -1."""
    return lib().lz4e_unregister_host_memory(addr)


def zero_copy_requests() -> int:
    """lz4e_debug_chunk_zero_copy_requests: chunk requests whose input the device gathered so far."""
    return int(lib().lz4e_debug_chunk_zero_copy_requests())


class HostArena:
    """A page-aligned host buffer, registered with the library while the
    ``with`` block runs (lz4e_register_host_memory on entry,
    lz4e_unregister_host_memory on exit) and handed out piecewise by
    :meth:`alloc`.  The memory exists from construction on, so the same
    buffers can be used before, inside and after the registration."""

    def __init__(self, nbytes: int):
        self.size = max(1, -(-int(nbytes) // PAGE_SIZE)) * PAGE_SIZE
        self._raw = np.zeros(self.size + PAGE_SIZE, dtype=np.uint8)
        start = -self._raw.ctypes.data % PAGE_SIZE
        self.buf = self._raw[start:start + self.size]
        self.base = self.buf.ctypes.data
        self.used = 0
        self.registered = False

    def alloc(self, nbytes: int, align: int = 16) -> np.ndarray:
        """The next ``nbytes`` of the arena at a multiple of ``align`` (a uint8 view)."""
        at = -(-(self.base + self.used) // align) * align - self.base
        if at + nbytes > self.size:
            raise MemoryError(f"HostArena: {nbytes} bytes asked, {self.size - at} left")
        self.used = at + nbytes
        return self.buf[at:at + nbytes]

    def reset(self) -> None:
        self.used = 0

    def __enter__(self) -> "HostArena":
        r = register_host_memory(self.base, self.size)
        if r == -EINVAL:
            raise ValueError("lz4e_register_host_memory: " + last_error())
        if r != 0:
            raise GpuUnavailable(last_error() or "lz4e_register_host_memory failed")
        self.registered = True
        return self

    def __exit__(self, *exc) -> None:
        self.registered = False
        r = unregister_host_memory(self.base)
        if r != 0 and exc[0] is None:
            raise RuntimeError(f"lz4e_unregister_host_memory: {r} {last_error()}")


def make_sg(data: bytes, segments: Sequence[int], offsets: Optional[Sequence[int]] = None,
            start_done: int = 0, capacity: Optional[int] = None, shuffle_seed: Optional[int] = None,
            fill: int = 0, arena: Optional[HostArena] = None) -> SgList:
    """Build a bio_vec list whose segments have the given lengths.

    Segment i lives at in-page offset offsets[i] (default 0) on its own run of
    pages (multi-page when offset + len > 4096); with ``shuffle_seed`` the page
    runs are placed in a shuffled order, so consecutive segments are not
    adjacent in memory.  ``data`` is written across the segments starting at
    byte ``start_done`` of segment 0; the iterator covers ``len(data)`` bytes
    (or ``capacity`` bytes for a destination list).  With ``arena`` the pages
    come out of that :class:`HostArena` instead of fresh numpy memory.
    """
    segments = list(segments)
    offsets = list(offsets) if offsets is not None else [0] * len(segments)
    runs = [max(1, -(-(o + ln) // PAGE_SIZE)) for o, ln in zip(offsets, segments)]
    order = list(range(len(segments)))
    if shuffle_seed is not None:
        rng = np.random.default_rng(shuffle_seed)
        rng.shuffle(order)
    start_page = [0] * len(segments)
    p = 0
    for i in order:
        start_page[i] = p
        p += runs[i]
    if arena is not None:
        raw = arena.alloc(max(1, p) * PAGE_SIZE, PAGE_SIZE)
        raw[:] = fill
    else:
        raw = np.full((p + 1) * PAGE_SIZE, fill, dtype=np.uint8)
    base = raw.ctypes.data
    aligned = (base + PAGE_SIZE - 1) // PAGE_SIZE * PAGE_SIZE
    bvecs = (BioVec * max(1, len(segments)))()
    addrs = []
    for i, (o, ln) in enumerate(zip(offsets, segments)):
        page = aligned + start_page[i] * PAGE_SIZE
        bvecs[i].bv_page = page
        bvecs[i].bv_len = ln
        bvecs[i].bv_offset = o
        addrs.append(page + o)
    # write data
    mv = memoryview(data)
    pos = 0
    for i, ln in enumerate(segments):
        lo = start_done if i == 0 else 0
        take = min(ln - lo, len(data) - pos)
        if take <= 0:
            break
        ctypes.memmove(addrs[i] + lo, bytes(mv[pos:pos + take]), take)
        pos += take
    size = capacity if capacity is not None else len(data)
    it = BvecIter(0, size, 0, start_done)
    return SgList(raw, bvecs, it, addrs)


def table_type(sg: SgList) -> int:
    """lz4e_sg_table_type: 1/3/7, or 0 for more than BIO_MAX_VECS segments."""
    return lib().lz4e_sg_table_type(sg.bvecs, ctypes.byref(sg.it))


# ---------------------------------------------------------------------------
# Reference entry points
# ---------------------------------------------------------------------------

def compress_default(src: SgList, dst: SgList, wrkmem: Optional[ctypes.Array] = None) -> int:
    """LZ4E_compress_default(src->bvecs, dst->bvecs, &src.it, &dst.it, wrkmem)."""
    _require_gpu()
    if wrkmem is None:
        wrkmem = (ctypes.c_uint8 * LZ4E_MEM_COMPRESS)()
    return lib().LZ4E_compress_default(src.bvecs, dst.bvecs, ctypes.byref(src.it),
                                       ctypes.byref(dst.it), wrkmem)


def decompress_safe(source: bytes, max_decompressed_size: int,
                    compressed_size: Optional[int] = None) -> Tuple[int, bytes]:
    """LZ4E_decompress_safe; returns (ret, dest[:max(ret, 0)])."""
    _require_gpu()
    csize = len(source) if compressed_size is None else compressed_size
    dst = ctypes.create_string_buffer(max(max_decompressed_size, 0) + 1)
    src = ctypes.create_string_buffer(bytes(source), max(len(source), 1))
    r = lib().LZ4E_decompress_safe(src, dst, csize, max_decompressed_size)
    return r, dst.raw[:max(r, 0)]


def decompress_safe_partial(source: bytes, target_output_size: int, dst_capacity: Optional[int] = None,
                            compressed_size: Optional[int] = None) -> Tuple[int, bytes]:
    """LZ4E_decompress_safe_partial into a buffer of dst_capacity bytes
    (default: the target); returns (ret, dest[:max(ret, 0)])."""
    _require_gpu()
    cap = target_output_size if dst_capacity is None else dst_capacity
    csize = len(source) if compressed_size is None else compressed_size
    dst = ctypes.create_string_buffer(max(cap, 0) + 1)
    src = ctypes.create_string_buffer(bytes(source), max(len(source), 1))
    r = lib().LZ4E_decompress_safe_partial(src, dst, csize, target_output_size, cap)
    return r, dst.raw[:max(r, 0)]


def compress_using_dict(src: SgList, dst: SgList, dictionary: bytes,
                        wrkmem: Optional[ctypes.Array] = None) -> int:
    """LZ4E_compress_usingDict (dictionary mode, include/lz4e.h)."""
    _require_gpu()
    if wrkmem is None:
        wrkmem = (ctypes.c_uint8 * LZ4E_MEM_COMPRESS)()
    d = ctypes.create_string_buffer(bytes(dictionary), max(len(dictionary), 1))
    return lib().LZ4E_compress_usingDict(src.bvecs, dst.bvecs, ctypes.byref(src.it),
                                         ctypes.byref(dst.it), wrkmem, d, len(dictionary))


def decompress_safe_using_dict(source: bytes, max_decompressed_size: int, dictionary: bytes,
                               compressed_size: Optional[int] = None) -> Tuple[int, bytes]:
    """LZ4E_decompress_safe_usingDict; returns (ret, dest[:max(ret, 0)])."""
    _require_gpu()
    csize = len(source) if compressed_size is None else compressed_size
    dst = ctypes.create_string_buffer(max(max_decompressed_size, 0) + 1)
    src = ctypes.create_string_buffer(bytes(source), max(len(source), 1))
    d = ctypes.create_string_buffer(bytes(dictionary), max(len(dictionary), 1))
    r = lib().LZ4E_decompress_safe_usingDict(src, dst, csize, max_decompressed_size, d,
                                             len(dictionary))
    return r, dst.raw[:max(r, 0)]


def decompress_batch_dict(frames: Sequence[bytes], caps: Sequence[int],
                          dicts: Sequence[bytes]) -> List[Tuple[int, bytes]]:
    """lz4e_decompress_batch_dict over host frames; returns (ret, bytes) per frame."""
    _require_gpu()
    n = len(frames)
    srcs = [ctypes.create_string_buffer(bytes(f), max(len(f), 1)) for f in frames]
    dsts = [ctypes.create_string_buffer(max(c, 0) + 1) for c in caps]
    dcs = [ctypes.create_string_buffer(bytes(d), max(len(d), 1)) for d in dicts]
    sp = (ctypes.c_void_p * n)(*[ctypes.addressof(s) for s in srcs])
    dp = (ctypes.c_void_p * n)(*[ctypes.addressof(d) for d in dsts])
    kp = (ctypes.c_void_p * n)(*[ctypes.addressof(d) for d in dcs])
    ks = (ctypes.c_int * n)(*[len(d) for d in dicts])
    cs = (ctypes.c_int * n)(*[len(f) for f in frames])
    cp = (ctypes.c_int * n)(*caps)
    rt = (ctypes.c_int * n)()
    if lib().lz4e_decompress_batch_dict(sp, cs, dp, cp, kp, ks, rt, n) < 0:
        raise GpuUnavailable(last_error())
    return [(rt[i], dsts[i].raw[:max(rt[i], 0)]) for i in range(n)]


def compress_sg_batch_dict(pairs: Sequence[Tuple[SgList, SgList]],
                           dicts: Sequence[bytes]) -> List[int]:
    """lz4e_compress_sg_batch_dict; returns each ret."""
    _require_gpu()
    n = len(pairs)
    reqs = (SgRequest * n)()
    for i, (s, d) in enumerate(pairs):
        reqs[i].src = s.bvecs
        reqs[i].dst = d.bvecs
        reqs[i].srcIter = ctypes.pointer(s.it)
        reqs[i].dstIter = ctypes.pointer(d.it)
    dcs = [ctypes.create_string_buffer(bytes(d), max(len(d), 1)) for d in dicts]
    kp = (ctypes.c_void_p * n)(*[ctypes.addressof(d) for d in dcs])
    ks = (ctypes.c_int * n)(*[len(d) for d in dicts])
    r = lib().lz4e_compress_sg_batch_dict(reqs, n, kp, ks)
    if r < 0:
        raise GpuUnavailable(last_error())
    return [reqs[i].ret for i in range(n)]


def compress_sg_batch(pairs: Sequence[Tuple[SgList, SgList]]) -> List[int]:
    """lz4e_compress_sg_batch over (src, dst) SG pairs; returns each ret."""
    _require_gpu()
    reqs = (SgRequest * len(pairs))()
    for i, (s, d) in enumerate(pairs):
        reqs[i].src = s.bvecs
        reqs[i].dst = d.bvecs
        reqs[i].srcIter = ctypes.pointer(s.it)
        reqs[i].dstIter = ctypes.pointer(d.it)
    r = lib().lz4e_compress_sg_batch(reqs, len(pairs))
    if r < 0:
        raise GpuUnavailable(last_error())
    return [reqs[i].ret for i in range(len(pairs))]


def decompress_batch(frames: Sequence[bytes], caps: Sequence[int]) -> List[Tuple[int, bytes]]:
    """lz4e_decompress_batch over host frames; returns (ret, bytes) per frame."""
    _require_gpu()
    n = len(frames)
    srcs = [ctypes.create_string_buffer(bytes(f), max(len(f), 1)) for f in frames]
    dsts = [ctypes.create_string_buffer(max(c, 0) + 1) for c in caps]
    sp = (ctypes.c_void_p * n)(*[ctypes.addressof(s) for s in srcs])
    dp = (ctypes.c_void_p * n)(*[ctypes.addressof(d) for d in dsts])
    cs = (ctypes.c_int * n)(*[len(f) for f in frames])
    cp = (ctypes.c_int * n)(*caps)
    rt = (ctypes.c_int * n)()
    if lib().lz4e_decompress_batch(sp, cs, dp, cp, rt, n) < 0:
        raise GpuUnavailable(last_error())
    return [(rt[i], dsts[i].raw[:max(rt[i], 0)]) for i in range(n)]


def decompress_partial_batch(frames: Sequence[bytes], targets: Sequence[int]) -> List[Tuple[int, bytes]]:
    """lz4e_decompress_partial_batch over host frames; returns (ret, bytes) per frame."""
    _require_gpu()
    n = len(frames)
    srcs = [ctypes.create_string_buffer(bytes(f), max(len(f), 1)) for f in frames]
    dsts = [ctypes.create_string_buffer(max(c, 0) + 1) for c in targets]
    sp = (ctypes.c_void_p * n)(*[ctypes.addressof(s) for s in srcs])
    dp = (ctypes.c_void_p * n)(*[ctypes.addressof(d) for d in dsts])
    cs = (ctypes.c_int * n)(*[len(f) for f in frames])
    cp = (ctypes.c_int * n)(*targets)
    rt = (ctypes.c_int * n)()
    if lib().lz4e_decompress_partial_batch(sp, cs, dp, cp, rt, n) < 0:
        raise GpuUnavailable(last_error())
    return [(rt[i], dsts[i].raw[:max(rt[i], 0)]) for i in range(n)]


def decompress_safe_sg(source: bytes, dst: SgList, compressed_size: Optional[int] = None) -> int:
    """lz4e_decompress_safe_sg: decode into dst's segments from dst.it (capacity dst.it.bi_size)."""
    _require_gpu()
    csize = len(source) if compressed_size is None else compressed_size
    src = ctypes.create_string_buffer(bytes(source), max(len(source), 1))
    return lib().lz4e_decompress_safe_sg(src, dst.bvecs, ctypes.byref(dst.it), csize)


def decompress_sg_batch(frames: Sequence[bytes], dsts: Sequence[SgList]) -> List[int]:
    """lz4e_decompress_sg_batch; returns ret per frame (dst iterators advance on success)."""
    _require_gpu()
    n = len(frames)
    srcs = [ctypes.create_string_buffer(bytes(f), max(len(f), 1)) for f in frames]
    sp = (ctypes.c_void_p * n)(*[ctypes.addressof(s) for s in srcs])
    cs = (ctypes.c_int * n)(*[len(f) for f in frames])
    dp = (ctypes.c_void_p * n)(*[ctypes.addressof(d.bvecs) for d in dsts])
    ip = (ctypes.c_void_p * n)(*[ctypes.addressof(d.it) for d in dsts])
    rt = (ctypes.c_int * n)()
    if lib().lz4e_decompress_sg_batch(sp, cs, dp, ip, rt, n) < 0:
        raise GpuUnavailable(last_error())
    return list(rt)


@dataclass
class GuardReport:
    """What chunk_write_batch(guard=G) saw around its buffers after the call:
    ``intact`` -- every guard byte on both sides of every data and frame
    buffer still holds the guard pattern; ``bad`` -- indices of the requests
    with a damaged guard; ``untouched[i]`` -- request i's data and frame
    buffers still hold their pre-call fill in every byte."""
    intact: bool
    bad: List[int]
    untouched: List[bool]


_GUARD_BYTE, _FILL_BYTE = 0xA5, 0x5A


def chunk_write_batch(srcs: Sequence[SgList], want_frames: bool = False,
                      stats: Optional[ChunkStats] = None, arena=None,
                      frame_caps: Optional[Sequence[Optional[int]]] = None, guard: int = 0):
    """lz4e_chunk_write_batch over WRITE bios given as SG lists.

    Returns (good, [(status, comp_size, data bytes, frame bytes or None)]),
    the chunk layer's result per request (lz4e_bdev/lz4e_req.c:144-213).

    ``arena``: the data and frame buffers come out of that HostArena (at byte
    granularity, so at every alignment) instead of fresh memory; a list
    gives each request its own choice: a HostArena, None (fresh memory), or a
    pair (arena of the data buffer, arena of the frame buffer).
    ``frame_caps``: per-request frame capacity (None: LZ4E_COMPRESSBOUND);
    giving it asks for frames like ``want_frames``.  ``guard`` > 0: every
    buffer is pre-filled with a pattern and sits between two runs of
    ``guard`` bytes of another, and a :class:`GuardReport` is returned as a
    third value."""
    _require_gpu()
    n = len(srcs)
    reqs = (ChunkRequest * max(1, n))()
    want_frames = want_frames or frame_caps is not None

    def arenas_of(i):
        a = arena[i] if isinstance(arena, list) else arena
        return a if isinstance(a, tuple) else (a, a)

    def buffer(size, arena):
        """(keep-alive object, whole array incl. guards or None, address of the payload)"""
        if arena is None and guard == 0:
            b = ctypes.create_string_buffer(max(1, size))
            return b, None, ctypes.addressof(b)
        total = max(1, size + 2 * guard)
        a = arena.alloc(total, 1) if arena is not None else np.empty(total, np.uint8)
        a[:] = _GUARD_BYTE if guard else 0
        if guard:
            a[guard:guard + size] = _FILL_BYTE
        return a, a, a.ctypes.data + guard

    datas, frames, caps = [], [], []
    for i, s in enumerate(srcs):
        size = s.it.bi_size
        cap = compress_bound(size)
        if frame_caps is not None and frame_caps[i] is not None:
            cap = int(frame_caps[i])
        d_arena, f_arena = arenas_of(i)
        d = buffer(size, d_arena)
        f = buffer(cap, f_arena) if want_frames else None
        datas.append(d)
        frames.append(f)
        caps.append(cap)
        reqs[i].src = s.bvecs
        reqs[i].srcIter = ctypes.pointer(s.it)
        reqs[i].data = d[2]
        reqs[i].frame = f[2] if f is not None else None
        reqs[i].frame_cap = cap if f is not None else 0
    good = lib().lz4e_chunk_write_batch(reqs, n, ctypes.byref(stats) if stats is not None else None)
    if good < 0:
        raise GpuUnavailable(last_error())

    def payload(b, size, k):
        return ctypes.string_at(b[2], min(k, size)) if size else b""

    out = []
    for i, s in enumerate(srcs):
        r = reqs[i]
        fr = payload(frames[i], caps[i], r.comp_size) if frames[i] is not None and r.status == 0 else None
        out.append((r.status, r.comp_size,
                    payload(datas[i], s.it.bi_size, s.it.bi_size) if r.status == 0 else None, fr))
    if not guard:
        return good, out
    bad, untouched = [], []
    for i, s in enumerate(srcs):
        ok, clean = True, True
        for b, size in ((datas[i], s.it.bi_size), (frames[i], caps[i])):
            if b is None:
                continue
            a = b[1]
            ok &= bool((a[:guard] == _GUARD_BYTE).all() and (a[guard + size:] == _GUARD_BYTE).all())
            clean &= bool((a[guard:guard + size] == _FILL_BYTE).all())
        if not ok:
            bad.append(i)
        untouched.append(clean)
    return good, out, GuardReport(not bad, bad, untouched)


# ---------------------------------------------------------------------------
# Device-resident batches (torch tensors on the HIP device)
# ---------------------------------------------------------------------------

def _ptr(t) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _check_dev(n: int, **tensors) -> None:
    """The kernels read raw pointers: every tensor must be contiguous, on one
    HIP device, of the element type the C ABI expects, and (descriptors) hold
    one entry per block -- a wrong dtype would be read as another width."""
    import torch
    want = {"src": torch.uint8, "dst": torch.uint8, "table_type": torch.uint8,
            "src_off": torch.int64, "dst_off": torch.int64, "src_len": torch.int32,
            "dst_cap": torch.int32, "ret": torch.int32, "aux": torch.int32,
            "frames": torch.uint8, "fr_off": torch.int64, "packed": torch.uint8,
            "pk_off": torch.int64, "pk_len": torch.int32, "pk_kind": torch.uint8,
            "pk_crc": torch.int32, "data": torch.uint8, "off": torch.int64, "len": torch.int32,
            "crc": torch.int32, "sel": torch.int32, "lo": torch.int32}
    per_block = {"src_off": 1, "dst_off": 1, "src_len": 1, "dst_cap": 1, "ret": 1,
                 "table_type": 1, "aux": 2, "fr_off": 1, "pk_len": 1, "pk_kind": 1,
                 "pk_crc": 1, "off": 1, "len": 1, "crc": 1}
    dev = None
    for name, t in tensors.items():
        if t is None:
            continue
        if t.dtype != want[name]:
            raise TypeError(f"{name}: dtype {t.dtype}, expected {want[name]}")
        if not t.is_cuda:
            raise ValueError(f"{name}: not a device tensor")
        if not t.is_contiguous():
            raise ValueError(f"{name}: not contiguous")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"{name}: on {t.device}, other tensors on {dev}")
        if name in per_block and t.numel() < per_block[name] * n:
            raise ValueError(f"{name}: {t.numel()} entries for {n} blocks")
        if name == "pk_off" and t.numel() < n + 1:
            raise ValueError(f"pk_off: {t.numel()} entries for {n} blocks (needs {n + 1})")


def compress_batch_dev(src, src_off, src_len, table_type_, dst, dst_off, dst_cap, ret,
                       aux=None, max_len: Optional[int] = None, stream=None) -> None:
    """lz4e_compress_batch_dev on torch tensors (uint8 / int64 / int32 views).

    src/dst: uint8; src_off/dst_off: int64; src_len/dst_cap/ret: int32;
    table_type_: uint8; aux: int32 [2*nblocks] or None.  Launch only (async on
    ``stream``, default: torch's current stream).
    """
    import torch  # local: the package itself does not need torch
    n = int(src_len.numel())
    _check_dev(n, src=src, src_off=src_off, src_len=src_len, table_type=table_type_, dst=dst,
               dst_off=dst_off, dst_cap=dst_cap, ret=ret, aux=aux)
    if max_len is None:
        max_len = int(src_len.max().item()) if n else 0
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    r = lib().lz4e_compress_batch_dev(_ptr(src), _ptr(src_off), _ptr(src_len), _ptr(table_type_),
                                      _ptr(dst), _ptr(dst_off), _ptr(dst_cap), _ptr(ret), _ptr(aux),
                                      n, int(max_len), stream)
    if r != 0:
        raise RuntimeError("lz4e_compress_batch_dev: " + last_error())


def decompress_batch_dev(src, src_off, src_len, dst, dst_off, dst_cap, ret, stream=None,
                         max_cap: Optional[int] = None) -> None:
    """lz4e_decompress_batch_dev2 on torch tensors (launch only).

    ``max_cap`` bounds dst_cap (default: read from it, which synchronises);
    16 KiB and more selects the pipelined 4-wave decoder, smaller blocks
    decode on one wave each."""
    import torch
    n = int(src_len.numel())
    if max_cap is None:
        max_cap = int(dst_cap.max().item()) if n else 0
    # decompress descriptors: frame offsets int64, frame sizes / capacities / ret int32
    _check_dev(n, src=src, src_off=src_off, src_len=src_len, dst=dst, dst_off=dst_off,
               dst_cap=dst_cap, ret=ret)
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    r = lib().lz4e_decompress_batch_dev2(_ptr(src), _ptr(src_off), _ptr(src_len), _ptr(dst),
                                         _ptr(dst_off), _ptr(dst_cap), _ptr(ret), n,
                                         max(0, int(max_cap)), stream)
    if r != 0:
        raise RuntimeError("lz4e_decompress_batch_dev2: " + last_error())


def decompress_partial_batch_dev(src, src_off, src_len, dst, dst_off, dst_cap, ret, stream=None,
                                 max_cap: Optional[int] = None, mode: Optional[int] = None) -> None:
    """lz4e_decompress_partial_batch_dev on torch tensors (launch only):
    dst_cap[i] is block i's target size and capacity.  ``mode`` forces a
    decoder through the diagnostic entry (1 one-wave, 2 pipelined, 6 LDS form;
    7, the group decoder, has no partial form and runs as 1)."""
    import torch
    n = int(src_len.numel())
    if max_cap is None:
        max_cap = int(dst_cap.max().item()) if n else 0
    _check_dev(n, src=src, src_off=src_off, src_len=src_len, dst=dst, dst_off=dst_off,
               dst_cap=dst_cap, ret=ret)
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    args = (_ptr(src), _ptr(src_off), _ptr(src_len), _ptr(dst), _ptr(dst_off), _ptr(dst_cap), _ptr(ret), n,
            max(0, int(max_cap)), stream)
    if mode is None:
        r = lib().lz4e_decompress_partial_batch_dev(*args)
    else:
        r = lib().lz4e_debug_decompress_partial(*args, int(mode))
    if r != 0:
        raise RuntimeError("lz4e_decompress_partial_batch_dev: " + last_error())


PACK_FRAME, PACK_RAW = 0, 1


def pack_batch_dev(frames, fr_off, ret, src, src_off, src_len, packed, pk_off, pk_len, pk_kind,
                   align: int = 1, packed_cap: Optional[int] = None, max_len: Optional[int] = None,
                   stream=None) -> None:
    """lz4e_pack_batch_dev on torch tensors (launch only).

    frames / fr_off / ret and src / src_off / src_len are the dst / dst_off /
    ret and input tensors of the compress_batch_dev call before it.  packed:
    uint8 (``packed_cap`` defaults to its size); pk_off: int64 [nblocks + 1];
    pk_len: int32; pk_kind: uint8.  ``max_len`` bounds src_len (default: read
    from it, which synchronises).  A bad ``align`` raises ValueError."""
    import torch
    n = int(src_len.numel())
    _check_dev(n, frames=frames, fr_off=fr_off, ret=ret, src=src, src_off=src_off, src_len=src_len,
               packed=packed, pk_off=pk_off, pk_len=pk_len, pk_kind=pk_kind)
    if packed_cap is None:
        packed_cap = int(packed.numel())
    if packed_cap < 0 or packed_cap > packed.numel():
        raise ValueError(f"packed_cap {packed_cap} for a tensor of {packed.numel()} bytes")
    if max_len is None:
        max_len = int(src_len.max().item()) if n else 0
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    r = lib().lz4e_pack_batch_dev(_ptr(frames), _ptr(fr_off), _ptr(ret), _ptr(src), _ptr(src_off),
                                  _ptr(src_len), _ptr(packed), int(packed_cap), int(align), _ptr(pk_off),
                                  _ptr(pk_len), _ptr(pk_kind), n, int(max_len), stream)
    if r == -22:
        raise ValueError("lz4e_pack_batch_dev: " + last_error())
    if r != 0:
        raise RuntimeError("lz4e_pack_batch_dev: " + last_error())


def unpack_batch_dev(packed, pk_off, pk_len, pk_kind, dst, dst_off, dst_cap, ret, stream=None,
                     max_cap: Optional[int] = None) -> None:
    """lz4e_unpack_batch_dev on torch tensors (launch only).  ``max_cap``
    bounds dst_cap and selects the decoder as in decompress_batch_dev
    (default: read from it, which synchronises)."""
    import torch
    n = int(pk_len.numel())
    _check_dev(n, packed=packed, pk_off=pk_off, pk_len=pk_len, pk_kind=pk_kind, dst=dst, dst_off=dst_off,
               dst_cap=dst_cap, ret=ret)
    if max_cap is None:
        max_cap = int(dst_cap.max().item()) if n else 0
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    r = lib().lz4e_unpack_batch_dev(_ptr(packed), _ptr(pk_off), _ptr(pk_len), _ptr(pk_kind), _ptr(dst),
                                    _ptr(dst_off), _ptr(dst_cap), _ptr(ret), n, max(0, int(max_cap)), stream)
    if r != 0:
        raise RuntimeError("lz4e_unpack_batch_dev: " + last_error())


def unpack_range_batch_dev(packed, pk_off, pk_len, pk_kind, sel, lo, len_, dst, dst_off, ret, max_end: int,
                           stream=None) -> None:
    """lz4e_unpack_range_batch_dev on torch tensors (launch only): request j
    reads bytes [lo[j], lo[j] + len_[j]) of entry sel[j] (``sel`` None: entry
    j) into dst + dst_off[j].  sel / lo / len_ / ret: int32 tensors, one
    entry per request (the C ABI reads sel as uint32: an entry number of
    2^31 or more is its int32 bit pattern); ``max_end`` bounds lo + len_."""
    import torch
    n = int(pk_len.numel())
    nreq = int(lo.numel())
    # one call: every tensor on one device; the index has n entries, the request arrays nreq
    _check_dev(0, packed=packed, pk_off=pk_off, pk_len=pk_len, pk_kind=pk_kind, sel=sel, lo=lo, len=len_, dst=dst,
               dst_off=dst_off, ret=ret)
    for name, t, need in (("pk_off", pk_off, n + 1), ("pk_len", pk_len, n), ("pk_kind", pk_kind, n), ("sel", sel, nreq),
                          ("lo", lo, nreq), ("len_", len_, nreq), ("dst_off", dst_off, nreq), ("ret", ret, nreq)):
        if t is not None and t.numel() < need:
            raise ValueError(f"{name}: {t.numel()} entries, needs {need}")
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    r = lib().lz4e_unpack_range_batch_dev(_ptr(packed), _ptr(pk_off), _ptr(pk_len), _ptr(pk_kind), n, _ptr(sel),
                                          _ptr(lo), _ptr(len_), _ptr(dst), _ptr(dst_off), _ptr(ret), nreq,
                                          max(0, int(max_end)), stream)
    if r != 0:
        raise RuntimeError("lz4e_unpack_range_batch_dev: " + last_error())


UNPACK_BAD_CRC = -2147483647  # LZ4E_UNPACK_BAD_CRC (INT32_MIN + 1)


def crc32c_batch_dev(data, off, len_, crc, max_len: Optional[int] = None, stream=None) -> None:
    """lz4e_crc32c_batch_dev on torch tensors (launch only): crc[i] = CRC-32C
    of the len_[i] bytes at data + off[i].

    data: uint8; off: int64; len_: int32; crc: int32 (torch has no unsigned
    32-bit arithmetic: the column's bit patterns; ``crc.cpu().numpy().view
    ("uint32")`` gives the values).  ``max_len`` is a sizing hint (default:
    read from len_, which synchronises); no result depends on it."""
    import torch
    n = int(len_.numel())
    _check_dev(n, data=data, off=off, len=len_, crc=crc)
    if max_len is None:
        max_len = max(0, int(len_.max().item())) if n else 0
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    r = lib().lz4e_crc32c_batch_dev(_ptr(data), _ptr(off), _ptr(len_), _ptr(crc), n, int(max_len), stream)
    if r != 0:
        raise RuntimeError("lz4e_crc32c_batch_dev: " + last_error())


def pack_crc_batch_dev(frames, fr_off, src, src_off, pk_len, pk_kind, pk_crc, max_len: Optional[int] = None,
                       stream=None) -> None:
    """lz4e_pack_crc_batch_dev on torch tensors (launch only): the index's
    checksum column, after pack_batch_dev on the same stream with the same
    frames / fr_off / src / src_off.  pk_crc: int32 (bit patterns, as
    crc32c_batch_dev's).  ``max_len`` as for pack_batch_dev (default: read
    from pk_len, which synchronises)."""
    import torch
    n = int(pk_len.numel())
    _check_dev(n, frames=frames, fr_off=fr_off, src=src, src_off=src_off, pk_len=pk_len, pk_kind=pk_kind,
               pk_crc=pk_crc)
    if max_len is None:
        max_len = max(0, int(pk_len.max().item())) if n else 0
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    r = lib().lz4e_pack_crc_batch_dev(_ptr(frames), _ptr(fr_off), _ptr(src), _ptr(src_off), _ptr(pk_len),
                                      _ptr(pk_kind), _ptr(pk_crc), n, int(max_len), stream)
    if r != 0:
        raise RuntimeError("lz4e_pack_crc_batch_dev: " + last_error())


def unpack_range_verified_batch_dev(packed, pk_off, pk_len, pk_kind, pk_crc, sel, lo, len_, dst, dst_off, ret,
                                    max_end: int, max_len: Optional[int] = None, stream=None) -> None:
    """lz4e_unpack_range_verified_batch_dev on torch tensors (launch only):
    unpack_range_batch_dev that checks each entry a request reads against
    pk_crc first (once per call, however many requests name it); every
    request with len_ > 0 on an entry whose stored bytes do not match gets ret
    UNPACK_BAD_CRC and nothing is written for it.  pk_crc: int32 bit patterns,
    as pack_crc_batch_dev writes them.  ``max_len`` is a sizing hint that
    bounds pk_len (default: read from pk_len, which synchronises); no result
    depends on it."""
    import torch
    n = int(pk_len.numel())
    nreq = int(lo.numel())
    _check_dev(0, packed=packed, pk_off=pk_off, pk_len=pk_len, pk_kind=pk_kind, pk_crc=pk_crc, sel=sel, lo=lo,
               len=len_, dst=dst, dst_off=dst_off, ret=ret)
    for name, t, need in (("pk_off", pk_off, n + 1), ("pk_len", pk_len, n), ("pk_kind", pk_kind, n),
                          ("pk_crc", pk_crc, n), ("sel", sel, nreq), ("lo", lo, nreq), ("len_", len_, nreq),
                          ("dst_off", dst_off, nreq), ("ret", ret, nreq)):
        if t is not None and t.numel() < need:
            raise ValueError(f"{name}: {t.numel()} entries, needs {need}")
    if max_len is None:
        max_len = max(0, int(pk_len.max().item())) if n else 0
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    r = lib().lz4e_unpack_range_verified_batch_dev(_ptr(packed), _ptr(pk_off), _ptr(pk_len), _ptr(pk_kind),
                                                   _ptr(pk_crc), n, _ptr(sel), _ptr(lo), _ptr(len_), _ptr(dst),
                                                   _ptr(dst_off), _ptr(ret), nreq, max(0, int(max_end)),
                                                   max(0, int(max_len)), stream)
    if r != 0:
        raise RuntimeError("lz4e_unpack_range_verified_batch_dev: " + last_error())


def unpack_verified_batch_dev(packed, pk_off, pk_len, pk_kind, pk_crc, dst, dst_off, dst_cap, ret, stream=None,
                              max_cap: Optional[int] = None) -> None:
    """lz4e_unpack_verified_batch_dev on torch tensors (launch only):
    unpack_batch_dev that checks each entry against pk_crc first; an entry
    whose stored bytes do not match gets ret UNPACK_BAD_CRC and nothing is
    written for it.  ``max_cap`` as for unpack_batch_dev."""
    import torch
    n = int(pk_len.numel())
    _check_dev(n, packed=packed, pk_off=pk_off, pk_len=pk_len, pk_kind=pk_kind, pk_crc=pk_crc, dst=dst,
               dst_off=dst_off, dst_cap=dst_cap, ret=ret)
    if max_cap is None:
        max_cap = int(dst_cap.max().item()) if n else 0
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    r = lib().lz4e_unpack_verified_batch_dev(_ptr(packed), _ptr(pk_off), _ptr(pk_len), _ptr(pk_kind), _ptr(pk_crc),
                                             _ptr(dst), _ptr(dst_off), _ptr(dst_cap), _ptr(ret), n,
                                             max(0, int(max_cap)), stream)
    if r != 0:
        raise RuntimeError("lz4e_unpack_verified_batch_dev: " + last_error())
