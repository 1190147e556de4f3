// lz4e_gpu.h -- internal (C++) launch interface of the gfx950 LZ4E kernels.
// The public C ABI is include/lz4e.h; lz4e_host.hip maps it onto these.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lz4e {

// Largest block whose bytes the compressor stages in LDS.  The parse is
// latency-bound per block, so the 16 KiB table alone (10 blocks per CU,
// input read through L1/L2) beats staging for anything but small blocks.
constexpr uint32_t kMaxLdsInput = 4096;

struct CompressBatch {
    const uint8_t* src;
    const uint64_t* src_off;
    const uint32_t* src_len;
    const uint8_t* table_type;
    uint8_t* dst;
    const uint64_t* dst_off;
    const uint32_t* dst_cap;
    int32_t* ret;
    uint32_t* aux;  // nullable, 2 words per block
    uint32_t nblocks;
    uint32_t max_len;
    // Dictionary mode (nullable): block i's dictionary is the dict_len[i]
    // (<= 64 KiB) bytes right before src + src_off[i]; byU32 blocks only.
    const uint32_t* dict_len = nullptr;
};

struct DecompressBatch {
    const uint8_t* src;
    const uint64_t* src_off;
    const int32_t* src_len;
    uint8_t* dst;
    const uint64_t* dst_off;
    const int32_t* dst_cap;
    int32_t* ret;
    uint32_t nblocks;
    // Upper bound of dst_cap[] (0: unknown); with the batch size it selects
    // the decoder (pick_decoder in lz4e_decompress.hip).
    uint32_t max_cap;
    uint32_t mode = 0;  // kDecAuto, or force kDecWave / kDecPipe / kDecSmall / kDecGroup / kDecGroupNoBail (tests, A/B)
    // Dictionary mode (nullable): block i decodes with the dict_len[i] bytes
    // right before dst + dst_off[i] as its dictionary (extDict semantics of
    // lz4e_decompress.c:299-302, 339-378; <= 64 KiB of it is ever read).
    const int32_t* dict_len = nullptr;
    // Partial decode (include/lz4e.h, LZ4E_decompress_safe_partial):
    // dst_cap[i] is block i's target size.  No dictionary, and never the
    // group decoder, which has no partial form: auto mode and
    // LZ4E_DECOMPRESS_MODE=g take the one-wave decoder in its place.
    bool partial = false;
};

// (3 was the streaming decoder, removed in round 4; 4 and 5 the chunked and
// relay decoders, removed in round 5: none was ever picked by auto mode)
// kDecGroupNoBail: the group decoder with its hand-over to the one-wave
// decoder disabled -- every block decoded to its end by its group (tests and
// A/B only; auto mode never picks it).
enum : uint32_t { kDecAuto = 0, kDecWave = 1, kDecPipe = 2, kDecSmall = 6, kDecGroup = 7, kDecGroupNoBail = 9 };

// Launch order policy (lz4e_order.h): 0 block order, 1 heavy first when the
// batch is large enough (default), 2 heavy first always.  From
// lz4e_debug_set_launch_order, else LZ4E_COMPRESS_ORDER / LZ4E_DECOMPRESS_ORDER
// (0 disables), else 1.
enum : int { kOrderNever = 0, kOrderAuto = 1, kOrderAlways = 2 };
int launch_order_mode(bool compress);

uint32_t compress_lds_bytes(uint32_t max_len, bool lds_input);
hipError_t launch_compress(const CompressBatch& a, hipStream_t stream);
// Diagnostic build: per-block phase cycle counters into dbg, kCompressStampWords
// x u64 per block: 6 phase cycle sums, 2 packed counts, the parse's shader
// cycles and its 100 MHz (s_memrealtime) ticks.
constexpr uint32_t kCompressStampWords = 16;
hipError_t launch_compress_stamped(const CompressBatch& a, hipStream_t stream, uint64_t* dbg);
hipError_t launch_decompress(const DecompressBatch& a, hipStream_t stream);
hipError_t launch_decompress_stamped(const DecompressBatch& a, hipStream_t stream, uint64_t* dbg);

// Zero-copy scatter-gather kernels (lz4e_sg.hip): the device reads and
// writes registered host memory itself.  The descriptor formats say nothing
// about the chunk pipeline, so the other host entry points can adopt them.
//
// Gather: `len` bytes at device-visible address `src` go to data + dst_off.
// The host splits a segment into descriptors of at most kSgPiece bytes (one
// workgroup each), so that a long segment is many PCIe reads in flight.
constexpr uint32_t kSgPiece = 16384;
struct SgGatherDesc {
    uint64_t src;
    uint64_t dst_off;
    uint32_t len;
    uint32_t reserved;
};
hipError_t launch_sg_gather(const SgGatherDesc* desc, uint32_t ndesc, uint8_t* data, hipStream_t stream);

// Deliver: request `entry` of a round-trip batch.  When ret[entry] > 0,
// dret[entry] == in_len[entry] and (frame == 0 or frame_cap >= ret[entry]),
// ret[entry] bytes at data + fr_off[entry] go to `frame` (if set) and
// in_len[entry] bytes at data + out_off[entry] to `data`; otherwise nothing
// is written.
struct SgDeliverDesc {
    uint64_t frame;  // device-visible address, 0: no frame wanted
    uint64_t data;   // device-visible address
    uint32_t entry;
    int32_t frame_cap;
};
struct SgDeliverBatch {
    const SgDeliverDesc* desc;
    uint32_t ndesc;
    const uint8_t* data;
    const uint64_t* fr_off;
    const uint64_t* out_off;
    const uint32_t* in_len;
    const int32_t* ret;
    const int32_t* dret;
    uint32_t max_len;  // upper bound of in_len[] (sizes the grid)
};
hipError_t launch_sg_deliver(const SgDeliverBatch& a, hipStream_t stream);

// Packed frame store (lz4e_pack.hip; include/lz4e.h lz4e_pack_batch_dev /
// lz4e_unpack_batch_dev).  Entry kinds as in the public header.
constexpr uint32_t kPackFrame = 0, kPackRaw = 1;
// Blocks per scan tile: one per thread of a 256-thread workgroup; the one
// wave that scans the tile sums takes 64 of them per round.
constexpr uint32_t kPackTile = 256;
struct PackBatch {
    const uint8_t* frames;  // the compress launch's dst / dst_off / ret
    const uint64_t* fr_off;
    const int32_t* ret;
    const uint8_t* src;  // and its src / src_off / src_len
    const uint64_t* src_off;
    const uint32_t* src_len;
    uint8_t* packed;
    uint64_t packed_cap;
    uint32_t align;    // power of two, 1..4096 (checked by the caller)
    uint64_t* pk_off;  // nblocks + 1
    int32_t* pk_len;
    uint8_t* pk_kind;
    uint32_t nblocks;
    uint32_t max_len;  // upper bound of src_len[] (sizes the copy's grid)
};
// Index (three launches: tile sums, scan of the tile sums, tile scan + base)
// and the gather; no scratch memory: the tile sums live in pk_off itself.
hipError_t launch_pack(const PackBatch& a, hipStream_t stream);
// masked[i] = pk_len[i] for a frame entry, 0 for every other kind: the
// decoders then return -1 for it and touch neither its input nor its output.
hipError_t launch_unpack_mask(const int32_t* pk_len, const uint8_t* pk_kind, uint32_t nblocks,
                              int32_t* masked, hipStream_t stream);
// Behind the decoders: the raw entries' bytes, and ret of every entry that is
// not a frame.
struct UnpackRawBatch {
    const uint8_t* packed;
    const uint64_t* pk_off;
    const int32_t* pk_len;
    const uint8_t* pk_kind;
    uint8_t* dst;
    const uint64_t* dst_off;
    const int32_t* dst_cap;
    int32_t* ret;
    uint32_t nblocks;
    uint32_t max_cap;  // upper bound of dst_cap[] (0: unknown)
};
hipError_t launch_unpack_raw(const UnpackRawBatch& a, hipStream_t stream);

// Range read of the packed store (include/lz4e.h,
// lz4e_unpack_range_batch_dev): request j wants bytes [lo[j], lo[j] + len[j])
// of entry sel[j] (sel null: entry j).  launch_range_gather writes the
// partial launch's descriptors -- g_off / g_len / g_tgt: the frame and the
// target min(lo + len, max_end), or 0 / 0 / 0 for a request no decoder may
// touch; s_off[j] = j * slot, its scratch slot (slot >= max_end) -- and
// launch_range_deliver, behind that launch (whose values are g_ret), copies
// the wanted bytes out of the slots, or out of the image for raw entries,
// and sets ret.
struct RangeBatch {
    const uint8_t* packed;
    const uint64_t* pk_off;
    const int32_t* pk_len;
    const uint8_t* pk_kind;
    uint32_t nentries;
    const uint32_t* sel;  // nullable
    const int32_t* lo;
    const int32_t* len;
    uint8_t* dst;
    const uint64_t* dst_off;
    int32_t* ret;
    uint32_t nreq;
    uint32_t max_end;  // upper bound of lo[] + len[]
    uint64_t slot;     // bytes of scratch per request
    uint8_t* scratch;
    uint64_t* g_off;
    int32_t* g_len;
    int32_t* g_tgt;
    uint64_t* s_off;
    int32_t* g_ret;
};
hipError_t launch_range_gather(const RangeBatch& a, hipStream_t stream);
hipError_t launch_range_deliver(const RangeBatch& a, hipStream_t stream);

// CRC-32C of every entry of a batch (lz4e_crc.hip; include/lz4e.h
// lz4e_crc32c_batch_dev, lz4e_pack_crc_batch_dev,
// lz4e_unpack_verified_batch_dev).  Entry i is the len[i] bytes at
// data + off[i]; with kinds given, a kPackRaw entry's bytes are at
// raw + raw_off[i] instead and an entry of any other kind than these two is
// not read.  len[i] <= 0: not read either.  crc[i] = 0 for an entry that is
// not read.
struct CrcBatch {
    const uint8_t* data;
    const uint64_t* off;
    const uint8_t* raw;       // used with kinds only
    const uint64_t* raw_off;
    const uint8_t* kind;      // nullable: every entry is at data + off[i]
    const int32_t* len;
    uint32_t* crc;
    uint32_t nblocks;
    uint32_t max_len;  // sizing hint: threads per entry (no result depends on it)
};
// Threads per entry = 1 << crc_team_shift (16 ... 16384).  Above 256 an entry
// spans workgroups, each leaves one partial word and a second launch combines
// them: crc_partial_words() words of scratch (0: none needed).
uint32_t crc_team_shift(uint32_t max_len, uint32_t nblocks);
uint64_t crc_partial_words(uint32_t max_len, uint32_t nblocks);
hipError_t launch_crc(const CrcBatch& a, uint32_t* partial, hipStream_t stream);
// The verified unpack is lz4e_unpack_batch_dev's composition with two more
// kernels.  Before the decoders: masked[i] as launch_unpack_mask's, but 0 for
// an entry that is invalid (unknown kind, negative length) or whose checksum
// got[i] differs from pk_crc[i]; shown[i] = pk_kind[i], kVerifyInvalid or
// kVerifyBadCrc is the kind launch_unpack_raw is shown, which copies nothing
// for the two markers.  After it: ret of the marked entries.
constexpr uint32_t kVerifyInvalid = 2, kVerifyBadCrc = 3;
constexpr int32_t kUnpackBadCrc = -2147483647;  // LZ4E_UNPACK_BAD_CRC
hipError_t launch_unpack_verify_mask(const int32_t* pk_len, const uint8_t* pk_kind, const uint32_t* pk_crc,
                                     const uint32_t* got, uint32_t nblocks, int32_t* masked, uint8_t* shown,
                                     hipStream_t stream);
hipError_t launch_unpack_verify_ret(const uint8_t* shown, uint32_t nblocks, int32_t* ret, hipStream_t stream);

// The verified range read (include/lz4e.h,
// lz4e_unpack_range_verified_batch_dev) is lz4e_unpack_range_batch_dev's
// composition between four thread-per-request kernels and launch_crc.  A
// request that is valid with len > 0 "wants" its entry.
//   init     every entry a request names: owner[e] = kNoOwner, shown[e] =
//            pk_kind[e].  shown is the kind column the range kernels are given.
//   elect    one wanting request per entry becomes its owner (one atomicCAS on
//            owner[e]; which one wins changes no result) and describes the
//            entry to launch_crc, c_off[j] / c_len[j]; every other request
//            describes 0 bytes, which launch_crc does not read.  So an entry
//            is summed once however many requests name it, and the bytes of
//            an entry nobody wants are not read.
//   launch_crc on (packed, c_off, c_len) over nreq entries -> got[nreq]
//   verdict  the owner with got[j] != pk_crc[e] sets shown[e] = kVerifyBadCrc:
//            launch_range_gather and launch_range_deliver, run on shown, take
//            the entry for one of unknown kind -- no descriptor, no read, no
//            write, ret -1.
//   ret      behind launch_range_deliver, by the real pk_kind: 0 for a valid
//            request with len 0 (deliver has said -1 if its entry was marked),
//            kUnpackBadCrc for every other valid request on a marked entry.
// owner / shown have nentries elements (only those named are touched), c_off /
// c_len / got nreq.
constexpr uint32_t kNoOwner = 0xFFFFFFFFu;
struct RangeVerifyBatch {
    const uint64_t* pk_off;
    const int32_t* pk_len;
    const uint8_t* pk_kind;
    const uint32_t* pk_crc;
    uint32_t nentries;
    const uint32_t* sel;  // nullable
    const int32_t* lo;
    const int32_t* len;
    int32_t* ret;
    uint32_t nreq;
    uint32_t* owner;
    uint8_t* shown;
    uint64_t* c_off;
    int32_t* c_len;
    uint32_t* got;
};
hipError_t launch_range_verify_init(const RangeVerifyBatch& a, hipStream_t stream);
hipError_t launch_range_verify_elect(const RangeVerifyBatch& a, hipStream_t stream);
hipError_t launch_range_verify_verdict(const RangeVerifyBatch& a, hipStream_t stream);
hipError_t launch_range_verify_ret(const RangeVerifyBatch& a, hipStream_t stream);

}  // namespace lz4e
