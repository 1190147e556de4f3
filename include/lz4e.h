/*
 * lz4e.h -- C ABI of the MI355X-native LZ4E scatter-gather block codec.
 *
 * Drop-in boundary for the reference's two exported symbols:
 *   LZ4E_compress_default  <- /root/reference/lz4e/include/lz4e.h:47-48
 *                             (definition lz4e/lz4e_compress.c:563-569)
 *   LZ4E_decompress_safe   <- /root/reference/lz4e/include/lz4e.h:50-51
 *                             (definition lz4e/lz4e_decompress.c:462-470)
 * plus the sizing macros of lz4e/include/lz4e.h:9-28,53-55 and the
 * LZ4E_stream_t work-memory layout of lz4e/include/lz4e.h:33-45.
 *
 * Both single-call entry points run on the GPU (gfx950): the host shim
 * gathers the bio_vec segments into pinned staging, copies them to HBM,
 * launches the hand-written HIP kernel and scatters the frame back into the
 * destination bio_vecs.  Like the reference they are reentrant.  Concurrent
 * callers on one device are coalesced: a caller queues its request, and a
 * caller that finds fewer than 4 batches in flight runs every queued
 * request of that device (its own included) as one batch launch on its own
 * thread and leased HIP stream while the others wait for their result; a
 * lone caller runs at once.  A batch that fails as a whole is rerun call by
 * call, so one caller's failure is not another's.  There is no CPU codec
 * behind these symbols; when no GPU is usable they fail (compress returns
 * 0, decompress returns a negative value) and lz4e_last_error() says why.
 *
 * The batched lz4e_*_batch_* entry points are the throughput path: many
 * independent blocks per launch, device-resident buffers, caller's stream.
 *
 * Placement contract of the device-resident entry points
 * (lz4e_compress_batch_dev, lz4e_decompress_batch_dev2 / _dev and their
 * _dict forms):
 *   - src_off[i] and dst_off[i] need no alignment; blocks may sit at any
 *     byte address, packed back to back.
 *   - Reads stay inside the aligned 4-byte words that hold block i's input
 *     bytes (and its dictionary's): at most 3 bytes before the first and
 *     3 bytes after the last byte.
 *   - Writes stay inside [dst_off[i], dst_off[i] + dst_cap[i]): no slack is
 *     needed after a slot, and a block that fails (compress returns 0,
 *     decompress a negative value) writes nowhere else either.  Bytes of a
 *     slot past the returned size are unspecified.
 * Evidence: tests/test_gpu_placement.py runs every residue mod 16 on the GPU
 * with every byte outside the slots checked (values and the write bullet; a
 * GPU test cannot observe reads).  The read bullet rests on the lane
 * emulator: tools/emu/emu_main --skew S,D runs the kernels' sources on
 * exactly sized, poisoned buffers under ASan (tests/test_emulator.py).
 *
 * Plain C, no torch types.  All sizes are bytes.
 */
#ifndef LZ4E_AMD_H
#define LZ4E_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* Userspace view of the kernel block-layer SG types (doc/API.md:47-82).     */
/* ------------------------------------------------------------------------ */
#ifndef LZ4E_HAVE_KERNEL_BVEC
/*
 * A page frame.  Userspace model: page_address(p) == (char *)p and a
 * multi-page bvec covers physically contiguous pages, so byte k of a bvec
 * lives at (char *)bv_page + bv_offset + k.
 */
struct page;

struct bio_vec {
	struct page *bv_page;   /* first page the segment lives on        */
	unsigned int bv_len;    /* segment length in bytes                */
	unsigned int bv_offset; /* offset of the segment inside bv_page   */
};

struct bvec_iter {
	uint64_t bi_sector;        /* unused by the codec                  */
	unsigned int bi_size;      /* residual bytes                       */
	unsigned int bi_idx;       /* current index into the bio_vec array */
	unsigned int bi_bvec_done; /* bytes done in the current bio_vec    */
};
#endif

#define LZ4E_PAGE_SIZE 4096u
#ifndef BIO_MAX_VECS
#define BIO_MAX_VECS 256
#endif

/* ------------------------------------------------------------------------ */
/* Sizing macros (values fixed by the reference: lz4e/include/lz4e.h)        */
/* ------------------------------------------------------------------------ */
#define LZ4E_NAME "lz4e"
#define LZ4E_ACCELERATION_DEFAULT 1
#define LZ4E_MEMORY_USAGE 14
#define LZ4E_HASHLOG (LZ4E_MEMORY_USAGE - 2)
#define LZ4E_HASH_SIZE_U32 (1 << LZ4E_HASHLOG)
#define LZ4E_HASH_SIZE_U64 (LZ4E_HASH_SIZE_U32 >> 1)
#define LZ4E_BV_ITER_SIZE_U64 (BIO_MAX_VECS >> 1)
#define LZ4E_STREAMSIZE_U64 (LZ4E_HASH_SIZE_U64 + LZ4E_BV_ITER_SIZE_U64 + 4)
#define LZ4E_STREAMSIZE (LZ4E_STREAMSIZE_U64 * sizeof(unsigned long long))
#define LZ4E_MEM_COMPRESS LZ4E_STREAMSIZE /* 17440 bytes */

#define LZ4E_MAX_INPUT_SIZE 0x7E000000 /* 2 113 929 216 bytes */
#define LZ4E_COMPRESSBOUND(isize)                                        \
	((unsigned int)(isize) > (unsigned int)LZ4E_MAX_INPUT_SIZE ? 0 :  \
	 (isize) + ((isize) / 255) + 16)

#ifndef LZ4E_DISTANCE_MAX
#define LZ4E_DISTANCE_MAX 65535
#endif

/* Work-memory layout (same size/shape as the reference's LZ4E_stream_t). */
typedef struct {
	uint32_t bvIterSize[BIO_MAX_VECS];
	uint32_t hashTable[LZ4E_HASH_SIZE_U32];
	uint32_t currentOffset;
	uint32_t initCheck;
	const uint8_t *dictionary;
	uint8_t *bufferStart;
	uint32_t dictSize;
} LZ4E_stream_t_internal;

typedef union {
	unsigned long long table[LZ4E_STREAMSIZE_U64];
	LZ4E_stream_t_internal internal_donotuse;
} LZ4E_stream_t;

/* Hash-table address classes chosen from the SG layout
 * (lz4e/include/lz4e_defs.h:689, rules lz4e/lz4e_compress.c:184-211). */
#define LZ4E_TABLE_BYU16 1
#define LZ4E_TABLE_BYU32 3
#define LZ4E_TABLE_BYU64 7

/* ------------------------------------------------------------------------ */
/* Reference entry points (drop-in).                                         */
/* ------------------------------------------------------------------------ */

/*
 * Compress srcIter->bi_size bytes read through the bio_vec list `src`
 * (starting at *srcIter) into one raw LZ4 block written through `dst`
 * starting at *dstIter; dstIter->bi_size is the output capacity.
 * Returns the block size, or 0 on failure (input too large, more than
 * BIO_MAX_VECS segments, output capacity too small, or no usable GPU).
 * On success *dstIter is advanced by (ret - last literal run) and *srcIter
 * to the last position the match finder visited, like the reference.
 * `wrkmem` must point to LZ4E_MEM_COMPRESS bytes; it is zeroed on entry
 * (the match finder's state itself lives in GPU LDS).
 * Replaces lz4e/lz4e_compress.c:563.
 */
int LZ4E_compress_default(const struct bio_vec *src, struct bio_vec *dst,
			  struct bvec_iter *srcIter, struct bvec_iter *dstIter,
			  void *wrkmem);

/*
 * Safe full-block decode of `compressedSize` bytes at `source` into at most
 * `maxDecompressedSize` bytes at `dest` (contiguous host buffers).
 * Returns the number of bytes written, or -(input position of the error)-1.
 * Replaces lz4e/lz4e_decompress.c:462 (and, with the same signature, the
 * kernel LZ4_decompress_safe call at lz4e_bdev/lz4e_chunk.c:125).
 */
int LZ4E_decompress_safe(const char *source, char *dest, int compressedSize,
			 int maxDecompressedSize);

/* ------------------------------------------------------------------------ */
/* Extensions                                                                */
/* ------------------------------------------------------------------------ */

/* Table class of an SG source (1/3/7), or 0 when it spans more than
 * BIO_MAX_VECS segments.  Only meaningful for bi_size >= 13 (smaller inputs
 * never consult the table).  Rules of lz4e/lz4e_compress.c:184-211. */
int lz4e_sg_table_type(const struct bio_vec *src, const struct bvec_iter *it);

/* Human-readable reason for the last failure on this thread ("" if none). */
const char *lz4e_last_error(void);

/* 1 if a gfx950 device is usable by the library, else 0. */
int lz4e_gpu_available(void);

/*
 * One SG compress request of a host batch.  Same meaning as the arguments
 * of LZ4E_compress_default; `ret` receives its return value.  The
 * iterators are updated exactly like the single-call form.
 */
struct lz4e_sg_request {
	const struct bio_vec *src;
	struct bio_vec *dst;
	struct bvec_iter *srcIter;
	struct bvec_iter *dstIter;
	int ret;
};

/* Compress `n` independent SG requests with one gather, one H2D copy, one
 * kernel launch, one D2H copy and one scatter.  Returns the number of
 * requests that succeeded (ret > 0), or -1 when no GPU is usable. */
int lz4e_compress_sg_batch(struct lz4e_sg_request *reqs, int n);

/* Decompress `n` independent contiguous host blocks (src[i], csize[i]) into
 * (dst[i], cap[i]); ret[i] receives LZ4E_decompress_safe's value.  Returns
 * the number of blocks with ret >= 0, or -1 when no GPU is usable. */
int lz4e_decompress_batch(const char *const *src, const int *csize,
			  char *const *dst, const int *cap, int *ret, int n);

/*
 * Device-resident batch compress (the throughput path).  All pointers are
 * device (HBM) pointers; `stream` is a hipStream_t (NULL = default stream).
 * Block i reads src_len[i] bytes at src + src_off[i], uses table class
 * table_type[i] (1/3/7, from lz4e_sg_table_type of its SG layout) and writes
 * at most dst_cap[i] bytes at dst + dst_off[i]; ret[i] receives the block
 * size or 0.  `aux` (nullable, 2 words per block) receives
 * {final src position, last literal run} for iterator post-state.
 * `max_len` bounds src_len[] (it selects the LDS staging mode).  Batches
 * of 1024+ blocks of 16 KiB+ are launched heaviest block first (a sampled
 * weight per block and a counting sort on `stream`, scratch from the
 * stream-ordered pool: hipMallocAsync / hipFreeAsync); the bytes written
 * never depend on it.
 * Returns 0 on a successful launch, else a negative error.
 *
 * ret[i] == LZ4E_COMPRESS_ABORTED: a block above the LDS staging limit is
 * compressed by two waves, a parser and a flusher that writes the frame from
 * the parser's sequence records; every wait between them is bounded (about a
 * second plus a term per input byte with no progress at all), and this value
 * says that one ran out: a broken invariant of the kernel, never a property
 * of the input.  The frame bytes are then undefined.  The value is negative,
 * so every path that takes ret <= 0 as "did not compress" (the host entry
 * points, lz4e_pack_batch_dev's raw fallback) handles it as such.
 */
#define LZ4E_COMPRESS_ABORTED (-2147483647 - 1)
int lz4e_compress_batch_dev(const uint8_t *src, const uint64_t *src_off,
			    const uint32_t *src_len, const uint8_t *table_type,
			    uint8_t *dst, const uint64_t *dst_off,
			    const uint32_t *dst_cap, int32_t *ret, uint32_t *aux,
			    uint32_t nblocks, uint32_t max_len, void *stream);

/*
 * Device-resident batch decompress.  Block i decodes src_len[i] bytes at
 * src + src_off[i] into at most dst_cap[i] bytes at dst + dst_off[i];
 * ret[i] receives LZ4E_decompress_safe's return value.  `max_cap` bounds
 * dst_cap[] (0 = unknown) and selects the decoder: 16-128 KiB (or unknown),
 * and any batch of at most 1024 blocks, the pipelined one (one parser wave
 * and three copier waves per block); <= 4608 bytes the group decoder for
 * batches of >= 16384 blocks (one block per group of 8 lanes, blocks of
 * short sequences handed to the one-wave decoder), the one-wave decoder's LDS
 * form for 1025-3328 blocks; otherwise one wave per block.  All return identical values and bytes.  Pipelined batches of more
 * than 1536 blocks are launched in decreasing compressed-size order (as for
 * compress, on `stream`).  LZ4E_DECOMPRESS_MODE=w|p|s|g (one-wave,
 * pipelined, LDS form, group) overrides the choice for experiments.
 * Returns 0 on a successful launch, else a negative error.
 *
 * ret[i] == LZ4E_DECODE_ABORTED: the pipelined decoder's watchdog fired
 * (one of its waves waited ~1 s while nothing it depends on moved: a broken
 * invariant of the decoder, never a property of the input).  The reference
 * has no such outcome (lz4e_decompress.c:449-459 returns bytes written or
 * -(ip - src) - 1); the host entry points turn it into a failed call:
 * lz4e_decompress_batch / _dict / _sg_batch return -1, LZ4E_decompress_safe
 * (and _usingDict / lz4e_decompress_safe_sg) return LZ4E_DECODE_ABORTED,
 * lz4e_chunk_write_batch returns -1, each with lz4e_last_error() saying so.
 * (A genuine -(ip - src) - 1 equals it only for ip = 2^31 - 1, an input the
 * 0x7E000000-byte block limit cannot produce.)
 *
 * lz4e_decompress_batch_dev2 is the current form; lz4e_decompress_batch_dev
 * keeps the round-1 signature (no max_cap: pipelined decoder throughout).
 */
#define LZ4E_DECODE_ABORTED (-2147483647 - 1)
int lz4e_decompress_batch_dev2(const uint8_t *src, const uint64_t *src_off,
			       const int32_t *src_len, uint8_t *dst,
			       const uint64_t *dst_off, const int32_t *dst_cap,
			       int32_t *ret, uint32_t nblocks, uint32_t max_cap,
			       void *stream);
int lz4e_decompress_batch_dev(const uint8_t *src, const uint64_t *src_off,
			      const int32_t *src_len, uint8_t *dst,
			      const uint64_t *dst_off, const int32_t *dst_cap,
			      int32_t *ret, uint32_t nblocks, void *stream);

/*
 * Partial decoding: stop as soon as `target` bytes exist (a READ of a few
 * KiB at the front of a 64 KiB chunk does not pay for the chunk).  The
 * reference decoder carries it -- LZ4E_decompress_generic's earlyEnd_directive
 * partialDecoding, lz4e/lz4e_decompress.c:229-246, 276-282, 306-314, 384-405
 * -- but its one exported entry (:462-469) never instantiates it.  These
 * entry points are that function with endOnInputSize, partial_decode, noDict
 * and outputSize = target, line for line, return codes included (bytes
 * written, at most target, or -(ip - src) - 1).  Against the full decode:
 *
 *  - a literal run that would end past the target is cut there; the (cut)
 *    run must still lie inside the input (:230-246); after it the decode ends
 *    when the target is reached or fewer than 3 input bytes remain (:281),
 *    and goes on to the offset otherwise, so a frame that breaks the
 *    end-of-block rules can be accepted;
 *  - after the unchanged offset and length checks, a match that would end
 *    past target - 12 is cut to min(length, target - op) bytes, and the decode
 *    ends when the target is reached (:388-405); the full decoder's "last 5
 *    bytes are literals" error (:425-431) cannot occur;
 *  - the special cases (:113-120) are unchanged: target 0 gives -1 unless the
 *    frame is the single byte 00 (the reference's behaviour, which upstream
 *    LZ4 does not share).
 *
 * For a frame the full decoder accepts with n bytes of output, target k >= 1
 * gives min(k, n) and the first min(k, n) bytes of that output.  Nothing is
 * written outside [dest, dest + target).
 *
 * One deviation: the reference skips its LZ4_write32(op, offset) in partial
 * mode (:309-314), so a match with offset 0 would repeat whatever the
 * destination held before.  Here it yields zeros, as in the full decoders.
 *
 * No partial entry point takes a dictionary (in the reference's extDict
 * branch a cut match does not end the decode, :339-378, and the next token
 * may lie past the frame).
 *
 * LZ4E_decompress_safe_partial decodes to min(targetOutputSize, dstCapacity)
 * bytes, as LZ4_decompress_safe_partial does (a negative value of either:
 * -1).  Concurrent calls are coalesced like LZ4E_decompress_safe's, in
 * launches of their own.
 */
int LZ4E_decompress_safe_partial(const char *source, char *dest,
				 int compressedSize, int targetOutputSize,
				 int dstCapacity);

/* Host batch: lz4e_decompress_batch with target[i] in place of cap[i];
 * ret[i] receives the partial decode's value. */
int lz4e_decompress_partial_batch(const char *const *src, const int *csize,
				  char *const *dst, const int *target,
				  int *ret, int n);

/*
 * Device-resident partial batch: lz4e_decompress_batch_dev2's arguments,
 * placement contract (any byte alignment of inputs and outputs, nothing
 * written outside [dst + dst_off[i], + dst_cap[i])) and stream-capture
 * legality (launches and stream-ordered pool scratch only); dst_cap[i] is
 * block i's target and capacity at once.  The decoder is chosen as there,
 * except that the group decoder has no partial form: the one-wave decoder
 * takes its place, and LZ4E_DECOMPRESS_MODE=g is read as auto.
 */
int lz4e_decompress_partial_batch_dev(const uint8_t *src,
				      const uint64_t *src_off,
				      const int32_t *src_len, uint8_t *dst,
				      const uint64_t *dst_off,
				      const int32_t *dst_cap, int32_t *ret,
				      uint32_t nblocks, uint32_t max_cap,
				      void *stream);

/*
 * Dictionary mode.  The reference stubs its dictionary
 * path out (lz4e/lz4e_compress.c:250-266, 315-324, 393-419, 472-482; the
 * dictionary fields of LZ4E_stream_t, lz4e/include/lz4e.h:36-40) and its
 * exported decoder never instantiates the extDict branches
 * (lz4e/lz4e_decompress.c:299-302, 339-378, 462-469).  This is the LZ4E
 * extension built on them; no reference run pins its frames (parity
 * unpinned), the decoder restates those branches exactly.
 *
 * LZ4E_compress_usingDict: LZ4E_compress_default's contract (bio_vec source
 * and destination, iterators, wrkmem) compressing against the last <= 64 KiB
 * of `dictionary` (ignored under 8 bytes): the hash table is preloaded the
 * way LZ4_loadDict does it (every third dictionary position, in order), the
 * table class is byU32 whatever the SG layout, and matches may start in the
 * dictionary (offsets <= LZ4E_DISTANCE_MAX) and run on into the block.  The
 * >256-segment and size limits of LZ4E_compress_default still return 0.
 *
 * LZ4E_decompress_safe_usingDict: LZ4E_decompress_safe with a dictionary that
 * logically precedes `dest` (extDict): match bytes before `dest` read the
 * dictionary's end; with dictSize < 64 KiB an offset reaching before the
 * dictionary fails (-(ip - src) - 1, :299-302).  dictSize 0 is
 * LZ4E_decompress_safe.  Frames of LZ4E_compress_usingDict decode with the
 * same dictionary, so do those of any LZ4 dictionary compressor.
 */
int LZ4E_compress_usingDict(const struct bio_vec *src, struct bio_vec *dst,
			    struct bvec_iter *srcIter, struct bvec_iter *dstIter,
			    void *wrkmem, const char *dictionary, int dictSize);
int LZ4E_decompress_safe_usingDict(const char *source, char *dest,
				   int compressedSize, int maxDecompressedSize,
				   const char *dictStart, int dictSize);

/* Batch forms: request i with dictionary (dicts[i], dict_sizes[i]) (NULL or
 * size 0: none, still byU32 on the compress side); returns as the
 * dictionary-less batch calls. */
int lz4e_compress_sg_batch_dict(struct lz4e_sg_request *reqs, int n,
				const char *const *dicts, const int *dict_sizes);
int lz4e_decompress_batch_dict(const char *const *src, const int *csize,
			       char *const *dst, const int *cap,
			       const char *const *dicts, const int *dict_sizes,
			       int *ret, int n);

/* Device-resident dictionary batches: block i's dictionary is the
 * dict_len[i] bytes right before its input (compress: src + src_off[i],
 * table_type[i] must be 3 = byU32; at most 64 KiB used) or right before its
 * output (decompress: dst + dst_off[i] -- e.g. the previous block of the
 * same stream decoded in place, so a stream decodes block after block while
 * many streams decode in parallel). */
int lz4e_compress_batch_dev_dict(const uint8_t *src, const uint64_t *src_off,
				 const uint32_t *src_len, const uint8_t *table_type,
				 uint8_t *dst, const uint64_t *dst_off,
				 const uint32_t *dst_cap, int32_t *ret, uint32_t *aux,
				 uint32_t nblocks, uint32_t max_len,
				 const uint32_t *dict_len, void *stream);
int lz4e_decompress_batch_dev_dict(const uint8_t *src, const uint64_t *src_off,
				   const int32_t *src_len, uint8_t *dst,
				   const uint64_t *dst_off, const int32_t *dst_cap,
				   int32_t *ret, uint32_t nblocks, uint32_t max_cap,
				   const int32_t *dict_len, void *stream);

/*
 * LZ4E_decompress_safe into a bio_vec list (the read
 * side without a bounce buffer).  Decodes compressedSize bytes at `source`
 * into the segments of `dst` from *dstIter on, with capacity
 * dstIter->bi_size.  Returns exactly what LZ4E_decompress_safe returns for
 * that capacity (bytes written, or -(ip - src) - 1 on malformed input,
 * lz4e/lz4e_decompress.c:449-459); on success *dstIter is advanced by the
 * return value, on error nothing is written and *dstIter is untouched.
 */
int lz4e_decompress_safe_sg(const char *source, struct bio_vec *dst,
			    struct bvec_iter *dstIter, int compressedSize);

/* Batch form: request i decodes (src[i], csize[i]) into (dst[i],
 * dstIter[i]); ret[i] as above.  Returns the number of requests with
 * ret >= 0, or -1 when no GPU is usable. */
int lz4e_decompress_sg_batch(const char *const *src, const int *csize,
			     struct bio_vec *const *dst,
			     struct bvec_iter *const *dstIter, int *ret, int n);

/*
 * Chunk-layer WRITE round trip, batched and streamed.
 * Per request this is the data path of lz4e_write_req_init
 * (lz4e_bdev/lz4e_req.c:144-213): lz4e_chunk_compress_ext
 * (lz4e_bdev/lz4e_chunk.c:139-159: LZ4E_compress_default of the bio's SG
 * payload into a LZ4E_COMPRESSBOUND-sized chunk, i.e. never output-limited),
 * then lz4e_chunk_decompress (lz4e_chunk.c:119-137: LZ4_decompress_safe of
 * that frame back into the chunk's contiguous source buffer, whose size must
 * equal the bio's, lz4e_chunk.c:133).  Requests flow through four pipeline
 * slots (pinned staging + HBM buffers + a HIP stream each) in sub-batches of
 * a quarter of the call (16-256 MiB of input): the SG gather of one
 * sub-batch overlaps the H2D copies, kernels and D2H copies of the others.
 */
struct lz4e_chunk_request {
	const struct bio_vec *src;       /* original bio's bi_io_vec            */
	const struct bvec_iter *srcIter; /* original bio's bi_iter (read only:
					    the chunk layer passes a copy)      */
	char *data;        /* src_buf.data: receives srcIter->bi_size bytes    */
	char *frame;       /* nullable: receives the frame (dst_buf.data)      */
	int frame_cap;     /* bytes available at frame                         */
	int comp_size;     /* out: dst_buf.data_size (0 on compress failure)   */
	int status;        /* out: 0, -EIO (-5) like the chunk layer, or
			      -ENOSPC (-28) when frame_cap < comp_size          */
};

/* Write-side counters, the reference's struct lz4e_stats
 * (lz4e_bdev/include/lz4e_stats.h:17-22) updated as lz4e_stats_update does
 * at bio completion (lz4e_bdev/lz4e_stats.c:39-52), which only runs from
 * lz4e_end_io (lz4e_req.c:231-246): only a request whose round trip
 * completed (status 0) counts.  It adds 1 to reqs_total, the bi_vcnt of the
 * bio the reference completes (its src buffer re-added by
 * lz4e_add_buf_to_bio, lz4e_req.c:191-197: one merged bio_vec per
 * contiguous non-empty buffer) to vec_count and its size to data_in_bytes.
 * A request that fails in the write path (-EIO: compress or decompress
 * failure, more than 256 segments, oversize; -ENOSPC) returns through
 * lz4e_dev.c:187-202 in the reference and touches no counter.
 * reqs_failed counts completed bios the underlying device failed
 * (lz4e_stats.c:43-45); this library has no underlying device, so it is
 * always 0.  frame_bytes (not in the reference) = sum of comp_size of the
 * counted requests. */
struct lz4e_chunk_stats {
	uint64_t reqs_total;
	uint64_t reqs_failed;
	uint64_t vec_count;
	uint64_t data_in_bytes;
	uint64_t frame_bytes;
};

/* Returns the number of requests with status 0, or -1 on failure (no usable
 * GPU, or a HIP error part way through): every status is then -EIO, every
 * comp_size 0, `stats` is left untouched and nothing of the call is still
 * in flight.  `stats` is nullable; on success it is added to. */
int lz4e_chunk_write_batch(struct lz4e_chunk_request *reqs, int n,
			   struct lz4e_chunk_stats *stats);

/*
 * Registered host memory: the zero-copy path of lz4e_chunk_write_batch.
 * A block-device server that owns its I/O buffers (a ublk or SPDK-style
 * buffer pool) registers them once.  A request whose memory is registered
 * is then served without the pipeline's pinned staging and without a host
 * memcpy on either side: the device gathers the source segments out of the
 * caller's pages over PCIe and writes `data` and `frame` there itself; only
 * descriptors go up and only metadata comes back.
 *
 * The path is chosen per request from its addresses, never on the caller's
 * word: a request is zero-copy when every source byte its iterator covers,
 * [data, data + bi_size) and, with `frame` set, [frame, frame + frame_cap)
 * each lie wholly inside one live registration.  Any other request is staged
 * as before, and one call may hold both kinds.  lz4e_chunk_write_batch's
 * results -- status, comp_size, the bytes at `data` and `frame`, the stats --
 * do not depend on registration; a failing request (-EIO, -ENOSPC) has
 * nothing written to its `data` or `frame` on either path.
 * LZ4E_CHUNK_ZERO_COPY=0 in the environment, read per call, stages every
 * request.
 *
 * lz4e_register_host_memory pins [ptr, ptr + len) (hipHostRegister, mapped
 * and portable) and records its device address.  Returns 0 on success; -22
 * (-EINVAL) for a bad argument, without calling HIP: ptr NULL, len 0, ptr or
 * len not a multiple of LZ4E_PAGE_SIZE, or a range that overlaps a live
 * registration (adjacent ranges are fine; a buffer must lie inside ONE
 * registration to count as registered); -1 when no gfx950 is usable or HIP
 * refuses, with the reason in lz4e_last_error().
 *
 * lz4e_unregister_host_memory takes the base pointer of a live
 * registration.  Returns 0; -2 (-ENOENT) when ptr is not such a base; -1 on
 * a HIP failure (the range is forgotten all the same).  It takes the chunk
 * pipeline's lock, so it waits for a lz4e_chunk_write_batch in flight and
 * never pulls memory from under one.  The memory must stay allocated from
 * register to unregister; unregister before freeing it.
 */
int lz4e_register_host_memory(void *ptr, size_t len);
int lz4e_unregister_host_memory(void *ptr);

/*
 * Packed frame store: keeping the compressed bytes.
 *
 * lz4e_compress_batch_dev leaves frame i in a slot of the caller's choosing
 * (LZ4E_COMPRESSBOUND bytes for a compress that cannot fail), so after it the
 * frames occupy more memory than the input did.  lz4e_pack_batch_dev compacts
 * them into one dense image with an index and stores raw every block that did
 * not shrink; lz4e_unpack_batch_dev decodes such an image back into blocks.
 *
 * All pointers are device pointers.  frames / fr_off / ret are the dst /
 * dst_off / ret arrays and src / src_off / src_len the input arrays of the
 * lz4e_compress_batch_dev call that came before on the same stream; max_len
 * bounds src_len[] (src_len[i] <= LZ4E_MAX_INPUT_SIZE).  Both calls only
 * launch work on `stream` and are legal under stream capture: no synchronise,
 * no host read of device data, no hipMalloc / hipFree / hipMemcpy (pack uses
 * no scratch memory at all, unpack nblocks words from the stream-ordered
 * pool).  Both return 0 on a successful launch and -1 on a HIP failure, with
 * lz4e_last_error() set.  lz4e_pack_batch_dev returns -22 (-EINVAL) without
 * launching anything for an `align` that is 0, above 4096 or not a power of
 * two.
 *
 * Pack, per block i:
 *   kind     LZ4E_PACK_FRAME with pk_len[i] = ret[i] when
 *            0 < ret[i] < src_len[i]; otherwise LZ4E_PACK_RAW with
 *            pk_len[i] = src_len[i]: a failed compress (ret == 0), a frame
 *            that is not smaller than its input (equality included), an
 *            empty block.
 *   offsets  pk_off[0] = 0, pk_off[i + 1] = pk_off[i] + roundup(pk_len[i],
 *            align); 64-bit; pk_off[nblocks] is the stored size.
 *   bytes    packed[pk_off[i], pk_off[i] + pk_len[i]) is the frame or the raw
 *            input; the padding up to pk_off[i + 1] is written as zeros, so
 *            packed[0, pk_off[nblocks]) is a pure function of the inputs (it
 *            can be checksummed, deduplicated and compared whole).
 *   index    pk_off, pk_len and pk_kind are written whatever packed_cap is:
 *            a caller sizes a buffer from pk_off[nblocks].
 *   all or nothing
 *            if pk_off[nblocks] > packed_cap no byte of `packed` is written;
 *            otherwise no byte at or past pk_off[nblocks] is written.
 *   reads    stay inside [frames + fr_off[i], + ret[i]) for a frame entry and
 *            inside [src + src_off[i], + src_len[i]) for a raw one, exactly
 *            (not rounded to words); a raw block's frame slot and a frame
 *            block's source are not read.
 *   aliasing `packed` overlaps neither `frames` nor `src`.
 *   nblocks == 0: pk_off[0] = 0 and nothing else happens.
 *
 * Unpack, per block i (max_cap bounds dst_cap[], 0 = unknown):
 *   LZ4E_PACK_FRAME  ret[i] and the bytes at dst + dst_off[i] are what
 *            lz4e_decompress_batch_dev2 gives for a frame of pk_len[i] bytes
 *            at packed + pk_off[i] with capacity dst_cap[i], error codes
 *            included; the decoder is chosen from max_cap and nblocks by the
 *            same rule and LZ4E_DECOMPRESS_MODE is honoured.
 *   LZ4E_PACK_RAW    pk_len[i] <= dst_cap[i]: the pk_len[i] bytes are copied
 *            and ret[i] = pk_len[i]; otherwise ret[i] = -1 and nothing is
 *            written.
 *   any other kind   ret[i] = -1 and nothing is written.
 *   writes   stay inside [dst_off[i], dst_off[i] + dst_cap[i]).
 * pk_off needs no alignment: the decoders take frames at any byte address.
 */
#define LZ4E_PACK_FRAME 0   /* entry holds an LZ4E frame                    */
#define LZ4E_PACK_RAW   1   /* entry holds the block's input bytes verbatim */
int lz4e_pack_batch_dev(const uint8_t *frames, const uint64_t *fr_off,
			const int32_t *ret, const uint8_t *src,
			const uint64_t *src_off, const uint32_t *src_len,
			uint8_t *packed, uint64_t packed_cap, uint32_t align,
			uint64_t *pk_off /* nblocks + 1 */, int32_t *pk_len,
			uint8_t *pk_kind, uint32_t nblocks, uint32_t max_len,
			void *stream);
int lz4e_unpack_batch_dev(const uint8_t *packed, const uint64_t *pk_off,
			  const int32_t *pk_len, const uint8_t *pk_kind,
			  uint8_t *dst, const uint64_t *dst_off,
			  const int32_t *dst_cap, int32_t *ret, uint32_t nblocks,
			  uint32_t max_cap, void *stream);

/*
 * Packed frame store: range reads.  A READ asks for a few KiB at some offset
 * inside a chunk; request j reads bytes [lo[j], lo[j] + len[j]) of entry
 * sel[j] (sel == NULL: entry j; an entry may be named by many requests) into
 * dst + dst_off[j], without decoding the entry past lo[j] + len[j]:
 *
 *   invalid  sel[j] >= nentries, an unknown pk_kind, a negative pk_len, a
 *            negative lo[j] or len[j]: ret[j] = -1, nothing is read or
 *            written (checked first).
 *   len[j] == 0   ret[j] = 0, nothing is read or written.
 *   LZ4E_PACK_FRAME  d = the partial decode of the frame with target
 *            lo[j] + len[j] (lz4e_decompress_partial_batch_dev: values, error
 *            codes and decoder choice, from max_end and nreq).  d < 0:
 *            ret[j] = d and nothing is written.  Otherwise ret[j] =
 *            max(0, d - lo[j]) and those bytes, [lo[j], d) of the entry's
 *            data, are written.
 *   LZ4E_PACK_RAW    d = min(pk_len, lo[j] + len[j]), copied straight from
 *            the image; ret[j] and the bytes as above.
 *   writes   stay inside [dst_off[j], dst_off[j] + ret[j]), exactly.
 *
 * max_end bounds lo[] + len[] (a request past it is read as if it ended at
 * max_end; at most 0x7FFFFFF0).  Composition, as for unpack: a small kernel
 * gathers (offset, length, target) per request, the partial launch decodes
 * into scratch, a team copy (exact at both ends) delivers the ranges and the
 * raw entries and sets ret; no kernel waits on another workgroup.  Launches
 * only, legal under stream capture.  Footprint: one allocation from the
 * stream-ordered pool (hipMallocAsync on `stream`, freed behind the last
 * launch) of nreq x (roundup(max_end, 16) + 28) + 16 bytes -- a request costs
 * scratch for its whole prefix, so for reads far into large entries
 * lz4e_unpack_batch_dev may be the better call.  If the pool refuses it the
 * call returns -1 with lz4e_last_error() set and nothing is launched.
 * The checksum column is not consulted: the range read that checks each
 * named entry against pk_crc first is lz4e_unpack_range_verified_batch_dev,
 * below.
 * Returns 0 on successful launches, -22 for max_end above the limit.
 */
int lz4e_unpack_range_batch_dev(const uint8_t *packed, const uint64_t *pk_off,
				const int32_t *pk_len, const uint8_t *pk_kind,
				uint32_t nentries, const uint32_t *sel,
				const int32_t *lo, const int32_t *len,
				uint8_t *dst, const uint64_t *dst_off,
				int32_t *ret, uint32_t nreq, uint32_t max_end,
				void *stream);

/*
 * Packed frame store: integrity.
 *
 * A checksum column for the index, computed on the device where the image
 * is produced, and an unpack that checks every entry against it before a
 * decoder or a copy sees the entry.  The checksum is CRC-32C (Castagnoli),
 * the one of the Linux block layer, btrfs, iSCSI and SPDK: reflected,
 * polynomial 0x1EDC6F41 (reversed 0x82F63B78), initial value 0xFFFFFFFF,
 * final xor 0xFFFFFFFF; the CRC of the empty string is 0 and that of
 * "123456789" is 0xE3069283.
 *
 * All pointers are device pointers.  Like pack and unpack the three calls
 * only launch work on `stream` and are legal under stream capture: no
 * synchronise, no host read of device data, no hipMalloc / hipFree /
 * hipMemcpy; scratch (one word per workgroup of an entry that spans several,
 * and the verified unpack's 9 bytes per block) comes from the stream-ordered
 * pool.  They return 0 on a successful launch and -1 on a HIP failure, with
 * lz4e_last_error() set.
 *
 * lz4e_crc32c_batch_dev: crc[i] = CRC-32C of the len[i] bytes at
 * data + off[i]; len[i] <= 0 reads nothing and gives 0 (len[i] <=
 * LZ4E_MAX_INPUT_SIZE).  off[] needs no alignment.  Reads stay inside
 * [data + off[i], + len[i]) exactly (not rounded to words).  Only
 * crc[0, nblocks) is written.  max_len is a sizing hint (it picks the
 * threads per entry): results never depend on it, too small or too large, a
 * wrong hint only costs time.  nblocks == 0: nothing happens.
 *
 * lz4e_pack_crc_batch_dev: the index's checksum column, after
 * lz4e_pack_batch_dev on the same stream.  pk_crc[i] = CRC-32C of entry i's
 * stored bytes, read from where pack read them (frames + fr_off[i] for
 * LZ4E_PACK_FRAME, src + src_off[i] for LZ4E_PACK_RAW, pk_len[i] bytes; the
 * padding is not covered).  Like the rest of the index it is written whatever
 * packed_cap was: `packed` itself is never read, so an image that did not
 * fit still gets its column.  Same read bounds as pack: a raw block's frame
 * slot and a frame block's source are not read.  max_len as for pack (a
 * hint here).  The column equals lz4e_crc32c_batch_dev(packed, pk_off,
 * pk_len) on an image that was written.
 *
 * lz4e_unpack_verified_batch_dev: lz4e_unpack_batch_dev that checks each
 * entry first.  Per entry i, in this order:
 *   1. pk_kind[i] is neither LZ4E_PACK_FRAME nor LZ4E_PACK_RAW, or
 *      pk_len[i] < 0: ret[i] = -1, nothing is written and the entry's bytes
 *      are not read (its length and offset are not to be trusted).
 *   2. the CRC-32C of packed[pk_off[i], + pk_len[i]) differs from pk_crc[i]:
 *      ret[i] = LZ4E_UNPACK_BAD_CRC, no byte of its destination is written
 *      and no decoder sees the entry.
 *   3. otherwise ret[i] and the destination bytes are exactly those of
 *      lz4e_unpack_batch_dev: decoder choice, LZ4E_DECOMPRESS_MODE, error
 *      codes, a raw entry larger than its capacity (-1).
 * LZ4E_UNPACK_BAD_CRC collides with no other value of ret[i]: a genuine
 * decode error is -(ip - src) - 1 >= -0x7E000001 (the input is at most
 * LZ4E_MAX_INPUT_SIZE bytes), and LZ4E_DECODE_ABORTED is INT32_MIN.
 * max_cap bounds dst_cap[] (0 = unknown) as for unpack and also sizes the
 * checksum's teams (a hint there).
 *
 * lz4e_unpack_range_verified_batch_dev: lz4e_unpack_range_batch_dev that
 * checks each entry a request reads against pk_crc first.  All arguments of
 * the range read keep their meaning; pk_crc is the column
 * lz4e_pack_crc_batch_dev wrote.  Per request j, in this order:
 *   1. invalid, by exactly the range read's test (sel[j] >= nentries, an
 *      unknown pk_kind, a negative pk_len, a negative lo[j] or len[j]):
 *      ret[j] = -1, nothing is written and the entry's bytes are not read.
 *   2. len[j] == 0: ret[j] = 0, nothing is read or written.  The entry is not
 *      checked on this request's account, and the request gets 0 even when
 *      another request of the same call finds the entry damaged.
 *   3. the CRC-32C of packed[pk_off[e], + pk_len[e]), e = sel[j], differs
 *      from pk_crc[e]: ret[j] = LZ4E_UNPACK_BAD_CRC for every such request
 *      that names e, no byte of their destinations is written, and no decoder
 *      and no copy sees the entry.
 *   4. otherwise ret[j] and the bytes are exactly those of
 *      lz4e_unpack_range_batch_dev: the partial decode's error codes,
 *      LZ4E_DECODE_ABORTED, the decoder choice from max_end and nreq,
 *      LZ4E_DECOMPRESS_MODE, the max_end clamp, and writes confined to
 *      [dst_off[j], dst_off[j] + ret[j]).
 * LZ4E_UNPACK_BAD_CRC still collides with no other value of ret[j]: a count
 * is >= 0, an invalid request is -1, a decode error is -(ip - src) - 1 >=
 * -0x7E000001 as above, and LZ4E_DECODE_ABORTED is INT32_MIN.
 * Two things a composition by hand (lz4e_crc32c_batch_dev on a gathered
 * sub-index, then the plain range read) does not give:
 *   once per entry      an entry named by any number of rule-3/4 requests of
 *            one call is summed once: one of them is elected on the device
 *            and sums for all.
 *   only what is named  the image bytes of an entry that no rule-3/4 request
 *            names are not read.  (The index columns may be read at any
 *            entry.)
 * max_len is a sizing hint for the checksum's teams: it bounds pk_len[] of
 * the named entries; 0 = unknown, read as 256 x 64 as the verified unpack
 * does.  No result depends on it.
 * Launches only (no kernel waits on another workgroup; the election is one
 * atomic compare-and-swap per request, its outcome read only behind the
 * kernel boundary), legal under stream capture.  Footprint: ONE allocation
 * from the stream-ordered pool of
 *   nreq x (roundup(max_end, 16) + 28) + 16      the range read's
 *   + 16 x nreq                   the checksum's offset, length and result
 *   + 5 x nentries                the elected request and the shadow kind
 *   + 4 x P                       P = 0 while a checksum team fits a
 *                                 workgroup (max_len <= 16 KiB), else
 *                                 nreq x T / 256, T = the team's threads
 * bytes (T: about max_len / 64, a power of two up to 16384, fewer for huge
 * batches).  Returns 0 on successful launches and for nreq == 0 (nothing is
 * launched), -22 for max_end above 0x7FFFFFF0 (checked before any HIP call),
 * -1 with lz4e_last_error() set on a HIP failure or when the pool refuses
 * the scratch (nothing is launched then).
 */
#define LZ4E_UNPACK_BAD_CRC (-2147483647)   /* INT32_MIN + 1 */
int lz4e_crc32c_batch_dev(const uint8_t *data, const uint64_t *off,
			  const int32_t *len, uint32_t *crc,
			  uint32_t nblocks, uint32_t max_len, void *stream);
int lz4e_pack_crc_batch_dev(const uint8_t *frames, const uint64_t *fr_off,
			    const uint8_t *src, const uint64_t *src_off,
			    const int32_t *pk_len, const uint8_t *pk_kind,
			    uint32_t *pk_crc, uint32_t nblocks,
			    uint32_t max_len, void *stream);
int lz4e_unpack_verified_batch_dev(const uint8_t *packed, const uint64_t *pk_off,
				   const int32_t *pk_len, const uint8_t *pk_kind,
				   const uint32_t *pk_crc, uint8_t *dst,
				   const uint64_t *dst_off, const int32_t *dst_cap,
				   int32_t *ret, uint32_t nblocks,
				   uint32_t max_cap, void *stream);
int lz4e_unpack_range_verified_batch_dev(const uint8_t *packed, const uint64_t *pk_off,
					 const int32_t *pk_len, const uint8_t *pk_kind,
					 const uint32_t *pk_crc, uint32_t nentries,
					 const uint32_t *sel, const int32_t *lo,
					 const int32_t *len, uint8_t *dst,
					 const uint64_t *dst_off, int32_t *ret,
					 uint32_t nreq, uint32_t max_end,
					 uint32_t max_len, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LZ4E_AMD_H */
