// Standalone driver of the lane emulator (sanitizer runs, debuggers):
//   emu_main BLOCK_FILE TABLE_CLASS [FRAME_OUT [DICT_FILE]]
//   emu_main -d FRAME_FILE CAPACITY [OUT_FILE [DICT_FILE]]   (one-wave decoder)
//   emu_main -p FRAME_FILE CAPACITY [OUT_FILE [DICT_FILE]]   (pipelined decoder,
//            4 waves: parser + 3 copiers)
//   emu_main -l FRAME_FILE CAPACITY [OUT_FILE [DICT_FILE]]   (one-wave decoder,
//            LDS output for blocks of <= 4608 bytes without a dictionary)
//   emu_main -g FRAME_FILE CAPACITY [OUT_FILE [DICT_FILE]]   (block-per-group
//            decoder, 8 lanes a block)
//   emu_main -G FRAME_FILE CAPACITY [OUT_FILE [DICT_FILE]]   (the same without
//            the hand-over: every block decoded to its end by its group)
// compresses one block through the unmodified kernel source, prints the
// return value and the iterator post-state words, and writes the frame.
// With DICT_FILE the block is compressed in dictionary mode against the
// file's last <= 64 KiB (staged right before the block, as the library does).
// Buffers are sized exactly (no slack) so that ASan sees any overrun.
// A leading "--skew S,D" (0..15 each) places the input S bytes and the output
// D bytes past a 16-byte boundary; the buffers still end exactly where the
// block does (inputs at the end of the aligned dword holding their last byte,
// which the kernels may read).
// A leading "--cap N" makes the compressor's output buffer exactly N bytes
// (default: the block's bound, n + n/255 + 16), so ASan and the canary see any
// store outside a limited output; a block that is refused (ret 0) writes no
// FRAME_OUT.
// A leading "--ring N" gives the compressor N record slots per block for its
// deferred emit (LZ4E_COMPRESS_RECORDS; 0: none, every block emits inline;
// default: the library's).
// A leading "--partial T1,T2,..." (with -d, -p or -l; refused with -g / -G,
// the group decoder has no partial form) decodes the frame once per listed
// target size in this one process, as a partial decode: each output is an
// allocation of exactly the target's size, CAPACITY is not used, every decode
// prints "target T ret R" and writes OUT_FILE.T when R > 0.
// A leading "--hbm" compresses through the HBM-image kernel whatever the
// block's size (the batch's max_len is then one byte above the 4 096-byte
// staging limit at least): two waves per block, a parser and a flusher, for
// every block that defers its emit.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "emu_harness.h"  // EMU_POISON, EMU_UNPOISON

static unsigned g_src_skew = 0, g_dst_skew = 0;
static bool g_skewed = false;  // without --skew the buffers start at the heap block's start
static bool g_hbm = false;     // --hbm
static std::vector<int32_t> g_partial;  // --partial: the targets

// `size` bytes whose byte `lead` sits `skew` bytes past a 16-byte boundary.
// The heap block ends at the region's end (input: rounded up to the aligned
// dword); the pad in front holds a canary, and its whole 8-byte granules are
// poisoned, so a store before the region is caught by ASan or by ok().
struct Skewed {
    uint8_t* base = nullptr;
    uint8_t* p = nullptr;
    size_t pad = 0;
    Skewed(size_t size, size_t lead, unsigned skew, bool input) {
        pad = g_skewed ? (size_t)((skew + 16 - lead % 16) % 16) : 0;
        if (!input && pad + size == 0) pad = 16;  // an empty output buffer: every store is in front of it
        size_t total = pad + size;
        if (input) total = (total + 3) & ~(size_t)3;
        if (posix_memalign((void**)&base, 16, total ? total : 1)) exit(2);
        memset(base, 0, total);
        memset(base, 0xC7, pad);
        EMU_POISON(base, pad & ~(size_t)7);
        p = base + pad;
    }
    bool ok() const {
        EMU_UNPOISON(base, pad & ~(size_t)7);
        for (size_t i = 0; i < pad; ++i)
            if (base[i] != 0xC7) return false;
        return true;
    }
    ~Skewed() { free(base); }
};

extern "C" int emu_compress_batch(const uint8_t* src, const uint64_t* src_off, const uint32_t* src_len,
                                  const uint8_t* table_type, uint8_t* dst, const uint64_t* dst_off,
                                  const uint32_t* dst_cap, int32_t* ret, uint32_t* aux,
                                  uint32_t nblocks, uint32_t max_len);
extern "C" int emu_compress_batch_dict(const uint8_t* src, const uint64_t* src_off,
                                       const uint32_t* src_len, const uint8_t* table_type,
                                       uint8_t* dst, const uint64_t* dst_off, const uint32_t* dst_cap,
                                       int32_t* ret, uint32_t* aux, uint32_t nblocks, uint32_t max_len,
                                       const uint32_t* dict_len);

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) exit(2);
    int c;
    while ((c = fgetc(f)) != EOF) v.push_back((uint8_t)c);
    fclose(f);
    return v;
}

extern "C" int emu_decode_results(const int32_t* ret, uint32_t n, char* err, uint32_t err_cap);
extern "C" int emu_decompress_batch_mode(const uint8_t* src, const uint64_t* src_off,
                                         const int32_t* src_len, uint8_t* dst, const uint64_t* dst_off,
                                         const int32_t* dst_cap, int32_t* ret, uint32_t nblocks,
                                         const int32_t* dict_len, uint32_t mode);

extern "C" int emu_decompress_partial_mode(const uint8_t* src, const uint64_t* src_off,
                                           const int32_t* src_len, uint8_t* dst, const uint64_t* dst_off,
                                           const int32_t* target, int32_t* ret, uint32_t nblocks,
                                           uint32_t max_cap, uint32_t mode);

// Partial decodes of one frame: an exactly sized output per target.
static int partial_main(int argc, char** argv) {
    const char m = argv[1][1];
    if (m == 'g' || m == 'G') {
        fprintf(stderr, "emu_main: --partial with -%c: the group decoder has no partial form\n", m);
        return 2;
    }
    const uint32_t mode = m == 'p' ? 2u : (m == 'l' ? 6u : 1u);
    std::vector<uint8_t> frame = slurp(argv[2]);
    const int32_t csize = (int32_t)frame.size();
    Skewed in(frame.empty() ? 1 : frame.size(), 0, g_src_skew, true);
    if (!frame.empty()) memcpy(in.p, frame.data(), frame.size());
    for (const int32_t target : g_partial) {
        Skewed out((size_t)target, 0, g_dst_skew, false);
        const uint64_t so = 0, doff = 0;
        int32_t ret = -7777;
        emu_decompress_partial_mode(in.p, &so, &csize, out.p, &doff, &target, &ret, 1, (uint32_t)target, mode);
        if (!out.ok() || !in.ok()) {
            fprintf(stderr, "emu_main: a store in front of a buffer (target %d)\n", target);
            return 3;
        }
        printf("target %d ret %d\n", target, ret);
        if (ret > target) return 3;
        if (argc > 4 && ret > 0) {
            const std::string path = std::string(argv[4]) + "." + std::to_string(target);
            FILE* o = fopen(path.c_str(), "wb");
            if (!o) return 2;
            fwrite(out.p, 1, (size_t)ret, o);
            fclose(o);
        }
    }
    return 0;
}

// Decode: the frame in an exactly sized buffer, the output buffer exactly
// [dictionary (last <= 64 KiB) | capacity] -- ASan sees any read before the
// dictionary or any write past the capacity.
static int decode_main(int argc, char** argv) {
    std::vector<uint8_t> frame = slurp(argv[2]);
    const int32_t cap = atoi(argv[3]);
    std::vector<uint8_t> dict;
    if (argc > 5) dict = slurp(argv[5]);
    const int32_t D = (int32_t)(dict.size() > 65536 ? 65536 : dict.size());
    Skewed out((size_t)D + (size_t)cap, (size_t)D, g_dst_skew, false);
    if (D) memcpy(out.p, dict.data() + dict.size() - D, (size_t)D);
    const int32_t csize = (int32_t)frame.size();
    const uint64_t so = 0, doff = (uint64_t)D;
    int32_t ret = -7777;
    // the decoder reads the input window by aligned dwords (the GPU's word
    // granularity: the dwords holding the first and the last byte); the heap
    // block covers them (at least one byte, a valid pointer for csize 0)
    Skewed in(frame.empty() ? 1 : frame.size(), 0, g_src_skew, true);
    if (!frame.empty()) memcpy(in.p, frame.data(), frame.size());
    // kDecPipe / kDecSmall / kDecGroup / kDecWave
    const char m = argv[1][1];
    const uint32_t mode = m == 'p' ? 2u : (m == 'l' ? 6u : (m == 'g' ? 7u : (m == 'G' ? 9u : 1u)));
    emu_decompress_batch_mode(in.p, &so, &csize, out.p, &doff, &cap, &ret, 1, &D, mode);
    if (!out.ok() || !in.ok()) {
        fprintf(stderr, "emu_main: a store in front of a buffer\n");
        return 3;
    }
    char err[256];
    const int good = emu_decode_results(&ret, 1, err, sizeof err);
    printf("ret %d\nresults %d %s\n", ret, good, err);
    if (argc > 4 && ret > 0) {
        FILE* o = fopen(argv[4], "wb");
        if (!o) return 2;
        fwrite(out.p + D, 1, (size_t)ret, o);
        fclose(o);
    }
    return 0;
}

int main(int argc, char** argv) {
    long cap_arg = -1;
    while (argc > 2 && (!strcmp(argv[1], "--skew") || !strcmp(argv[1], "--cap") || !strcmp(argv[1], "--ring") ||
                        !strcmp(argv[1], "--hbm") || !strcmp(argv[1], "--partial"))) {
        if (!strcmp(argv[1], "--hbm")) {
            g_hbm = true;
            argv[1] = argv[0];
            argv += 1;
            argc -= 1;
            continue;
        }
        if (!strcmp(argv[1], "--partial")) {
            for (const char* q = argv[2]; *q;) {
                char* end = nullptr;
                const long t = strtol(q, &end, 10);
                if (end == q || t < 0 || t > 0x7FFFFFFFL || (*end && *end != ',')) return 2;
                g_partial.push_back((int32_t)t);
                q = *end ? end + 1 : end;
            }
            if (g_partial.empty()) return 2;
        } else if (!strcmp(argv[1], "--ring")) {
            char* end = nullptr;
            const long ring = strtol(argv[2], &end, 10);
            if (!*argv[2] || *end || ring < 0 || ring > 4096) return 2;
            setenv("LZ4E_COMPRESS_RECORDS", argv[2], 1);
        } else if (!strcmp(argv[1], "--cap")) {
            char* end = nullptr;
            cap_arg = strtol(argv[2], &end, 10);
            if (!*argv[2] || *end || cap_arg < 0 || cap_arg > 0x7FFFFFFFL) return 2;
        } else {
            if (sscanf(argv[2], "%u,%u", &g_src_skew, &g_dst_skew) != 2 || g_src_skew > 15 || g_dst_skew > 15)
                return 2;
            g_skewed = true;
        }
        argv[2] = argv[0];
        argv += 2;
        argc -= 2;
    }
    if (argc > 3 && argv[1][0] == '-' &&
        (argv[1][1] == 'd' || argv[1][1] == 'p' || argv[1][1] == 'l' || argv[1][1] == 'g' || argv[1][1] == 'G'))
        return g_partial.empty() ? decode_main(argc, argv) : partial_main(argc, argv);
    if (!g_partial.empty()) return 2;  // --partial is a decode option
    if (argc < 3) {
        fprintf(stderr, "usage: emu_main [--skew S,D] [--cap N] [--ring N] [--hbm] BLOCK_FILE TABLE_CLASS [FRAME_OUT [DICT_FILE]]\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> in;
    int c;
    while ((c = fgetc(f)) != EOF) in.push_back((uint8_t)c);
    fclose(f);
    const uint32_t n = (uint32_t)in.size();
    const uint8_t tt = (uint8_t)atoi(argv[2]);
    const uint32_t cap = cap_arg >= 0 ? (uint32_t)cap_arg : n + n / 255 + 16;
    std::vector<uint8_t> dict;
    if (argc > 4) dict = slurp(argv[4]);
    uint32_t D = (uint32_t)dict.size() > 65536 ? 65536 : (uint32_t)dict.size();
    Skewed src((size_t)D + n, (size_t)D, g_src_skew, true), dst(cap, 0, g_dst_skew, false);
    if (D) memcpy(src.p, dict.data() + dict.size() - D, (size_t)D);
    if (n) memcpy(src.p + D, in.data(), n);
    const uint64_t so = D, doff = 0;
    int32_t ret = -7;
    uint32_t aux[2] = {0, 0};
    const uint32_t max_len = g_hbm && n < 4097 ? 4097 : n;
    if (argc > 4)
        emu_compress_batch_dict(src.p, &so, &n, &tt, dst.p, &doff, &cap, &ret, aux, 1, max_len, &D);
    else
        emu_compress_batch(src.p, &so, &n, &tt, dst.p, &doff, &cap, &ret, aux, 1, max_len);
    if (!dst.ok() || !src.ok()) {
        fprintf(stderr, "emu_main: a store in front of a buffer\n");
        return 3;
    }
    printf("ret %d aux %u %u\n", ret, aux[0], aux[1]);
    if (argc > 3 && ret > 0) {
        FILE* o = fopen(argv[3], "wb");
        if (!o) return 2;
        fwrite(dst.p, 1, (size_t)ret, o);
        fclose(o);
    }
    return 0;
}
