// Lane emulator of the LZ4E compress kernel (debug/test tooling, tools/emu):
// compiles the unmodified kernel source (and csrc/lz4e_wave.h, with
// -DLZ4E_EMU) as host C++ and runs each workgroup as 64 threads per wave
// (emu_harness.h: kEmuThreads).
#include <stdint.h>
#include <string.h>

#include "emu_harness.h"

namespace lz4e {
namespace {
alignas(16) uint32_t smem[(16384 + 65536 + 64) / 4];
}
}  // namespace lz4e

#include "lz4e_compress.hip"

// The emulator launches in block order (no pool for the order's scratch).
// The launch's record buffer (deferred emit) is a heap block of its exact
// size here, and under LZ4E_EMU the LDS-image kernel gets one as well:
// unlimited blocks of any size record and flush by default
// (LZ4E_COMPRESS_RECORDS / emu_main --ring N sets the slots per block, 0 none).
// The HBM-image kernel (blocks above the staging limit, a dictionary, or
// emu_main --hbm) runs as its two waves, parser and flusher: 128 threads that
// meet through the hand-over counters in the emulated LDS.
namespace lz4e {
int launch_order_mode(bool) { return kOrderNever; }
}  // namespace lz4e

// Every kernel of this build (the decoders of emu_dec.cpp included) runs as
// fresh host threads, 64 per wave; before each workgroup the emulated LDS is
// filled, since LDS is not zeroed on the GPU.
const EmuKernelMode emu_modes[] = {{nullptr, kEmuThreads}};
static const bool g_lds_hook = (emu_block_hook = [] { memset(lz4e::smem, 0xA5, sizeof(lz4e::smem)); }, true);

extern "C" int emu_compress_batch(const uint8_t* src, const uint64_t* src_off, const uint32_t* src_len,
                                  const uint8_t* table_type, uint8_t* dst, const uint64_t* dst_off,
                                  const uint32_t* dst_cap, int32_t* ret, uint32_t* aux,
                                  uint32_t nblocks, uint32_t max_len) {
    lz4e::CompressBatch a{src, src_off, src_len, table_type, dst, dst_off, dst_cap, ret, aux,
                          nblocks, max_len};
    return lz4e::launch_compress(a, nullptr) == hipSuccess ? 0 : -1;
}

// Dictionary mode: block i's dictionary is the dict_len[i] bytes before it.
extern "C" int emu_compress_batch_dict(const uint8_t* src, const uint64_t* src_off,
                                       const uint32_t* src_len, const uint8_t* table_type,
                                       uint8_t* dst, const uint64_t* dst_off, const uint32_t* dst_cap,
                                       int32_t* ret, uint32_t* aux, uint32_t nblocks, uint32_t max_len,
                                       const uint32_t* dict_len) {
    lz4e::CompressBatch a{src, src_off, src_len, table_type, dst, dst_off, dst_cap, ret, aux,
                          nblocks, max_len, dict_len};
    return lz4e::launch_compress(a, nullptr) == hipSuccess ? 0 : -1;
}
