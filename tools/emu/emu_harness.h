// The lane emulator's harness (debug/test tooling, tools/emu): what its five
// programs -- libemu.so, emu_main, emu_sg, emu_pack, emu_crc -- share, each
// thing once.  emu_harness.cpp defines the emulated-thread globals that
// <hip/hip_runtime.h> declares, emu_launch and the failure count; this header
// has the sanitizer's poison macros, the kernel mode table's types, CHECK,
// the generator's step and Buf.
//
// How a kernel runs.  The shim's hipLaunchKernelGGL hands the kernel's name to
// emu_launch, which looks it up in the program's emu_modes table (by the exact
// name; the entry with a null name is the default) and runs the grid's
// workgroups one after the other in that mode:
//   kEmuThreads  fresh host threads per workgroup, 64 per wave, any number of
//                waves (the compressor and the decoders);
//   kEmuPool     a workgroup of 1 to 4 waves on 256 lane threads that live as
//                long as the program (thousands of small launches: a fresh
//                set of threads for each was most of the run time); for
//                kernels with cross-lane operations or barriers;
//   kEmuSerial   all lanes one after the other on the calling thread, no wave
//                state: only for kernels with neither;
//   kEmuNone     the program does not run this kernel: a launch aborts.
// A name with no entry in a table without a default aborts as well.
// (How to put a new kernel file under the emulator: DESIGN.md, section 4.)
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include <hip/hip_runtime.h>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#define EMU_POISON(p, n) __asan_poison_memory_region((p), (n))
#define EMU_UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#endif
#endif
#ifndef EMU_POISON
#define EMU_POISON(p, n) ((void)0)
#define EMU_UNPOISON(p, n) ((void)0)
#endif

enum EmuMode { kEmuNone, kEmuThreads, kEmuPool, kEmuSerial };
struct EmuKernelMode {
    const char* kernel;  // nullptr: the table's last entry, the mode of every name not listed
    EmuMode mode;
};
extern const EmuKernelMode emu_modes[];  // each program's, next to its main
extern void (*emu_block_hook)();         // runs before every workgroup, if set
extern uint64_t g_groups_run;            // workgroups that kEmuPool has run

extern int g_failures;
#define CHECK(c, ...)                        \
    do {                                     \
        if (!(c)) {                          \
            fprintf(stderr, "FAIL: " __VA_ARGS__); \
            fprintf(stderr, "\n");           \
            g_failures++;                    \
        }                                    \
    } while (0)
// The end of main: "<program> ok" and 0, or the failure count and 1.
int emu_finish(const char* program);

// The generator's step.  Each program has a sequence of its own: it names its
// seed, and in rnd() the bits it takes.
inline uint32_t emu_lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
uint8_t rnd();

constexpr uint8_t kCanary = 0xC3, kFill = 0x5A;

// n bytes at alignment `align` (mod 16), ending where their heap block ends
// (ASan's redzone follows).  The whole 8-byte granules of the `align` bytes in
// front are poisoned; the up to 7 left (ASan cannot poison the front of a
// granule) hold a canary.
struct Buf {
    uint8_t* base;
    uint8_t* p;
    size_t align, n;
    Buf(size_t align_, size_t n_) : align(align_ & 15), n(n_) {
        base = static_cast<uint8_t*>(malloc(align + n));
        if (!base) abort();
        p = base + align;
        memset(base, kCanary, align);
        EMU_POISON(base, align & ~size_t(7));
    }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() {
        EMU_UNPOISON(base, align & ~size_t(7));
        free(base);
    }
    void fill_random() {
        for (size_t i = 0; i < n; ++i) p[i] = rnd();
    }
    void fill(uint8_t v) { memset(p, v, n); }
    bool all(uint8_t v) const {
        for (size_t i = 0; i < n; ++i)
            if (p[i] != v) return false;
        return true;
    }
    bool canary_ok() const {
        for (size_t i = align & ~size_t(7); i < align; ++i)
            if (base[i] != kCanary) return false;
        return true;
    }
    template <class T>
    T* as() {
        return reinterpret_cast<T*>(p);
    }
};
typedef std::unique_ptr<Buf> BufP;

// The lowest address of a set of buffers: the batch's base pointer, so that
// every offset is a forward one.
inline const uint8_t* lowest(const std::vector<BufP>& v) {
    const uint8_t* lo = nullptr;
    for (const BufP& b : v)
        if (!lo || b->p < lo) lo = b->p;
    return lo;
}
