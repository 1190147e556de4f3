// The lane emulator's harness: what a program defines once (emu_harness.h).
#include "emu_harness.h"

#include <thread>

thread_local EmuWave* g_emu_wave;
thread_local uint32_t g_emu_lane;
thread_local EmuBarrier* g_emu_group;
dim3 blockIdx, gridDim;
thread_local dim3 threadIdx;

void (*emu_block_hook)() = nullptr;
uint64_t g_groups_run = 0;
int g_failures = 0;

int emu_finish(const char* program) {
    if (g_failures) {
        fprintf(stderr, "%s: %d failures\n", program, g_failures);
        return 1;
    }
    printf("%s ok\n", program);
    return 0;
}

namespace {
void enter_lane(EmuWave* waves, EmuBarrier* group, uint32_t t) {
    g_emu_wave = waves ? &waves[t / 64] : nullptr;
    g_emu_lane = t % 64;
    g_emu_group = group;
    threadIdx = dim3(t);
}

constexpr uint32_t kPoolLanes = 256;
struct LanePool {
    EmuBarrier start{kPoolLanes + 1}, end{kPoolLanes + 1};
    EmuWave waves[kPoolLanes / 64];
    EmuBarrier* group = nullptr;  // of the launch's `threads` lanes; the others sit the launch out
    uint32_t threads = 0;
    std::function<void()>* body = nullptr;
    bool quit = false;
    std::vector<std::thread> th;
    LanePool() {
        for (uint32_t t = 0; t < kPoolLanes; ++t)
            th.emplace_back([this, t]() {
                for (;;) {
                    start.arrive_and_wait();
                    if (quit) return;
                    if (t < threads) {
                        enter_lane(waves, group, t);
                        (*body)();
                    }
                    end.arrive_and_wait();
                }
            });
    }
    ~LanePool() {
        quit = true;
        start.arrive_and_wait();
        for (auto& x : th) x.join();
    }
};

EmuMode mode_of(const char* kernel) {
    const EmuKernelMode* m = emu_modes;
    while (m->kernel && strcmp(m->kernel, kernel) != 0) ++m;
    return m->mode;
}
}  // namespace

void emu_launch(const char* kernel, uint32_t nblocks, uint32_t threads, std::function<void()> body) {
    const EmuMode mode = mode_of(kernel);
    const uint32_t nw = (threads + 63) / 64;
    if (mode == kEmuNone || (mode == kEmuPool && (threads % 64 != 0 || threads > kPoolLanes))) {
        fprintf(stderr, "emu_launch: this program has no mode for %s with %u threads\n", kernel, threads);
        abort();
    }
    gridDim = dim3(nblocks);
    for (uint32_t b = 0; b < nblocks; ++b) {
        blockIdx = dim3(b);
        if (emu_block_hook) emu_block_hook();
        if (mode == kEmuSerial) {
            for (uint32_t t = 0; t < threads; ++t) {
                enter_lane(nullptr, nullptr, t);
                body();
            }
        } else if (mode == kEmuPool) {
            static LanePool pool;
            EmuBarrier group((std::ptrdiff_t)threads);
            pool.group = &group;
            pool.threads = threads;
            pool.body = &body;
            pool.start.arrive_and_wait();
            pool.end.arrive_and_wait();
            ++g_groups_run;
        } else {
            std::unique_ptr<EmuWave[]> waves(new EmuWave[nw]);
            EmuBarrier group((std::ptrdiff_t)(64 * nw));
            std::vector<std::thread> th;
            for (uint32_t t = 0; t < 64 * nw; ++t)
                th.emplace_back([&, t]() {
                    enter_lane(waves.get(), &group, t);
                    body();
                });
            for (auto& x : th) x.join();
        }
    }
}
