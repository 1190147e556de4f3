"""The registered-host-memory registry and its C entry points, without a GPU.

csrc/lz4e_hostreg.h decides which requests of lz4e_chunk_write_batch the
device serves straight from the caller's memory: it is plain C++, so a small
stand-alone program around it runs here under ASan + UBSan.  The library's
side needs no GPU either for what is checked here: the symbols exist and
lz4e_register_host_memory refuses bad arguments with -22 before it calls HIP.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/llvm/bin/clang++"

PROGRAM = r"""
#include <stdio.h>
#include "lz4e_hostreg.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); failures++; } } while (0)

int main() {
    using lz4e::HostRegistry;
    const uint64_t NC = HostRegistry::kNotContained;
    auto P = [](uintptr_t a) { return reinterpret_cast<const void*>(a); };
    HostRegistry r;
    CHECK(r.empty());
    CHECK(r.translate(P(0x10000), 1) == NC);
    CHECK(r.translate(P(0x10000), 0) == NC);

    // insert, translate, erase
    CHECK(r.insert(0x10000, 0x4000, 0xA000000));
    CHECK(!r.empty() && r.size() == 1);
    CHECK(r.translate(P(0x10000), 0x4000) == 0xA000000);          // the whole range
    CHECK(r.translate(P(0x10000), 1) == 0xA000000);
    CHECK(r.translate(P(0x10001), 1) == 0xA000001);               // offsets are exact
    CHECK(r.translate(P(0x12345), 0x10) == 0xA002345);
    CHECK(r.translate(P(0x13FFF), 1) == 0xA003FFF);               // the last byte
    CHECK(r.translate(P(0x13FF0), 0x10) == 0xA003FF0);            // ends at the end
    CHECK(r.translate(P(0xFFFF), 1) == NC);                       // one byte before
    CHECK(r.translate(P(0xFFFF), 2) == NC);                       // starts outside
    CHECK(r.translate(P(0x14000), 1) == NC);                      // one byte past
    // straddles the end, no neighbour
    CHECK(r.translate(P(0x13FFF), 2) == NC);
    CHECK(r.translate(P(0x10000), 0x4001) == NC);
    CHECK(r.translate(P(0x13000), 0x2000) == NC);
    // a length that wraps the address space
    CHECK(r.translate(P(0x10010), ~size_t(0)) == NC);
    CHECK(r.translate(P(0x10010), ~size_t(0) - 0x10000) == NC);
    // zero-length lookups: the address itself must lie inside
    CHECK(r.translate(P(0x10000), 0) == 0xA000000);
    CHECK(r.translate(P(0x13FFF), 0) == 0xA003FFF);
    CHECK(r.translate(P(0x14000), 0) == NC);
    CHECK(r.translate(P(0xFFFF), 0) == NC);

    // overlap refused: identical, nested, left-overlapping, right-overlapping, enclosing
    CHECK(!r.insert(0x10000, 0x4000, 1));
    CHECK(!r.insert(0x11000, 0x1000, 1));
    CHECK(!r.insert(0x10000, 0x1000, 1));
    CHECK(!r.insert(0x13000, 0x1000, 1));
    CHECK(!r.insert(0xF000, 0x1001, 1));
    CHECK(!r.insert(0xF000, 0x2000, 1));
    CHECK(!r.insert(0x13000, 0x2000, 1));
    CHECK(!r.insert(0x13FFF, 0x1000, 1));
    CHECK(!r.insert(0xF000, 0x6000, 1));
    CHECK(r.overlaps(0x13FFF, 1) && !r.overlaps(0x14000, 1) && !r.overlaps(0xF000, 0x1000));
    // empty and wrapping ranges refused
    CHECK(!r.insert(0x20000, 0, 1));
    CHECK(!r.insert(UINTPTR_MAX - 0xFFF, 0x2000, 1));
    CHECK(r.size() == 1);
    CHECK(r.translate(P(0x10001), 1) == 0xA000001);  // refused inserts changed nothing

    // adjacent ranges accepted, on both sides; their device addresses are unrelated
    CHECK(r.insert(0x14000, 0x1000, 0x5000000));
    CHECK(r.insert(0xF000, 0x1000, 0x7000000));
    CHECK(r.size() == 3);
    CHECK(r.translate(P(0x14000), 0x1000) == 0x5000000);
    CHECK(r.translate(P(0x14800), 0x800) == 0x5000800);
    CHECK(r.translate(P(0xF000), 0x1000) == 0x7000000);
    CHECK(r.translate(P(0xFFFF), 1) == 0x7000FFF);
    // straddling the end of a registration with an adjacent neighbour: not contained
    CHECK(r.translate(P(0x13FFF), 2) == NC);
    CHECK(r.translate(P(0x13000), 0x2000) == NC);
    CHECK(r.translate(P(0xFFFF), 2) == NC);
    CHECK(r.translate(P(0xF000), 0x6000) == NC);
    CHECK(r.translate(P(0x13FFF), 1) == 0xA003FFF);
    CHECK(r.translate(P(0x14000), 0) == 0x5000000);  // now the neighbour's first byte
    // find() returns the registration that holds an address
    CHECK(r.find(0x13FFF) && r.find(0x13FFF)->base == 0x10000);
    CHECK(r.find(0x14000) && r.find(0x14000)->base == 0x14000);
    CHECK(!r.find(0x15000) && !r.find(0xEFFF));

    // erase takes a base only
    CHECK(!r.erase(0x10001));
    CHECK(!r.erase(0x13FFF));
    CHECK(!r.erase(0x15000));
    CHECK(r.size() == 3);
    CHECK(r.erase(0x10000));
    CHECK(!r.erase(0x10000));
    CHECK(r.translate(P(0x10000), 1) == NC);
    CHECK(r.translate(P(0x13FFF), 1) == NC);
    CHECK(r.translate(P(0x14000), 1) == 0x5000000);  // the neighbours stay
    CHECK(r.translate(P(0xFFFF), 1) == 0x7000FFF);
    // the hole can be registered again, also in pieces
    CHECK(r.insert(0x10000, 0x2000, 0xB000000));
    CHECK(r.insert(0x12000, 0x2000, 0xC000000));
    CHECK(r.translate(P(0x11FFF), 1) == 0xB001FFF);
    CHECK(r.translate(P(0x12000), 1) == 0xC000000);
    CHECK(r.translate(P(0x11FFF), 2) == NC);
    CHECK(r.erase(0xF000) && r.erase(0x10000) && r.erase(0x12000) && r.erase(0x14000));
    CHECK(r.empty());

    // the top of the address space
    CHECK(r.insert(UINTPTR_MAX - 0xFFF, 0x1000, 0x100));
    CHECK(r.translate(P(UINTPTR_MAX), 1) == 0x100 + 0xFFF);
    CHECK(r.translate(P(UINTPTR_MAX), 2) == NC);
    CHECK(r.translate(P(UINTPTR_MAX - 0xFFF), 0x1000) == 0x100);

    if (failures) return 1;
    printf("hostreg ok\n");
    return 0;
}
"""


def test_registry_sanitized(tmp_path):
    """insert / translate / erase, the overlap rules, adjacency, ranges that
    straddle the end of a registration (with and without an adjacent
    neighbour), zero-length lookups and exact offsets, under ASan + UBSan."""
    if not os.path.exists(CXX):
        pytest.skip("no clang++")
    src = tmp_path / "hostreg_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "hostreg_main"
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "lz4-sgori_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr
    assert "hostreg ok" in out.stdout


def test_symbols_exported(amd):
    out = subprocess.run(["nm", "-D", "--defined-only", amd.LIB_PATH], capture_output=True, text=True)
    L = amd.lib()
    for n in ("lz4e_register_host_memory", "lz4e_unregister_host_memory",
              "lz4e_debug_chunk_zero_copy_requests"):
        assert hasattr(L, n)
        assert f" T {n}\n" in out.stdout, n
    assert "lz4e_register_host_memory" in amd.EXPORTED_SYMBOLS
    assert "lz4e_unregister_host_memory" in amd.EXPORTED_SYMBOLS
    # a debug hook, not part of include/lz4e.h
    assert "lz4e_debug_chunk_zero_copy_requests" not in open(os.path.join(REPO, "include", "lz4e.h")).read()
    assert isinstance(amd.zero_copy_requests(), int)


def test_register_rejects_bad_arguments(amd):
    """-22 for NULL, an unaligned pointer, an unaligned length and a zero
    length: decided before HIP is called, so also without a GPU."""
    raw = np.zeros(4 * amd.PAGE_SIZE, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data % amd.PAGE_SIZE)
    L = amd.lib()
    assert L.lz4e_register_host_memory(None, amd.PAGE_SIZE) == -22
    assert L.lz4e_register_host_memory(base + 1, amd.PAGE_SIZE) == -22
    assert L.lz4e_register_host_memory(base + 512, amd.PAGE_SIZE) == -22
    assert L.lz4e_register_host_memory(base, amd.PAGE_SIZE + 1) == -22
    assert L.lz4e_register_host_memory(base, 100) == -22
    assert L.lz4e_register_host_memory(base, 0) == -22
    assert "lz4e_register_host_memory" in amd.last_error()
    # nothing was registered by any of them
    assert L.lz4e_unregister_host_memory(base) == -2
    assert L.lz4e_unregister_host_memory(None) == -2
    if not amd.gpu_available():
        # a good range without a GPU: -1 and the reason, never a registration
        assert L.lz4e_register_host_memory(base, amd.PAGE_SIZE) == -1
        assert "lz4e" in amd.last_error()
        assert L.lz4e_unregister_host_memory(base) == -2
        with pytest.raises(amd.GpuUnavailable):
            with amd.HostArena(amd.PAGE_SIZE):
                pass
