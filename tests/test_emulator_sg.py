"""The zero-copy scatter-gather kernels' own source on the CPU, under ASan + UBSan.

tools/emu/emu_sg.cpp compiles lz4-sgori_amd/csrc/lz4e_sg.hip unmodified as
host C++ (EMU_SG=1 tools/emu/build.sh) and runs sg_gather_kernel and
sg_deliver_kernel lane by lane.  These kernels read and write the caller's
registered memory, where the byte after a buffer may be someone else's data
or an unmapped page, so the rule under test is: no load and no store outside
[src, src + n) and [dst, dst + n).  Every source segment and every
destination is its own heap allocation ending exactly at the buffer's last
byte, so ASan reports a single byte of over-read or over-write.

What the program runs (it exits 0 only if every case matched):

gather -- segment lengths 1, 15, 16, 17, 31, 33, 511, 512, 4096, 4097; every
source alignment 0..15 against every destination alignment 0..15 for the
lengths up to 33; all ten lengths as one request; a segment longer than one
descriptor's piece and iterators that start inside a segment; 256 segments
of 16 B; an empty request.  The gathered bytes equal the host gather's
(csrc/lz4e_host.hip sg_gather, restated in the program).

deliver -- success with and without a frame, ret <= 0, dret != len,
frame_cap == ret, frame_cap == ret - 1 and frame_cap == 0, with the same
alignment sweep for the destinations; failing requests leave every
destination byte as it was.

UBSan's alignment check is off, as in test_emulator.py: the kernels'
unaligned 16-byte loads are legal on gfx950 and are emulated as plain loads.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def emu_sg_exe(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("no clang++ for the emulator")
    b = tmp_path_factory.mktemp("emu_sg")
    env = dict(os.environ, EMU_SG="1", EMU_BUILD=str(b), CXX=CXX)
    env.pop("EMU_EXE", None)
    subprocess.run(["bash", os.path.join(REPO, "tools", "emu", "build.sh"),
                    "-fsanitize=address,undefined", "-fno-sanitize=alignment",
                    "-fno-sanitize-recover=all"], check=True, env=env, capture_output=True)
    exe = b / "emu_sg"
    assert exe.exists()
    yield str(exe)
    shutil.rmtree(b, ignore_errors=True)


def test_emulated_sg_kernels_sanitized(emu_sg_exe):
    out = subprocess.run([emu_sg_exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr
    assert "FAIL" not in out.stderr
    assert out.stdout.strip() == "emu_sg ok"
