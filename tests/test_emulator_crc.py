"""The store's checksum kernels' own source on the CPU, under ASan + UBSan.

tools/emu/emu_crc.cpp compiles lz4-sgori_amd/csrc/lz4e_crc.hip unmodified as
host C++ (EMU_CRC=1 tools/emu/build.sh) and runs crc_team_kernel (a workgroup
of it is 256 host threads: it fills a table in LDS behind a barrier and XORs
across lanes), crc_combine_kernel, unpack_verify_mask_kernel and
unpack_verify_ret_kernel; lz4e_pack.hip's raw copy runs between the last two,
the decoders' part is played by a stand-in.  The kernels read the caller's
memory at byte granularity: every entry is its own heap allocation ending
exactly at its last byte, so ASan reports a single byte read outside the
contract.  Expected values come from a bitwise CRC-32C inside the program.

What the program runs (it prints "emu_crc ok" and exits 0 only if every case
matched):

crc32c -- entry lengths 0, 1, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 511,
512, 4096, 4097, 70000 and a negative one, with hints 1, 70000 and 0x7E000000
on the same batch (the last splits every entry over 64 workgroups); every
start residue 0..15 for the lengths up to 65, with four hints; for every team
size the launcher can pick (16 ... 16384 threads, the sizes above 256 span
workgroups) one byte under, at and over one 16-byte vector per thread, the
hint's 64 bytes per thread, and the lengths at which a wave's 64 and a
workgroup's 256 threads are just busy; the same bytes between different
neighbours; 0, 1 ... 5, 15, 16, 17, 33 entries with 16, 4, 2 and 1 entries to
a workgroup and with two workgroups to an entry.

pack_crc -- frame and raw entries of every length; a frame entry's source and
a raw entry's frame slot are allocations of 0 bytes.

verified unpack -- clean frame and raw entries, a wrong pk_crc on each, a raw
entry over capacity with a good and with a bad checksum, kinds 2 and 255 and
negative lengths whose pk_off points outside every allocation; masked
lengths, ret and every destination byte.

UBSan's alignment check is off, as in test_emulator_pack.py: the kernels'
unaligned 16-byte loads are legal on gfx950 and are emulated as plain loads.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def emu_crc_exe(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("no clang++ for the emulator")
    b = tmp_path_factory.mktemp("emu_crc")
    env = dict(os.environ, EMU_CRC="1", EMU_BUILD=str(b), CXX=CXX)
    for other in ("EMU_EXE", "EMU_SG", "EMU_PACK"):
        env.pop(other, None)
    subprocess.run(["bash", os.path.join(REPO, "tools", "emu", "build.sh"),
                    "-fsanitize=address,undefined", "-fno-sanitize=alignment",
                    "-fno-sanitize-recover=all"], check=True, env=env, capture_output=True)
    exe = b / "emu_crc"
    assert exe.exists()
    yield str(exe)
    shutil.rmtree(b, ignore_errors=True)


def test_emulated_crc_kernels_sanitized(emu_crc_exe):
    out = subprocess.run([emu_crc_exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr
    assert "FAIL" not in out.stderr
    assert out.stdout.strip() == "emu_crc ok"
