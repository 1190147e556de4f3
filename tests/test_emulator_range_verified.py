"""The verified range read's composition on the CPU, under ASan + UBSan.

`emu_crc rangev` (tools/emu/emu_crc.cpp, built by EMU_CRC=1
tools/emu/build.sh from the unmodified lz4-sgori_amd/csrc/lz4e_crc.hip and
lz4e_pack.hip) issues lz4e_unpack_range_verified_batch_dev's launches one for
one -- init, elect, the checksum (crc_team_kernel on 256 host threads per
workgroup, crc_combine_kernel), verdict, range_gather_kernel, a stand-in for
the decoders that takes a frame's bytes for its data, range_deliver_kernel,
ret.  Every entry is a heap allocation of exactly its length, every scratch
array one of exactly its size, every destination one of exactly the bytes its
request must get, so a byte read or written outside the contract is an ASan
report; an entry that must not be read has an offset outside every allocation.
Expected values come from a bitwise CRC-32C and a plain loop inside the
program, which prints "emu_crc rangev ok" and exits 0 only if all matched:

  * entry lengths 0, 1, 15, 16, 17, 300, 4097 and 70000, frame and raw, each
    clean and damaged (a wrong pk_crc, a flipped bit in the first byte, in the
    last), five ranges of each interleaved at random; hints 1, 70000 and
    0x7E000000 on one batch (8 and 64 workgroups per request: partials and
    the combine), hint 0, and a max_end that clamps;
  * entries nobody names, a damaged entry named only by len == 0 requests,
    kinds 2 and 255 and negative lengths, all with offsets that point nowhere;
    invalid requests on a damaged entry and past the index;
  * 1, 2, 17 and 300 requests on one clean entry interleaved with as many on
    a damaged one, every third of those with len == 0;
  * 1, 255, 256 and 257 entries, null sel (also with the last entry unnamed)
    and a random sel with repeats;
  * no request, with and without entries: nothing runs;
  * after every call: one owner per wanted entry, and no other request
    describes a byte to the checksum; ret, every destination byte, the bytes
    in front of every destination and of every entry.

UBSan's alignment check is off, as in test_emulator_crc.py.
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
    b = tmp_path_factory.mktemp("emu_rangev")
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


def test_emulated_verified_range_read_sanitized(emu_crc_exe):
    out = subprocess.run([emu_crc_exe, "rangev"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr
    assert "FAIL" not in out.stderr
    assert out.stdout.strip() == "emu_crc rangev ok"
