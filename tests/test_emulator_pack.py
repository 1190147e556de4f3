"""The packed frame store's kernels' own source on the CPU, under ASan + UBSan.

tools/emu/emu_pack.cpp compiles lz4-sgori_amd/csrc/lz4e_pack.hip unmodified
as host C++ (EMU_PACK=1 tools/emu/build.sh) and runs the four pack kernels,
unpack_mask_kernel and unpack_raw_kernel lane by lane (the decoders that run
between the two are test_emulator.py's).  The kernels read and write the
caller's memory at byte granularity: every frame slot, every source block,
`packed`, every unpack destination and every index array is its own heap
allocation ending exactly at the last byte the contract allows, a frame
entry's source and a raw entry's frame slot are 0 bytes long, so ASan reports
a single byte read or written outside the contract.

What the program runs (it prints "emu_pack ok" and exits 0 only if every case
matched the plain-C restatement inside it):

pack -- entry lengths 0, 1, 15, 16, 17, 31, 33, 511, 512, 4096, 4097, 70000;
every source residue 0..15 against every `packed` residue 0..15 for the
lengths up to 33 (align 1, fillers put each entry at the wanted residue);
align 1, 16, 512, 4096 with the padding compared to zero; all-raw, all-frame
and alternating batches (raw: ret 0, ret == n, ret > n, ret < 0); block
counts 0, 1, T - 1, T, T + 1, 2 T + 1 for the scan tile T = 256, and
64 T + 1, which takes the one-wave scan of the tile sums round twice;
packed_cap equal to the total, total - 1 and 0, the last two leaving
`packed` untouched while the index is complete.

unpack -- the masked lengths (frame: pk_len, anything else: 0); raw entries
with dst_cap = len, len + 9, len - 1 and 0 at every destination and packed
residue; kinds 2 and 255 and a negative length: ret -1, nothing written;
frame entries left alone by the raw kernel.

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
def emu_pack_exe(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("no clang++ for the emulator")
    b = tmp_path_factory.mktemp("emu_pack")
    env = dict(os.environ, EMU_PACK="1", EMU_BUILD=str(b), CXX=CXX)
    env.pop("EMU_EXE", None)
    env.pop("EMU_SG", None)
    subprocess.run(["bash", os.path.join(REPO, "tools", "emu", "build.sh"),
                    "-fsanitize=address,undefined", "-fno-sanitize=alignment",
                    "-fno-sanitize-recover=all"], check=True, env=env, capture_output=True)
    exe = b / "emu_pack"
    assert exe.exists()
    yield str(exe)
    shutil.rmtree(b, ignore_errors=True)


def test_emulated_pack_kernels_sanitized(emu_pack_exe):
    out = subprocess.run([emu_pack_exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr
    assert "FAIL" not in out.stderr
    assert out.stdout.strip() == "emu_pack ok"
