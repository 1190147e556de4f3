#!/bin/bash
# Builds the lane emulator: the kernels run on host threads, with the
# product's own csrc/lz4e_wave.h (compiled with -DLZ4E_EMU; the amdgcn
# builtins come from tools/emu/include/hip/hip_runtime.h).  Every target is
# its sources and the harness (emu_harness.cpp).
#   tools/emu/build.sh [flags...]         -> $EMU_BUILD/libemu.so (default tools/emu/build):
#                                            the compress kernel and the decoders
#   EMU_EXE=1 tools/emu/build.sh [flags]  -> $EMU_BUILD/emu_main (the same, standalone)
#   EMU_SG=1 tools/emu/build.sh [flags]   -> $EMU_BUILD/emu_sg (standalone: the
#                                            zero-copy kernels of csrc/lz4e_sg.hip)
#   EMU_PACK=1 tools/emu/build.sh [flags] -> $EMU_BUILD/emu_pack (standalone: the
#                                            packed frame store's kernels,
#                                            csrc/lz4e_pack.hip)
#   EMU_CRC=1 tools/emu/build.sh [flags]  -> $EMU_BUILD/emu_crc (standalone: the
#                                            store's checksum kernels,
#                                            csrc/lz4e_crc.hip)
# Pass extra flags, e.g. -fsanitize=address,undefined or -DLZ4E_SPIN_MAX=1.
set -e
here=$(cd "$(dirname "$0")" && pwd)
csrc="$here/../../lz4-sgori_amd/csrc"
b="${EMU_BUILD:-$here/build}"
mkdir -p "$b"
CXX=${CXX:-/opt/rocm/llvm/bin/clang++}
t=libemu.so
[ -n "$EMU_EXE" ] && t=emu_main
[ -n "$EMU_SG" ] && t=emu_sg
[ -n "$EMU_PACK" ] && t=emu_pack
[ -n "$EMU_CRC" ] && t=emu_crc
case $t in  # target -> sources, what else its command line needs
    libemu.so) srcs=(emu.cpp emu_dec.cpp); extra=(-fPIC -shared) ;;
    emu_main)  srcs=(emu.cpp emu_dec.cpp emu_main.cpp); extra=() ;;
    *)         srcs=("$t.cpp"); extra=(-I "$here/../../include") ;;  # include/lz4e.h
esac
$CXX -std=c++20 -O1 -g -pthread -x c++ -DLZ4E_EMU -I "$here/include" -I "$csrc" "${extra[@]}" "$@" \
    "${srcs[@]/#/$here/}" "$here/emu_harness.cpp" -o "$b/$t"
echo "built $b/$t"
