#!/bin/bash
# Line coverage of compress_block on the lane emulator.
#   tools/emu/coverage.sh MANIFEST [JOBS]
# MANIFEST: one emu_main argument list per line, e.g.
#   /tmp/blk7.bin 1
#   --cap 120 /tmp/blk7.bin 3
#   /tmp/blk9.bin 3 /dev/null /tmp/dict9.bin
# Builds emu_main with --coverage into a scratch directory, runs every line
# (JOBS at a time, default 4), runs gcov from the directory the build ran in
# and prints the stripped source text of every line of compress_block that no
# run executed, one per line (with "[i of n]" after a text that occurs n times), without the lines that exist only in the stamped
# or traced builds (kStamps, LZ4E_TR).  tests/golden/compress_unreached.txt
# lists the lines that are expected here, with a reason each.
set -e
set -o pipefail
here=$(cd "$(dirname "$0")" && pwd)
manifest=$(cd "$(dirname "$1")" && pwd)/$(basename "$1")
jobs=${2:-4}
GCOV=${GCOV:-gcov}
work=$(mktemp -d "${TMPDIR:-/tmp}/emucov.XXXXXX")
trap 'rm -rf "$work"' EXIT
cd "$work"
EMU_EXE=1 EMU_BUILD="$work" bash "$here/build.sh" --coverage >&2
# the runs add their counts to the same .gcda files (the profile runtime locks them)
xargs -a "$manifest" -P "$jobs" -L 1 "$work/emu_main" > "$work/runs.out"
"$GCOV" -o "$work" "$work"/emu_main-emu.gcda > "$work/gcov.out" 2>&1 || { cat "$work/gcov.out" >&2; exit 1; }
# gcov prints a line once with the counts of all instantiations added up, and
# again per instantiation for function heads: the first print of a line counts.
awk '
    {
        split($0, f, ":")
        no = f[2] + 0
        if (no == 0 || (no in first)) next
        first[no] = 1
        text = $0
        sub(/^[^:]*:[^:]*:/, "", text)
        if (text ~ /LZ4E_DEV CResult compress_block\(/) inside = 1
        if (!inside) next
        if (text ~ /^}/) { inside = 0; next }
        gsub(/^[ \t]+|[ \t]+$/, "", text)
        n++
        line[n] = text
        missed[n] = (f[1] ~ /#####|=====/)
        ord[n] = ++count[text]
    }
    END {
        for (i = 1; i <= n; i++) {
            t = line[i]
            if (!missed[i] || t ~ /kStamps|LZ4E_TR/) continue
            # a text that occurs several times in compress_block is told apart by its ordinal
            print (count[t] > 1 ? t "  [" ord[i] " of " count[t] "]" : t)
        }
    }
' "$work/lz4e_compress.hip.gcov"
