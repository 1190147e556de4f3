"""The compressor's deferred emit on the lane emulator, under ASan + UBSan.

The emulator runs unlimited blocks through the record buffer by default (the
LDS-image kernel too, which the GPU build leaves inline), so tests/test_emulator.py
already compares the deferred frames with the oracle at the default number of
record slots.  Here emu_main --ring N sets it: 64 slots (a flush in every
window that found a sequence) and 128 for every planted family, and 0 (no
record buffer: the inline fast-chain emit, which no default run reaches any
more) for two cases of each.  The record buffer is a heap block of exactly
nblocks x N x 8 bytes, so ASan sees a record stored past it.
"""
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_ref
import parse_synth
from lz4e_amd import BYU16, BYU32, BYU64, corpus
from test_emulator import _JOBS, _family_cases, _one_per_family, emu_exe  # noqa: F401


def _run(exe, tmp_path, key, block, tt, ring, dic=b""):
    """One block through emu_main --ring against the oracle -> None or what differs."""
    blk, frame, dct = tmp_path / f"b{key}.bin", tmp_path / f"f{key}.bin", tmp_path / f"d{key}.bin"
    blk.write_bytes(block)
    args = [exe, "--ring", str(ring), str(blk), str(tt), str(frame)]
    if dic:
        dct.write_bytes(dic)
        args.append(str(dct))
    out = subprocess.run(args, capture_output=True, text=True, timeout=1200)
    if out.returncode != 0 or "ERROR: AddressSanitizer" in out.stderr or "runtime error" in out.stderr:
        return (key, tt, ring, out.returncode, out.stderr[-1500:])
    _, r, _, fs, lr = out.stdout.split()
    if dic:
        er, ef = oracle_ref.compress_dict(block, dic)
        eaux = None
    else:
        er, ef, efs, elr = oracle_ref.compress(block, tt)
        eaux = (efs, elr)
    if int(r) != er:
        return (key, tt, ring, "value", int(r), er)
    if frame.read_bytes() != ef:
        return (key, tt, ring, "frame")
    if eaux is not None and (int(fs), int(lr)) != eaux:
        return (key, tt, ring, "post-state", (int(fs), int(lr)), eaux)
    return None


def _all(exe, tmp_path, runs):
    """runs: [(label, block, tt, ring, dic)] -> asserts that none differs."""
    with ThreadPoolExecutor(_JOBS) as ex:
        bad = [b for b in ex.map(lambda kr: _run(exe, tmp_path, f"{kr[0]}", *kr[1][1:]), enumerate(runs)) if b]
    assert not bad, [(runs[int(b[0])][0],) + b[1:] for b in bad[:5]]


@pytest.mark.parametrize("ring", [64, 128])
@pytest.mark.parametrize("family", parse_synth.FAMILIES)
def test_planted_family_with_ring(emu_exe, tmp_path, family, ring):  # noqa: F811
    _all(emu_exe, tmp_path, [(c.label, c.block, c.tt, ring, c.dic) for c in _family_cases(family)])


def test_planted_inline_emit_without_ring(emu_exe, tmp_path):  # noqa: F811
    """--ring 0: the launch has no record buffer and every block emits inline."""
    runs = [(c.label, c.block, c.tt, 0, c.dic) for f in parse_synth.FAMILIES for c in _one_per_family(f)]
    _all(emu_exe, tmp_path, runs)


def test_long_blocks_flush_many_times(emu_exe, tmp_path):  # noqa: F811
    """Text, records, long runs and random bytes above the staging limit (the
    HBM-image kernel), thousands of sequences through 64 and 128 slots, and
    through none."""
    rng = np.random.default_rng(77)
    runs_of = np.concatenate([np.full(int(rng.integers(300, 3000)), v, np.uint8) for v in range(12)])
    blocks = [("text", corpus.text_proxy(20000, 5).tobytes(), BYU16),
              ("records", corpus._records(16384, rng).tobytes(), BYU32),
              ("runs", runs_of.tobytes(), BYU64),
              ("random", rng.integers(0, 256, 9000, dtype=np.uint8).tobytes(), BYU16)]
    _all(emu_exe, tmp_path, [(lb, b, tt, ring, b"") for lb, b, tt in blocks for ring in (64, 128, 0)])
