"""The compressor's two-wave blocks on the lane emulator, under ASan + UBSan.

The HBM-image records kernel runs a block that defers its emit as two waves:
wave 0 parses and stores records into a ring, wave 1 (the flusher) writes the
frame from the records wave 0 has published (flusher_wave,
lz4-sgori_amd/csrc/lz4e_compress.hip).  The emulator runs both waves as host
threads that meet through the LDS counters.  emu_main --hbm sends a block of
any size through that kernel (blocks of at most 4 096 bytes otherwise take the
LDS-image kernel, which stays one wave), --ring N sets the ring's slots: with
64 the parser waits for the flusher in every window that found a sequence.
Frames, return values and post-states equal the oracle's.  Only the stand-alone
emu_main program runs; nothing is loaded into Python.
"""
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import flusher_inputs as fi
import oracle_ref
import parse_synth
from lz4e_amd import BYU16
from test_emulator import _JOBS, _build_emu, _family_cases, emu_exe  # noqa: F401

RINGS = [pytest.param(64, id="r64"), pytest.param(128, id="r128"), pytest.param(None, id="default")]
ABORTED = -2**31  # LZ4E_COMPRESS_ABORTED (include/lz4e.h)


def _emu(exe, tmp_path, key, block, tt, ring, dic=b""):
    """One block through emu_main --hbm -> (ret, frame or None, (final_src, last_run))."""
    blk, frame, dct = tmp_path / f"b{key}.bin", tmp_path / f"f{key}.bin", tmp_path / f"d{key}.bin"
    blk.write_bytes(block)
    args = [exe, "--hbm"] + ([] if ring is None else ["--ring", str(ring)]) + [str(blk), str(tt), str(frame)]
    if dic:
        dct.write_bytes(dic)
        args.append(str(dct))
    out = subprocess.run(args, capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0 and "ERROR: AddressSanitizer" not in out.stderr and \
        "runtime error" not in out.stderr, (key, out.returncode, out.stderr[-1500:])
    _, r, _, fs, lr = out.stdout.split()
    return int(r), frame.read_bytes() if frame.exists() else None, (int(fs), int(lr))


def _run(exe, tmp_path, key, block, tt, ring, dic=b""):
    """-> None or what differs from the oracle."""
    r, frame, aux = _emu(exe, tmp_path, key, block, tt, ring, dic)
    if dic:
        er, ef = oracle_ref.compress_dict(block, dic)
        eaux = None
    else:
        er, ef, efs, elr = oracle_ref.compress(block, tt)
        eaux = (efs, elr)
    if r != er:
        return (key, tt, ring, "value", r, er)
    if frame != ef:
        return (key, tt, ring, "frame")
    if eaux is not None and aux != eaux:
        return (key, tt, ring, "post-state", aux, eaux)
    return None


def _all(exe, tmp_path, runs):
    """runs: [(label, block, tt, ring, dic)] -> asserts that none differs."""
    with ThreadPoolExecutor(_JOBS) as ex:
        bad = [b for b in ex.map(lambda kr: _run(exe, tmp_path, kr[0], *kr[1][1:]), enumerate(runs)) if b]
    assert not bad, [(runs[int(b[0])][0],) + b[1:] for b in bad[:5]]


def test_special_blocks_show_what_they_are_built_for():
    fi.check_special_blocks()


@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("family", parse_synth.FAMILIES)
def test_planted_family_two_waves(emu_exe, tmp_path, family, ring):  # noqa: F811
    """Every planted case as a two-wave block; 64 slots: a hand-over in every window."""
    _all(emu_exe, tmp_path, [(c.label, c.block, c.tt, ring, c.dic) for c in _family_cases(family)])


@pytest.mark.parametrize("ring", RINGS)
def test_special_blocks_two_waves(emu_exe, tmp_path, ring):  # noqa: F811
    """Thousands of sequences against a ring of 64 (the parser's ring-full wait
    runs constantly), no sequence at all, blocks on both sides of kMinLength,
    and the literal and match lengths of the wide path and the extensions."""
    _all(emu_exe, tmp_path, [(lb, b, tt, ring, b"") for lb, b, tt in fi.special_blocks()])


@pytest.fixture(scope="module")
def emu_exe_cspin1(tmp_path_factory):
    """Built with a hand-over wait bound of one sleep and no per-byte term."""
    b, exe = _build_emu(tmp_path_factory, "-DLZ4E_CSPIN_MAX=1", "-DLZ4E_CSPIN_PER_BYTE=0")
    yield exe
    shutil.rmtree(b, ignore_errors=True)


def test_forced_expiry_returns_the_documented_value(emu_exe_cspin1, tmp_path):
    """The flusher's wait for the parser's first records gives up after one
    sleep: the block's value is LZ4E_COMPRESS_ABORTED, both waves leave and
    the program ends (emulator only)."""
    r, frame, _ = _emu(emu_exe_cspin1, tmp_path, "x", fi.units(65536, 11), BYU16, 64)
    assert r == ABORTED and frame is None
