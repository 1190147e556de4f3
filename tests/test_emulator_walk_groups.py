"""The parser's chain walk and clash groups on the lane emulator, under ASan + UBSan.

The blocks of tests/walk_group_inputs.py through the kernels' own source
(tools/emu, the stand-alone emu_main program; nothing is loaded into Python):
as they are through the LDS-image kernel, with --hbm through the HBM-image
kernel's two waves, and both again with an output one byte under the bound,
which emits inline and walks exactly; the same blocks padded to 4 097..8 192
bytes take the HBM-image kernel by their size.  The clash groups' exchange
(group_lanes: a store, a 64-bit atomic OR and a load per lane in the emulated
LDS) runs in every window with a shared hash, the walk's one-bit test in every
fast chain.  Frames, return values and post-states equal the oracle's.
"""
import subprocess
from concurrent.futures import ThreadPoolExecutor

import oracle_ref
import parse_synth as ps
import walk_group_inputs as wg
from lz4e_amd import BYU16, BYU32
from test_emulator import _JOBS, _planted_run, emu_exe  # noqa: F401


def _run(exe, tmp_path, key, label, block, tt, hbm, cap):
    """One block through emu_main -> None or what differs from the oracle."""
    if not hbm:
        bad = _planted_run(exe, tmp_path, key, ps.Case(label, block, tt, b"", [], []), cap=cap)
        return bad and (label,) + tuple(bad[1:])
    blk, frame = tmp_path / f"b{key}.bin", tmp_path / f"f{key}.bin"
    blk.write_bytes(block)
    args = [exe, "--hbm"] + (["--cap", str(cap)] if cap is not None else []) + [str(blk), str(tt), str(frame)]
    out = subprocess.run(args, capture_output=True, text=True, timeout=1200)
    if out.returncode != 0 or "ERROR: AddressSanitizer" in out.stderr or "runtime error" in out.stderr:
        return (label, tt, cap, "hbm", out.returncode, out.stderr[-1500:])
    _, r, _, fs, lr = out.stdout.split()
    er, ef, efs, elr = oracle_ref.compress(block, tt, cap)
    if int(r) != er:
        return (label, tt, cap, "hbm", "value", int(r), er)
    if er > 0 and frame.read_bytes() != ef:
        return (label, tt, cap, "hbm", "frame")
    if er > 0 and (int(fs), int(lr)) != (efs, elr):
        return (label, tt, cap, "hbm", "post-state", (int(fs), int(lr)), (efs, elr))
    return None


def _all(exe, tmp_path, runs):
    """runs: [(label, block, tt, hbm, cap)] -> asserts that none differs."""
    with ThreadPoolExecutor(_JOBS) as ex:
        bad = [b for b in ex.map(lambda kr: _run(exe, tmp_path, kr[0], *kr[1]), enumerate(runs)) if b]
    assert not bad, bad[:5]


def test_inputs_show_what_they_are_built_for():
    """The oracle's parse of the inputs: a period-k block is one match at
    offset k, a walk block holds its 8 planted chains, a
    collider block's members share a slot and differ."""
    for tt in ps.CLASSES:
        for label, b, _ in wg.period_blocks(tt):
            seqs, _ = ps.parse_frame(oracle_ref.compress(b, tt)[1])
            if label.startswith("period-") and label[7:].isdigit() and int(label[7:]) < 60:
                assert seqs and seqs[0][2] == int(label[7:]), (label, tt, seqs[:2])
    for tt in (BYU16, BYU32):
        for label, b, _ in wg.walk_blocks(tt):
            seqs, _ = ps.parse_frame(oracle_ref.compress(b, tt)[1])
            # per shift: the restart and the planted ones (a chance hash hit may merge two)
            planted = int(label.split("-")[1]) if label.split("-")[1].isdigit() else 24
            assert len(seqs) >= 8 * (planted + 1) - 3, (label, tt, len(seqs), planted)
        lb, b, _ = wg.group_blocks(tt)[-1]
        w = ps.hash_width(tt)
        assert lb == "groups-colliders"
        assert len({ps.hash_at(b, 1 + ln, tt) for ln in (5, 19, 37)}) == 1
        assert len({b[1 + ln:1 + ln + w] for ln in (5, 19, 37)}) == 3


def test_small_blocks_lds_image_kernel(emu_exe, tmp_path):  # noqa: F811
    """At most 4 096 bytes: the LDS-image kernel, deferred and (one byte under
    the bound) inline."""
    runs = []
    for label, b, tt in wg.all_small():
        runs += [(label, b, tt, False, None), (label, b, tt, False, ps.bound(len(b)) - 1)]
    _all(emu_exe, tmp_path, runs)


def test_small_blocks_hbm_image_two_waves(emu_exe, tmp_path):  # noqa: F811
    """The same blocks through the HBM-image kernel: parser and flusher, and
    (one byte under the bound) the parser alone emitting inline."""
    runs = []
    for label, b, tt in wg.all_small():
        runs += [(label, b, tt, True, None), (label, b, tt, True, ps.bound(len(b)) - 1)]
    _all(emu_exe, tmp_path, runs)


def test_padded_blocks_take_the_hbm_image_kernel_by_size(emu_exe, tmp_path):  # noqa: F811
    """4 097..8 192 bytes, byU16: the launch picks the HBM-image kernel itself."""
    runs = []
    for i, (label, b, tt) in enumerate(wg.hbm(BYU16)):
        assert 4097 <= len(b) <= 8192
        runs.append((label, b, tt, False, ps.bound(len(b)) - 1 if i % 4 == 3 else None))
    _all(emu_exe, tmp_path, runs)
