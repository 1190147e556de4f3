"""Partial decoding through the kernels' own sources on the CPU, under ASan +
UBSan (tools/emu, see tests/test_emulator.py).

emu_main --partial T1,T2,... decodes one frame once per target, each into a
heap block of exactly the target's size, so a store past the target -- the one
thing a partial decode must never do -- is an ASan report.  Values and bytes
must equal tests/partial_model.py on the one-wave decoder (-d), its LDS form
(-l) and the pipelined decoder (-p); the group decoder is refused.

Targets: every k from 0 to n + 19 for the 300-byte `boundary` case and the
600-byte text block; partial_model.sampled_targets (k < 40, |k - n| < 20 and
60 seeded values) for the 2 000-, 4 500- and 20 000-byte cases.  Two sets are
smaller than that, because a decode here costs a third of a second of 64 or
256 host threads: the hand-built frames run at the 31 targets listed in
test_hand_built_frames (every cut the model test names, the copies' 16- and
64-byte piece boundaries and both sides of each frame's end), and the picked
`invalid` and `ends` frames at 7 targets around their capacity.  The GPU tests
run all of these at the full sampled set."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import frame_synth
import partial_model
from test_emulator import _build_emu

_JOBS = max(1, min(8, os.cpu_count() or 1))
# The pipelined decoder is 256 host threads a block: its processes run one at
# a time, as in tests/test_emulator.py (several at once gain nothing on a few
# CPUs), the one-wave processes _JOBS at a time.
_JOBS_PIPE = 1
_CHUNK = 40  # targets per process
# A process of _CHUNK decodes takes from 10 s (small frames) to about 100 s
# (the 20 000-byte frame on the pipelined decoder); one that is still running
# after this long is reported as stuck instead of holding the suite.
_STUCK_S = 900
FLAGS = ["-d", "-l", "-p"]


@pytest.fixture(scope="module")
def emu_partial_exe(tmp_path_factory):
    b, exe = _build_emu(tmp_path_factory)
    yield exe
    shutil.rmtree(b, ignore_errors=True)


def _run(exe, tmp_path, key, label, frame, flag, targets, skew):
    """One process: the frame at every target -> None or what differs."""
    f, o = tmp_path / f"f{key}.bin", tmp_path / f"o{key}"
    f.write_bytes(frame)
    args = [exe, "--partial", ",".join(str(k) for k in targets)]
    if skew is not None:
        args += ["--skew", "%d,%d" % skew]
    try:
        out = subprocess.run(args + [flag, str(f), "0", str(o)], capture_output=True, text=True, timeout=_STUCK_S)
    except subprocess.TimeoutExpired as e:
        done = (e.stdout or b"").decode(errors="replace").strip().split("\n")[-1:]
        return (label, flag, skew, "stuck: no end after %d s; last line" % _STUCK_S, done, targets)
    if out.returncode != 0 or "ERROR: AddressSanitizer" in out.stderr or "runtime error" in out.stderr:
        return (label, flag, skew, out.returncode, out.stdout[-200:], out.stderr[-1500:])
    lines = out.stdout.strip().split("\n")
    if len(lines) != len(targets):
        return (label, flag, "lines", len(lines), len(targets))
    for k, line in zip(targets, lines):
        w = line.split()
        if w[0] != "target" or int(w[1]) != k:
            return (label, flag, "output", line)
        r, want = int(w[3]), partial_model.decode(frame, k, True)
        if r != want[0]:
            return (label, flag, skew, "value", k, r, want[0])
        p = tmp_path / f"o{key}.{k}"
        if r > 0 and p.read_bytes() != want[1]:
            return (label, flag, skew, "bytes", k)
    return None


def _run_all(exe, tmp_path, work):
    """work: [(label, frame, flag, targets)] -> asserts that nothing differs."""
    jobs = []
    for label, frame, flag, targets in work:
        for c in range(0, len(targets), _CHUNK):
            k = len(jobs)
            skew = None if k % 3 == 0 else (k % 16, (5 * k + 3) % 16)
            jobs.append((k, label, frame, flag, targets[c:c + _CHUNK], skew))
    pipe = any(j[3] == "-p" for j in jobs)
    with ThreadPoolExecutor(_JOBS_PIPE if pipe else _JOBS) as ex:
        bad = [b for b in ex.map(lambda j: _run(exe, tmp_path, *j), jobs) if b]
    assert not bad, (len(bad), bad[:4])


def _case(size):
    return next(c for c in frame_synth.cases("boundary") if c.label.endswith("-0") and abs(c.cap - size) < size // 4)


@pytest.mark.parametrize("flag", FLAGS)
def test_every_target_of_two_small_frames(emu_partial_exe, tmp_path, flag):
    c = _case(300)
    name, data, frame = partial_model.oracle_blocks()[0]
    _run_all(emu_partial_exe, tmp_path, [(c.label, c.frame, flag, list(range(0, c.cap + 20))),
                                         (name, frame, flag, list(range(0, len(data) + 20)))])


@pytest.mark.parametrize("flag", FLAGS)
def test_hand_built_frames(emu_partial_exe, tmp_path, flag):
    work = []
    for name, (frame, full) in partial_model.hand_frames().items():
        n = len(full)
        ks = sorted({0, 1, 11, 12, 13, 19, 20, 21, 22, 23, 24, 35, 36, 37, 83, 84, 85, 147, 148, 292, 300,
                     524, 525, 526, 548, 549, 550, n - 1, n, n + 1, n + 19})
        work.append((name, frame, flag, ks))
    for f in (b"\x00", b"\x10a", b"\xf0\x05" + b"a" * 14, b"\x50abc", b"\x10a\x05\x00zzzz",
              b"\x1fa\x01\x00\xff\x00\x00"):
        work.append(("error-site", f, flag, [0, 1, 2, 3, 4, 10, 20, 64]))
    _run_all(emu_partial_exe, tmp_path, work)


@pytest.mark.parametrize("flag", FLAGS)
def test_sampled_targets_of_larger_frames(emu_partial_exe, tmp_path, flag):
    work = []
    for size in (2000, 4500):
        c = _case(size)
        work.append((c.label, c.frame, flag, partial_model.sampled_targets(c.cap, size)))
    for label in ("invalid-offset-k63", "invalid-literal-ext-cut-255", "invalid-match-past-cap-68-6",
                  "ends-l4-m12-c32", "ends-l0-m4-c0"):
        c = next(c for p in ("invalid", "ends") for c in frame_synth.cases(p) if c.label == label)
        work.append((c.label, c.frame, flag, sorted({0, 1, 7, c.cap // 2, max(c.cap - 13, 0), c.cap, c.cap + 5})))
    _run_all(emu_partial_exe, tmp_path, work)


@pytest.mark.parametrize("flag", ["-d", "-p"])
def test_sampled_targets_of_a_20000_byte_frame(emu_partial_exe, tmp_path, flag):
    c = frame_synth.cases("boundary", large=True)[0]
    assert 15000 < c.cap < 25000
    _run_all(emu_partial_exe, tmp_path,
             [(c.label, c.frame, flag, partial_model.sampled_targets(c.cap, 5))])


@pytest.mark.parametrize("flag", ["-g", "-G"])
def test_group_decoder_is_refused(emu_partial_exe, tmp_path, flag):
    f = tmp_path / "f.bin"
    f.write_bytes(b"\x10a")
    out = subprocess.run([emu_partial_exe, "--partial", "1", flag, str(f), "0"], capture_output=True, text=True)
    assert out.returncode == 2 and "no partial form" in out.stderr


def test_range_kernels_sanitized(tmp_path_factory):
    """The range read's gather and deliver kernels (csrc/lz4e_pack.hip)
    through tools/emu/emu_pack.cpp's `range` cases: lo and len at every
    residue pair mod 16 for a frame and a raw entry, ranges around and past
    an entry's end, decode errors, invalid requests, repeated, permuted and
    null sel; every destination an allocation of exactly the bytes it gets."""
    from test_emulator import CXX, REPO
    if not os.path.exists(CXX):
        pytest.skip("no clang++ for the emulator")
    b = tmp_path_factory.mktemp("emu_range")
    env = dict(os.environ, EMU_PACK="1", EMU_BUILD=str(b), CXX=CXX)
    subprocess.run(["bash", os.path.join(REPO, "tools", "emu", "build.sh"), "-fsanitize=address,undefined",
                    "-fno-sanitize=alignment", "-fno-sanitize-recover=all"], check=True, env=env, capture_output=True)
    out = subprocess.run([str(b / "emu_pack"), "range"], capture_output=True, text=True, timeout=600)
    shutil.rmtree(b, ignore_errors=True)
    assert out.returncode == 0 and "emu_pack range ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr
