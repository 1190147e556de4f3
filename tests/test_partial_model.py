"""tests/partial_model.py against the oracle (CPU).

With the partial flag off the model must be the oracle -- value and bytes
[0, ret) -- on valid, damaged and truncated frames at capacities on both sides
of every end rule: the partial rules are stated as changes to that walk, so
the walk itself has to be right.  With the flag on, every frame the oracle
accepts must give min(k, n) and that prefix at every target k, and hand-built
frames must give the values worked out by hand below."""
import numpy as np
import pytest

import frame_synth
import oracle_ref
import partial_model
from partial_model import decode

PROFILES = [p for p in frame_synth.PROFILES if p != "dict"]


def _variants(frame: bytes, seed: int):
    rng = np.random.default_rng(seed)
    yield "intact", frame
    yield "cut1", frame[:-1]
    yield "half", frame[:len(frame) // 2]
    if frame:
        b = bytearray(frame)
        i = int(rng.integers(0, len(b)))
        b[i] ^= 1 << int(rng.integers(0, 8))
        yield "flip", bytes(b)


@pytest.mark.parametrize("profile", PROFILES)
def test_full_mode_is_the_oracle(profile):
    n = 0
    cs = frame_synth.cases(profile) + frame_synth.cases(profile, large=True)
    for ci, c in enumerate(cs):
        for vname, f in _variants(c.frame, ci):
            for cap in (c.cap, c.cap - 1, c.cap - 13, c.cap + 5, c.cap // 2, 1, 0):
                if cap < 0:
                    continue
                want = oracle_ref.decompress(f, cap)
                got = decode(f, cap)
                assert got[0] == want[0] and got[1][:max(want[0], 0)] == want[1], (c.label, vname, cap, got[0], want[0])
                n += 1
    assert n > 100


def _check_prefixes(label, frame, full, seed=0):
    n = len(full)
    for k in partial_model.sampled_targets(n, seed):
        r, out = decode(frame, k, partial=True)
        if k == 0:
            assert r == (0 if frame == b"\x00" else -1), (label, r)
            continue
        assert r == min(k, n) and out == full[:r], (label, k, r)


@pytest.mark.parametrize("profile", PROFILES)
def test_partial_is_a_prefix_on_accepted_frames(profile):
    seen = 0
    for ci, c in enumerate(frame_synth.cases(profile) + frame_synth.cases(profile, large=True)):
        r, full = oracle_ref.decompress(c.frame, c.cap)
        if r < 0:
            continue
        _check_prefixes(c.label, c.frame, full, ci)
        seen += 1
    assert seen > 0


def test_partial_is_a_prefix_on_oracle_frames():
    for name, data, frame in partial_model.oracle_blocks():
        assert oracle_ref.decompress(frame, len(data)) == (len(data), data)
        _check_prefixes(name, frame, data)


def test_cut_inside_a_literal_run():
    frame, full = partial_model.hand_frames()["lit525"]
    assert len(full) == 525 + 8 + 7 and frame[:4] == b"\xf4\xff\xff\x00"
    for k in (1, 100, 524):
        assert decode(frame, k, True) == (k, full[:k])
    # the whole run and nothing else: the output is full after the copy (:281)
    assert decode(frame, 525, True) == (525, full[:525])
    # one byte of room: the run is whole, the 8-byte match is cut to 1
    assert decode(frame, 526, True) == (526, full[:526])


@pytest.mark.parametrize("off", partial_model.MATCH_OFFSETS)
def test_cut_inside_a_long_match(off):
    frame, full = partial_model.hand_frames()["match529-o%d" % off]
    assert len(full) == 20 + 529 + 6
    if off == 0:
        assert full[20:549] == bytes(529)
    # 0, 1, 2 and 3 match bytes, cuts at and around the copies' 16- and
    # 64-byte pieces, the last byte of the match, and the literals behind it
    for k in (20, 21, 22, 23, 24, 35, 36, 37, 83, 84, 85, 300, 548, 549, 550, 555):
        assert decode(frame, k, True) == (k, full[:k]), k
    assert decode(frame, 556, True) == (555, full)


def test_fewer_than_five_last_literals():
    frame, full = partial_model.hand_frames()["last4"]
    assert len(frame) == 22 and len(full) == 296
    # full: the match ends at 292 > 296 - 5, failing after its length bytes (ip = 17)
    assert oracle_ref.decompress(frame, 296)[0] == -18 and decode(frame, 296)[0] == -18
    # partial: no such rule; every target gives its prefix
    for k in range(1, 297):
        assert decode(frame, k, True) == (k, full[:k]), k
    # and a larger target leaves through ip >= iend - 2 with less than the target
    assert decode(frame, 300, True) == (296, full)
    assert decode(frame, 4096, True) == (296, full)


def test_partial_error_sites():
    # target 0 (:113-114), empty input (:119-120)
    assert decode(b"\x00", 0, True) == (0, b"") and decode(b"\x10a", 0, True)[0] == -1
    assert decode(b"", 5, True)[0] == -1
    # literal length extension with fewer than 16 bytes behind it (:197-200): ip = 1
    assert decode(b"\xf0\x05" + b"a" * 14, 64, True)[0] == -2
    # a literal run that claims 5 bytes of an input that has 3 (:238-246): ip = 1 ...
    assert decode(b"\x50abc", 10, True)[0] == -2
    # ... unless the target cuts the run to what the input holds
    assert decode(b"\x50abc", 3, True) == (3, b"abc")
    assert decode(b"\x50abc", 4, True)[0] == -2
    # an offset before the start of the output (:299-302): after the offset, ip = 4
    assert decode(b"\x10a\x05\x00zzzz", 20, True)[0] == -5
    # a match length extension that runs into the last 5 input bytes (:322-323): ip = 5
    assert decode(b"\x1fa\x01\x00\xff\x00\x00", 64, True)[0] == -6
    # the same frames in full mode fail too (where is the oracle's business)
    for f in (b"\x50abc", b"\x10a\x05\x00zzzz", b"\x1fa\x01\x00\xff\x00\x00"):
        assert decode(f, 64)[0] == oracle_ref.decompress(f, 64)[0] < 0


def test_invalid_frames_fail_or_stop_inside_the_target():
    """Damaged frames in partial mode: whatever the value, the output never
    exceeds the target and an error names a position inside the frame."""
    for c in frame_synth.cases("invalid"):
        for k in (1, 7, c.cap // 2, c.cap, c.cap + 9):
            r, out = decode(c.frame, k, True)
            assert len(out) <= k and -len(c.frame) - 1 <= r <= k, (c.label, k, r)
