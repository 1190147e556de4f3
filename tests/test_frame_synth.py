"""The frame synthesizer against the oracle (CPU).

The oracle is the truth for values and bytes; tests/frame_synth.py's
pure-Python LZ model checks the oracle wherever the oracle accepts.  Frames of
the profiles built to obey the reference's end rules (last literals >= 5,
last match length + last literals >= 12) must all be accepted; the `ends` and
`invalid` profiles must see both outcomes, and every error must name an input
position inside the frame."""
import numpy as np
import pytest

import frame_synth
import oracle_ref


def _check(c):
    r, out = oracle_ref.decompress_dict(c.frame, c.cap, c.dic)
    assert -r - 1 <= len(c.frame), (c.label, r)
    if r >= 0:
        assert c.model is not None, (c.label, r)
        assert r == len(c.model) and out == c.model, (c.label, r, len(c.model))
    else:
        assert not c.must_accept, (c.label, r)
    if c.want_ret is not None:
        assert r == c.want_ret, (c.label, r, c.want_ret)
    return r


def test_model_is_lz_semantics():
    """emit() on hand-written sequences: literals, an overlapping match, an
    offset-0 match (zeros), a match out of a dictionary into the block."""
    rng = np.random.default_rng(1)
    frame, out = frame_synth.emit([(3, 1, 6), (0, 0, 5), (2, 11, 4)], 5, rng)
    assert out[3:9] == out[2:3] * 6 and out[9:14] == bytes(5) and out[16:20] == out[5:9]
    assert len(out) == 3 + 6 + 5 + 2 + 4 + 5
    assert frame[0] == 0x32 and frame[4:6] == b"\x01\x00" and frame[6] == 0x01
    dic = bytes(range(50, 60))
    frame, out = frame_synth.emit([(1, 4, 8)], 5, rng, dic)
    assert out[1:9] == dic[-3:] + out[0:1] + dic[-3:] + out[0:1]
    frame, out = frame_synth.emit([(300, 1, 19 + 255)], 15, rng)
    assert frame[:3] == b"\xff\xff\x1e" and frame[303:307] == b"\x01\x00\xff\x00"
    assert frame[-17] == 0xF0 and frame[-16] == 0


@pytest.mark.parametrize("large", [False, True], ids=["small", "large"])
@pytest.mark.parametrize("profile", ["boundary", "chains", "far", "dict"])
def test_oracle_accepts_every_rule_abiding_frame(profile, large):
    n = 0
    for seed in range(2 if large else 6):
        for c in frame_synth.cases(profile, seed, large):
            r = _check(c)
            n += r >= 0
            if profile != "dict":
                assert c.must_accept and r >= 0
            if not large:
                assert c.cap <= 4608
    assert n > 0


@pytest.mark.parametrize("profile", ["ends", "invalid"])
def test_both_outcomes_occur(profile):
    rets = [_check(c) for c in frame_synth.cases(profile)]
    if profile == "ends":
        assert any(r >= 0 for r in rets) and any(r < 0 for r in rets)
        cs = frame_synth.cases(profile)
        assert len(cs) == 14 * 9 * 4
        # at the exact capacity the end rules decide
        for c, r in zip(cs, rets):
            last, ml, extra = (int(x[1:]) for x in c.label.split("-")[1:])
            if extra == 0:
                assert (r >= 0) == (last >= 5 and last + ml >= 12), (c.label, r)
    else:
        cs = frame_synth.cases(profile)
        assert any(r >= 0 for r in rets) and any(r < 0 for r in rets)
        assert all((r >= 0) == c.must_accept for c, r in zip(cs, rets))
        assert len({r for r in rets}) > 70
        assert sum(c.want_ret is not None for c in cs) == 71


def _parse(frame):
    """The sequences of a valid frame, read back from its bytes alone ->
    [(literal length, offset, match length, output position of the match)]."""
    seqs, ip, op = [], 0, 0
    while True:
        tok = frame[ip]
        ip += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                ll += frame[ip]
                ip += 1
                if frame[ip - 1] != 255:
                    break
        ip += ll
        op += ll
        if ip == len(frame):
            return seqs
        off = frame[ip] | frame[ip + 1] << 8
        ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                ml += frame[ip]
                ip += 1
                if frame[ip - 1] != 255:
                    break
        ml += 4
        seqs.append((ll, off, ml, op))
        op += ml


def test_boundary_cases_emit_every_named_value():
    """Every literal length, match length and offset the `boundary` profile
    names is in the frames the GPU tests decode (seed 0: the small cases on
    all six modes hold all but offset 65535, which needs 65535 bytes of
    output before it or a 64 KiB dictionary: the large cases and the `dict`
    profile's small 64 KiB case hold it), and so is an offset equal to the
    output so far.  Read back from the frames, not from the builder."""
    small = [q for c in frame_synth.cases("boundary") for q in _parse(c.frame)]
    large = [q for c in frame_synth.cases("boundary", large=True) for q in _parse(c.frame)]
    assert set(frame_synth.BOUNDARY_LITS) <= {q[0] for q in small}
    assert set(frame_synth.BOUNDARY_MATCHES) <= {q[2] for q in small}
    assert set(frame_synth.BOUNDARY_OFFSETS) - {65535} <= {q[1] for q in small}
    assert any(q[1] == q[3] for q in small) and any(q[1] == q[3] for q in large)
    assert 65535 in {q[1] for q in large}
    in_dict = [q for c in frame_synth.cases("dict") if len(c.dic) == 65536 and c.must_accept
               for q in _parse(c.frame)]
    assert any(q[1] == 65535 and q[3] < 4608 for q in in_dict)
    # an offset 0 inside a run of fast sequences and with an extended match
    assert any(q[1] == 0 and q[2] <= 18 for q in small) and any(q[1] == 0 and q[2] > 18 for q in small)
