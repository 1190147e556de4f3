"""A pure-Python statement of the LZ4E block decoder's rules, full and partial
(test infrastructure; no product code).

decode(frame, cap) follows the reference's safe decoder
(lz4e/lz4e_decompress.c:62-460, instance endOnInputSize + noDict) check by
check and in its order, so that the value -- the output size, or the error
code -(ip) - 1 of the input position where a check failed -- is the
reference's.  decode(frame, target, partial=True) is the same walk with the
partial_decode branches the reference carries but never instantiates:

  * literal run (:226-282): the special branch is entered when the run ends
    past oend - 12 or its input past iend - 8.  A run that ends past oend is
    cut to oend - op; the (cut) run must lie inside the input; after the copy
    the decode ends when the output is full or fewer than 3 input bytes
    remain, and goes on to the offset otherwise.
  * match (:298-405): after the offset and extension checks of the full
    decoder, a match that ends past oend - 12 is cut to min(length, oend - op)
    and the decode ends when the output is full.  The full decoder's rule
    that the last 5 bytes be literals (:425-431) is not checked.
  * special cases (:113-120) are the full decoder's: target 0 gives -1
    unless the frame is the single byte 00.

One stated deviation, shared with the project's full decoders
(frame_synth.MODEL_OFFSET_ZERO): a match with offset 0 yields zeros.  The
reference writes the offset into the output before the copy in full mode
(:313), which gives zeros, and skips that store in partial mode (:309-314),
where the copy would repeat whatever the destination held before.

Dictionaries are outside this model (no partial entry point takes one).
"""
from typing import List, Tuple

import numpy as np

from frame_synth import MODEL_OFFSET_ZERO


def _match(out: bytearray, off: int, n: int) -> None:
    if n <= 0:
        return
    if off == 0:
        out += bytes([MODEL_OFFSET_ZERO]) * n
        return
    start = len(out) - off
    if off >= n:
        out += out[start:start + n]
    else:
        pat = bytes(out[start:])
        out += (pat * (n // off + 1))[:n]


def decode(frame: bytes, cap: int, partial: bool = False) -> Tuple[int, bytes]:
    """-> (value, output bytes written in order).  cap is the capacity of a
    full decode and the target size of a partial one."""
    src = bytes(frame)
    iend, oend = len(src), cap
    if cap == 0:                                    # :113-114
        return (0 if iend == 1 and src[0] == 0 else -1), b""
    if iend == 0:                                   # :119-120
        return -1, b""
    out = bytearray()
    ip = 0
    shortiend, shortoend = iend - 14 - 2, oend - 14 - 18   # :100-103
    while True:
        token = src[ip]
        ip += 1
        length = token >> 4
        if length != 15 and ip < shortiend and len(out) <= shortoend:   # :150-191
            out += src[ip:ip + length]
            ip += length
            offset = src[ip] | src[ip + 1] << 8
            ip += 2
            length = token & 15
            if length != 15 and offset >= 8 and offset <= len(out):
                _match(out, offset, length + 4)
                continue
        else:
            if length == 15:                        # :194-220
                if ip >= iend - 15:
                    return -ip - 1, bytes(out)
                while True:
                    s = src[ip]
                    ip += 1
                    length += s
                    if not (ip < iend - 15 and s == 255):
                        break
            op = len(out)
            cpy = op + length
            if cpy > oend - 12 or ip + length > iend - 8:   # :226-282
                if partial:
                    if cpy > oend:
                        cpy, length = oend, oend - op
                    if ip + length > iend:
                        return -ip - 1, bytes(out)
                elif ip + length != iend or cpy > oend:
                    return -ip - 1, bytes(out)
                out += src[ip:ip + length]
                ip += length
                if not partial or cpy == oend or ip >= iend - 2:
                    break
            else:
                out += src[ip:ip + length]
                ip += length
            offset = src[ip] | src[ip + 1] << 8     # :291-296
            ip += 2
            length = token & 15
        op = len(out)
        if offset > op:                             # :299-302
            return -ip - 1, bytes(out)
        if length == 15:                            # :316-334
            while True:
                s = src[ip] if ip < iend else 0     # (a byte at iend fails the next check whatever it is)
                ip += 1
                if ip > iend - 5:
                    return -ip - 1, bytes(out)
                length += s
                if s != 255:
                    break
        length += 4
        if partial:
            if op + length > oend - 12:             # :388-405
                _match(out, offset, min(length, oend - op))
                if len(out) == oend:
                    break
                continue
        elif op + length > oend - 5:                # :422-431
            return -ip - 1, bytes(out)
        _match(out, offset, length)
    return len(out), bytes(out)


def sampled_targets(n: int, seed: int = 0, extra: int = 60) -> List[int]:
    """The targets the tests decode a frame of n output bytes at: every k from
    0 to n + 19 for n <= 400, else k < 40, |k - n| < 20 and `extra` seeded
    values in between."""
    if n <= 400:
        return list(range(0, n + 20))
    rng = np.random.default_rng(seed + n)
    ks = set(range(0, 40)) | set(range(n - 19, n + 20)) | {int(k) for k in rng.integers(40, n - 19, extra)}
    return sorted(ks)


# ---------------------------------------------------------------------------
# Frames the tests share (built once per process)
# ---------------------------------------------------------------------------

MATCH_OFFSETS = [0, 1, 3, 7, 8, 15, 16]  # the long match of hand_frames()


def hand_frames():
    """-> {name: (frame, full output)}: one 525-byte literal run; a 529-byte
    match after 20 literals at each of MATCH_OFFSETS; a frame whose last
    literal run has 4 bytes (the full decoder rejects it)."""
    import frame_synth

    rng = np.random.default_rng(4242)
    out = {"lit525": frame_synth.emit([(525, 1, 8)], 7, rng)}
    for off in MATCH_OFFSETS:
        out["match529-o%d" % off] = frame_synth.emit([(20, off, 529)], 6, rng)
    out["last4"] = frame_synth.emit([(12, 4, 280)], 4, rng)
    return out


_blocks = None


def oracle_blocks():
    """-> [(name, data, frame)]: blocks compressed by the oracle -- text of
    600 B, 4 KiB and 64 KiB, 300 random bytes, 4 KiB of zeros."""
    global _blocks
    if _blocks is None:
        import oracle_ref
        import pack_model

        data = [("text600", pack_model.text_block(600, 1)), ("text4k", pack_model.text_block(4096, 2)),
                ("text64k", pack_model.text_block(65536, 3)), ("random300", pack_model.random_block(300, 4)),
                ("zeros4k", bytes(4096))]
        _blocks = []
        for name, d in data:
            r, frame, _, _ = oracle_ref.compress(d, 1 if len(d) < 65536 else 3)  # byU16 / byU32
            assert r > 0, name
            _blocks.append((name, d, frame))
    return _blocks
