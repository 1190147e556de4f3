"""Grammar-directed LZ4 block frames that no LZ4E encoder emits -- TEST
INFRASTRUCTURE ONLY.

The decoders' fast paths are keyed on token values (batches of up to 64
sequences with literals <= 14 and matches <= 18, the 256-byte token window,
in-batch dependency rounds, the spans of the two previous batches, the group
decoder's period and doubling copies, offset 0).  A greedy hash-table parse
with a 12-byte end margin reaches little of that space, so this module writes
frames from a list of sequences instead and keeps a pure-Python LZ model of
what they decode to.

``emit(seqs, last_literals, rng)`` is the builder; the ``profile_*``
functions return lists of ``Case`` for the CPU, emulator and GPU tests.  The
oracle stays the truth for values and bytes; the model checks the oracle
wherever the oracle accepts.

A frame decodes at its exact size only if its last sequence obeys the
reference's end rules (lz4e_decompress.c:223-288, 422-431):
last literals >= 5 and last match length + last literals >= 12.
"""
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

MODEL_OFFSET_ZERO = 0  # the byte an offset-0 match yields (lz4e_decompress.c:313)

# a "fast" sequence: both token nibbles below 15
FAST_LIT_MAX, FAST_MATCH_MAX = 14, 18
BATCH = 64  # sequences per fast batch of the decoders

BOUNDARY_LITS = [0, 1, 14, 15, 16, 17, 46, 47, 269, 270, 271, 525]
BOUNDARY_MATCHES = [4, 5, 18, 19, 20, 22, 50, 51, 68, 273, 274, 275, 529]
BOUNDARY_OFFSETS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257,
                    4095, 4096, 65535]

DICT_SIZES = [5, 100, 4096, 65536]
SMALL_SIZES = [300, 2000, 4500]   # every decoder mode (capacities stay <= 4608)
LARGE_SIZES = [20000, 65536]      # one-wave, pipelined and auto only
BOUNDARY_LARGE_SIZES = [20000, 66300]  # past 65535 bytes, so that the largest offset is valid


class Case(NamedTuple):
    label: str
    frame: bytes
    cap: int
    dic: bytes
    model: Optional[bytes]   # what a successful decode yields (None: cannot succeed)
    must_accept: bool        # built to obey the end rules: the oracle must accept it
    want_ret: Optional[int]  # the error value the construction predicts, where it does


def _length_ext(n: int) -> bytes:
    """Extension bytes of a nibble-15 length: n = value - 15."""
    return b"\xff" * (n // 255) + bytes([n % 255])


def _rand(rng, n: int) -> bytes:
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def emit_ex(seqs: Sequence[Tuple[int, int, int]], last_literals: int, rng, dictionary: bytes = b""):
    """-> (frame, model_output, offset_pos): offset_pos[k] is the input
    position of sequence k's offset field.  The model follows LZ semantics:
    byte t of a match at output position op with offset o is out[op - o + t],
    read from the dictionary's end for positions before the block; offset 0
    yields zeros; a position before the dictionary reads as zero (such a
    frame is invalid unless the dictionary is a full 64 KiB window)."""
    frame, out, offset_pos = bytearray(), bytearray(), []
    D = len(dictionary)
    for ll, off, ml in seqs:
        assert ll >= 0 and ml >= 4 and 0 <= off <= 65535
        m = ml - 4
        frame.append((min(ll, 15) << 4) | min(m, 15))
        if ll >= 15:
            frame += _length_ext(ll - 15)
        lits = _rand(rng, ll)
        frame += lits
        out += lits
        offset_pos.append(len(frame))
        frame += bytes([off & 255, off >> 8])
        if m >= 15:
            frame += _length_ext(m - 15)
        if off == 0:
            out += bytes([MODEL_OFFSET_ZERO]) * ml
        else:
            for _ in range(ml):
                p = len(out) - off
                out.append(out[p] if p >= 0 else (dictionary[D + p] if D + p >= 0 else 0))
    frame.append(min(last_literals, 15) << 4)
    if last_literals >= 15:
        frame += _length_ext(last_literals - 15)
    lits = _rand(rng, last_literals)
    frame += lits
    out += lits
    return bytes(frame), bytes(out), offset_pos


def emit(seqs, last_literals, rng, dictionary: bytes = b""):
    """-> (frame, model_output) of the sequences (literal length, offset,
    match length) followed by `last_literals` literals."""
    return emit_ex(seqs, last_literals, rng, dictionary)[:2]


def _out_len(seqs) -> int:
    return sum(ll + ml for ll, _, ml in seqs)


def _fast_seq(rng, op: int, max_off: int = 65535) -> Tuple[int, int, int]:
    """A plain fast sequence with a valid non-zero offset at output position op."""
    ll = int(rng.integers(1 if op == 0 else 0, FAST_LIT_MAX + 1))
    ml = int(rng.integers(4, FAST_MATCH_MAX + 1))
    off = int(rng.integers(1, min(op + ll, max_off) + 1))
    return ll, off, ml


def _valid_tail(rng) -> Tuple[Tuple[int, int, int], int]:
    """A closing sequence and last literals that obey both end rules."""
    last = int(rng.integers(5, 14))
    return (int(rng.integers(1, 8)), 1, int(rng.integers(max(4, 12 - last), 19))), last


def _grow(rng, target: int, step, seed_lits: int = 24) -> Tuple[List[Tuple[int, int, int]], int]:
    """Sequences from step(rng, op, index, room=bytes left) until ~target bytes, then a valid
    tail.  The first sequence carries seed literals for offsets to reach."""
    seqs = [(seed_lits, 1, 4)]
    op = seed_lits + 4
    while op < target - 64:
        s = step(rng, op, len(seqs), room=target - 40 - op)
        if op + s[0] + s[2] > target - 40:
            s = _fast_seq(rng, op)
        seqs.append(s)
        op += s[0] + s[2]
    tail, last = _valid_tail(rng)
    seqs.append(tail)
    return seqs, last


def _case(label, seqs, last, rng, cap_extra=0, dic=b"", must_accept=True) -> Case:
    frame, model = emit(seqs, last, rng, dic)
    return Case(label, frame, len(model) + cap_extra, dic, model, must_accept, None)


# ---------------------------------------------------------------------------
# profiles
# ---------------------------------------------------------------------------

def profile_boundary(seed: int, sizes=SMALL_SIZES, per_size: int = 3) -> List[Case]:
    """Literal and match lengths on both sides of every token and extension
    boundary, offsets around every power of two the copies special-case, 0,
    and "the output so far", mixed with plain fast sequences."""
    rng = np.random.default_rng(seed)
    # values not emitted yet by this call: taken first (the largest admissible
    # one), so that coverage of the lists does not hang on the seed
    todo_l, todo_m, todo_o = set(BOUNDARY_LITS), set(BOUNDARY_MATCHES), set(BOUNDARY_OFFSETS + [-1])

    def pick(todo, allowed):
        left = [v for v in allowed if v in todo]
        v = max(left) if left else int(rng.choice(allowed))
        todo.discard(v)
        return v

    zero_todo = ["long", "fast", "fast", "fast"]  # offset 0 in and out of a fast batch

    def step(rng, op, k, room):
        if zero_todo and k % 5 == 3 and room >= 80:
            if zero_todo.pop() == "fast":
                return int(rng.integers(0, FAST_LIT_MAX + 1)), 0, int(rng.integers(4, FAST_MATCH_MAX + 1))
            return 1, 0, 68
        if rng.integers(0, 3) == 0:
            return _fast_seq(rng, op)
        ll = pick(todo_l, [v for v in BOUNDARY_LITS if v <= max(room - 4, 1)])
        ml = pick(todo_m, [v for v in BOUNDARY_MATCHES if v <= max(room - ll, 4)])
        pos = op + ll
        # -1 stands for "the output so far": the block's first byte
        off = pick(todo_o, [o for o in BOUNDARY_OFFSETS if o <= pos] + ([-1] if pos <= 65535 else []))
        return ll, pos if off < 0 else off, ml

    out = []
    for size in sizes:
        for j in range(per_size):
            seqs, last = _grow(rng, size, step)
            out.append(_case(f"boundary-{size}-{j}", seqs, last, rng, cap_extra=(0, 32, 12)[j % 3]))
    return out


def profile_chains(seed: int, sizes=SMALL_SIZES, per_size: int = 2) -> List[Case]:
    """At least 200 sequences in a row of literals 0 or 1, matches 4..18 and
    offsets 1..20: every sequence reads what the ones just before it wrote,
    through whole 64-sequence batches and across their borders."""
    rng = np.random.default_rng(seed)

    def step(rng, op, k, room=None):
        ll = int(rng.integers(0, 2))
        return ll, int(rng.integers(1, min(20, op + ll) + 1)), int(rng.integers(4, FAST_MATCH_MAX + 1))

    out = []
    for size in sizes:
        for j in range(per_size):
            seqs, last = _grow(rng, max(size, 3000), step, seed_lits=int(rng.integers(1, 21)))
            assert len(seqs) >= 200
            out.append(_case(f"chains-{size}-{j}", seqs, last, rng, cap_extra=(0, 32)[j % 2]))
    return out


def profile_far(seed: int, sizes=SMALL_SIZES, per_size: int = 2) -> List[Case]:
    """Fast sequences whose sources lie 1, 2 and 3 or more 64-sequence batches
    back: the pipelined decoder serves the two previous spans from LDS and
    anything older from HBM."""
    rng = np.random.default_rng(seed)
    starts: List[int] = []

    def step(rng, op, k, room=None):
        while len(starts) <= k:
            starts.append(op)
        starts[k] = op
        ll = int(rng.integers(0, FAST_LIT_MAX + 1))
        ml = int(rng.integers(4, FAST_MATCH_MAX + 1))
        back = int(rng.choice([0, 1, 1, 2, 2, 3, 5, 9]))
        b = k // BATCH - back
        if back == 0 or b < 0:
            lo, hi = 0 if b < 0 else starts[(k // BATCH) * BATCH], op + ll
        else:
            lo, hi = starts[b * BATCH], starts[(b + 1) * BATCH]
        src = int(rng.integers(lo, max(hi, lo + 1)))
        off = min(max(op + ll - src, 1), min(op + ll, 65535))
        return ll, off, ml

    out = []
    for size in sizes:
        for j in range(per_size):
            del starts[:]
            seqs, last = _grow(rng, size, step)
            out.append(_case(f"far-{size}-{j}", seqs, last, rng, cap_extra=(0, 32)[j % 2]))
    return out


def profile_ends(seed: int, head: int = 3) -> List[Case]:
    """Last literals 0..13 x last match length 4..12 x capacities of len,
    len + 1, len + 12 and len + 32: both sides of every end rule."""
    rng = np.random.default_rng(seed)
    out = []
    for last in range(14):
        for ml in range(4, 13):
            seqs, op = [(20, 1, 4)], 24
            for _ in range(head):
                s = _fast_seq(rng, op)
                seqs.append(s)
                op += s[0] + s[2]
            seqs.append((2, int(rng.integers(1, op + 3)), ml))
            frame, model = emit(seqs, last, rng)
            for extra in (0, 1, 12, 32):
                out.append(Case(f"ends-l{last}-m{ml}-c{extra}", frame, len(model) + extra, b"", model,
                                False, None))
    return out


def profile_invalid(seed: int) -> List[Case]:
    """Frames that must fail, each at a known input position (and five valid
    twins whose offset is exactly the output so far): an offset one
    past the output so far at sequence k of a run of fast sequences
    (k = 0..70: every lane of a fast batch and the first of the next), a
    literal run past the input's end, a 255-run of extension bytes cut by
    the input's end, and a match running past the capacity."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(71):
        seqs, op = [], 0
        for i in range(k + 8):
            s = _fast_seq(rng, op)
            if i == k:
                s = (s[0], op + s[0] + 1, s[2])
            seqs.append(s)
            op += s[0] + s[2]
        tail, last = _valid_tail(rng)
        frame, model, opos = emit_ex(seqs + [tail], last, rng)
        # the reference reports the input position after the offset field (:299-302)
        out.append(Case(f"invalid-offset-k{k}", frame, len(model) + 32 * (k % 2), b"", None, False,
                        -(opos[k] + 2) - 1))
        if k in (0, 31, 63, 64, 70):
            # the valid twin: the offset equals the output so far (the block's first byte)
            seqs[k] = (seqs[k][0], seqs[k][1] - 1, seqs[k][2])
            out.append(_case(f"invalid-twin-offset-k{k}", seqs + [tail], last, rng, cap_extra=32 * (k % 2)))
    for j, cut in enumerate([1, 2, 5, 8, 9, 20, 37]):
        seqs, last = _grow(rng, 400, lambda r, op, k, room=None: _fast_seq(r, op))
        frame, model = emit(seqs, 40, rng)
        out.append(Case(f"invalid-literals-past-end-{j}", frame[:-cut], len(model), b"", None, False, None))
    for j, run in enumerate([0, 1, 2, 14, 15, 16, 17, 255, 300]):
        seqs, last = _grow(rng, 200 + 100 * (j % 3), lambda r, op, k, room=None: _fast_seq(r, op))
        body = emit(seqs, 0, rng)[0][:-1]
        out.append(Case(f"invalid-literal-ext-cut-{run}", body + b"\xf0" + b"\xff" * run, 100000, b"",
                        None, False, None))
        out.append(Case(f"invalid-match-ext-cut-{run}", body + b"\x1f\x41\x01\x00" + b"\xff" * run, 100000,
                        b"", None, False, None))
    for j, (ml, short) in enumerate([(4, 1), (12, 1), (18, 3), (19, 5), (68, 6), (68, 30), (529, 1),
                                     (529, 300), (18, 18), (40, 12)]):
        seqs, last = _grow(rng, 300 + 500 * (j % 4), lambda r, op, k, room=None: _fast_seq(r, op))
        seqs = seqs[:-1] + [(3, int(rng.integers(1, 9)), ml)]
        frame, model = emit(seqs, 5, rng)
        out.append(Case(f"invalid-match-past-cap-{ml}-{short}", frame, len(model) - 5 - short, b"", None,
                        False, None))
    return out


def profile_dict(seed: int, sizes=(300, 2000), dict_sizes=DICT_SIZES) -> List[Case]:
    """Offsets reaching into a dictionary of 5, 100, 4096 or 65536 bytes that
    logically precedes the output: its last byte, its middle, exactly its
    first byte, and one byte before it (an error below 64 KiB), with matches
    that stay inside it and matches that run on into the block."""
    rng = np.random.default_rng(seed)
    out = []
    for dsize in dict_sizes:
        dic = _rand(rng, dsize)
        max_off_done = [False]
        for size in sizes:
            for before in (0, 1):
                def step(rng, op, k, dsize=dsize, before=before, room=None):
                    if rng.integers(0, 2) == 0:
                        return _fast_seq(rng, op)
                    ll = int(rng.choice([0, 1, 3, 14, 15, 40]))
                    pos = op + ll
                    reach = [r for r in (1, max(1, dsize // 2), dsize) if pos + r <= 65535]
                    if dsize == 65536 and not max_off_done[0] and room >= ll + 19:
                        # the largest offset a frame can hold, at a small position
                        max_off_done[0] = True
                        return ll, 65535, int(rng.choice([4, 18, 19]))
                    if not reach:
                        return _fast_seq(rng, op)
                    r = int(rng.choice(reach))
                    # matches inside the dictionary, ending at its end, and running on into the block
                    ml = int(rng.choice([4, 5, 18, 19, 68, 300, max(4, r), r + 7]))
                    return ll, pos + r, ml

                seqs, last = _grow(rng, size, step)
                label = f"dict-{dsize}-{size}"
                if before:
                    # one byte before the dictionary's first byte, mid-frame
                    k = len(seqs) // 2
                    pos = _out_len(seqs[:k]) + seqs[k][0]
                    if pos + dsize + 1 > 65535:
                        continue
                    seqs[k] = (seqs[k][0], pos + dsize + 1, seqs[k][2])
                    label += "-before"
                frame, model = emit(seqs, last, rng, dic)
                out.append(Case(label, frame, len(model) + 32 * before, dic, None if before else model,
                                not before, None))
    return out


PROFILES = {"boundary": profile_boundary, "chains": profile_chains, "far": profile_far,
            "ends": profile_ends, "invalid": profile_invalid, "dict": profile_dict}
SIZED = ("boundary", "chains", "far")  # profiles that take output sizes


def cases(profile: str, seed: int = 0, large: bool = False) -> List[Case]:
    """The profile's cases: outputs of <= 4608 bytes (every decoder mode), or
    with large=True of about 20000 and 65536 bytes (one-wave, pipelined, auto)."""
    f = PROFILES[profile]
    base = 1000 * (sorted(PROFILES).index(profile) + 1) + seed
    if profile in SIZED:
        return f(base + 500, BOUNDARY_LARGE_SIZES if profile == "boundary" else LARGE_SIZES, 1) if large else f(base)
    if profile == "dict":
        return f(base + 500, (20000,), DICT_SIZES) if large else f(base)
    return [] if large else f(base)
