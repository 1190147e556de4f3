"""Inputs for the parser's chain walk and clash groups -- TEST INFRASTRUCTURE ONLY.

The window code of compress_block (lz4-sgori_amd/csrc/lz4e_compress.hip) has
two pieces these blocks aim at:

  * the clash groups of a window (group_lanes): the lanes of a window whose
    positions share a table slot, found by an exchange through 64 LDS slots;
  * the serial chain walk: per lane the next link with a flag bit "the walk
    ends after this link", read four links at a time by the scalar loop.

The first window of a block covers positions 1..64 (lane k <-> position 1 + k),
so a plan laid on those positions is a plan of lanes; later windows start where
the parse sends them, and those plans are repeated at every shift of 0..7 bytes
so that each link position of an iteration, lane 63 and lane 64 are all met.
Every block is small (the content is at most 4 096 bytes: the LDS-image
kernel); hbm() appends incompressible bytes to 4 097..8 192 for the HBM-image
kernel, which leaves the content's windows where they were.  Seeded and
deterministic; the oracle's frame is the expectation, nothing here predicts it.
"""
import functools

import numpy as np

import parse_synth as ps
from parse_synth import BYU16, BYU32, BYU64

PERIODS = (1, 2, 3, 4, 5, 6, 7, 8, 31, 32, 33, 63, 64, 65)
LINKS = (0, 1, 2, 3, 4, 5, 7, 8, 9)  # planted sequences; the restart's match is one link more
SHIFTS = range(8)


def _rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _period(rng, k, n):
    unit = _rand(rng, k)
    return (unit * (n // k + 1))[:n]


def period_blocks(tt):
    """Period-k data: 2 to 64 lanes of the first window share a hash (k = 1:
    all of them, k = 65: none, the next window's first lane).  One block per
    k of 64..200 bytes, a 13-byte one, and all periods in one block, each for
    80 bytes with 9 literals between them."""
    out = []
    rng = np.random.default_rng(100 + tt)
    for i, k in enumerate(PERIODS):
        out.append((f"period-{k}", _period(rng, k, 64 + 10 * i + (6 if i == 13 else 0)), tt))
    out.append(("period-3-len13", _period(rng, 3, 13), tt))
    parts = []
    for k in PERIODS:
        parts += [_period(rng, k, 80), _rand(rng, 9)]
    out.append(("period-all", b"".join(parts) + _rand(rng, 13), tt))
    return out


def _plant(buf, pos, data):
    buf[pos:pos + len(data)] = data


def group_blocks(tt):
    """Groups laid on the lanes of the first window (position = lane + 1)."""
    out = []
    w = ps.hash_width(tt)
    rng = np.random.default_rng(200 + tt)

    def block(label, groups, n=120):
        """groups: [[lanes]]: the lanes of a group hold the same w + 2 bytes."""
        b = bytearray(_rand(rng, n))
        for lanes in groups:
            x = _rand(rng, w + 2)
            for ln in lanes:
                _plant(b, 1 + ln, x)
        out.append((label, bytes(b), tt))

    block("groups-2", [[3, 20], [30, 50]])
    block("groups-3", [[3, 20], [11, 40, 55], [30, 62]])
    block("groups-lane0-lane63", [[0, 63]])
    block("groups-lane0", [[0, 17, 41]])
    block("groups-lane63", [[9, 33, 63]])
    block("groups-lane0-and-lane63", [[0, 25], [40, 63]])
    # a group across the last valid lane of the last window: the same bytes at
    # mflimit - 6, mflimit - 1 (the last probe), mflimit + 2 and mflimit + 5 (invalid lanes)
    for n in (40, 77, 78, 79, 141):
        b = bytearray(_rand(rng, n))
        mfl = n - ps.MFLIMIT
        x = _rand(rng, w)
        for d in (-6, -1, 2, 5):
            _plant(b, mfl + d, x + bytes([(x[0] + d) & 0xFF]))  # w equal bytes, then they differ
        out.append((f"groups-straddle-end-{n}", bytes(b[:n]), tt))
    # different bytes with one hash (found by search, parse_synth.colliders):
    # the group's members do not match each other; then a real copy of each
    b = bytearray(_rand(rng, 150))
    x = _rand(rng, w + 2)
    y1, y2 = ps.colliders(x, tt, 2)
    _plant(b, 1 + 5, x)
    _plant(b, 1 + 19, y1 + x[w:])
    _plant(b, 1 + 37, y2 + x[w:])
    _plant(b, 1 + 50, x)
    _plant(b, 1 + 70, y1 + x[w:])
    _plant(b, 1 + 90, y2 + x[w:])
    out.append(("groups-colliders", bytes(b), tt))
    return out


def _chain(b, links, step_lits, step_match):
    """`links` sequences of step_lits literals and a step_match-byte match of
    the bytes that start the run (the periodic continuation, always probed)."""
    for i in range(links):
        k = step_lits[i % len(step_lits)]
        m = step_match[i % len(step_match)]
        u = b.lit(max(k, 2) if m == 4 else k)
        b.match(u, m)


def _lead(b, shift):
    """A short match that restarts the search (so that the next 66 positions
    are all probed), then 20 + shift literals."""
    b.lit(2)
    b.match(1, 6)
    b.lit(20 + shift)


def walk_blocks(tt):
    """A restart of the search, then N sequences, the first after 20..27
    literals and the others short (a chain of N links, N + 1 with the
    restart's own match), then what ends a fast chain: a
    match of 40 bytes (32+: kStop), 70 literals (no hit in the window), a
    catch-up of 6 (over the 4 bytes in registers); and chains that run on
    across windows.  Each at shifts of 0..7 bytes (_lead)."""
    out = []
    lo = 5 if tt == BYU32 else 4  # byU32 hashes 5 bytes
    for links in LINKS:
        for stop in ("long", "literals", "catchup"):
            b = ps._B(3000 + 10 * links + len(stop) + tt)
            b.lit(20)
            for sh in SHIFTS:
                _lead(b, sh)
                _chain(b, links, (2, 1, 3), (lo, lo + 1, lo + 3))
                if stop == "long":
                    u = b.lit(3)
                    b.match(u, 40)
                elif stop == "literals":
                    b.lit(70)
                else:
                    # six bytes equal before the copy's first probed position
                    src = b.lit(14)
                    b.lit(2)
                    b.match(len(b.b) - 2, 6)  # resets the search: the next probes are consecutive
                    b.lit(1)
                    b.lit(data=bytes(b.b[src:src + 14]))
            out.append((f"walk-{links}-links-{stop}", b.tail(), tt))
    # uniform links of 6, 7 and 9 bytes for 40 links: the chain leaves every
    # window, at every link position of an iteration, over lanes 63 and 64
    for step, (k, m) in ((6, (1, 5)), (7, (2, 5)), (9, (3, 6)), (12, (4, 8))):
        b = ps._B(3500 + step + tt)
        b.lit(20)
        for sh in SHIFTS:
            _lead(b, sh)
            _chain(b, 40 if step < 12 else 24, (k,), (m,))
        out.append((f"walk-uniform-{step}", b.tail(), tt))
    return out


@functools.lru_cache(maxsize=None)
def small(tt):
    """[(label, block, class)]: every block at most 4 096 bytes."""
    out = period_blocks(tt) + group_blocks(tt) + walk_blocks(tt)
    assert all(len(b) <= 4096 for _, b, _ in out), [(lb, len(b)) for lb, b, _ in out if len(b) > 4096]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def hbm(tt):
    """The same blocks with incompressible bytes appended, 4 097..8 192 bytes."""
    rng = np.random.default_rng(400 + tt)
    out = []
    for i, (label, b, _) in enumerate(small(tt)):
        n = 4097 + (i * 1021) % 4096 if i else 8192
        out.append((label + "-hbm", b + _rand(rng, n - len(b)), tt))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def all_small():
    """byU16 and byU32 in full; byU64 for the period and group blocks."""
    return small(BYU16) + small(BYU32) + tuple(period_blocks(BYU64) + group_blocks(BYU64))


@functools.lru_cache(maxsize=None)
def all_hbm():
    n64 = len(period_blocks(BYU64) + group_blocks(BYU64))
    return hbm(BYU16) + hbm(BYU32) + hbm(BYU64)[:n64]
