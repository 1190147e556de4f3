"""Inputs for the compressor's two-wave blocks (parser and flusher waves,
lz4-sgori_amd/csrc/lz4e_compress.hip), shared by tests/test_emulator_flusher.py
and tests/test_gpu_flusher.py.  Every block is seeded; what a block is built to
show is checked in the oracle's frame by `shows`.
"""
import numpy as np

import oracle_ref
import parse_synth as ps
from lz4e_amd import BYU16, BYU32, BYU64

TINY = (0, 1, 12, 13)  # both sides of kMinLength (13)


def units(n, seed, copy=4):
    """n bytes of 8-byte units: 4 fresh bytes, then a copy of the `copy` bytes
    that end where the fresh ones begin -- a sequence every 8 bytes (about
    n / 8 of them: 8 k in 64 KiB), far more than any record ring holds."""
    rng = np.random.default_rng(seed)
    out = bytearray(rng.integers(0, 256, 8, dtype=np.uint8).tobytes())
    fresh = rng.integers(0, 256, (n // 8 + 1, 4), dtype=np.uint8)
    for row in fresh:
        out += row.tobytes()
        out += out[-4 - copy:-4]
        if len(out) >= n:
            break
    return bytes(out[:n])


def random_bytes(n, seed):
    """No sequence at all: the block is its last-literals record."""
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def tiny(n):
    return bytes((7 * i + 3) & 0xFF for i in range(n))


# (literal run, match length) of the lengths block, in order: the wide literal
# copy from 33 bytes, the second literal extension byte from 270 (15 + 255),
# the second match extension byte from 274 (4 + 15 + 255)
# (a match after 270+ literals is found by a search whose step has grown: tens of bytes long)
LENGTHS = [(33, 273), (32, 8), (269, 274), (270, 600), (271, 40), (600, 64), (14, 1100)]


def lengths_block(seed=0xF1A5):
    """A pool, then literal runs and matches of LENGTHS.  The pool is units of
    48 random bytes and a 12-byte match, so that the search that crosses it
    stays at step 1 and every unit's start is in the hash table; each planned
    match copies from the start of a unit no other match uses."""
    unit = 60
    b = ps._B(seed)
    b.lit(64)
    pool = len(b.b) + 12
    for _ in range((sum(m for _, m in LENGTHS) + unit * len(LENGTHS)) // unit + 2):
        b.match(8, 12)
        b.lit(48)
    b.match(8, 12)
    at = pool + 2
    for L, m in LENGTHS:
        b.lit(L)
        b.match(at, m)
        at = pool + ((at + m - pool) // unit + 1) * unit + 2
    return b.tail()


def shows(block, tt, lits=(), matches=(), nseq=None):
    """The oracle's frame of `block` holds these literal-run and match lengths
    (and at least nseq sequences)."""
    seqs, _ = ps.parse_frame(oracle_ref.compress(block, tt)[1])
    have_l, have_m = {s[1] for s in seqs}, {s[3] for s in seqs}
    assert set(lits) <= have_l, (sorted(set(lits) - have_l))
    assert set(matches) <= have_m, (sorted(set(matches) - have_m))
    if nseq is not None:
        assert len(seqs) >= nseq, len(seqs)
    return True


def special_blocks():
    """[(label, block, class)]: the blocks the flusher tests name."""
    out = [("units64k", units(65536, 11), BYU16), ("units64k-u32", units(65536, 12, copy=5), BYU32),
           ("random64k", random_bytes(65536, 13), BYU16), ("random9000", random_bytes(9000, 14), BYU64),
           ("lengths", lengths_block(), BYU16), ("lengths-u32", lengths_block(0xF1A6), BYU32)]
    out += [(f"tiny{n}", tiny(n), tt) for n in TINY for tt in (BYU16, BYU32)]
    return out


def check_special_blocks():
    """What the special blocks are built to show, in the oracle's frames."""
    shows(units(65536, 11), BYU16, nseq=7000)
    shows(units(65536, 12, copy=5), BYU32, nseq=7000)
    assert ps.parse_frame(oracle_ref.compress(random_bytes(65536, 13), BYU16)[1]) == ([], 65536)
    for seed, tt in ((0xF1A5, BYU16), (0xF1A6, BYU32)):
        shows(lengths_block(seed), tt, lits=[L for L, _ in LENGTHS], matches=[m for _, m in LENGTHS])
