"""Device batches off the 16-byte grid, with guards (tests/gpu_batch.py).

include/lz4e.h requires no alignment of src_off or dst_off and promises at
most dst_cap[i] bytes written at dst + dst_off[i].  Every other device test
places its blocks on 16-byte boundaries; here every block sits at a source
and a destination residue of its own, and every byte outside the output
slots is checked after the call.  That reaches what only runs on a GPU off
the grid: stage_block's byte loop and HbmImage's alignbyte reads, the
word-aligned window base (shift = a & 3) with its LDS staging and ring index,
the fast-batch span stores, unaligned dword and 16-byte global stores,
unaligned DS accesses.  Values, bytes and iterator post-state equal the
oracle's.  Sizes are the smallest that reach each launch and decoder form.
"""
import functools
import zlib

import numpy as np
import pytest

import gpu_batch
import oracle_ref
from gpu_batch import DEC_AUTO, DEC_PIPE, DEC_WAVE, DEC_NAMES, FORCED_MODES
from lz4e_amd import BYU16, BYU32, compress_bound, corpus

pytestmark = pytest.mark.gpu

CORPORA = ["mixed", "small_alpha", "random"]
ALL_MODES = FORCED_MODES + [DEC_AUTO]
LARGE_MODES = [DEC_WAVE, DEC_PIPE, DEC_AUTO]
_ids = lambda modes: [DEC_NAMES[m] for m in modes]


@functools.lru_cache(maxsize=None)
def _pool(kind):
    n = 1 << 20
    rng = np.random.default_rng(zlib.crc32(kind.encode()))
    if kind == "small_alpha":  # long matches
        return rng.integers(0, 3, n, dtype=np.uint8).tobytes()
    if kind == "random":       # long literal runs
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return corpus.silesia_proxy(n, 0x91ACE).tobytes()


def _cut(kind, n, k):
    """Block k of length n of a corpus: a different stretch for every k."""
    pool = _pool(kind)
    s = (k * 40507 + n * 31) % (len(pool) - n)
    return pool[s:s + n]


def _skews(n):
    """Block i: source residue i % 16, destination residue (5 i + 3) % 16."""
    i = np.arange(n)
    return i % 16, (5 * i + 3) % 16


# ---------------------------------------------------------------------------
# compress
# ---------------------------------------------------------------------------

LDS_LENGTHS = [0, 1, 12, 13, 14, 100, 4095, 4096]
HBM_LENGTHS = [13, 4097, 20000, 65536]


def _compress_case(gpu, kind, cls, lengths):
    blocks = [_cut(kind, n, i) for n in lengths for i in range(16)]
    ss, ds = _skews(16)
    ss, ds = np.tile(ss, len(lengths)), np.tile(ds, len(lengths))
    r, frames, aux = gpu_batch.compress(gpu, blocks, [cls] * len(blocks), src_skew=ss, dst_skew=ds,
                                        max_len=max(lengths))
    for i, b in enumerate(blocks):
        er, ef, efs, elr = oracle_ref.compress(b, cls)
        where = (kind, cls, len(b), f"src {ss[i]} dst {ds[i]} mod 16")
        assert r[i] == er, where
        assert frames[i] == ef, where
        assert (aux[i][0], aux[i][1]) == (efs, elr), where


@pytest.mark.parametrize("kind", CORPORA)
@pytest.mark.parametrize("cls", [BYU16, BYU32], ids=["byU16", "byU32"])
def test_compress_lds_staged_launch_every_residue(gpu, cls, kind):
    """max_len <= 4096: the block is staged in LDS (stage_block: vector loads
    on the grid, the byte loop off it) and parsed from there."""
    _compress_case(gpu, kind, cls, LDS_LENGTHS)


@pytest.mark.parametrize("kind", CORPORA)
@pytest.mark.parametrize("cls", [BYU16, BYU32], ids=["byU16", "byU32"])
def test_compress_hbm_launch_every_residue(gpu, cls, kind):
    """max_len > 4096: the parse reads HBM through the word-aligned window."""
    _compress_case(gpu, kind, cls, HBM_LENGTHS + ([65537, 131072] if cls == BYU32 else []))


@pytest.mark.parametrize("n", [4096, 20000], ids=["lds", "hbm"])
def test_compress_limited_output_skewed(gpu, n):
    """Capacities from 40 below to 11 above the oracle's frame size at skewed
    destinations: the limitedOutput checks decide as the oracle's do, and a
    refused block (return 0) stays inside its capacity too (guards)."""
    blocks, caps = [], []
    for k, delta in enumerate(range(-40, 12)):
        b = _cut("mixed", n, k % 4)
        full = oracle_ref.compress(b, BYU16)[0]
        blocks.append(b)
        caps.append(min(max(0, full + delta), compress_bound(n)))
    ss, ds = _skews(len(blocks))
    r, frames, _ = gpu_batch.compress(gpu, blocks, [BYU16] * len(blocks), caps, src_skew=ss, dst_skew=ds,
                                      max_len=n)
    refused = 0
    for i, b in enumerate(blocks):
        er, ef, _, _ = oracle_ref.compress(b, BYU16, cap=caps[i])
        assert r[i] == er, (i, caps[i], f"dst {ds[i]} mod 16")
        assert frames[i] == ef, (i, caps[i])
        refused += er == 0
    assert 0 < refused < len(blocks)


@pytest.mark.parametrize("n", [4096, 20000])
def test_compress_dict_every_source_residue(gpu, n):
    """lz4e_compress_batch_dev_dict: dictionaries of 5, 8, 100, 4096 and 65536
    bytes right before blocks at all 16 source residues."""
    pool = _pool("mixed")
    blocks, dicts = [], []
    for dsize in (5, 8, 100, 4096, 65536):
        for i in range(16):
            s0 = 65536 + (i * 52361 + dsize * 7) % (len(pool) - 65536 - n)
            dicts.append(pool[s0 - dsize:s0])
            blocks.append(pool[s0:s0 + n])
    ss, ds = _skews(len(blocks))
    r, frames, _ = gpu_batch.compress(gpu, blocks, [BYU32] * len(blocks), src_skew=ss, dst_skew=ds,
                                      dicts=dicts, max_len=n)
    for i, b in enumerate(blocks):
        er, ef = oracle_ref.compress_dict(b, dicts[i])
        where = (n, len(dicts[i]), f"src {ss[i]} dst {ds[i]} mod 16")
        assert r[i] == er, where
        assert frames[i] == ef, where


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _decode_cases(sizes, reps):
    """Oracle frames for outputs of `sizes` bytes of the three corpora, each in
    four variants -- exact capacity, capacity + 32, capacity short by 1..40,
    frame truncated -- `reps` times over (other data each time), with the
    oracle's value and bytes, and a source and a destination residue per
    case: all 4 word residues of the source cross all 16 destination residues,
    once over the cases that decode and once over those that are refused."""
    rng = np.random.default_rng(len(sizes) * 1000 + reps)
    frames, caps, want, labels = [], [], [], []
    for rep in range(reps):
        for n in sizes:
            for kind in CORPORA:
                b = _cut(kind, n, rep)
                f = oracle_ref.compress(b, BYU16)[1]
                for variant in ("exact", "plus32", "short", "truncated"):
                    ff, cap = f, n
                    if variant == "plus32":
                        cap = n + 32
                    elif variant == "short":
                        cap = max(0, n - int(rng.integers(1, 41)))
                    elif variant == "truncated":
                        ff = f[:int(rng.integers(1, len(f)))]
                    frames.append(ff)
                    caps.append(cap)
                    want.append(oracle_ref.decompress(ff, cap))
                    labels.append(f"{kind}-{n}-{variant}")
    # Placements are dealt to the accepted and to the rejected cases separately
    # (only an accepted case has its bytes compared): the a-th of either kind
    # sits at placement 37 a mod 64 (a permutation of 0..63, so neighbouring
    # sizes and variants land far apart), source residue q % 4 plus a multiple
    # of 4, destination residue q // 4.
    ss, ds = np.zeros(len(frames), np.int64), np.zeros(len(frames), np.int64)
    for kind in (True, False):
        for a, i in enumerate([i for i, (r, _) in enumerate(want) if (r >= 0) == kind]):
            q = 37 * a % 64
            ss[i], ds[i] = q % 4 + 4 * ((a // 7) % 4), q // 4
    return frames, caps, want, labels, ss, ds


def _decode_check(gpu, mode, sizes, reps):
    frames, caps, want, labels, ss, ds = _decode_cases(sizes, reps)
    for kind in (True, False):  # decoded and compared byte for byte / refused
        assert len({(int(s) % 4, int(d)) for s, d, (r, _) in zip(ss, ds, want) if (r >= 0) == kind}) == 64
    for n in sizes:  # every size decodes at many destination residues
        assert len({int(d) for d, lb, (r, _) in zip(ds, labels, want) if r >= 0 and f"-{n}-" in lb}) >= 10
    r, outs = gpu_batch.decompress(gpu, frames, caps, mode=mode, src_skew=ss, dst_skew=ds)
    for i, (er, eb) in enumerate(want):
        where = (DEC_NAMES[mode], labels[i], f"src {ss[i]} dst {ds[i]} mod 16", r[i], er)
        assert r[i] == er, where
        if er >= 0:
            assert outs[i] == eb, where


@pytest.mark.parametrize("mode", ALL_MODES, ids=_ids(ALL_MODES))
def test_decode_small_blocks_every_placement(gpu, mode):
    """Outputs of up to 4608 bytes.  The forced LDS form (`small`) takes a
    block only when its capacity is <= 4608 and it has no dictionary: the
    4608 + 32 capacities here decode on the one-wave HBM form instead."""
    _decode_check(gpu, mode, (1, 13, 100, 4095, 4096, 4608), 4)


@pytest.mark.parametrize("mode", LARGE_MODES, ids=_ids(LARGE_MODES))
def test_decode_large_blocks_every_placement(gpu, mode):
    _decode_check(gpu, mode, (20000, 65536), 6)


@functools.lru_cache(maxsize=None)
def _dict_cases(sizes):
    pool = _pool("mixed")
    rng = np.random.default_rng(sum(sizes))
    frames, caps, dicts, want, labels = [], [], [], [], []
    k = 0
    for di, dsize in enumerate((5, 100, 4096, 65536)):
        for res in range(16):
            n = sizes[res % len(sizes)]
            s0 = 65536 + (k * 48619) % (len(pool) - 65536 - n)
            k += 1
            dic, blk = pool[s0 - dsize:s0], pool[s0:s0 + n]
            # the block opens with a repeat of the dictionary's tail: matches
            # start in the dictionary and run on into the block
            blk = ((dic[-200:] * 3)[:int(rng.integers(20, 90))] + blk)[:n]
            f = oracle_ref.compress_dict(blk, dic)[1]
            cap = n
            variant = ("exact", "plus32", "short", "truncated")[(res + res // 4 + di) % 4]
            if variant == "plus32":
                cap += 32
            elif variant == "short":
                cap = max(0, n - int(rng.integers(1, 41)))
            elif variant == "truncated":
                f = f[:int(rng.integers(1, len(f)))]
            frames.append(f)
            caps.append(cap)
            dicts.append(dic)
            want.append(oracle_ref.decompress_dict(f, cap, dic))
            labels.append(f"dict{dsize}-{n}-{variant}")
    j = np.arange(len(frames))
    return frames, caps, dicts, want, labels, (3 * j + 1) % 16, j % 16


def _dict_check(gpu, mode, sizes):
    frames, caps, dicts, want, labels, ss, ds = _dict_cases(sizes)
    assert {int(d) for d, (r, _) in zip(ds, want) if r >= 0} == set(range(16))
    r, outs = gpu_batch.decompress(gpu, frames, caps, mode=mode, src_skew=ss, dst_skew=ds, dicts=dicts)
    for i, (er, eb) in enumerate(want):
        where = (DEC_NAMES[mode], labels[i], f"src {ss[i]} dst {ds[i]} mod 16", r[i], er)
        assert r[i] == er, where
        if er >= 0:
            assert outs[i] == eb, where


@pytest.mark.parametrize("mode", ALL_MODES, ids=_ids(ALL_MODES))
def test_decode_dict_small_blocks_skewed_outputs(gpu, mode):
    """lz4e_debug_decompress_dict (forced decoders) and
    lz4e_decompress_batch_dev_dict (auto): dictionaries of 5, 100, 4096 and
    65536 bytes right before outputs at all 16 destination residues (every
    residue with a frame that decodes).  A block with a dictionary never takes
    the LDS form: the `small` case decodes on the one-wave HBM form, like
    `wave`."""
    _dict_check(gpu, mode, (100, 4096, 1500))


@pytest.mark.parametrize("mode", LARGE_MODES, ids=_ids(LARGE_MODES))
def test_decode_dict_large_blocks_skewed_outputs(gpu, mode):
    _dict_check(gpu, mode, (20000,))
