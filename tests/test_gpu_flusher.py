"""The compressor's two-wave blocks on the GPU: a block of the HBM-image kernel
whose output is unlimited is parsed by wave 0 and written by wave 1, the
flusher, from the records wave 0 publishes (flusher_wave,
lz4-sgori_amd/csrc/lz4e_compress.hip).  Frames, return values and post-states
equal the oracle's, byte for byte, with 64, 128 and the default number of
record slots per block (LZ4E_COMPRESS_RECORDS), in batches of 300-600 blocks
so that several workgroups share a CU: the inputs of tests/flusher_inputs.py
and every planted case, spread among 100-200 blocks of 16-64 KiB of text,
8-byte units and random bytes; limited blocks (inline emit, wave 1 leaves at once) mixed with
unlimited ones; the byU32 class with a dictionary; and a batch of 4 KiB blocks,
which the one-wave LDS-image kernel compresses as before.  tests/gpu_batch.py
checks the guard bytes around every slot on every call.
"""
import numpy as np
import pytest

import flusher_inputs as fi
import gpu_batch
import oracle_ref
import parse_synth as ps
from lz4e_amd import BYU16, BYU32, corpus

pytestmark = pytest.mark.gpu

RINGS = [pytest.param("64", id="r64"), pytest.param("128", id="r128"), pytest.param(None, id="default")]
SIZES = (16384, 24577, 32768, 49153, 65536)


def _ring(monkeypatch, ring):
    if ring is None:
        monkeypatch.delenv("LZ4E_COMPRESS_RECORDS", raising=False)
    else:
        monkeypatch.setenv("LZ4E_COMPRESS_RECORDS", ring)


def _filler(count, seed):
    """`count` blocks of 16-64 KiB: text, 8-byte units and random bytes in turn -> [(label, block, class)]."""
    out = []
    for i in range(count):
        n = SIZES[i % len(SIZES)]
        tt = ps.CLASSES[i % 3]
        if i % 3 == 0:
            b = corpus.text_proxy(n, seed + i).tobytes()
        elif i % 3 == 1:
            b = fi.units(n, seed + i, copy=ps.hash_width(tt))
        else:
            b = fi.random_bytes(n, seed + i)
        out.append((f"fill{i}", b, tt))
    return out


def _spread(small, filler):
    """The filler blocks spread evenly among the small ones."""
    step = max(1, len(small) // len(filler))
    out = []
    for i, f in enumerate(filler):
        out += small[i * step:(i + 1) * step] + [f]
    return out + small[len(filler) * step:]


@pytest.fixture(scope="module")
def batches():
    """Two batches of 300-600 blocks with the oracle's results, computed once:
    the special blocks and the byU16 planted cases among 200 blocks of
    16-64 KiB, the byU32 and byU64 planted cases among 100."""
    fi.check_special_blocks()
    planted = {tt: [(c.label, c.block, c.tt) for c in ps.plain_cases(tt)] for tt in ps.CLASSES}
    rest = [x for pair in zip(planted[ps.CLASSES[1]], planted[ps.CLASSES[2]]) for x in pair]
    rest += planted[ps.CLASSES[1]][len(rest) // 2:] + planted[ps.CLASSES[2]][len(rest) // 2:]
    assert len(rest) == len(planted[ps.CLASSES[1]]) + len(planted[ps.CLASSES[2]])
    out = []
    for small, nfill, seed in ((fi.special_blocks() + planted[BYU16], 200, 500), (rest, 100, 800)):
        labelled = _spread(small, _filler(nfill, seed))
        assert 300 <= len(labelled) <= 600, len(labelled)
        out.append((labelled, [oracle_ref.compress(b, tt) for _, b, tt in labelled]))
    return out


def _check(gpu, labelled, expected, caps=None):
    r, frames, aux = gpu_batch.compress(gpu, [b for _, b, _ in labelled], [tt for _, _, tt in labelled], caps=caps,
                                        max_len=65536, dst_skew=[(7 * i + 1) % 16 for i in range(len(labelled))])
    for i, (label, _, tt) in enumerate(labelled):
        er, ef, efs, elr = expected[i]
        assert int(r[i]) == er, (label, tt, int(r[i]), er)
        assert frames[i] == ef, (label, tt)
        if er > 0:
            assert (aux[i][0], aux[i][1]) == (efs, elr), (label, tt)


@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("which", [0, 1], ids=["special-u16", "u32-u64"])
def test_two_wave_batch(gpu, batches, monkeypatch, which, ring):
    _ring(monkeypatch, ring)
    _check(gpu, *batches[which])


@pytest.mark.parametrize("ring", RINGS)
def test_limited_blocks_among_two_wave_blocks(gpu, batches, monkeypatch, ring):
    """Every third block one byte under its bound: it emits inline on wave 0
    (wave 1 leaves at once), its neighbours defer."""
    _ring(monkeypatch, ring)
    labelled, full = batches[0]
    caps, expected = [], []
    for i, (_, b, tt) in enumerate(labelled):
        limited = i % 3 == 1
        caps.append(ps.bound(len(b)) - (1 if limited else 0))
        expected.append(oracle_ref.compress(b, tt, caps[-1]) if limited else full[i])
    _check(gpu, labelled, expected, caps=caps)


@pytest.mark.parametrize("ring", RINGS)
def test_dictionary_batch_two_waves(gpu, monkeypatch, ring):
    """byU32 with a dictionary: the parse starts behind the dictionary, the
    flusher's input position too.  300 blocks of 16 KiB text and units against
    8 KiB dictionaries, and the planted dictionary cases."""
    _ring(monkeypatch, ring)
    blocks, dicts = [], []
    for i in range(300 - len(ps.cases("dict", BYU32))):
        text = corpus.text_proxy(16384 + 8192, 900 + i % 7).tobytes()
        dicts.append(text[:8192] if i % 5 else b"")
        blocks.append(text[8192:] if i % 2 else fi.units(16384, 40 + i, copy=5))
    for c in ps.cases("dict", BYU32):
        blocks.append(c.block)
        dicts.append(c.dic)
    r, frames, _ = gpu_batch.compress(gpu, blocks, [BYU32] * len(blocks), dicts=dicts, max_len=16384)
    memo = {}
    for i, (b, d) in enumerate(zip(blocks, dicts)):
        if (b, d) not in memo:
            memo[(b, d)] = oracle_ref.compress_dict(b, d)
        er, ef = memo[(b, d)]
        assert int(r[i]) == er, (i, int(r[i]), er)
        assert frames[i] == ef, i


def test_small_blocks_keep_the_one_wave_kernel(gpu):
    """512 blocks of at most 4 KiB (max_len 4 096: the LDS-image kernel)."""
    rng = np.random.default_rng(4)
    blocks, tts = [], []
    for i in range(512):
        n = int(rng.integers(0, 4097)) if i % 4 else 4096
        kind = i % 3
        b = corpus.text_proxy(max(n, 16), 70 + i).tobytes()[:n] if kind == 0 else \
            (fi.units(n + 8, 90 + i)[:n] if kind == 1 else fi.random_bytes(n, 110 + i))
        blocks.append(b)
        tts.append(ps.CLASSES[i % 3])
    r, frames, aux = gpu_batch.compress(gpu, blocks, tts, max_len=4096)
    for i, (b, tt) in enumerate(zip(blocks, tts)):
        er, ef, efs, elr = oracle_ref.compress(b, tt)
        assert int(r[i]) == er and frames[i] == ef and (aux[i][0], aux[i][1]) == (efs, elr), (i, len(b), tt)
