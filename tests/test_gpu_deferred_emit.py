"""The compressor's deferred emit on the GPU: blocks whose output is unlimited
record their sequences and write the frame 64 records at a time (flush_records,
lz4-sgori_amd/csrc/lz4e_compress.hip).  Frames, return values and iterator
post-states equal the oracle's with 64, 128 and the default number of record
slots per block (LZ4E_COMPRESS_RECORDS): blocks of several sizes and data
kinds in every table class through the HBM-image kernel, blocks whose frames
hold a number of sequences right at the record buffer's size, limited blocks
(inline emit) mixed with unlimited ones, and guard bytes after every slot
(tests/gpu_batch.py checks them on every call).
"""
import numpy as np
import pytest

import gpu_batch
import oracle_ref
import parse_synth as ps
from lz4e_amd import corpus

pytestmark = pytest.mark.gpu

_CLS = [pytest.param(tt, id=ps.CLASS_NAME[tt]) for tt in ps.CLASSES]
RINGS = [pytest.param("64", id="r64"), pytest.param("128", id="r128"), pytest.param(None, id="default")]
SIZES = (4097, 4608, 8193, 65536)
HBM = 4097  # max_len above the 4096-byte staging limit: the HBM-image kernel


def _records32(n, rng):
    """32-byte records: a fixed layout in which a few bytes change per record."""
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    arr = np.tile(base, (n // 32 + 1, 1))
    arr[:, 3] = rng.integers(0, 256, arr.shape[0])
    arr[:, 17:19] = rng.integers(0, 4, (arr.shape[0], 2))
    return arr.reshape(-1)[:n]


def _long_runs(n, rng):
    """Runs of one byte, 300 to 3000 long (match-length extensions of two to
    twelve bytes), a few random bytes between them."""
    out = np.empty(0, np.uint8)
    while out.size < n:
        run = np.full(int(rng.integers(300, 3000)), rng.integers(0, 256), np.uint8)
        out = np.concatenate([out, run, rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8)])
    return out[:n]


KINDS = {
    "text": lambda n, rng: corpus.text_proxy(n, int(rng.integers(1, 1 << 30))),
    "records": _records32,
    "runs": _long_runs,
    "random": lambda n, rng: rng.integers(0, 256, n, dtype=np.uint8),  # one literal run of n bytes
}


@pytest.fixture(scope="module")
def expected():
    """(block, class, capacity) -> the oracle's (ret, frame, final_src, last_run), computed once."""
    memo = {}

    def get(block, tt, cap=None):
        k = (block, tt, cap)
        if k not in memo:
            memo[k] = oracle_ref.compress(block, tt, cap) if cap is not None else oracle_ref.compress(block, tt)
        return memo[k]
    return get


@pytest.fixture(scope="module")
def kind_blocks():
    rng = np.random.default_rng(0xDEFE)
    return [(f"{kind}{n}", bytes(make(n, rng).tobytes())) for n in SIZES for kind, make in KINDS.items()]


def _ring(monkeypatch, ring):
    if ring is None:
        monkeypatch.delenv("LZ4E_COMPRESS_RECORDS", raising=False)
    else:
        monkeypatch.setenv("LZ4E_COMPRESS_RECORDS", ring)


def _check(gpu, expected, labelled, tts, caps=None, dst_skew=None):
    blocks = [b for _, b in labelled]
    r, frames, aux = gpu_batch.compress(gpu, blocks, tts, caps=caps, max_len=max(HBM, max(map(len, blocks))),
                                        dst_skew=dst_skew)
    for i, (label, b) in enumerate(labelled):
        er, ef, efs, elr = expected(b, tts[i], None if caps is None else int(caps[i]))
        assert int(r[i]) == er, (label, tts[i], int(r[i]), er)
        assert frames[i] == ef, (label, tts[i])
        if er > 0:
            assert (aux[i][0], aux[i][1]) == (efs, elr), (label, tts[i])


@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("tt", _CLS)
def test_sizes_and_kinds(gpu, expected, kind_blocks, monkeypatch, tt, ring):
    """(a) 4 097, 4 608, 8 193 and 65 536 bytes of text, 32-byte records, long
    runs and random bytes (65 536 random bytes: one literal run)."""
    _ring(monkeypatch, ring)
    _check(gpu, expected, kind_blocks, [tt] * len(kind_blocks),
           dst_skew=[(7 * i + 1) % 16 for i in range(len(kind_blocks))])


@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("tt", _CLS)
def test_planted_families(gpu, expected, monkeypatch, tt, ring):
    """(a) every planted case of the class through the HBM-image kernel."""
    _ring(monkeypatch, ring)
    cs = ps.plain_cases(tt)
    _check(gpu, expected, [(c.label, c.block) for c in cs], [tt] * len(cs))


def _unit_block(units, seed, copy=4):
    """`units` units of 4 fresh bytes and a copy of the `copy` bytes that end
    where the fresh ones begin (8-byte units; byU32 hashes 5 bytes, so its
    units copy 5)."""
    rng = np.random.default_rng(seed)
    out = bytearray(rng.integers(0, 256, 8, dtype=np.uint8).tobytes())
    for _ in range(units):
        out += bytes(rng.integers(0, 256, 4, dtype=np.uint8).tobytes())
        out += out[-4 - copy:-4]
    return bytes(out) + b"\x00\x01\x02\x03\x04\x05\x06\x07\x08\x09\x0a\x0b\x0c"


def _block_with_sequences(want, tt):
    """A unit block whose oracle frame holds exactly `want` match sequences."""
    for seed in range(16):
        for units in range(max(1, want - 4), want + 48):
            b = _unit_block(units, 1000 * want + seed, ps.hash_width(tt))
            got = len(ps.parse_frame(oracle_ref.compress(b, tt)[1])[0])
            if got == want:
                return b
            if got > want:
                break
    raise AssertionError(f"no unit block with {want} sequences")


@pytest.mark.parametrize("slots", [64, 128, 1024])
def test_sequence_counts_at_the_buffer_size(gpu, expected, monkeypatch, slots):
    """(b) frames of exactly R - 2 .. R + 1, 2R - 1 and 2R sequences for R
    record slots (1 024: the default), counted in the oracle's frame."""
    monkeypatch.setenv("LZ4E_COMPRESS_RECORDS", str(slots))
    counts = [slots - 2, slots - 1, slots, slots + 1, 2 * slots - 1, 2 * slots]
    labelled, tts = [], []
    for tt in ps.CLASSES:
        for want in counts:
            b = _block_with_sequences(want, tt)
            assert len(ps.parse_frame(expected(b, tt)[1])[0]) == want
            labelled.append((f"units{want}", b))
            tts.append(tt)
    _check(gpu, expected, labelled, tts, dst_skew=[(3 * i) % 16 for i in range(len(tts))])


@pytest.mark.parametrize("ring", RINGS)
def test_limited_among_unlimited(gpu, expected, kind_blocks, monkeypatch, ring):
    """(c) limited blocks (capacity one byte and more under the bound: inline
    emit, some refused) between unlimited ones in one batch."""
    _ring(monkeypatch, ring)
    picked = [kb for kb in kind_blocks if len(kb[1]) <= 8193]
    labelled, tts, caps = [], [], []
    for i, (label, b) in enumerate(picked):
        tt = ps.CLASSES[i % 3]
        bound = ps.bound(len(b))
        full = expected(b, tt)[0]
        for cap in (bound, bound - 1, full, full - 1, bound, len(b) // 2):
            labelled.append((f"{label}@{cap}", b))
            tts.append(tt)
            caps.append(cap)
    assert any(expected(b, tt, c)[0] == 0 for (_, b), tt, c in zip(labelled, tts, caps))
    _check(gpu, expected, labelled, tts, caps=caps, dst_skew=[(5 * i + 3) % 16 for i in range(len(tts))])
