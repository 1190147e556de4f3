"""The packed frame store's numpy model (tests/pack_model.py) on hand-written
cases, and the oracle facts the GPU tests of the frame / raw decision rest
on: planted blocks whose frame is one byte smaller than, as large as and one
byte larger than the block, for each table class, and the sizes a store
meets in the field (random 4 KiB -> 4114, zeros -> 26, limited output -> 0).
No GPU."""
import numpy as np
import pytest

import oracle_ref
import pack_model
from pack_model import FRAME, RAW, pack_expected, plant, unpack_expected

CLASSES = (1, 3, 7)  # byU16, byU32, byU64


def test_model_by_hand():
    blocks = [b"abcdefgh", b"", b"xyz", b"0123456789", b"QQ"]
    frames = [b"FRAME", b"", b"LONGER!", b"0123456789", b"??"]
    rets = [5, 0, 7, 10, 0]  # a frame; empty; larger than the block; equal; a failed compress
    image, off, ln, kind = pack_expected(blocks, frames, rets, 1)
    assert kind.tolist() == [FRAME, RAW, RAW, RAW, RAW]
    assert ln.tolist() == [5, 0, 3, 10, 2]
    assert off.tolist() == [0, 5, 5, 8, 18, 20]
    assert image.tobytes() == b"FRAME" + b"xyz" + b"0123456789" + b"QQ"
    image, off, ln, kind = pack_expected(blocks, frames, rets, 4)
    assert off.tolist() == [0, 8, 8, 12, 24, 28]
    assert image.tobytes() == b"FRAME\0\0\0" + b"xyz\0" + b"0123456789\0\0" + b"QQ\0\0"
    assert off.dtype == np.int64 and ln.dtype == np.int32 and kind.dtype == np.uint8
    image, off, ln, kind = pack_expected([], [], [], 512)
    assert image.size == 0 and off.tolist() == [0] and ln.size == 0 and kind.size == 0


def test_model_alignment_and_ret_edges():
    blocks = [bytes(range(100)), bytes(100)]
    frames = [bytes(99) + b"!", bytes(200)]
    # ret == n - 1 is the largest frame kept; a negative ret is a failed compress
    image, off, ln, kind = pack_expected(blocks, frames, [99, -3], 4096)
    assert kind.tolist() == [FRAME, RAW] and ln.tolist() == [99, 100] and off.tolist() == [0, 4096, 8192]
    assert image[:99].tobytes() == frames[0][:99] and not image[99:4096].any()
    assert image[4096:4196].tobytes() == blocks[1] and not image[4196:].any()


def test_inverse_by_hand():
    image = np.frombuffer(b"rawbytes" + b"\x10a" + b"zz", dtype=np.uint8)
    off = np.array([0, 8, 10, 10, 12])
    ln = np.array([8, 2, 0, 2])
    kind = np.array([RAW, FRAME, RAW, 2])
    r, outs = unpack_expected(image, off, ln, kind, [8, 4, 0, 9], oracle_ref.decompress)
    assert r.tolist() == [8, 1, 0, -1] and outs == [b"rawbytes", b"a", b"", b""]
    r, outs = unpack_expected(image, off, ln, kind, [7, 0, 5, 9], oracle_ref.decompress)
    assert r[0] == -1 and outs[0] == b"" and r[1] < 0 and r[2] == 0


def test_model_round_trip_through_the_oracle():
    blocks = [pack_model.text_block(700, 1), pack_model.random_block(300, 2), bytes(512), b"", b"a"]
    comp = [oracle_ref.compress(b, 3) for b in blocks]
    rets, frames = [c[0] for c in comp], [c[1] for c in comp]
    for align in (1, 512):
        image, off, ln, kind = pack_expected(blocks, frames, rets, align)
        assert kind.tolist() == [FRAME, RAW, FRAME, RAW, RAW]
        r, outs = unpack_expected(image, off, ln, kind, [len(b) for b in blocks], oracle_ref.decompress)
        assert r.tolist() == [len(b) for b in blocks] and outs == blocks


@pytest.mark.parametrize("tt", CLASSES)
def test_boundary_plants_hit_all_three_differences(tt):
    """The frame / raw decision turns on ret < n: the plants give ret = n - 1
    (the last frame kept), n and n + 1 for every table class.  A plant that
    misses fails here; nothing downstream shrinks silently."""
    for diff, n in ((-1, 25), (0, 24), (+1, 32)):
        for seed in range(4):
            b = plant(diff, seed)
            assert len(b) == n
            r = oracle_ref.compress(b, tt)[0]
            assert r - len(b) == diff, (tt, diff, seed, r)
            assert pack_model.entry_of(len(b), r)[0] == (FRAME if diff < 0 else RAW)


@pytest.mark.parametrize("tt", CLASSES)
def test_oracle_sizes_a_store_meets(tt):
    rnd = pack_model.random_block(4096, 11)
    assert oracle_ref.compress(rnd, tt)[0] == 4114  # raw: the frame is larger
    assert oracle_ref.compress(bytes(4096), tt)[0] == 26  # frame
    for n in (13, 64, 1000, 4096):  # limited output on random data fails -> raw
        b = pack_model.random_block(n, n)
        assert oracle_ref.compress(b, tt, cap=n - 1)[0] == 0
