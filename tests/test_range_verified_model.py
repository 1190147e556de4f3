"""The verified range read without a GPU: tests/range_verified_model.py's
statement of lz4e_unpack_range_verified_batch_dev's four rules on hand-written
indexes (every expected value written out here), the model against the plain
range read's rules on a clean column, the damage the GPU test plants, and the
entry point's argument checks through ctypes."""
import ctypes
import os

import numpy as np
import pytest

import crc_model
import oracle_ref
import pack_model
import partial_model
import range_verified_model as rv
from lz4e_amd import BYU16

BAD = -2147483647
FRAME, RAW = 0, 1


def _store(entries):
    """entries: [(kind, stored bytes, pk_len or None, crc or None)] at align 8
    -> (image, pk_off, pk_len, pk_kind, pk_crc); None: the true value."""
    off, image = [], bytearray()
    for _, body, _, _ in entries:
        off.append(len(image))
        image += body + b"\xEE" * (-len(body) % 8)
    off.append(len(image))
    ln = [len(b) if l is None else l for _, b, l, _ in entries]
    crc = [crc_model.crc32c(b) if c is None else c for _, b, _, c in entries]
    return (np.frombuffer(bytes(image), np.uint8), np.array(off, np.int64), np.array(ln, np.int32),
            np.array([k for k, _, _, _ in entries], np.uint8), np.array(crc, np.uint32))


def test_crc_of_the_empty_string_is_zero():
    assert crc_model.crc32c(b"") == 0 and rv.crc_of(b"123456789") == 0xE3069283


def test_the_four_rules_on_a_hand_written_index():
    lit = bytes([0x80]) + b"abcdefgh"  # one run of 8 literals
    assert partial_model.decode(lit, 5, True) == (5, b"abcde")
    hello = b"hello world!"
    twenty = bytes(range(100, 120))
    store = _store([
        (RAW, hello, None, None),                                 # 0 clean
        (RAW, twenty, None, crc_model.crc32c(twenty) ^ 0x400),    # 1 a wrong pk_crc
        (RAW, b"", None, 0),                                      # 2 empty, pk_crc 0
        (RAW, b"", None, 1),                                      # 3 empty, pk_crc 1
        (2, twenty, None, 7),                                     # 4 an unknown kind, and a wrong checksum too
        (FRAME, lit, None, None),                                 # 5 clean frame
        (FRAME, lit, None, crc_model.crc32c(lit) ^ 1),            # 6 the same frame, refused
        (RAW, twenty, -20, None),                                 # 7 a negative length
    ])
    reqs = [(1, 0, 5), (1, 3, 4), (1, 2, 0),          # a damaged entry named three times, once for nothing
            (1, -1, 4), (1, 2, -4), (4, 0, 4),        # invalid requests on damaged entries
            (2, 0, 8), (2, 5, 1), (2, 0, 0),          # an empty entry with the empty string's checksum
            (3, 0, 8), (3, 0, 0),                     # and with another
            (0, 6, 100), (0, 0, 5), (0, 12, 3), (0, 40, 3),
            (5, 0, 5), (5, 2, 3), (5, 2, 100), (6, 0, 5), (6, 0, 0),
            (7, 0, 4), (8, 0, 4), (-1, 0, 0)]
    got = rv.expected(*store, reqs)
    assert got == [(BAD, b""), (BAD, b""), (0, b""),
                   (-1, b""), (-1, b""), (-1, b""),
                   (0, b""), (0, b""), (0, b""),
                   (BAD, b""), (0, b""),
                   (6, b"world!"), (5, b"hello"), (0, b""), (0, b""),
                   (5, b"abcde"), (3, b"cde"), (6, b"cdefgh"), (BAD, b""), (0, b""),
                   (-1, b""), (-1, b""), (-1, b"")]
    # max_end clamps a request's end
    assert rv.expected(*store, [(0, 6, 100), (5, 2, 100), (1, 0, 50)], max_end=8) == [(2, b"wo"), (6, b"cdefgh"), (BAD, b"")]
    # the padding is not covered
    image = store[0].copy()
    image[int(store[1][0]) + len(hello)] ^= 0xFF
    assert rv.expected(image, *store[1:], [(0, 0, 5)]) == [(5, b"hello")]
    image[int(store[1][0]) + len(hello) - 1] ^= 0x01
    assert rv.expected(image, *store[1:], [(0, 0, 5), (0, 0, 0)]) == [(BAD, b""), (0, b"")]


def _plain(image, pk_off, pk_len, pk_kind, reqs):
    """lz4e_unpack_range_batch_dev's rules, as tests/test_gpu_range.py states them."""
    n = len(pk_len)
    out = []
    for e, lo, ln in reqs:
        if not (0 <= e < n) or lo < 0 or ln < 0 or pk_kind[e] not in (FRAME, RAW) or pk_len[e] < 0:
            out.append((-1, b""))
        elif ln == 0:
            out.append((0, b""))
        else:
            body = image[int(pk_off[e]):int(pk_off[e]) + int(pk_len[e])].tobytes()
            if pk_kind[e] == RAW:
                d, data = min(len(body), lo + ln), body
            else:
                d, data = partial_model.decode(body, lo + ln, True)
            out.append((d, b"") if d < 0 else (max(0, d - lo), data[lo:d]))
    return out


def test_with_a_clean_column_the_model_is_the_plain_range_read():
    blocks = [pack_model.text_block(3000, 1), pack_model.random_block(700, 2), b"", pack_model.text_block(1500, 3),
              pack_model.text_block(64, 4), pack_model.random_block(1, 5)]
    tts = [BYU16] * len(blocks)
    caps = [len(b) + len(b) // 255 + 16 for b in blocks]
    rets, frames = pack_model.oracle_frames(blocks, tts, caps)
    image, pk_off, pk_len, pk_kind = pack_model.pack_expected(blocks, frames, rets, 16)
    assert (pk_kind == FRAME).sum() >= 2 and (pk_kind == RAW).sum() >= 3
    # a frame that fails half way, an unknown kind and a negative length: the clean column covers them as they are
    image = image.copy()
    at = int(pk_off[3])
    p, bad = rv.rejected_damage(image[at:at + int(pk_len[3])].tobytes(), 1000)
    image[at:at + len(bad)] = np.frombuffer(bad, np.uint8)
    pk_kind[4], pk_len[5] = 9, -1
    crc = rv.crc_column(image, pk_off[:-1], pk_len)
    assert np.array_equal(crc, crc_model.crc_column(image, pk_off[:-1], pk_len))
    rng = np.random.default_rng(11)
    reqs = [(int(rng.integers(-1, 8)), int(rng.integers(-2, 3200)), int(rng.integers(-1, 900))) for _ in range(400)]
    reqs += [(e, lo, ln) for e in range(6) for lo in (0, 1, 2999, 3000) for ln in (0, 1, 4096)]
    want = _plain(image, pk_off, pk_len, pk_kind, reqs)
    assert any(v < -1 for v, _ in want) and any(v == -1 for v, _ in want) and any(v > 0 for v, _ in want)
    assert rv.expected(image, pk_off, pk_len, pk_kind, crc, reqs) == want


def test_the_damage_the_gpu_test_plants_is_found_on_its_frame():
    """tests/test_gpu_range_verified.py damages entry 0 of its store, the
    frame of text_block(65536, 40), so that the partial decode rejects it and
    recomputes pk_crc: the search must find such damage, and the model then
    lets the decode error through (rule 4)."""
    block = pack_model.text_block(65536, 40)
    r, frame = oracle_ref.compress(block, BYU16, cap=65536 + 65536 // 255 + 16)[:2]
    assert 0 < r < 65536
    found = rv.rejected_damage(bytes(frame[:r]))
    assert found is not None
    p, bad = found
    assert 2 <= p < 600 and len(bad) == r and bad != bytes(frame[:r])
    store = _store([(FRAME, bad, None, None), (FRAME, bad, None, crc_model.crc32c(bytes(frame[:r])))])
    got = rv.expected(*store, [(0, 0, 4096), (0, 60000, 5000), (1, 0, 4096)])
    assert got[0][0] < -1 and got[1][0] < -1 and got[0][0] != BAD and got[1][0] != BAD
    assert got[2] == (BAD, b"")


# ---- the entry point's argument checks: no GPU is touched ---------------------

def test_the_symbol_and_its_checks_before_any_hip_call(amd):
    L = amd.lib()
    f = L.lz4e_unpack_range_verified_batch_dev
    assert "lz4e_unpack_range_verified_batch_dev" in amd.EXPORTED_SYMBOLS
    assert callable(amd.unpack_range_verified_batch_dev)
    null = [None] * 5
    # no request: nothing happens, whatever else is passed
    assert f(*null, 5, None, None, None, None, None, None, 0, 0x7FFFFFF1, 0, None) == 0
    assert f(*null, 0, None, None, None, None, None, None, 0, 0, 65536, None) == 0
    # max_end above the limit: refused before any pointer is looked at
    assert f(*null, 5, None, None, None, None, None, None, 1, 0x7FFFFFF1, 0, None) == -22
    assert b"max_end" in L.lz4e_last_error()
    assert f(*null, 0, None, None, None, None, None, None, 1, 0xFFFFFFFF, 65536, None) == -22
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lz4e.h")).read()
    assert "lz4e_unpack_range_verified_batch_dev(" in header and "no verified range read" not in header
