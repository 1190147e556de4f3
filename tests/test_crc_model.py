"""The store's checksum model (tests/crc_model.py) on published vectors and
hand-written cases: CRC-32C itself (RFC 3720 B.4 and the classic check
string), the pk_crc column of pack_model.pack_expected's image, and the ret
a verified unpack must give by include/lz4e.h's three-step rule.  No GPU."""
import numpy as np

import crc_model
import oracle_ref
import pack_model
from crc_model import BAD_CRC, crc32c, pack_crc_expected, unpack_verified_expected
from pack_model import FRAME, RAW, pack_expected


def test_published_vectors():
    assert crc32c(b"123456789") == 0xE3069283
    assert crc32c(bytes(32)) == 0x8A9136AA
    assert crc32c(b"\xff" * 32) == 0x62A8AB43
    assert crc32c(bytes(range(32))) == 0x46DD794E
    assert crc32c(bytes(range(31, -1, -1))) == 0x113FDB5C
    assert crc32c(b"") == 0


def test_striped_path_equals_bytewise():
    """Inputs of 256 KiB and more take the striped path: against the plain
    byte recurrence at the threshold, with and without a head."""
    rng = np.random.default_rng(3)
    for n in (64 * 4096 - 1, 64 * 4096, 64 * 4096 + 1, 300007):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert crc32c(d) == crc_model._bytewise(0xFFFFFFFF, d) ^ 0xFFFFFFFF, n


def test_zero_bytes_are_a_multiplication():
    """state(A || B) = state(A) x^(8 |B|) ^ state0(B), the identity the kernel's teams rest on."""
    rng = np.random.default_rng(4)
    for la, lb in ((0, 5), (1, 1), (7, 64), (100, 4097), (33, 0)):
        a = rng.integers(0, 256, la, dtype=np.uint8).tobytes()
        b = rng.integers(0, 256, lb, dtype=np.uint8).tobytes()
        sa = crc_model._bytewise(0xFFFFFFFF, a)
        assert crc_model._zeros(sa, lb) ^ crc_model._bytewise(0, b) == crc_model._bytewise(0xFFFFFFFF, a + b)
    assert crc_model._zeros(0x80000000, 1) == 0x00800000 and crc_model._zeros(0x80000000, 4) == 0x82F63B78


def test_pack_crc_column_by_hand():
    blocks = [b"abcdefgh", b"", b"xyz", b"123456789", b"QQ"]
    frames = [b"FRAME", b"", b"LONGER!", b"123456789", b"??"]
    rets = [5, 0, 7, 9, 0]
    for align in (1, 4, 512):
        image, off, ln, kind = pack_expected(blocks, frames, rets, align)
        col = pack_crc_expected(image, off, ln)
        assert col.dtype == np.uint32
        # the stored bytes only: the padding changes nothing
        assert col.tolist() == [crc32c(b"FRAME"), 0, crc32c(b"xyz"), 0xE3069283, crc32c(b"QQ")]
    assert pack_crc_expected(*pack_expected([], [], [], 512)[:3]).size == 0


def _store():
    text = pack_model.text_block(700, 1)
    blocks = [text, pack_model.random_block(300, 2), bytes(512), b"", b"a"]
    comp = [oracle_ref.compress(b, 3) for b in blocks]
    image, off, ln, kind = pack_expected(blocks, [c[1] for c in comp], [c[0] for c in comp], 16)
    return blocks, image, off, ln, kind, pack_crc_expected(image, off, ln)


def test_verified_unpack_of_a_clean_image_is_the_plain_unpack():
    blocks, image, off, ln, kind, col = _store()
    caps = [len(b) for b in blocks]
    assert kind.tolist() == [FRAME, RAW, FRAME, RAW, RAW]
    r, outs = unpack_verified_expected(image, off, ln, kind, col, caps, oracle_ref.decompress)
    assert r.tolist() == caps and outs == blocks
    # a raw entry over its capacity is the plain unpack's -1, not a checksum matter
    caps[1] -= 1
    r, outs = unpack_verified_expected(image, off, ln, kind, col, caps, oracle_ref.decompress)
    assert r.tolist() == [700, -1, 512, 0, 1] and outs[1] == b""


def test_verified_unpack_three_step_rule():
    blocks, image, off, ln, kind, col = _store()
    caps = [len(b) for b in blocks]
    # one flipped bit in a frame, in a raw entry, and in the padding after the last entry
    bad = image.copy()
    bad[off[0] + 3] ^= 0x10
    bad[off[1] + ln[1] - 1] ^= 0x01
    bad[off[4] + ln[4]] ^= 0x80
    r, outs = unpack_verified_expected(bad, off, ln, kind, col, caps, oracle_ref.decompress)
    assert r.tolist() == [BAD_CRC, BAD_CRC, 512, 0, 1]
    assert outs[0] == b"" and outs[1] == b"" and outs[2:] == blocks[2:]
    # an intact entry with a wrong pk_crc; the empty entry's checksum is 0 and nothing else
    wrong = col.copy()
    wrong[2] ^= 1
    wrong[3] = 5
    r, _ = unpack_verified_expected(image, off, ln, kind, wrong, caps, oracle_ref.decompress)
    assert r.tolist() == [700, 300, BAD_CRC, BAD_CRC, 1]
    # rule 1 comes first: unknown kinds and a negative length are -1 whatever the checksum says,
    # and a raw entry over capacity with a bad checksum is a checksum failure
    k2, l2, c2 = kind.copy(), ln.copy(), list(caps)
    k2[0], k2[1], l2[2] = 2, 255, -4
    c2[4] = 0
    wrong = col.copy()
    wrong[4] ^= 0x8000
    r, _ = unpack_verified_expected(bad, off, l2, k2, wrong, c2, oracle_ref.decompress)
    assert r.tolist() == [-1, -1, -1, 0, BAD_CRC]
    assert BAD_CRC == -(2 ** 31) + 1 and BAD_CRC < -0x7E000001
