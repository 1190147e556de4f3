"""Verified range reads from the packed frame store on the GPU
(lz4e_unpack_range_verified_batch_dev) against tests/range_verified_model.py.

The store is tests/test_gpu_range.py's: 40 blocks of 64 KiB compressed and
packed on the device at align 512 -- text, incompressible blocks (stored raw),
an empty block and blocks whose compress was refused (stored raw) -- plus the
checksum column lz4e_pack_crc_batch_dev wrote, checked against crc_model
first.  With max_len = 65536 the checksum's teams span four workgroups, the
smallest shape that reaches the partial + combine path.  Every destination
slot is exactly the bytes the request must get, inside a pattern-filled
tensor; the image must be unchanged after every call.  Every damage case runs
on a copy of the image of its own, with clean entries served in the same call.
Nothing here provokes a fault: a damaged entry is hidden from every kernel
that would trust it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import crc_model
import pack_model
import range_verified_model as rv
from lz4e_amd import BYU16
from range_verified_model import BAD_CRC

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS = 65536
N = 40
RANDOM, EMPTY, REFUSED = (3, 17), (9,), (5, 22)


class Store:
    pass


@pytest.fixture(scope="module")
def store(gpu):
    texts = [pack_model.text_block(BS, 40 + s) for s in range(4)]
    blocks = []
    for i in range(N):
        if i in RANDOM:
            blocks.append(pack_model.random_block(BS, i))
        elif i in EMPTY:
            blocks.append(b"")
        else:
            blocks.append(texts[i % 4])
    lens = np.array([len(b) for b in blocks], dtype=np.int64)
    caps = lens + lens // 255 + 16
    caps[list(REFUSED)] = 100  # a refused compress: a capacity below what the block needs
    tts = [BYU16] * N
    k = np.arange(N)
    st = pack_model.DevStore(gpu, blocks, src_skew=k % 16).compress(tts, caps, dst_skew=k * 5 % 16)
    rets, frames = pack_model.oracle_frames(blocks, tts, caps)
    assert np.array_equal(st.ret.cpu().numpy(), rets)
    image, *want = pack_model.pack_expected(blocks, frames, rets, 512)
    got = st.pack(512, image.size, skew=5)
    pack_model.check_index(got, want, "pack")
    st.packed.check(image, "pack")
    s = Store()
    s.blocks, s.image = blocks, image
    s.pk_off, s.pk_len, s.pk_kind = want
    assert all(s.pk_kind[i] == pack_model.RAW for i in RANDOM + EMPTY + REFUSED)
    assert sum(s.pk_kind == pack_model.FRAME) == N - 5
    g, col = crc_model.pack_crc(gpu, st, max_len=BS)
    s.crc = rv.crc_column(image, s.pk_off[:N], s.pk_len)
    crc_model.check_column(g, s.crc, "pack_crc")
    s.dev = rv.Dev(st.packed, st.pk_off, st.pk_len, st.pk_kind, col)
    return s


def model(s, reqs, image=None, pk_len=None, pk_kind=None, crc=None, decode_frames=False):
    """-> [(ret, bytes)].  A frame entry of the clean image decodes to its
    block's prefix (tests/test_gpu_range.py checks that once per distinct
    frame); decode_frames: partial_model's walk of the bytes as they are."""
    prefix = None if decode_frames else (lambda e, body, end: (min(len(s.blocks[e]), end), s.blocks[e]))
    return rv.expected(s.image if image is None else image, s.pk_off, s.pk_len if pk_len is None else pk_len,
                       s.pk_kind if pk_kind is None else pk_kind, s.crc if crc is None else crc, reqs, frame=prefix)


def on_copy(s, image, crc=None, pk_len=None, pk_kind=None):
    """The store's device arrays with another image (a guarded copy) and / or other columns."""
    kw = {"packed": pack_model.Guarded(image.size, 5, image)}
    if crc is not None:
        kw["pk_crc"] = rv.dev_column(crc, np.uint32)
    if pk_len is not None:
        kw["pk_len"] = rv.dev_column(pk_len, np.int32)
    if pk_kind is not None:
        kw["pk_kind"] = rv.dev_column(pk_kind, np.uint8)
    return s.dev.replaced(**kw)


def _grid(s):
    reqs = []
    for e in range(N):
        n = len(s.blocks[e])
        for lo in (0, 1, 4095, n - 1, n, n + 5):
            for ln in (0, 1, 4096, n):
                reqs.append((e, lo, ln))
    return reqs


# ---- the clean store ----------------------------------------------------------

def test_clean_store_equals_the_model_and_the_plain_range_read(gpu, store):
    reqs = _grid(store)
    assert len(reqs) == N * 24
    order = np.random.default_rng(5).permutation(len(reqs))
    reqs = [reqs[i] for i in order]  # an entry's 24 requests are spread over the batch
    want = model(store, reqs)
    assert BAD_CRC not in [r for r, _ in want]
    plain = rv.read(gpu, store.dev, reqs, want, verified=False)
    for hint in (1, BS, 0):  # 16 threads per entry, four workgroups, one workgroup
        got = rv.read(gpu, store.dev, reqs, want, max_len=hint)
        assert np.array_equal(got[0], plain[0]), hint
        assert np.array_equal(got[1], plain[1]), hint
    # the binding's own hint: read from pk_len
    rv.read(gpu, store.dev, reqs[:100], want[:100], max_len=None)


def test_null_sel_and_repeated_sel(gpu, store):
    reqs = [(j, 7 + j, 5000) for j in range(N)]
    rv.read(gpu, store.dev, reqs, model(store, reqs), null_sel=True)
    reqs = [(2, 100 * j, 300 + j) for j in range(70)] + [(3, 64 * j + 1, 4096) for j in range(70)]
    want = model(store, reqs)
    got = rv.read(gpu, store.dev, reqs, want)
    plain = rv.read(gpu, store.dev, reqs, want, verified=False)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])


# ---- damage -------------------------------------------------------------------

FRAME_E, RAW_E = 6, 17  # a frame entry and a raw one


def _requests_around(e):
    """Requests on entry e (some for nothing, some invalid) between requests on clean entries."""
    return [(0, 0, 4096), (e, 0, 4096), (1, 10, 20), (e, 30000, 100), (e, 5, 0), (3, 60000, 5000), (e, 65530, 10),
            (e, -1, 16), (9, 0, 16), (e, 3, -16), (7, 1000, 1), (e, 0, 65536), (5, 1, 1)]


@pytest.mark.parametrize("entry", [FRAME_E, RAW_E])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_flipped_bit_in_an_entry(gpu, store, entry, where):
    s = store
    ln = int(s.pk_len[entry])
    at = int(s.pk_off[entry]) + {"first": 0, "middle": ln // 2, "last": ln - 1}[where]
    image = s.image.copy()
    image[at] ^= 0x08
    reqs = _requests_around(entry)
    want = model(s, reqs, image=image)
    assert [r for r, _ in want] == [4096, BAD_CRC, 20, BAD_CRC, 0, 5000, BAD_CRC, -1, 0, -1, 1, BAD_CRC, 1]
    rv.read(gpu, on_copy(s, image), reqs, want)


def test_a_wrong_checksum_on_an_intact_entry(gpu, store):
    s = store
    crc = s.crc.copy()
    crc[FRAME_E] ^= 0x80000000
    crc[RAW_E] += 1
    crc[9] = 1  # the empty entry: the checksum of no bytes is 0
    reqs = _requests_around(FRAME_E) + _requests_around(RAW_E)
    want = model(s, reqs, crc=crc)
    half = [4096, BAD_CRC, 20, BAD_CRC, 0, 5000, BAD_CRC, -1, BAD_CRC, -1, 1, BAD_CRC, 1]
    assert [r for r, _ in want] == half + half
    rv.read(gpu, s.dev.replaced(pk_crc=rv.dev_column(crc, np.uint32)), reqs, want)


def test_flips_in_the_padding_change_nothing(gpu, store):
    s = store
    image = s.image.copy()
    flipped = 0
    for e in (FRAME_E, 0, 1, 2):  # (a raw 64 KiB entry and the empty one have no padding at align 512)
        pad = range(int(s.pk_off[e]) + int(s.pk_len[e]), int(s.pk_off[e + 1]))
        for at in (pad[0], pad[-1]) if len(pad) else ():
            image[at] ^= 0xFF
            flipped += 1
    assert flipped >= 4
    reqs = _requests_around(FRAME_E) + _requests_around(2)
    want = model(s, reqs, image=image)
    assert want == model(s, reqs) and BAD_CRC not in [r for r, _ in want]
    rv.read(gpu, on_copy(s, image), reqs, want)


def test_invalid_requests_also_on_damaged_entries(gpu, store):
    s = store
    image = s.image.copy()
    for e in (1, 3, 4, 17, 6):
        image[int(s.pk_off[e]) + 2] ^= 0x40
    kind, ln = s.pk_kind.copy(), s.pk_len.copy()
    kind[1], kind[3] = 2, 255
    ln[4], ln[17] = -1, -65536
    reqs = [(e, lo, 64) for e in (0, 1, 3, 4, 17, 6) for lo in (0, 33)]
    reqs += [(N, 0, 16), (0xFFFFFFFF, 0, 16), (N + 7, 5, 0), (6, -3, 16), (6, 3, -16), (6, 3, 0), (2, 0, 16)]
    want = model(s, [(e if e < 2 ** 31 else -1, lo, n) for e, lo, n in reqs], image=image, pk_len=ln, pk_kind=kind)
    assert [r for r, _ in want] == [64, 64] + [-1] * 8 + [BAD_CRC, BAD_CRC] + [-1, -1, -1, -1, -1, 0, 16]
    rv.read(gpu, on_copy(s, image, pk_len=ln, pk_kind=kind), reqs, want)


def test_a_damaged_entry_nobody_reads(gpu, store):
    s = store
    image = s.image.copy()
    image[int(s.pk_off[FRAME_E]) + 100] ^= 0x01
    image[int(s.pk_off[RAW_E]) + 100] ^= 0x01
    # named only by requests for nothing: 0, not BAD_CRC
    reqs = [(0, 0, 4096), (FRAME_E, 0, 0), (RAW_E, 70000, 0), (1, 5, 50), (FRAME_E, 4096, 0)]
    want = model(s, reqs, image=image)
    assert [r for r, _ in want] == [4096, 0, 0, 50, 0]
    dev = on_copy(s, image)
    rv.read(gpu, dev, reqs, want)
    # named by none: the call is as on the clean store
    reqs = [(e, 100 + e, 3000) for e in range(N) if e not in (FRAME_E, RAW_E)]
    want = model(s, reqs, image=image)
    assert want == model(s, reqs)
    got = rv.read(gpu, dev, reqs, want)
    clean = rv.read(gpu, s.dev, reqs, want)
    assert np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1])


def test_a_rejected_frame_with_a_matching_checksum_gives_the_decode_error(gpu, store):
    s = store
    at, ln = int(s.pk_off[0]), int(s.pk_len[0])
    assert s.pk_kind[0] == pack_model.FRAME
    found = rv.rejected_damage(s.image[at:at + ln].tobytes())
    if found is None:
        pytest.fail("no damage found that the model rejects")
    image = s.image.copy()
    image[at:at + ln] = np.frombuffer(found[1], np.uint8)
    crc = s.crc.copy()
    crc[0] = crc_model.crc32c(found[1])
    reqs = [(0, 0, 4096), (0, 10, 20), (0, 60000, 5000), (1, 0, 4096)]
    want = model(s, reqs, image=image, crc=crc, decode_frames=True)
    assert want[0][0] < -1 and want[2][0] < -1 and want[3][0] == 4096 and BAD_CRC not in [r for r, _ in want]
    rv.read(gpu, on_copy(s, image, crc=crc), reqs, want)
    # with the column as it was the same bytes are refused
    want = model(s, reqs, image=image, decode_frames=True)
    assert [r for r, _ in want] == [BAD_CRC, BAD_CRC, BAD_CRC, 4096]
    rv.read(gpu, on_copy(s, image), reqs, want)


# ---- many small entries ---------------------------------------------------------

def test_many_small_raw_entries_every_seventh_damaged(gpu):
    """A synthetic index (no compress): 700 raw entries of 0..300 bytes at
    align 1, 1000 requests with repeated sel -- three workgroups of the
    per-request kernels, the entries' owners anywhere among them."""
    rng = np.random.default_rng(700)
    n, m = 700, 1000
    lens = rng.integers(0, 301, n)
    lens[:4] = (0, 300, 1, 0)
    pk_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    image = rng.integers(0, 256, int(pk_off[n]), dtype=np.uint8)
    kind = np.full(n, pack_model.RAW, np.uint8)
    crc = rv.crc_column(image, pk_off[:n], lens)
    damaged = np.arange(n) % 7 == 3
    for e in np.flatnonzero(damaged):
        if lens[e]:
            image[pk_off[e] + (e % lens[e])] ^= 1 << (e % 8)
        else:
            crc[e] ^= 1 + e
    dev = rv.Dev(pack_model.Guarded(image.size, 3, image), rv.dev_column(pk_off, np.int64),
                 rv.dev_column(lens, np.int32), rv.dev_column(kind, np.uint8), rv.dev_column(crc, np.uint32))
    sel = rng.integers(0, n, m)
    sel[::5] = sel[1::5][:len(sel[::5])]  # neighbours that share an entry
    reqs = [(int(e), int(rng.integers(0, 200)), int(rng.integers(0, 320))) for e in sel]
    want = rv.expected(image, pk_off, lens, kind, crc, reqs)
    rets = [r for r, _ in want]
    assert rets.count(BAD_CRC) > 80 and sum(r > 0 for r in rets) > 400 and rets.count(0) > 20
    assert all(r == BAD_CRC or r == 0 for (r, _), (e, _, ln) in zip(want, reqs) if damaged[e])
    for hint in (300, BS):
        rv.read(gpu, dev, reqs, want, max_len=hint)


# ---- graph capture and a forced decoder -------------------------------------------

def test_under_graph_capture_with_a_damaged_entry(gpu, store):
    s = store
    image = s.image.copy()
    image[int(s.pk_off[FRAME_E]) + int(s.pk_len[FRAME_E]) - 1] ^= 0x80
    reqs = [(e, 1000 + e, 4096) for e in range(N)] + [(FRAME_E, 0, 0), (FRAME_E, 0, 1)]
    want = model(s, reqs, image=image)
    assert [r for r, _ in want].count(BAD_CRC) == 2
    rv.read(gpu, on_copy(s, image), reqs, want, graph=True)


def test_forced_decoder_in_a_child_process(gpu):
    """LZ4E_DECOMPRESS_MODE is read once per process: a fresh child."""
    env = dict(os.environ, LZ4E_DECOMPRESS_MODE="p")
    code = ("import sys; sys.path[:0] = [%r, %r]; import range_verified_model; range_verified_model.forced_mode_child()"
            % (os.path.join(REPO, "lz4-sgori_amd"), os.path.join(REPO, "tests")))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "forced mode verified range read ok" in out.stdout
