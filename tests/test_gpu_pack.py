"""The packed frame store on the GPU: lz4e_pack_batch_dev and
lz4e_unpack_batch_dev against the numpy model (tests/pack_model.py) and the
oracle.  `packed` and every unpack destination carry gpu_batch.pattern with
guard space; every byte outside what include/lz4e.h lets a call write is
compared afterwards, and the inputs are compared to what they held before.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import frame_synth
import oracle_ref
import pack_model
from pack_model import FRAME, RAW, DevStore, Guarded, T, check_index, pack_expected, random_block, text_block

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = (0, 1, 15, 16, 17, 31, 33, 511, 512, 4096, 4097, 70000)


def synthetic(seed=5, lens=LENS):
    """Arbitrary byte strings as 'frames' with chosen ret: per length a frame
    entry and raw entries for ret 0, ret == n, ret > n and ret < 0.
    -> (blocks, slots, rets)."""
    rng = np.random.default_rng(seed)
    rb = lambda n: rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()
    blocks, slots, rets = [], [], []
    for L in lens:
        if L:  # a frame of L bytes for a block of L + 1 ... L + 8
            blocks.append(rb(L + 1 + rng.integers(0, 8)))
            slots.append(rb(L + 6))
            rets.append(L)
        for r in (0, L, L + 5, -3):
            blocks.append(rb(L))
            slots.append(rb(L + 6))  # present, and never to be copied
            rets.append(r)
    return blocks, slots, rets


def synth_store(gpu, blocks, slots, rets):
    k = np.arange(len(blocks))
    return DevStore(gpu, blocks, src_skew=(k * 5 + 3) % 16).synth_frames(slots, rets, fr_skew=k % 16)


# ---- 1. synthetic index ----------------------------------------------------

@pytest.mark.parametrize("align", [1, 512, 4096])
def test_synthetic_index_and_image(gpu, align):
    blocks, slots, rets = synthetic()
    image, *want = pack_expected(blocks, slots, rets, align)
    assert (want[2] == FRAME).sum() == len(LENS) - 1 and (want[2] == RAW).sum() == 4 * len(LENS)
    for skew in (0, 7):
        st = synth_store(gpu, blocks, slots, rets)
        got = st.pack(align, image.size, skew=skew)
        check_index(got, want, f"align {align}")
        st.packed.check(image, f"align {align}, packed at {skew} mod 16")


# ---- 2. boundary plants through the real compressor -------------------------

def plant_batch():
    blocks, tt, limited = [], [], []
    for cls in (1, 3, 7):
        for diff in (-1, 0, +1):
            for seed in (0, 1):
                blocks.append(pack_model.plant(diff, seed))
                tt.append(cls)
                limited.append(False)
        for b, lim in ((text_block(5000, cls), False), (bytes(4096), False), (random_block(4096, cls), False),
                       (random_block(4096, 10 + cls), True), (random_block(13, cls), True),
                       (text_block(3000, 20 + cls), True), (b"", False), (b"z", False)):
            blocks.append(b)
            tt.append(cls)
            limited.append(lim)
    return blocks, tt, limited


@pytest.mark.parametrize("align", [1, 512])
def test_boundary_plants_through_the_compressor(gpu, align):
    blocks, tt, limited = plant_batch()
    kinds = pack_model.roundtrip(gpu, blocks, tt, limited, align)
    per_class = len(blocks) // 3
    for c in range(3):
        k = kinds[c * per_class:(c + 1) * per_class]
        # n - 1 is kept as a frame; n and n + 1 are stored raw
        assert k[:6].tolist() == [FRAME, FRAME, RAW, RAW, RAW, RAW]
        # text, zeros: frames; random, limited random (ret 0): raw; limited text still shrinks
        assert k[6:].tolist() == [FRAME, FRAME, RAW, RAW, RAW, FRAME, RAW, RAW]


# ---- 3. round trip ----------------------------------------------------------

def sized_batch():
    blocks, tt, limited = [], [], []
    for n in (0, 1, 12, 13, 4096, 65536, 262145):
        for j, b in enumerate((text_block(n, n), bytes(n), random_block(n, n), random_block(n, n + 1),
                               text_block(n, n + 2))):
            blocks.append(b)
            tt.append((1, 3, 7)[j % 3] if n <= 65536 else 3)
            limited.append(j >= 3)
    return blocks, tt, limited


@pytest.mark.parametrize("align", [1, 512, 4096])
def test_round_trip_every_size(gpu, align):
    kinds = pack_model.roundtrip(gpu, *sized_batch(), align)
    assert (kinds == FRAME).any() and (kinds == RAW).any()


# One batch per rule of lz4e_decompress_batch_dev2's decoder choice
# (csrc/lz4e_decompress.hip pick_decoder), 64 distinct blocks repeated.
DECODER_BATCHES = {
    "pipelined_by_capacity": (6, 65536),   # capacity 16-128 KiB
    "group": (16384, 4096),                # <= 4608 bytes, >= 16384 blocks
    "pipelined_by_count": (1000, 8192),    # <= 1024 blocks
    "lds_form": (1100, 4096),              # <= 4608 bytes, 1025-3328 blocks
    "one_wave": (1100, 8192),              # everything else
}


@pytest.mark.parametrize("rule", list(DECODER_BATCHES))
def test_round_trip_each_decoder_rule(gpu, rule):
    count, size = DECODER_BATCHES[rule]
    blocks, tt, lim = pack_model.small_mixed_blocks(count, size)
    kinds = pack_model.roundtrip(gpu, blocks, tt, lim, 512, max_cap=size)
    assert (kinds == FRAME).any() and (kinds == RAW).any()


@pytest.mark.parametrize("mode", ["w", "p", "s", "g"])
def test_round_trip_forced_decoder(gpu, mode):
    """LZ4E_DECOMPRESS_MODE is read once per process: a fresh child for each."""
    env = dict(os.environ, LZ4E_DECOMPRESS_MODE=mode)
    code = ("import sys; sys.path[:0] = [%r, %r]; import pack_model; pack_model.forced_mode_child()"
            % (os.path.join(REPO, "lz4-sgori_amd"), os.path.join(REPO, "tests")))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "forced mode round trip ok" in out.stdout


# ---- 4. unpack errors -------------------------------------------------------

def test_unpack_errors_and_their_neighbours(gpu):
    text = text_block(3000, 77)
    good = oracle_ref.compress(text, 3)[1]
    raw = random_block(100, 78)
    entries = []  # (kind, bytes stored, pk_len, cap)

    def neighbour():
        entries.append((FRAME, good, len(good), len(text)))
        entries.append((RAW, raw, len(raw), len(raw)))

    neighbour()
    for cut in (1, 3, len(good) // 2, len(good) - 1):  # truncated frames
        entries.append((FRAME, good, len(good) - cut, len(text)))
        neighbour()
    bad = [c for c in frame_synth.profile_invalid(3) if not c.dic][:12]  # offsets before the block, ...
    assert len(bad) >= 8
    for c in bad:
        entries.append((FRAME, c.frame, len(c.frame), c.cap))
        neighbour()
    entries.append((FRAME, good, len(good), len(text) - 1))  # capacity one short
    neighbour()
    entries.append((RAW, raw, len(raw), len(raw) - 1))  # raw, capacity one short
    neighbour()
    entries.append((RAW, raw, len(raw), 0))
    entries.append((2, raw, len(raw), len(raw) + 50))  # unknown kinds
    neighbour()
    entries.append((255, good, len(good), len(text)))
    entries.append((RAW, b"", 0, 0))
    neighbour()

    n = len(entries)
    pk_off = np.concatenate([[0], np.cumsum([len(e[1]) for e in entries])]).astype(np.int64)
    pk_len = np.array([e[2] for e in entries], dtype=np.int32)
    pk_kind = np.array([e[0] for e in entries], dtype=np.uint8)
    caps = np.array([e[3] for e in entries], dtype=np.int64)
    image = np.frombuffer(b"".join(e[1] for e in entries), dtype=np.uint8)
    want_r, want_o = pack_model.unpack_expected(image, pk_off, pk_len, pk_kind, caps, oracle_ref.decompress)
    assert (want_r < 0).sum() >= 4 + 8 + 5

    st = DevStore(gpu, [b""] * n)
    st.packed = Guarded(image.size, skew=9, content=image)
    r, outs = st.unpack(caps, dst_skew=np.arange(n) * 7 % 16, pk=(pk_off, pk_len, pk_kind))
    assert np.array_equal(r, want_r), [(i, int(r[i]), int(want_r[i])) for i in np.flatnonzero(r != want_r)]
    for i in range(n):
        if want_r[i] >= 0:
            assert outs[i] == want_o[i], f"entry {i}"
        elif pk_kind[i] != FRAME:  # a raw or unknown entry that fails writes nothing
            lo = int(st.dst_offs[i])
            assert np.array_equal(st.dst_host[lo:lo + caps[i]], st.dst_image[lo:lo + caps[i]]), f"entry {i} written"


# ---- 5. scan ---------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, T - 1, T, T + 1, 64 * T + 1, 300001])
def test_scan_counts(gpu, n):
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 41, n)
    rets = np.where(rng.random(n) < 0.5, (lens * rng.random(n)).astype(np.int64), lens + rng.integers(0, 3, n))
    data = rng.integers(0, 256, 48, dtype=np.uint8).tobytes()
    blocks = [data[:k] for k in lens]
    slots = [data[5:5 + max(int(r), 0)] for r in rets]
    align = 1 if n % 2 else 16
    image, *want = pack_expected(blocks, slots, rets, align)
    st = DevStore(gpu, blocks).synth_frames(slots, rets)
    got = st.pack(align, image.size, skew=n % 16)
    check_index(got, want, f"n {n}")
    st.packed.check(image, f"n {n}")


def test_scan_past_4_gib_without_room(gpu):
    """1 048 600 one-byte raw entries at align 4096: pk_off[n] exceeds 2^32;
    with packed_cap 0 the index is complete and nothing is copied."""
    import torch
    n, align = 1048600, 4096
    dev = torch.device("cuda")
    src = torch.arange(n, device=dev).to(torch.uint8)
    src_off = torch.arange(n, device=dev, dtype=torch.int64)
    src_len = torch.ones(n, device=dev, dtype=torch.int32)
    ret = torch.zeros(n, device=dev, dtype=torch.int32)
    frames = torch.zeros(64, device=dev, dtype=torch.uint8)
    fr_off = torch.zeros(n, device=dev, dtype=torch.int64)
    packed = Guarded(0)
    pk_off = torch.full((n + 1,), -99, device=dev, dtype=torch.int64)
    pk_len = torch.full((n,), -99, device=dev, dtype=torch.int32)
    pk_kind = torch.full((n,), 99, device=dev, dtype=torch.uint8)
    gpu.pack_batch_dev(frames, fr_off, ret, src, src_off, src_len, packed.view, pk_off, pk_len, pk_kind,
                       align=align, packed_cap=0, max_len=1)
    torch.cuda.synchronize()
    want = torch.cat([torch.zeros(1, device=dev, dtype=torch.int64),
                      torch.cumsum(torch.full((n,), align, device=dev, dtype=torch.int64), 0)])
    assert int(want[n]) == n * align > 1 << 32
    assert torch.equal(pk_off, want)
    assert bool((pk_len == 1).all()) and bool((pk_kind == RAW).all())
    packed.check(None, "packed_cap 0")


# ---- 6. overflow ------------------------------------------------------------

@pytest.mark.parametrize("align", [1, 512])
def test_overflow_is_all_or_nothing(gpu, align):
    blocks, slots, rets = synthetic(seed=6)
    image, *want = pack_expected(blocks, slots, rets, align)
    total = image.size
    for cap in (total - 1, 0):
        st = synth_store(gpu, blocks, slots, rets)
        got = st.pack(align, total, packed_cap=cap, room=total + 64)
        check_index(got, want, f"cap {cap}")
        st.packed.check(None, f"packed_cap {cap} < {total}")
    st = synth_store(gpu, blocks, slots, rets)
    got = st.pack(align, total, packed_cap=total, room=total + 64)  # the byte at `total` stays
    check_index(got, want, "cap == total")
    st.packed.check(image, "packed_cap == total")


# ---- 7. bad arguments --------------------------------------------------------

@pytest.mark.parametrize("align", [0, 3, 8192])
def test_bad_align(gpu, align):
    import torch
    blocks, slots, rets = synthetic(seed=7, lens=(16, 33))
    st = synth_store(gpu, blocks, slots, rets)
    with pytest.raises(ValueError):
        st.pack(align, 4096)
    # the C call itself: -22, nothing launched, no output touched
    packed = Guarded(4096)
    pk_off = torch.full((st.n + 1,), -99, dtype=torch.int64, device=packed.full.device)
    pk_len = torch.full((st.n,), -99, dtype=torch.int32, device=packed.full.device)
    pk_kind = torch.full((st.n,), 99, dtype=torch.uint8, device=packed.full.device)
    r = gpu.lib().lz4e_pack_batch_dev(st.frames.data_ptr(), st.fr_off.data_ptr(), st.ret.data_ptr(), st.src.data_ptr(),
                                      st.src_off.data_ptr(), st.src_len.data_ptr(), packed.view.data_ptr(), 4096, align,
                                      pk_off.data_ptr(), pk_len.data_ptr(), pk_kind.data_ptr(), st.n, st.max_len,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert r == -22 and "align" in gpu.last_error()
    assert bool((pk_off == -99).all()) and bool((pk_len == -99).all()) and bool((pk_kind == 99).all())
    packed.check(None, f"align {align}")
