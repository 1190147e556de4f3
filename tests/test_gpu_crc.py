"""The packed frame store's integrity on the GPU: lz4e_crc32c_batch_dev,
lz4e_pack_crc_batch_dev and lz4e_unpack_verified_batch_dev against the numpy
model (tests/crc_model.py).  Every checksum column and every unpack
destination sits in a pattern-filled range with guard space; every byte
outside what include/lz4e.h lets a call write is compared afterwards, and the
inputs are compared to what they held before.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import crc_model
import oracle_ref
import pack_model
import test_gpu_pack as packs
from crc_model import BAD_CRC, crc_column, pack_crc_expected
from pack_model import FRAME, RAW, DevStore, Guarded, check_index, pack_expected, random_block, text_block

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tools/emu/emu_crc.cpp's list
LENS = (0, 1, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 511, 512, 4096, 4097, 70000)
HUGE = 0x7E000000


# ---- 1. crc32c_batch_dev ----------------------------------------------------

@pytest.mark.parametrize("hint", [1, max(LENS), HUGE])
def test_crc32c_every_length(gpu, hint):
    """Entry k at residue (5k + 3) % 16; the hint only picks the threads per
    entry (16; 2048; 16384, every entry split over 64 workgroups)."""
    chunks = [random_block(n, 100 + n) for n in LENS]
    host, offs = pack_model.place(chunks, (5 * np.arange(len(LENS)) + 3) % 16)
    crc_model.dev_crc32c(gpu, host, offs, np.array(LENS), hint, f"hint {hint}")


def test_crc32c_one_entry_across_workgroups(gpu):
    n = 5 * (1 << 20) + 3
    host, offs = pack_model.place([random_block(n, 9)], [5])
    crc_model.dev_crc32c(gpu, host, offs, np.array([n]), n, "5 MiB + 3")
    crc_model.dev_crc32c(gpu, host, offs, np.array([n]), 1, "5 MiB + 3 on 16 threads")


def test_crc32c_many_small_entries(gpu):
    n = 70000
    rng = np.random.default_rng(70)
    lens = rng.integers(0, 41, n)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]) + 3  # back to back: every residue
    host = rng.integers(0, 256, int(lens.sum()) + 3, dtype=np.uint8)
    crc_model.dev_crc32c(gpu, host, offs, lens, int(lens.max()), "70000 entries")


def test_crc32c_no_entry_and_negative_lengths(gpu):
    import torch
    host = np.frombuffer(random_block(64, 1), dtype=np.uint8)
    crc_model.dev_crc32c(gpu, host, np.array([5, 0, 9]), np.array([-1, 0, -2147483647]), 1, "nothing to read")
    data = pack_model._t(host, np.uint8)
    none64 = torch.empty(0, dtype=torch.int64, device=data.device)
    none32 = torch.empty(0, dtype=torch.int32, device=data.device)
    g, col = crc_model.guarded_column(0)
    gpu.crc32c_batch_dev(data, none64, none32, col, max_len=0)
    torch.cuda.synchronize()
    g.check(None, "nblocks 0")


# ---- 2. pack_crc_batch_dev --------------------------------------------------

@pytest.mark.parametrize("align", [1, 512])
def test_pack_crc_on_synthetic_stores(gpu, align):
    import torch
    blocks, slots, rets = packs.synthetic()
    image, *want = pack_expected(blocks, slots, rets, align)
    want_col = pack_crc_expected(image, want[0], want[1])
    assert (want[2] == FRAME).any() and (want[2] == RAW).sum() == 4 * len(packs.LENS)
    st = packs.synth_store(gpu, blocks, slots, rets)
    check_index(st.pack(align, image.size, skew=7), want, f"align {align}")
    for hint in (None, 1, HUGE):
        g, _ = crc_model.pack_crc(gpu, st, max_len=hint)
        crc_model.check_column(g, want_col, f"pack_crc, align {align}, hint {hint}")
    # the same column from the image itself
    g, col = crc_model.guarded_column(st.n)
    gpu.crc32c_batch_dev(st.packed.view, st.pk_off, st.pk_len, col, max_len=st.max_len)
    torch.cuda.synchronize()
    crc_model.check_column(g, want_col, f"crc32c of the image, align {align}")
    st.packed.check(image, f"align {align}")
    # an image that did not fit still gets its column
    st = packs.synth_store(gpu, blocks, slots, rets)
    check_index(st.pack(align, image.size, packed_cap=0, room=image.size + 64), want, "cap 0")
    g, _ = crc_model.pack_crc(gpu, st)
    crc_model.check_column(g, want_col, f"pack_crc with packed_cap 0, align {align}")
    st.packed.check(None, "packed_cap 0")


@pytest.mark.parametrize("align", [1, 512])
def test_pack_crc_after_a_real_compress(gpu, align):
    blocks, tt, limited = packs.plant_batch()
    n = len(blocks)
    k = np.arange(n)
    lens = np.array([len(b) for b in blocks], dtype=np.int64)
    caps = np.where(np.asarray(limited, dtype=bool) & (lens > 0), lens - 1, lens + lens // 255 + 16)
    st = DevStore(gpu, blocks, src_skew=k % 16).compress(tt, caps, dst_skew=k * 5 % 16)
    rets, frames = pack_model.oracle_frames(blocks, tt, caps)
    image, *want = pack_expected(blocks, frames, rets, align)
    assert (want[2] == FRAME).any() and (want[2] == RAW).any()
    check_index(st.pack(align, image.size, skew=3), want, f"align {align}")
    g, _ = crc_model.pack_crc(gpu, st)
    crc_model.check_column(g, pack_crc_expected(image, want[0], want[1]), f"plants, align {align}")


# ---- 3. verified unpack of a clean image -------------------------------------

@pytest.mark.parametrize("rule", list(packs.DECODER_BATCHES))
def test_verified_unpack_equals_unpack_each_decoder_rule(gpu, rule):
    count, size = packs.DECODER_BATCHES[rule]
    blocks, tt, lim = pack_model.small_mixed_blocks(count, size)
    kinds = crc_model.clean_compare(gpu, blocks, tt, lim, 512, max_cap=size)
    assert (kinds == FRAME).any() and (kinds == RAW).any()


@pytest.mark.parametrize("mode", ["p", "g"])
def test_verified_unpack_equals_unpack_forced_decoder(gpu, mode):
    """LZ4E_DECOMPRESS_MODE is read once per process: a fresh child for each."""
    env = dict(os.environ, LZ4E_DECOMPRESS_MODE=mode)
    code = ("import sys; sys.path[:0] = [%r, %r]; import crc_model; crc_model.forced_mode_child()"
            % (os.path.join(REPO, "lz4-sgori_amd"), os.path.join(REPO, "tests")))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "forced mode verified unpack ok" in out.stdout


# ---- 4. verified unpack of a damaged image -----------------------------------

def test_verified_unpack_of_a_damaged_image(gpu):
    align = 512
    text = text_block(3000, 77)
    good = oracle_ref.compress(text, 3)[1]
    raw = random_block(700, 78)
    assert 16 < len(good) < len(text) and len(good) % align and len(raw) % align  # every entry has padding
    F, R = (FRAME, good, len(text)), (RAW, raw, len(raw))
    # (entry, damage): a byte of the entry to flip a bit in, "crc", "pad", or a broken index
    plan = [(F, None), (R, None),
            (F, 0), (F, len(good) // 2), (F, len(good) - 1),
            (R, 0), (R, len(raw) // 2), (R, len(raw) - 1),
            (F, "crc"), (R, "crc"),
            (F, "pad"), (R, "pad"),
            (F, "kind"), (R, "len"),
            (F, None), (R, None)]
    n = len(plan)
    pk_kind = np.array([p[0][0] for p in plan], dtype=np.uint8)
    pk_len = np.array([len(p[0][1]) for p in plan], dtype=np.int32)
    caps = np.array([p[0][2] for p in plan], dtype=np.int64)
    pk_off = np.concatenate([[0], np.cumsum(pack_model.roundup(pk_len.astype(np.int64), align))]).astype(np.int64)
    image = np.zeros(int(pk_off[n]), dtype=np.uint8)
    for i, p in enumerate(plan):
        image[pk_off[i]:pk_off[i] + pk_len[i]] = np.frombuffer(p[0][1], dtype=np.uint8)
    col = pack_crc_expected(image, pk_off, pk_len)

    bad_image, bad_col, bad_kind, bad_len = image.copy(), col.copy(), pk_kind.copy(), pk_len.copy()
    for i, (_, dmg) in enumerate(plan):
        if isinstance(dmg, int):
            bad_image[pk_off[i] + dmg] ^= 1 << (i % 8)
        elif dmg == "crc":
            bad_col[i] ^= 1 << (3 * i % 32)
        elif dmg == "pad":
            bad_image[pk_off[i] + pk_len[i]] ^= 0x40       # the first padding byte
            bad_image[pk_off[i + 1] - 1] ^= 0x01           # and the last
        elif dmg == "kind":
            bad_kind[i] = 7
        elif dmg == "len":
            bad_len[i] = -int(pk_len[i])

    def run(img, column, kind, ln):
        st = DevStore(gpu, [b""] * n)
        st.packed = Guarded(img.size, skew=9, content=img)
        return crc_model.unpack_verified(gpu, st, pack_model._t(column.view(np.int32), np.int32), caps,
                                         dst_skew=np.arange(n) * 7 % 16, pk=(pk_off, ln, kind))

    clean_r, clean_d, _, doffs = run(image, col, pk_kind, pk_len)
    assert clean_r.tolist() == caps.tolist()
    r, d, before, doffs2 = run(bad_image, bad_col, bad_kind, bad_len)
    assert np.array_equal(doffs, doffs2)
    slot = lambda a, i: a[doffs[i]:doffs[i] + caps[i]]
    for i, (entry, dmg) in enumerate(plan):
        what = f"entry {i} (kind {entry[0]}, damage {dmg!r})"
        if isinstance(dmg, int) or dmg == "crc":
            assert r[i] == BAD_CRC, f"{what}: ret {r[i]}"
            assert np.array_equal(slot(d, i), slot(before, i)), f"{what}: its destination was written"
        elif dmg in ("kind", "len"):
            assert r[i] == -1, f"{what}: ret {r[i]}"
            assert np.array_equal(slot(d, i), slot(before, i)), f"{what}: its destination was written"
        else:  # intact, or damaged in its padding only
            assert r[i] == clean_r[i] == caps[i], f"{what}: ret {r[i]}, clean {clean_r[i]}"
            assert np.array_equal(slot(d, i), slot(clean_d, i)), f"{what}: differs from the clean run"
            assert slot(d, i).tobytes() == (text if entry[0] == FRAME else raw), f"{what}: wrong bytes"
