"""The packed frame store's model and device helpers -- TEST INFRASTRUCTURE ONLY.

  * pack_expected / unpack_expected: include/lz4e.h's contract of
    lz4e_pack_batch_dev and lz4e_unpack_batch_dev restated in numpy.
  * plant: blocks whose frame comes out one byte smaller than, as large as and
    one byte larger than the input (the frame / raw decision's boundary).
  * DevStore: compress -> pack -> unpack on guarded, skewed device tensors in
    the manner of gpu_batch (its pattern, placement and check_guards): every
    byte outside what the contract lets a call write is compared afterwards.
"""
import numpy as np

import gpu_batch
from gpu_batch import EDGE, GAP, check_guards, pattern

FRAME, RAW = 0, 1
T = 256  # blocks per scan tile (csrc/lz4e_gpu.h kPackTile)


def roundup(v, align):
    return (v + align - 1) // align * align


def entry_of(block_len: int, ret: int):
    """-> (kind, length) of a block of block_len bytes whose compress returned ret."""
    return (FRAME, int(ret)) if 0 < ret < block_len else (RAW, int(block_len))


def pack_expected(blocks, frames, rets, align):
    """-> (image uint8[pk_off[n]], pk_off int64[n + 1], pk_len int32[n], pk_kind uint8[n]).
    frames[i] holds at least rets[i] bytes when block i is stored as a frame."""
    n = len(blocks)
    pk_off = np.zeros(n + 1, dtype=np.int64)
    pk_len = np.zeros(n, dtype=np.int32)
    pk_kind = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        pk_kind[i], pk_len[i] = entry_of(len(blocks[i]), int(rets[i]))
        pk_off[i + 1] = pk_off[i] + roundup(int(pk_len[i]), align)
    image = np.zeros(int(pk_off[n]), dtype=np.uint8)
    for i in range(n):
        body = bytes(frames[i])[:pk_len[i]] if pk_kind[i] == FRAME else bytes(blocks[i])
        assert len(body) == pk_len[i]
        image[pk_off[i]:pk_off[i] + pk_len[i]] = np.frombuffer(body, dtype=np.uint8)
    return image, pk_off, pk_len, pk_kind


def unpack_expected(image, pk_off, pk_len, pk_kind, caps, decode):
    """The inverse -> (ret[], outputs[]); decode(frame, cap) -> (ret, bytes) is
    the decoder a frame entry is handed to (oracle_ref.decompress)."""
    rets, outs = [], []
    for i in range(len(pk_len)):
        body = image[int(pk_off[i]):int(pk_off[i]) + max(int(pk_len[i]), 0)].tobytes()
        if pk_kind[i] == FRAME:
            r, o = decode(body, int(caps[i]))
        elif pk_kind[i] == RAW and 0 <= pk_len[i] <= caps[i]:
            r, o = int(pk_len[i]), body
        else:
            r, o = -1, b""
        rets.append(r)
        outs.append(o)
    return np.array(rets, dtype=np.int32), outs


# (m, tail) of the three boundary plants, by frame size - block size
PLANTS = {-1: (5, 12), 0: (4, 12), +1: (4, 20)}


def plant(diff: int, seed: int) -> bytes:
    """random(8) + its first m bytes again + a random tail whose first byte
    differs from the byte that would extend the match."""
    m, tail = PLANTS[diff]
    rng = np.random.default_rng(seed)
    head = rng.integers(0, 256, 8, dtype=np.uint8)
    t = rng.integers(0, 256, tail, dtype=np.uint8)
    if t[0] == head[m]:
        t[0] ^= 0x55
    return head.tobytes() + head[:m].tobytes() + t.tobytes()


def random_block(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def text_block(n: int, seed: int) -> bytes:
    from lz4e_amd import corpus
    return corpus.text_proxy(n, seed).tobytes()[:n]


# ---------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------

def _t(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(torch.device("cuda"))


def _skews(v, n):
    return gpu_batch._per_block(v, n)


class Guarded:
    """A device byte range [base, base + size) inside a pattern-filled tensor
    with EDGE bytes and more around it."""

    def __init__(self, size: int, skew: int = 0, content=None):
        self.base = EDGE + skew
        self.size = size
        self.before = pattern(self.base + size + EDGE)
        if content is not None:
            self.before[self.base:self.base + len(content)] = content
        self.full = _t(self.before, np.uint8)
        self.view = self.full[self.base:]

    def host(self):
        return self.full.cpu().numpy()

    def check(self, want, what: str):
        """[base, base + len(want)) holds want (None: nothing was to be
        written at all), every other byte the pattern."""
        got = self.host()
        k = 0 if want is None else len(want)
        if k:
            at = self.base
            bad = np.flatnonzero(got[at:at + k] != want)
            assert bad.size == 0, f"{what}: image differs at byte {int(bad[0])} of {k} ({bad.size} bytes differ)"
        rest = got != self.before
        rest[self.base:self.base + k] = False
        assert not rest.any(), (f"{what}: byte {int(np.flatnonzero(rest)[0]) - self.base} (relative to packed) "
                                f"written; only [0, {k}) may be")


def place(chunks, skews=None, gap=16):
    """Byte strings at 16-byte boundaries plus skews inside a pattern-filled
    host array -> (array, offs)."""
    n = len(chunks)
    sizes = np.array([len(c) for c in chunks], dtype=np.int64)
    offs, total = gpu_batch._place(sizes, _skews(skews, n), gap=gap)
    host = pattern(total)
    for i, c in enumerate(chunks):
        host[offs[i]:offs[i] + sizes[i]] = np.frombuffer(bytes(c), dtype=np.uint8)
    return host, offs


class DevStore:
    """The device arrays of one compress launch (real, or synthesized from
    chosen slot contents and ret values) and what pack and unpack make of them."""

    def __init__(self, amd, blocks, src_skew=None):
        self.amd = amd
        self.blocks = [bytes(b) for b in blocks]
        self.n = len(blocks)
        self.lens = np.array([len(b) for b in blocks], dtype=np.int64)
        self.src_host, self.src_offs = place(self.blocks, src_skew)
        self.src = _t(self.src_host, np.uint8)
        self.src_off = _t(self.src_offs, np.int64)
        self.src_len = _t(self.lens, np.int32)
        self.max_len = int(self.lens.max()) if self.n else 0

    def synth_frames(self, slots, rets, fr_skew=None):
        """Slot i holds the bytes slots[i]; its compress 'returned' rets[i]."""
        self.fr_host, self.fr_offs = place(slots, fr_skew, gap=GAP)
        self.frames = _t(self.fr_host, np.uint8)
        self.fr_off = _t(self.fr_offs, np.int64)
        self.ret = _t(np.asarray(rets), np.int32)
        return self

    def compress(self, ttypes, caps=None, dst_skew=None):
        """lz4e_compress_batch_dev into guarded slots; the tensors stay on the device."""
        import torch
        caps = self.lens + self.lens // 255 + 16 if caps is None else np.asarray(caps, dtype=np.int64)
        self.fr_offs, total = gpu_batch._place(caps, _skews(dst_skew, self.n), gap=GAP)
        image = pattern(total)
        self.frames = _t(image, np.uint8)
        self.fr_off = _t(self.fr_offs, np.int64)
        self.ret = torch.full((self.n,), -7, dtype=torch.int32, device=self.frames.device)
        self.amd.compress_batch_dev(self.src, self.src_off, self.src_len, _t(ttypes, np.uint8), self.frames,
                                    self.fr_off, _t(caps, np.int32), self.ret, max_len=self.max_len)
        torch.cuda.synchronize()
        self.fr_host = self.frames.cpu().numpy()
        check_guards(self.fr_host, image, self.fr_offs, caps, "compress")
        return self

    def pack(self, align, total, packed_cap=None, skew=0, room=None, check_inputs=True):
        """lz4e_pack_batch_dev into a guarded range of `room` bytes (default:
        the expected total) -> (pk_off, pk_len, pk_kind) as numpy; the device
        tensors stay in self.pk_*; self.packed is the Guarded range."""
        import torch
        room = total if room is None else room
        self.packed = Guarded(room, skew)
        dev = self.packed.full.device
        self.pk_off = torch.full((self.n + 1,), -99, dtype=torch.int64, device=dev)
        self.pk_len = torch.full((self.n,), -99, dtype=torch.int32, device=dev)
        self.pk_kind = torch.full((self.n,), 99, dtype=torch.uint8, device=dev)
        self.amd.pack_batch_dev(self.frames, self.fr_off, self.ret, self.src, self.src_off, self.src_len,
                                self.packed.view, self.pk_off, self.pk_len, self.pk_kind, align=align,
                                packed_cap=room if packed_cap is None else packed_cap, max_len=self.max_len)
        torch.cuda.synchronize()
        if check_inputs:
            assert np.array_equal(self.frames.cpu().numpy(), self.fr_host), "pack: the frame slots changed"
            assert np.array_equal(self.src.cpu().numpy(), self.src_host), "pack: the source changed"
        return self.pk_off.cpu().numpy(), self.pk_len.cpu().numpy(), self.pk_kind.cpu().numpy()

    def unpack(self, caps, dst_skew=None, max_cap=None, pk=None):
        """lz4e_unpack_batch_dev of self.packed (pk: another (pk_off, pk_len,
        pk_kind) numpy triple in place of the packed one) -> (ret[], outputs[])."""
        import torch
        n = self.n
        caps = np.asarray(caps, dtype=np.int64)
        doffs, total = gpu_batch._place(caps, _skews(dst_skew, n), gap=GAP)
        image = pattern(total)
        dst = _t(image, np.uint8)
        ret = torch.full((n,), -7777, dtype=torch.int32, device=dst.device)
        off, ln, kind = (self.pk_off, self.pk_len, self.pk_kind) if pk is None else (
            _t(pk[0], np.int64), _t(pk[1], np.int32), _t(pk[2], np.uint8))
        before = self.packed.host()
        if max_cap is None:
            max_cap = int(caps.max()) if n else 0
        self.amd.unpack_batch_dev(self.packed.view, off, ln, kind, dst, _t(doffs, np.int64), _t(caps, np.int32), ret,
                                  max_cap=max_cap)
        torch.cuda.synchronize()
        r = ret.cpu().numpy()
        d = dst.cpu().numpy()
        check_guards(d, image, doffs, caps, "unpack")
        assert np.array_equal(self.packed.host(), before), "unpack: the packed image changed"
        self.dst_host, self.dst_image, self.dst_offs = d, image, doffs
        return r, [d[doffs[i]:doffs[i] + max(int(r[i]), 0)].tobytes() for i in range(n)]


def check_index(got, want, what: str):
    for name, g, w in zip(("pk_off", "pk_len", "pk_kind"), got, want):
        bad = np.flatnonzero(np.asarray(g) != np.asarray(w))
        assert bad.size == 0, f"{what}: {name}[{int(bad[0])}] = {g[bad[0]]}, expected {w[bad[0]]} ({bad.size} differ)"


def oracle_frames(blocks, ttypes, caps):
    """oracle_ref.compress of every block (equal blocks computed once) -> (rets, frames)."""
    import oracle_ref
    memo, rets, frames = {}, [], []
    for b, tt, cap in zip(blocks, ttypes, caps):
        key = (bytes(b), int(tt), int(cap))
        if key not in memo:
            memo[key] = oracle_ref.compress(key[0], key[1], cap=key[2])[:2]
        rets.append(memo[key][0])
        frames.append(memo[key][1])
    return np.array(rets, dtype=np.int32), frames


def roundtrip(amd, blocks, ttypes, limited, align, max_cap=None):
    """compress -> pack -> unpack of the blocks (limited[i]: block i is
    compressed with dst_cap = n - 1) on skewed, guarded tensors; ret, index
    and image against the model built from the oracle's frames, the unpacked
    bytes against the input.  -> pk_kind."""
    n = len(blocks)
    k = np.arange(n)
    lens = np.array([len(b) for b in blocks], dtype=np.int64)
    caps = np.where(np.asarray(limited, dtype=bool) & (lens > 0), lens - 1, lens + lens // 255 + 16)
    st = DevStore(amd, blocks, src_skew=k % 16).compress(ttypes, caps, dst_skew=k * 5 % 16)
    rets, frames = oracle_frames(blocks, ttypes, caps)
    got_ret = st.ret.cpu().numpy()
    assert np.array_equal(got_ret, rets), f"compress: ret differs from the oracle at {np.flatnonzero(got_ret != rets)[:5]}"
    image, *want = pack_expected(blocks, frames, rets, align)
    got = st.pack(align, image.size, skew=(3 * align + 5) % 16)
    check_index(got, want, f"pack align {align}")
    st.packed.check(image, f"pack align {align}")
    r, outs = st.unpack(lens, dst_skew=k * 3 % 16, max_cap=max_cap)
    assert np.array_equal(r, lens), f"unpack: ret != src_len at {np.flatnonzero(r != lens)[:5]}: {r[r != lens][:5]}"
    for i in range(n):
        assert outs[i] == bytes(blocks[i]), f"unpack: block {i} (kind {want[2][i]}, {lens[i]} bytes) differs"
    return want[2]


def small_mixed_blocks(count: int, size: int = 4096, distinct: int = 64):
    """count blocks of <= size bytes repeating `distinct` ones: text, zeros,
    fio-style half-random, random (raw) and limited-output blocks.
    -> (blocks, ttypes, limited)."""
    from lz4e_amd import corpus
    base = []
    for d in range(distinct):
        n = size if d % 8 else size - 1 - 7 * d
        kind = d % 4
        b = (text_block(n, d) if kind == 0 else bytes(n) if kind == 1
             else corpus.fio_pattern(n, d).tobytes() if kind == 2 else random_block(n, d))
        base.append((b, (1, 3, 7)[d % 3], d % 16 == 7 or d % 16 == 10))
    pick = [base[i % distinct] for i in range(count)]
    return [p[0] for p in pick], [p[1] for p in pick], [p[2] for p in pick]


def forced_mode_child():
    """Run in a fresh process with LZ4E_DECOMPRESS_MODE set (the library reads
    it once): one round trip of blocks every decoder takes."""
    import lz4e_amd
    blocks, tt, lim = small_mixed_blocks(300)
    kinds = roundtrip(lz4e_amd, blocks, tt, lim, 16)
    assert (kinds == FRAME).any() and (kinds == RAW).any()
    print("forced mode round trip ok")
