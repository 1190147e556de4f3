"""CRC-32C and the packed frame store's integrity rules in numpy -- TEST
INFRASTRUCTURE ONLY.

  * crc32c: table-driven CRC-32C (Castagnoli: reflected, polynomial
    0x1EDC6F41, initial value and final xor 0xFFFFFFFF); long inputs go as
    4096 stripes at a time so that megabytes take a moment.
  * pack_crc_expected: the pk_crc column of a packed image.
  * unpack_verified_expected: include/lz4e.h's three-step rule of
    lz4e_unpack_verified_batch_dev on top of pack_model.unpack_expected.
"""
import numpy as np

import pack_model

POLY = 0x82F63B78
BAD_CRC = -2147483647  # LZ4E_UNPACK_BAD_CRC


def _table():
    t = np.zeros(256, dtype=np.uint32)
    for v in range(256):
        c = v
        for _ in range(8):
            c = (c >> 1) ^ (POLY if c & 1 else 0)
        t[v] = c
    return t


_T = _table()
_T0 = [int(v) for v in _T]


def _bytewise(state: int, data: bytes) -> int:
    for b in data:
        state = _T0[(state ^ b) & 0xFF] ^ (state >> 8)
    return state


def _zeros(state: int, n: int) -> int:
    """The state after n more zero bytes: multiplication by x^(8n) mod P,
    square-and-multiply over the bits of n."""
    def mul(a, b):
        r = 0
        for i in range(32):
            if b & (0x80000000 >> i):
                r ^= a
            a = (a >> 1) ^ (POLY if a & 1 else 0)
        return r
    p = 0x00800000  # x^8
    while n:
        if n & 1:
            state = mul(state, p)
        p = mul(p, p)
        n >>= 1
    return state


def crc32c(data) -> int:
    """CRC-32C of a bytes-like object.  Long inputs are cut into 4096 equal
    stripes that numpy advances together one byte per step (the state of a
    stripe started from 0), then the stripes are combined through the
    identity state(A || B) = state(A) x^(8 |B|) ^ state0(B)."""
    data = bytes(data)
    n = len(data)
    stripes = 4096
    if n < 64 * stripes:
        return _bytewise(0xFFFFFFFF, data) ^ 0xFFFFFFFF
    w = n // stripes
    head = n - w * stripes  # the first `head` bytes go bytewise, with the initial value
    a = np.frombuffer(data, dtype=np.uint8, count=w * stripes, offset=head).reshape(stripes, w)
    s = np.zeros(stripes, dtype=np.uint32)
    t0 = _T
    for k in range(w):
        s = t0[(s ^ a[:, k]) & 0xFF] ^ (s >> 8)
    # Horner over the stripes: state = state * x^(8 w) ^ stripe
    state = _bytewise(0xFFFFFFFF, data[:head])
    # multiplication by x^(8 w) is linear: as a 32 x 32 bit matrix, one row per state bit
    rows = [_zeros(1 << b, w) for b in range(32)]
    for v in s.tolist():
        adv = 0
        b = 0
        x = state
        while x:
            if x & 1:
                adv ^= rows[b]
            x >>= 1
            b += 1
        state = adv ^ v
    return state ^ 0xFFFFFFFF


def crc_column(image, off, ln) -> np.ndarray:
    """crc32c of image[off[i], off[i] + ln[i]) per entry; ln[i] <= 0 gives 0."""
    image = np.asarray(image, dtype=np.uint8)
    return np.array([crc32c(image[int(o):int(o) + int(l)].tobytes()) if l > 0 else 0
                     for o, l in zip(off, ln)], dtype=np.uint32)


def pack_crc_expected(image, pk_off, pk_len) -> np.ndarray:
    """The pk_crc column of pack_model.pack_expected's image: the stored bytes
    of each entry, without its padding."""
    return crc_column(image, pk_off[:len(pk_len)], pk_len)


def unpack_verified_expected(image, pk_off, pk_len, pk_kind, pk_crc, caps, decode):
    """-> (ret[], outputs[]).  Per entry: an unknown kind or a negative length
    gives -1 and the entry is not looked at; a checksum that differs gives
    BAD_CRC and no output; everything else is pack_model.unpack_expected."""
    rets, outs = pack_model.unpack_expected(image, pk_off, pk_len, pk_kind, caps, decode)
    rets = rets.copy()
    image = np.asarray(image, dtype=np.uint8)
    for i in range(len(pk_len)):
        if pk_kind[i] not in (pack_model.FRAME, pack_model.RAW) or pk_len[i] < 0:
            rets[i], outs[i] = -1, b""
        elif crc32c(image[int(pk_off[i]):int(pk_off[i]) + int(pk_len[i])].tobytes()) != int(pk_crc[i]):
            rets[i], outs[i] = BAD_CRC, b""
    return rets, outs


# ---------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------

def guarded_column(n: int):
    """An int32 column of n words inside a pattern-filled guarded range
    -> (Guarded, tensor)."""
    import torch
    g = pack_model.Guarded(4 * n)
    return g, g.view[:4 * n].view(torch.int32)


def check_column(g, want, what: str):
    """The column holds `want` (uint32) and no byte around it changed."""
    g.check(np.ascontiguousarray(want, dtype=np.uint32).view(np.uint8), what)


def dev_crc32c(amd, host, offs, lens, hint, what: str) -> None:
    """lz4e_crc32c_batch_dev of the entries (offs, lens) of the host array:
    the guarded column against crc_column, the input against itself."""
    import torch
    n = len(lens)
    data = pack_model._t(host, np.uint8)
    g, col = guarded_column(n)
    amd.crc32c_batch_dev(data, pack_model._t(offs, np.int64), pack_model._t(lens, np.int32), col, max_len=hint)
    torch.cuda.synchronize()
    assert np.array_equal(data.cpu().numpy(), host), f"{what}: the input changed"
    check_column(g, crc_column(host, offs, lens), what)


def pack_crc(amd, st, max_len=None):
    """lz4e_pack_crc_batch_dev after st.pack -> (Guarded, tensor); the inputs
    are compared to what they held before."""
    import torch
    g, col = guarded_column(st.n)
    amd.pack_crc_batch_dev(st.frames, st.fr_off, st.src, st.src_off, st.pk_len, st.pk_kind, col,
                           max_len=st.max_len if max_len is None else max_len)
    torch.cuda.synchronize()
    assert np.array_equal(st.frames.cpu().numpy(), st.fr_host), "pack_crc: the frame slots changed"
    assert np.array_equal(st.src.cpu().numpy(), st.src_host), "pack_crc: the source changed"
    return g, col


def unpack_verified(amd, st, pk_crc, caps, dst_skew=None, max_cap=None, pk=None):
    """lz4e_unpack_verified_batch_dev of st.packed into destinations placed as
    DevStore.unpack places them -> (ret[], dst bytes, dst before, offsets)."""
    import torch
    import gpu_batch
    n = st.n
    caps = np.asarray(caps, dtype=np.int64)
    doffs, total = gpu_batch._place(caps, pack_model._skews(dst_skew, n), gap=gpu_batch.GAP)
    image = gpu_batch.pattern(total)
    dst = pack_model._t(image, np.uint8)
    ret = torch.full((n,), -7777, dtype=torch.int32, device=dst.device)
    off, ln, kind = (st.pk_off, st.pk_len, st.pk_kind) if pk is None else (
        pack_model._t(pk[0], np.int64), pack_model._t(pk[1], np.int32), pack_model._t(pk[2], np.uint8))
    before = st.packed.host()
    if max_cap is None:
        max_cap = int(caps.max()) if n else 0
    amd.unpack_verified_batch_dev(st.packed.view, off, ln, kind, pk_crc, dst, pack_model._t(doffs, np.int64),
                                  pack_model._t(caps, np.int32), ret, max_cap=max_cap)
    torch.cuda.synchronize()
    d = dst.cpu().numpy()
    gpu_batch.check_guards(d, image, doffs, caps, "verified unpack")
    assert np.array_equal(st.packed.host(), before), "verified unpack: the packed image changed"
    return ret.cpu().numpy(), d, image, doffs


def clean_compare(amd, blocks, ttypes, limited, align, max_cap=None):
    """compress -> pack -> pack_crc, then the plain and the verified unpack of
    the same image into equally placed destinations: ret and every
    destination byte must be identical.  -> pk_kind."""
    n = len(blocks)
    k = np.arange(n)
    lens = np.array([len(b) for b in blocks], dtype=np.int64)
    caps = np.where(np.asarray(limited, dtype=bool) & (lens > 0), lens - 1, lens + lens // 255 + 16)
    st = pack_model.DevStore(amd, blocks, src_skew=k % 16).compress(ttypes, caps, dst_skew=k * 5 % 16)
    r = st.ret.cpu().numpy()
    kept = np.where((r > 0) & (r < lens), r, lens)
    total = int(((kept + align - 1) // align * align).sum())
    _, _, kinds = st.pack(align, total, skew=(3 * align + 5) % 16)
    _, col = pack_crc(amd, st)
    plain_r, _ = st.unpack(lens, dst_skew=k * 3 % 16, max_cap=max_cap)
    ver_r, ver_d, _, _ = unpack_verified(amd, st, col, lens, dst_skew=k * 3 % 16, max_cap=max_cap)
    assert np.array_equal(plain_r, lens), f"unpack: ret != src_len at {np.flatnonzero(plain_r != lens)[:5]}"
    assert np.array_equal(ver_r, plain_r), f"verified unpack: ret differs at {np.flatnonzero(ver_r != plain_r)[:5]}: {ver_r[ver_r != plain_r][:5]}"
    bad = np.flatnonzero(ver_d != st.dst_host)
    assert bad.size == 0, f"verified unpack: destination byte {int(bad[0])} differs from the plain unpack ({bad.size} do)"
    return kinds


def forced_mode_child():
    """Run in a fresh process with LZ4E_DECOMPRESS_MODE set (the library reads
    it once): the clean comparison on blocks every decoder takes."""
    import lz4e_amd
    blocks, tt, lim = pack_model.small_mixed_blocks(300)
    kinds = clean_compare(lz4e_amd, blocks, tt, lim, 16)
    assert (kinds == pack_model.FRAME).any() and (kinds == pack_model.RAW).any()
    print("forced mode verified unpack ok")
