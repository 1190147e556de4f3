"""The verified range read's model and device helpers -- TEST INFRASTRUCTURE ONLY.

  * expected: include/lz4e.h's four rules of
    lz4e_unpack_range_verified_batch_dev restated in Python on top of
    crc_model.crc32c and partial_model.decode.
  * rejected_damage: two bytes of a frame overwritten so that the partial
    decode fails (the damage a checksum recomputed to match lets through).
  * Dev / read: one guarded call of the verified or the plain range read on
    the device, every destination slot exactly the bytes its request must get.
"""
import numpy as np

import crc_model
import gpu_batch
import pack_model
import partial_model

BAD_CRC = crc_model.BAD_CRC
FRAME, RAW = pack_model.FRAME, pack_model.RAW

_crc_memo = {}


def crc_of(body: bytes) -> int:
    """crc_model.crc32c, each distinct byte string summed once per process."""
    if body not in _crc_memo:
        _crc_memo[body] = crc_model.crc32c(body)
    return _crc_memo[body]


def crc_column(image, pk_off, pk_len) -> np.ndarray:
    image = np.asarray(image, dtype=np.uint8)
    return np.array([crc_of(image[int(o):int(o) + int(l)].tobytes()) if l > 0 else 0
                     for o, l in zip(pk_off, pk_len)], dtype=np.uint32)


def expected(image, pk_off, pk_len, pk_kind, pk_crc, reqs, max_end=None, frame=None):
    """reqs: [(sel, lo, len)] -> [(ret, bytes)].  pk_crc: uint32 values.
    frame(e, body, target) -> (value, data) is the partial decode of a frame
    entry (default: partial_model.decode); max_end None: no clamp."""
    n = len(pk_len)
    image = np.asarray(image, dtype=np.uint8)
    verdict = {}  # entry -> damaged, looked at once per call
    out = []
    for e, lo, ln in reqs:
        # 1. invalid: the plain range read's test
        if not 0 <= e < n or lo < 0 or ln < 0 or pk_kind[e] not in (FRAME, RAW) or pk_len[e] < 0:
            out.append((-1, b""))
            continue
        # 2. nothing wanted: the entry is not looked at
        if ln == 0:
            out.append((0, b""))
            continue
        body = image[int(pk_off[e]):int(pk_off[e]) + int(pk_len[e])].tobytes()
        if e not in verdict:
            verdict[e] = crc_of(body) != int(pk_crc[e]) & 0xFFFFFFFF
        # 3. the stored bytes changed
        if verdict[e]:
            out.append((BAD_CRC, b""))
            continue
        # 4. the plain range read
        end = lo + ln if max_end is None else min(lo + ln, max_end)
        if pk_kind[e] == RAW:
            d, data = min(len(body), end), body
        elif frame is not None:
            d, data = frame(e, body, end)
        else:
            d, data = partial_model.decode(body, end, True)
        out.append((d, b"") if d < 0 else (max(0, d - lo), data[lo:d]))
    return out


def rejected_damage(body: bytes, target: int = 2048):
    """-> (position p, damaged body): 0xFF 0xFF at the first p in [2, 600)
    where the partial decode to `target` then fails; None when there is none."""
    for p in range(2, min(600, len(body) - 1)):
        b = bytearray(body)
        b[p:p + 2] = b"\xff\xff"
        if partial_model.decode(bytes(b), target, True)[0] < 0:
            return p, bytes(b)
    return None


# ---------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------

class Dev:
    """The device arrays of one store: packed is a pack_model.Guarded range,
    pk_crc an int32 tensor of the column's bit patterns."""

    def __init__(self, packed, pk_off, pk_len, pk_kind, pk_crc):
        self.packed, self.pk_off, self.pk_len, self.pk_kind, self.pk_crc = packed, pk_off, pk_len, pk_kind, pk_crc

    def replaced(self, **kw):
        d = Dev(self.packed, self.pk_off, self.pk_len, self.pk_kind, self.pk_crc)
        for k, v in kw.items():
            setattr(d, k, v)
        return d


def dev_column(values, dt):
    """A numpy index column (uint32 values as their int32 bit patterns) on the device."""
    a = np.ascontiguousarray(values)
    if dt is np.uint32:
        return gpu_batch._dev(a.astype(np.uint32).view(np.int32), np.int32)
    return gpu_batch._dev(a, dt)


def read(amd, dev, reqs, want, verified=True, null_sel=False, max_len=65536, max_end=None, graph=False):
    """One lz4e_unpack_range_verified_batch_dev (verified=False: the plain
    range read) into exact-size guarded slots; asserts ret, the bytes, the
    guards and that the image did not change.  -> (ret, dst bytes)."""
    import torch
    m = len(reqs)
    sizes = np.array([max(r, 0) for r, _ in want], dtype=np.int64)
    doffs, total = gpu_batch._place(sizes, [(7 * j + 2) % 16 for j in range(m)], gap=gpu_batch.GAP)
    img = gpu_batch.pattern(total)
    dst = gpu_batch._dev(img, np.uint8)
    ret = torch.full((m,), -7777, dtype=torch.int32, device=dst.device)
    _d = gpu_batch._dev
    sel = None if null_sel else _d(np.array([e & 0xFFFFFFFF for e, _, _ in reqs], np.uint32).view(np.int32), np.int32)
    lo = _d([q[1] for q in reqs], np.int32)
    ln = _d([q[2] for q in reqs], np.int32)
    if max_end is None:
        max_end = max([q[1] + q[2] for q in reqs if q[1] >= 0 and q[2] >= 0] + [0])
    tail = (sel, lo, ln, dst, _d(doffs, np.int64), ret, max_end)
    if verified:
        def call():
            amd.unpack_range_verified_batch_dev(dev.packed.view, dev.pk_off, dev.pk_len, dev.pk_kind, dev.pk_crc,
                                                *tail, max_len=max_len)
    else:
        def call():
            amd.unpack_range_batch_dev(dev.packed.view, dev.pk_off, dev.pk_len, dev.pk_kind, *tail)
    before = dev.packed.host()
    if graph:
        call()  # warm-up outside the capture
        torch.cuda.synchronize()
        dst.copy_(torch.from_numpy(img).to(dst.device))
        ret.fill_(-7777)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        torch.cuda.synchronize()
        assert bool((ret == -7777).all()), "the capture itself ran the kernels"
        g.replay()
    else:
        call()
    torch.cuda.synchronize()
    r = ret.cpu().numpy()
    d = dst.cpu().numpy()
    bad = [(j, reqs[j], int(r[j]), want[j][0]) for j in range(m) if r[j] != want[j][0]]
    assert not bad, (len(bad), bad[:6])
    gpu_batch.check_guards(d, img, doffs, sizes, "range read")
    for j in range(m):
        assert d[doffs[j]:doffs[j] + sizes[j]].tobytes() == want[j][1], (j, reqs[j])
    assert np.array_equal(dev.packed.host(), before), "range read: the packed image changed"
    return r, d


def forced_mode_child():
    """Run in a fresh process with LZ4E_DECOMPRESS_MODE set (the library reads
    it once): verified and plain range reads of a store of blocks every
    decoder takes, one entry with a wrong pk_crc."""
    import lz4e_amd
    blocks, tt, lim = pack_model.small_mixed_blocks(300)
    n = len(blocks)
    k = np.arange(n)
    lens = np.array([len(b) for b in blocks], dtype=np.int64)
    caps = np.where(np.asarray(lim, dtype=bool) & (lens > 0), lens - 1, lens + lens // 255 + 16)
    st = pack_model.DevStore(lz4e_amd, blocks, src_skew=k % 16).compress(tt, caps, dst_skew=k * 5 % 16)
    r = st.ret.cpu().numpy()
    kept = np.where((r > 0) & (r < lens), r, lens)
    pk_off, pk_len, pk_kind = st.pack(16, int(((kept + 15) // 16 * 16).sum()), skew=5)
    assert (pk_kind == FRAME).any() and (pk_kind == RAW).any()
    _, col = crc_model.pack_crc(lz4e_amd, st)
    crc = col.cpu().numpy().view(np.uint32).copy()
    image = st.packed.host()[st.packed.base:]
    dev = Dev(st.packed, st.pk_off, st.pk_len, st.pk_kind, col)
    reqs = [(e, (37 * e) % 3000, 1 + (101 * e) % 1500) for e in range(n)] + [(e, 0, 4096) for e in range(0, n, 3)]
    prefix = lambda e, body, end: (min(len(blocks[e]), end), blocks[e])
    want = expected(image, pk_off, pk_len, pk_kind, crc, reqs, frame=prefix)
    assert all(v >= 0 for v, _ in want)
    got = read(lz4e_amd, dev, reqs, want, max_len=4096)
    plain = read(lz4e_amd, dev, reqs, want, verified=False)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    frame3 = int(np.flatnonzero(pk_kind == FRAME)[3])
    crc[frame3] ^= 0x10
    want = expected(image, pk_off, pk_len, pk_kind, crc, reqs, frame=prefix)
    assert sum(v == BAD_CRC for v, _ in want) >= 1
    read(lz4e_amd, dev.replaced(pk_crc=dev_column(crc, np.uint32)), reqs, want, max_len=4096)
    print("forced mode verified range read ok")
