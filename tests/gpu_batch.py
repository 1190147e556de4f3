"""Guarded, skewable device batches -- TEST INFRASTRUCTURE ONLY.

One helper for every test that calls the device-resident entry points
(lz4e_compress_batch_dev, lz4e_decompress_batch_dev2, their _dict forms and
the forced-decoder diagnostics):

  * placement: block i's input starts `src_skew[i]` bytes and its output slot
    `dst_skew[i]` bytes (0..15) past a 16-byte boundary; include/lz4e.h
    requires no alignment of src_off or dst_off.
  * an optional per-block dictionary right before the block's input
    (compress) or output (decompress).
  * guards: both tensors are pre-filled with a position-dependent byte
    pattern (a stray store of a constant cannot hide in it), output slots are
    at least 64 bytes apart with 16 or more bytes before the first and after
    the last block, and after the call every byte outside the union of
    [dst_off[i], dst_off[i] + dst_cap[i]) must still hold the pattern (or
    the dictionary placed there).  Bytes inside a slot past ret[i] are not
    constrained.
"""
import ctypes

import numpy as np

DEC_AUTO, DEC_WAVE, DEC_PIPE, DEC_SMALL, DEC_GROUP = 0, 1, 2, 6, 7
DEC_GROUP_NB = 9  # the group decoder without its hand-over (every block decoded by its group)
DEC_NAMES = {DEC_AUTO: "auto", DEC_WAVE: "wave", DEC_PIPE: "pipe", DEC_SMALL: "small",
             DEC_GROUP: "group", DEC_GROUP_NB: "group_nobail"}
FORCED_MODES = [DEC_WAVE, DEC_PIPE, DEC_SMALL, DEC_GROUP, DEC_GROUP_NB]

GAP = 64    # bytes between two output slots, at least
EDGE = 64   # bytes before the first and after the last block of a tensor (>= 16)
_PERIOD = 65521  # prime: the pattern never lines up with a power-of-two stride


def pattern(n: int) -> np.ndarray:
    """n bytes of a position-dependent fill: neighbouring bytes always differ
    (by 167 or 180 mod 256), the same position always holds the same byte."""
    i = np.arange(min(n, _PERIOD), dtype=np.int64)
    base = ((i * 167 + (i >> 8) * 13 + 0x5B) & 0xFF).astype(np.uint8)
    return np.resize(base, n)


def _per_block(v, n):
    a = np.zeros(n, dtype=np.int64) if v is None else np.broadcast_to(np.asarray(v, dtype=np.int64), (n,)).copy()
    assert ((a >= 0) & (a < 16)).all(), "skews are 0..15 bytes past a 16-byte boundary"
    return a


def _place(sizes, skews, before=None, gap=16):
    """Offsets of n regions of `sizes` bytes, region i at a 16-byte boundary
    plus skews[i], with before[i] bytes reserved right in front of it and at
    least `gap` bytes between regions (reservations included).  -> (offs, total)."""
    n = len(sizes)
    offs = np.zeros(n, dtype=np.int64)
    cur = EDGE - gap
    for i in range(n):
        b = int(before[i]) if before is not None else 0
        offs[i] = (cur + gap + b + 15) // 16 * 16 + int(skews[i])
        cur = int(offs[i]) + max(int(sizes[i]), 0)
    return offs, cur + EDGE + 15


class GuardError(AssertionError):
    pass


def check_guards(got: np.ndarray, image: np.ndarray, offs, caps, what: str) -> None:
    """Every byte of `got` outside the slots [offs[i], offs[i] + caps[i]) must
    equal `image` (the tensor before the call)."""
    n = len(offs)
    order = np.argsort(offs, kind="stable")
    lo = 0
    for k in range(n + 1):
        i = int(order[k]) if k < n else -1
        hi = int(offs[i]) if k < n else got.size
        if hi > lo and not np.array_equal(got[lo:hi], image[lo:hi]):
            p = lo + int(np.flatnonzero(got[lo:hi] != image[lo:hi])[0])
            q = lo + int(np.flatnonzero(got[lo:hi] != image[lo:hi])[-1])
            prev = int(order[k - 1]) if k else -1
            msg = f"{what}: write outside the output slots at byte {p}"
            if prev >= 0:
                msg += (f": block {prev} (dst_off {int(offs[prev])} = {int(offs[prev]) % 16} mod 16, "
                        f"cap {int(caps[prev])}) + {p - lo} past its slot's end")
            if i >= 0:
                msg += f"; {hi - q} bytes before block {i}'s slot (dst_off {hi} = {hi % 16} mod 16)"
            raise GuardError(msg + f"; {int((got[lo:hi] != image[lo:hi]).sum())} bytes differ in this gap")
        if k < n:
            lo = max(lo, hi + max(int(caps[i]), 0))


def device_pattern(n: int, device):
    """pattern(n) as a device tensor, built on the device (for tensors too
    large to fill from the host)."""
    import torch
    base = torch.from_numpy(pattern(_PERIOD)).to(device)
    return base.repeat(-(-n // _PERIOD))[:n].clone()


def check_guards_strided(t, image, stride: int, caps, what: str) -> None:
    """The guard check for equal-stride layouts, on the device: slot i is
    [i * stride, i * stride + caps[i]) of the uint8 tensor `t`; every other
    byte, the tail after the last stride included, must equal `image` (a
    tensor of the same size holding what `t` held before the call)."""
    import torch
    n = len(caps)
    capt = torch.as_tensor(np.asarray(caps, dtype=np.int64), device=t.device)[:, None]
    col = torch.arange(stride, device=t.device)[None, :]
    bad = (t[:n * stride].view(n, stride) != image[:n * stride].view(n, stride)) & (col >= capt)
    if bool(bad.any()):
        i, c = (int(x) for x in bad.nonzero()[0])
        raise GuardError(f"{what}: write outside the output slots: block {i} (dst_off {i * stride} = "
                         f"{i * stride % 16} mod 16, cap {int(caps[i])}) + {c - int(caps[i])} past its slot's "
                         f"end; {int(bad.sum())} bytes differ in all")
    if not torch.equal(t[n * stride:], image[n * stride:]):
        raise GuardError(f"{what}: write past the last block's stride (block {n - 1})")


def _dev(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(torch.device("cuda"))


def compress(amd, blocks, ttypes, caps=None, src_skew=None, dst_skew=None, dicts=None, guards=True,
             max_len=None):
    """lz4e_compress_batch_dev (with `dicts`: lz4e_compress_batch_dev_dict)
    -> (ret[], frames[], aux[n, 2])."""
    import torch
    n = len(blocks)
    lens = np.array([len(b) for b in blocks], dtype=np.int64)
    dlen = np.array([len(d) for d in dicts], dtype=np.int64) if dicts is not None else None
    offs, total = _place(lens, _per_block(src_skew, n), dlen)
    host = pattern(total)
    for i, b in enumerate(blocks):
        host[offs[i]:offs[i] + lens[i]] = np.frombuffer(bytes(b), dtype=np.uint8)
        if dicts is not None and dlen[i]:
            host[offs[i] - dlen[i]:offs[i]] = np.frombuffer(bytes(dicts[i]), dtype=np.uint8)
    bounds = lens + lens // 255 + 16
    caps = bounds if caps is None else np.asarray(caps, dtype=np.int64)
    doffs, dtotal = _place(caps, _per_block(dst_skew, n), gap=GAP)
    image = pattern(dtotal)
    src = torch.from_numpy(host).to(torch.device("cuda"))
    dst = _dev(image, np.uint8)
    ret = torch.full((n,), -7, dtype=torch.int32, device=dst.device)
    aux = torch.zeros(2 * n, dtype=torch.int32, device=dst.device)
    a = [_dev(offs, np.int64), _dev(lens, np.int32), _dev(ttypes, np.uint8), _dev(doffs, np.int64),
         _dev(caps, np.int32)]
    if dicts is None:
        amd.compress_batch_dev(src, a[0], a[1], a[2], dst, a[3], a[4], ret, aux, max_len=max_len)
    else:
        L = amd.lib()
        P = ctypes.c_void_p
        L.lz4e_compress_batch_dev_dict.argtypes = [P] * 9 + [ctypes.c_uint32, ctypes.c_uint32, P, P]
        d_dl = _dev(dlen, np.int32)
        ml = int(lens.max()) if max_len is None and n else int(max_len or 0)
        assert L.lz4e_compress_batch_dev_dict(src.data_ptr(), a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(),
                                              dst.data_ptr(), a[3].data_ptr(), a[4].data_ptr(), ret.data_ptr(),
                                              aux.data_ptr(), n, ml, d_dl.data_ptr(), None) == 0, amd.last_error()
    torch.cuda.synchronize()
    r = ret.cpu().numpy()
    d = dst.cpu().numpy()
    ax = aux.cpu().numpy().reshape(-1, 2)
    if guards:
        check_guards(d, image, doffs, caps, "compress" + ("_dict" if dicts is not None else ""))
        assert torch.equal(src.cpu(), torch.from_numpy(host)), "compress: the source tensor changed"
    frames = [d[doffs[i]:doffs[i] + max(r[i], 0)].tobytes() for i in range(n)]
    return r, frames, ax


def decompress(amd, frames, caps, csizes=None, max_cap=None, mode=DEC_AUTO, src_skew=None, dst_skew=None,
               dicts=None, guards=True):
    """lz4e_decompress_batch_dev2, or with a forced `mode` the diagnostic
    lz4e_debug_decompress_stamped; with `dicts` lz4e_decompress_batch_dev_dict
    / lz4e_debug_decompress_dict, block i's dictionary right before its
    output.  -> (ret[], outputs[])."""
    import torch
    n = len(frames)
    csizes = [len(f) for f in frames] if csizes is None else csizes
    flen = np.array([len(f) for f in frames], dtype=np.int64)
    offs, total = _place(np.maximum(flen, np.asarray(csizes, dtype=np.int64)), _per_block(src_skew, n))
    host = pattern(total)
    for i, f in enumerate(frames):
        host[offs[i]:offs[i] + flen[i]] = np.frombuffer(bytes(f), dtype=np.uint8)
    caps = np.asarray(caps, dtype=np.int64)
    dlen = np.array([len(d) for d in dicts], dtype=np.int64) if dicts is not None else None
    doffs, dtotal = _place(caps, _per_block(dst_skew, n), dlen, gap=GAP)
    image = pattern(dtotal)
    if dicts is not None:
        for i, dic in enumerate(dicts):
            if dlen[i]:
                image[doffs[i] - dlen[i]:doffs[i]] = np.frombuffer(bytes(dic), dtype=np.uint8)
    src = torch.from_numpy(host).to(torch.device("cuda"))
    dst = _dev(image, np.uint8)
    ret = torch.full((n,), -7777, dtype=torch.int32, device=dst.device)
    a = [_dev(offs, np.int64), _dev(csizes, np.int32), _dev(doffs, np.int64), _dev(caps, np.int32)]
    L = amd.lib()
    P, U32 = ctypes.c_void_p, ctypes.c_uint32
    if max_cap is None:
        max_cap = int(caps.max()) if n else 0
    max_cap = max(0, int(max_cap))
    if dicts is not None:
        d_dl = _dev(dlen, np.int32)
        L.lz4e_debug_decompress_dict.argtypes = [P] * 7 + [U32, U32, P, P, U32]
        L.lz4e_decompress_batch_dev_dict.argtypes = [P] * 7 + [U32, U32, P, P]
        args = [src.data_ptr(), a[0].data_ptr(), a[1].data_ptr(), dst.data_ptr(), a[2].data_ptr(),
                a[3].data_ptr(), ret.data_ptr(), n, max_cap, d_dl.data_ptr(), None]
        if mode == DEC_AUTO:
            assert L.lz4e_decompress_batch_dev_dict(*args) == 0, amd.last_error()
        else:
            assert L.lz4e_debug_decompress_dict(*args, mode) == 0, amd.last_error()
    elif mode == DEC_AUTO:
        amd.decompress_batch_dev(src, a[0], a[1], dst, a[2], a[3], ret, max_cap=max_cap)
    else:
        L.lz4e_debug_decompress_stamped.argtypes = [P] * 7 + [U32, P, P, U32, U32]
        assert L.lz4e_debug_decompress_stamped(src.data_ptr(), a[0].data_ptr(), a[1].data_ptr(),
                                               dst.data_ptr(), a[2].data_ptr(), a[3].data_ptr(),
                                               ret.data_ptr(), n, None, None, 0, mode) == 0
    torch.cuda.synchronize()
    r = ret.cpu().numpy()
    d = dst.cpu().numpy()
    if guards:
        check_guards(d, image, doffs, caps, f"decompress[{DEC_NAMES.get(mode, mode)}]"
                     + ("_dict" if dicts is not None else ""))
        assert torch.equal(src.cpu(), torch.from_numpy(host)), "decompress: the source tensor changed"
    return r, [d[doffs[i]:doffs[i] + max(r[i], 0)].tobytes() for i in range(n)]
