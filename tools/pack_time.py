"""Diagnostic: what keeping the frames costs.  On silesia64k and fio4k, with
device events, alternating in one process after a warm-up of every shape:

  (a) compress into slots                      lz4e_compress_batch_dev
  (b) pack at align 1 and at align 4096        lz4e_pack_batch_dev
  (c) hipMemcpyDtoDAsync of pk_off[n] bytes    the yardstick: a copy that
                                               moves the same bytes
  (d) decompress from the slots                lz4e_decompress_batch_dev2
  (e) unpack of the packed image (align 1)     lz4e_unpack_batch_dev

Prints medians and min-max over REPS (default 20) repetitions, pack as a
share of (a) and as a multiple of (c), (e) against (d), and checks the round
trip.  `--once` runs each leg once (for a rocprofv3 --kernel-trace --stats
run, which gives the kernel times)."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lz4-sgori_amd"))
import lz4e_amd  # noqa
from lz4e_amd import corpus  # noqa


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run(name, data, bs, reps):
    dev = torch.device("cuda")
    n = data.size // bs
    offs = torch.arange(n, dtype=torch.int64, device=dev) * bs
    lens = torch.full((n,), bs, dtype=torch.int32, device=dev)
    tt = torch.full((n,), 1, dtype=torch.uint8, device=dev)
    cap = bs + bs // 255 + 16
    slot = (cap + 79) // 16 * 16
    doffs = torch.arange(n, dtype=torch.int64, device=dev) * slot
    caps = torch.full((n,), cap, dtype=torch.int32, device=dev)
    src = torch.from_numpy(data).to(dev)
    slots = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    ret = torch.zeros(n, dtype=torch.int32, device=dev)
    out = torch.zeros(n * bs + 64, dtype=torch.uint8, device=dev)
    dret = torch.zeros(n, dtype=torch.int32, device=dev)
    idx = {a: (torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
               torch.zeros(n, dtype=torch.uint8, device=dev)) for a in (1, 4096)}
    packed = {a: torch.zeros(n * (bs + 4096), dtype=torch.uint8, device=dev) for a in (1, 4096)}
    mirror = torch.zeros(n * bs, dtype=torch.uint8, device=dev)

    def compress():
        lz4e_amd.compress_batch_dev(src, offs, lens, tt, slots, doffs, caps, ret, max_len=bs)

    def pack(a):
        lz4e_amd.pack_batch_dev(slots, doffs, ret, src, offs, lens, packed[a], *idx[a], align=a, max_len=bs)

    compress()
    pack(1)
    pack(4096)
    torch.cuda.synchronize()
    total = {a: int(idx[a][0][n]) for a in (1, 4096)}
    raw = int((idx[1][2] == lz4e_amd.PACK_RAW).sum())

    def memcpy():
        mirror[:total[1]].copy_(packed[1][:total[1]])  # hipMemcpyDtoDAsync on the current stream

    def decompress():
        lz4e_amd.decompress_batch_dev(slots, doffs, ret, out, offs, lens, dret, max_cap=bs)

    def unpack():
        lz4e_amd.unpack_batch_dev(packed[1], *idx[1], out, offs, lens, dret, max_cap=bs)

    legs = [("compress", compress), ("pack_a1", lambda: pack(1)), ("pack_a4096", lambda: pack(4096)),
            ("memcpy_d2d", memcpy), ("decompress", decompress), ("unpack", unpack)]
    for _, fn in legs:  # warm-up of every shape
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k, _ in legs}
    for _ in range(reps):
        for k, fn in legs:
            t[k].append(timed(fn))
    ok = bool((dret == lens).all()) and torch.equal(out[:n * bs], src)  # the last leg was the unpack
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(f"== {name}: {n} blocks of {bs} B, stored {total[1]} B at align 1 ({n * bs / total[1]:.4f}:1), "
          f"{total[4096]} B at align 4096, {raw} raw entries, unpack round trip ok={ok}")
    for k, _ in legs:
        print(f"{k:12s} median {med[k]:8.3f} ms  min {min(t[k]):8.3f}  max {max(t[k]):8.3f}")
    print(f"pack_a1 / compress {med['pack_a1'] / med['compress']:.3f}   pack_a1 / memcpy {med['pack_a1'] / med['memcpy_d2d']:.2f}   "
          f"pack_a4096 / compress {med['pack_a4096'] / med['compress']:.3f}   "
          f"unpack / decompress {med['unpack'] / med['decompress']:.3f} "
          f"(decompress spread {min(t['decompress']) / med['decompress']:.3f}-{max(t['decompress']) / med['decompress']:.3f})",
          flush=True)


if __name__ == "__main__":
    reps = 1 if "--once" in sys.argv else int(os.environ.get("REPS", "20"))
    run("silesia64k", corpus.silesia_proxy(3234 * 65536, 0x5157), 65536, reps)
    run("fio4k", corpus.fio_pattern(262144 * 4096), 4096, reps)
