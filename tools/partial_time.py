"""Diagnostic: what a prefix costs against the whole block.  On silesia64k
(3 234 blocks of 64 KiB), with device events, alternating in one process after
a warm-up of every shape:

  (a) decompress every block completely       lz4e_decompress_batch_dev2
  (b) the first 4 KiB of every block          lz4e_decompress_partial_batch_dev
  (c) the first 16 KiB of every block         lz4e_decompress_partial_batch_dev
  (d) every block at its full size, partial   lz4e_decompress_partial_batch_dev
      entry (the price of the partial parse)
  (e) unpack of the packed image (align 1)     lz4e_unpack_batch_dev
  (f) 4 KiB at a random offset of every entry  lz4e_unpack_range_batch_dev
  (g) the first 4 KiB of every entry           lz4e_unpack_range_batch_dev

Prints medians and min-max over REPS (default 20) repetitions and each leg
against (a), and checks every leg's values and bytes.  `--once` runs each leg
once (for a rocprofv3 --kernel-trace --stats run, which gives the kernel
times)."""
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
    lz4e_amd.compress_batch_dev(src, offs, lens, tt, slots, doffs, caps, ret, max_len=bs)
    torch.cuda.synchronize()
    assert bool((ret > 0).all())
    want = src.view(n, bs)
    idx = (torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
           torch.zeros(n, dtype=torch.uint8, device=dev))
    packed = torch.zeros(n * bs, dtype=torch.uint8, device=dev)
    lz4e_amd.pack_batch_dev(slots, doffs, ret, src, offs, lens, packed, *idx, align=1, max_len=bs)
    rng = np.random.default_rng(7)
    lo_host = rng.integers(0, bs - 4096 + 1, n)
    lo_rand = torch.from_numpy(lo_host.astype(np.int32)).to(dev)
    lo_zero = torch.zeros(n, dtype=torch.int32, device=dev)
    len4k = torch.full((n,), 4096, dtype=torch.int32, device=dev)
    roffs = torch.arange(n, dtype=torch.int64, device=dev) * 4096
    rout = torch.zeros(n * 4096, dtype=torch.uint8, device=dev)

    def unpack():
        lz4e_amd.unpack_batch_dev(packed, *idx, out, offs, lens, dret, max_cap=bs)

    def rread(lo, max_end):
        return lambda: lz4e_amd.unpack_range_batch_dev(packed, *idx, None, lo, len4k, rout, roffs, dret, max_end)

    def range_ok(lo):
        at = lo.to(torch.int64)[:, None] + torch.arange(4096, device=dev)[None, :]
        return bool((dret == 4096).all()) and torch.equal(rout.view(n, 4096), torch.gather(want, 1, at))

    def full():
        lz4e_amd.decompress_batch_dev(slots, doffs, ret, out, offs, lens, dret, max_cap=bs)

    def prefix(k):
        tg = torch.full((n,), k, dtype=torch.int32, device=dev)
        return lambda: lz4e_amd.decompress_partial_batch_dev(slots, doffs, ret, out, offs, tg, dret, max_cap=k)

    legs = [("full", full, bs), ("partial_4k", prefix(4096), 4096), ("partial_16k", prefix(16384), 16384),
            ("partial_all", prefix(bs), bs), ("unpack", unpack, bs), ("range_4k_rand", rread(lo_rand, bs), 4096),
            ("range_4k_front", rread(lo_zero, 4096), 4096)]
    ok = {}
    for k, fn, size in legs:  # warm-up of every shape, and the check
        out.zero_()
        rout.zero_()
        fn()
        torch.cuda.synchronize()
        if k.startswith("range"):
            ok[k] = range_ok(lo_rand if k == "range_4k_rand" else lo_zero)
        else:
            ok[k] = bool((dret == size).all()) and torch.equal(out[:n * bs].view(n, bs)[:, :size], want[:, :size])
    t = {k: [] for k, _, _ in legs}
    for _ in range(reps):
        for k, fn, _ in legs:
            t[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(f"== {name}: {n} blocks of {bs} B, values and bytes ok={ok}")
    for k, _, size in legs:
        print(f"{k:12s} median {med[k]:8.3f} ms  min {min(t[k]):8.3f}  max {max(t[k]):8.3f}  "
              f"/ full {med[k] / med['full']:.3f}  ({n * size / med[k] / 1e6:.1f} GB/s of output)")
    print(f"full spread {min(t['full']) / med['full']:.3f}-{max(t['full']) / med['full']:.3f}", flush=True)


if __name__ == "__main__":
    reps = 1 if "--once" in sys.argv else int(os.environ.get("REPS", "20"))
    run("silesia64k", corpus.silesia_proxy(3234 * 65536, 0x5157), 65536, reps)
