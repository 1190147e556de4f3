"""Diagnostic: what the store's integrity costs.  On silesia64k and fio4k, with
device events, alternating in one process after a warm-up of every shape:

  (a) compress into slots                      lz4e_compress_batch_dev
  (b) pack at align 1                          lz4e_pack_batch_dev
  (c) the index's checksum column              lz4e_pack_crc_batch_dev
  (d) the same column from the image           lz4e_crc32c_batch_dev(packed, pk_off, pk_len)
  (e) hipMemcpyDtoDAsync of pk_off[n] bytes    the yardstick: a copy that
                                               moves the same bytes
  (f) unpack of the packed image               lz4e_unpack_batch_dev
  (g) the same, every entry checked first      lz4e_unpack_verified_batch_dev

Prints medians and min-max over REPS (default 20) repetitions, pack_crc as a
share of (a), as a multiple of (b) and of (e), (g) against (f), and checks
both columns against each other and the round trip.  With an argument, also
writes the table as JSON to that path.  `--once` runs each leg once (for a
rocprofv3 --kernel-trace --stats run, which gives the kernel times)."""
import json
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
    pk_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    pk_len = torch.zeros(n, dtype=torch.int32, device=dev)
    pk_kind = torch.zeros(n, dtype=torch.uint8, device=dev)
    pk_crc = torch.zeros(n, dtype=torch.int32, device=dev)
    img_crc = torch.zeros(n, dtype=torch.int32, device=dev)
    packed = torch.zeros(n * bs, dtype=torch.uint8, device=dev)
    mirror = torch.zeros(n * bs, dtype=torch.uint8, device=dev)

    def compress():
        lz4e_amd.compress_batch_dev(src, offs, lens, tt, slots, doffs, caps, ret, max_len=bs)

    def pack():
        lz4e_amd.pack_batch_dev(slots, doffs, ret, src, offs, lens, packed, pk_off, pk_len, pk_kind, align=1, max_len=bs)

    def pack_crc():
        lz4e_amd.pack_crc_batch_dev(slots, doffs, src, offs, pk_len, pk_kind, pk_crc, max_len=bs)

    def crc_image():
        lz4e_amd.crc32c_batch_dev(packed, pk_off, pk_len, img_crc, max_len=bs)

    compress()
    pack()
    torch.cuda.synchronize()
    total = int(pk_off[n])
    raw = int((pk_kind == lz4e_amd.PACK_RAW).sum())

    def memcpy():
        mirror[:total].copy_(packed[:total])  # hipMemcpyDtoDAsync on the current stream

    def unpack():
        lz4e_amd.unpack_batch_dev(packed, pk_off, pk_len, pk_kind, out, offs, lens, dret, max_cap=bs)

    def unpack_verified():
        lz4e_amd.unpack_verified_batch_dev(packed, pk_off, pk_len, pk_kind, pk_crc, out, offs, lens, dret, max_cap=bs)

    legs = [("compress", compress), ("pack", pack), ("pack_crc", pack_crc), ("crc_image", crc_image),
            ("memcpy_d2d", memcpy), ("unpack", unpack), ("unpack_verified", unpack_verified)]
    for _, fn in legs:  # warm-up of every shape
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k, _ in legs}
    for _ in range(reps):
        for k, fn in legs:
            t[k].append(timed(fn))
    # the last leg was the verified unpack
    ok = bool((dret == lens).all()) and torch.equal(out[:n * bs], src) and torch.equal(pk_crc, img_crc)
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(f"== {name}: {n} blocks of {bs} B, stored {total} B ({n * bs / total:.4f}:1), {raw} raw entries, "
          f"columns equal and verified round trip ok={ok}")
    for k, _ in legs:
        print(f"{k:16s} median {med[k]:8.3f} ms  min {min(t[k]):8.3f}  max {max(t[k]):8.3f}   "
              f"{total / med[k] / 1e6 if k in ('pack_crc', 'crc_image', 'memcpy_d2d') else n * bs / med[k] / 1e6:9.1f} GB/s")
    ratios = {"pack_crc / compress": med["pack_crc"] / med["compress"],
              "pack_crc / pack": med["pack_crc"] / med["pack"],
              "pack_crc / memcpy_d2d": med["pack_crc"] / med["memcpy_d2d"],
              "crc_image / pack_crc": med["crc_image"] / med["pack_crc"],
              "unpack_verified / unpack": med["unpack_verified"] / med["unpack"]}
    print("   ".join(f"{k} {v:.3f}" for k, v in ratios.items()), flush=True)
    return {"workload": name, "blocks": n, "block_bytes": bs, "stored_bytes": total, "raw_entries": raw, "ok": ok,
            "reps": reps, "ms": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in t.items()},
            "ratios": ratios}


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--once"]
    reps = 1 if "--once" in sys.argv else int(os.environ.get("REPS", "20"))
    results = [run("silesia64k", corpus.silesia_proxy(3234 * 65536, 0x5157), 65536, reps),
               run("fio4k", corpus.fio_pattern(262144 * 4096), 4096, reps)]
    if args:
        with open(args[0], "w") as f:
            json.dump(results, f, indent=1)
    if not all(r["ok"] for r in results):
        sys.exit("crc_time: a column or a round trip did not match")
