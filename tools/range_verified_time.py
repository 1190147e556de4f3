"""Diagnostic: what the check costs a range read.  On silesia64k (3 234 entries
of 64 KiB, packed at align 1, with the checksum column of
lz4e_pack_crc_batch_dev), with device events, alternating in one process after
a warm-up of every shape:

  (f) 4 KiB at a random offset of every entry   lz4e_unpack_range_batch_dev
  (g) the first 4 KiB of every entry            lz4e_unpack_range_batch_dev
  (h) the checksum of every entry of the image  lz4e_crc32c_batch_dev
  (i) (f)'s requests, verified                  lz4e_unpack_range_verified_batch_dev
  (j) (g)'s requests, verified                  lz4e_unpack_range_verified_batch_dev
  (k) 16 requests on every 16th entry (3 234 requests on 203 distinct entries),
      4 KiB at random offsets                   lz4e_unpack_range_batch_dev
  (l) (k)'s requests, verified                  lz4e_unpack_range_verified_batch_dev
  (m) the checksum of those 203 entries only    lz4e_crc32c_batch_dev

Checks every leg's values and bytes (the checksum legs against the column),
prints medians and min-max over REPS (default 20) repetitions, each verified
leg against the sum of the plain read and the checksum it is made of --
(i) / ((f) + (h)), (j) / ((g) + (h)), (l) / ((k) + (m)) -- and the run-to-run
spread of the plain legs.  `--once` runs each leg once (for a rocprofv3
--kernel-trace --stats run)."""
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
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(dev)
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
    lz4e_amd.compress_batch_dev(src, offs, lens, tt, slots, doffs, caps, ret, max_len=bs)
    torch.cuda.synchronize()
    assert bool((ret > 0).all())
    want = src.view(n, bs)
    pk_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    pk_len = torch.zeros(n, dtype=torch.int32, device=dev)
    pk_kind = torch.zeros(n, dtype=torch.uint8, device=dev)
    pk_crc = torch.zeros(n, dtype=torch.int32, device=dev)
    packed = torch.zeros(n * bs, dtype=torch.uint8, device=dev)
    lz4e_amd.pack_batch_dev(slots, doffs, ret, src, offs, lens, packed, pk_off, pk_len, pk_kind, align=1, max_len=bs)
    lz4e_amd.pack_crc_batch_dev(slots, doffs, src, offs, pk_len, pk_kind, pk_crc, max_len=bs)
    torch.cuda.synchronize()
    idx = (pk_off, pk_len, pk_kind)

    rng = np.random.default_rng(7)
    lo_rand = i32(rng.integers(0, bs - 4096 + 1, n))
    lo_zero = torch.zeros(n, dtype=torch.int32, device=dev)
    lo_fan = i32(rng.integers(0, bs - 4096 + 1, n))
    sel_host = np.arange(n) // 16 * 16
    sel_fan = i32(sel_host)
    named = np.unique(sel_host)
    sub_off = pk_off[torch.from_numpy(named).to(dev)].contiguous()
    sub_len = pk_len[torch.from_numpy(named).to(dev)].contiguous()
    sub_crc = torch.zeros(named.size, dtype=torch.int32, device=dev)
    all_crc = torch.zeros(n, dtype=torch.int32, device=dev)
    len4k = torch.full((n,), 4096, dtype=torch.int32, device=dev)
    roffs = torch.arange(n, dtype=torch.int64, device=dev) * 4096
    rout = torch.zeros(n * 4096, dtype=torch.uint8, device=dev)
    rret = torch.zeros(n, dtype=torch.int32, device=dev)

    def plain(sel, lo, max_end):
        return lambda: lz4e_amd.unpack_range_batch_dev(packed, *idx, sel, lo, len4k, rout, roffs, rret, max_end)

    def verified(sel, lo, max_end):
        return lambda: lz4e_amd.unpack_range_verified_batch_dev(packed, *idx, pk_crc, sel, lo, len4k, rout, roffs,
                                                                rret, max_end, max_len=bs)

    def range_ok(sel, lo):
        rows = want if sel is None else want[sel.to(torch.int64)]
        at = lo.to(torch.int64)[:, None] + torch.arange(4096, device=dev)[None, :]
        return bool((rret == 4096).all()) and torch.equal(rout.view(n, 4096), torch.gather(rows, 1, at))

    def crc_all():
        lz4e_amd.crc32c_batch_dev(packed, pk_off, pk_len, all_crc, max_len=bs)

    def crc_named():
        lz4e_amd.crc32c_batch_dev(packed, sub_off, sub_len, sub_crc, max_len=bs)

    named_dev = torch.from_numpy(named).to(dev)
    legs = [("f range_rand", plain(None, lo_rand, bs), lambda: range_ok(None, lo_rand)),
            ("g range_front", plain(None, lo_zero, 4096), lambda: range_ok(None, lo_zero)),
            ("h crc_all", crc_all, lambda: torch.equal(all_crc, pk_crc)),
            ("i verified_rand", verified(None, lo_rand, bs), lambda: range_ok(None, lo_rand)),
            ("j verified_front", verified(None, lo_zero, 4096), lambda: range_ok(None, lo_zero)),
            ("k range_fan16", plain(sel_fan, lo_fan, bs), lambda: range_ok(sel_fan, lo_fan)),
            ("l verified_fan16", verified(sel_fan, lo_fan, bs), lambda: range_ok(sel_fan, lo_fan)),
            ("m crc_named", crc_named, lambda: torch.equal(sub_crc, pk_crc[named_dev]))]
    ok = {}
    for k, fn, check in legs:  # warm-up of every shape, and the check
        rout.zero_()
        rret.zero_()
        all_crc.zero_()
        sub_crc.zero_()
        fn()
        torch.cuda.synchronize()
        ok[k] = bool(check())
    t = {k: [] for k, _, _ in legs}
    for _ in range(reps):
        for k, fn, _ in legs:
            t[k].append(timed(fn))
    med = {k[0]: float(np.median(v)) for k, v in t.items()}
    print(f"== {name}: {n} entries of {bs} B, {named.size} named by the fan-in legs, values and bytes ok={ok}")
    for k, _, _ in legs:
        print(f"{k:16s} median {med[k[0]]:8.3f} ms  min {min(t[k]):8.3f}  max {max(t[k]):8.3f}  "
              f"spread {min(t[k]) / med[k[0]]:.3f}-{max(t[k]) / med[k[0]]:.3f}")
    for v, p, c in (("i", "f", "h"), ("j", "g", "h"), ("l", "k", "m")):
        print(f"({v}) / (({p}) + ({c})) = {med[v]:.3f} / ({med[p]:.3f} + {med[c]:.3f}) = "
              f"{med[v] / (med[p] + med[c]):.3f}   (target: at most 1.10)")
    print(f"(l) against 16 x (m), the checksum work without the election: {med['l']:.3f} vs "
          f"{med['k'] + 16 * med['m']:.3f} ms", flush=True)
    return all(ok.values())


if __name__ == "__main__":
    reps = 1 if "--once" in sys.argv else int(os.environ.get("REPS", "20"))
    sys.exit(0 if run("silesia64k", corpus.silesia_proxy(3234 * 65536, 0x5157), 65536, reps) else 1)
