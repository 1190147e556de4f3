"""Diagnostic: bench.py's end-to-end leg alone (lz4e_chunk_write_batch over
host bio_vec lists, PCIe-inclusive) per workload, for A/B of the chunk
pipeline's host side (LZ4E_LIB picks the library; LZ4E_CHUNK_PROF=1 adds
the per-phase host times on stderr).

--registered: the input and the output array live in host memory registered
with lz4e_register_host_memory, so every request takes the zero-copy path
(the library picks the path from the addresses: bench.end_to_end itself is
unchanged).  bench.end_to_end allocates its output with np.empty; for this
leg that one call is answered out of a registered arena.  The line then also
carries the requests the device gathered and the pinned host bytes the
pipeline holds after the call.

--each: five separate one-repetition measurements per workload (each after
its own warm-up call) instead of one median of five, all five values on the
line ("runs_gib_s"), for a leg whose spread matters.

usage: python tools/e2e.py [--registered] [--each] [workloads, e.g. silesia64k,text256k,fio4k]"""
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
registered = "--registered" in sys.argv[1:]
each = "--each" in sys.argv[1:]
names = args[0].split(",") if args else ["silesia64k", "text256k", "fio4k"]


class _ArenaNumpy:
    """numpy as bench.end_to_end sees it in the registered leg: np.empty of
    uint8 comes out of the arena, everything else is numpy's."""

    def __init__(self, arena):
        self._arena = arena

    def __getattr__(self, name):
        return getattr(np, name)

    def empty(self, shape, dtype=float, *a, **k):
        if np.dtype(dtype) == np.uint8 and np.ndim(shape) == 0 and not a and not k:
            return self._arena.alloc(int(shape), 4096)
        return np.empty(shape, dtype, *a, **k)


def pinned_bytes():
    import lz4e_amd
    L = lz4e_amd.lib()
    if not hasattr(L, "lz4e_debug_chunk_pinned_bytes"):
        return None
    L.lz4e_debug_chunk_pinned_bytes.restype = ctypes.c_uint64
    return int(L.lz4e_debug_chunk_pinned_bytes())


def measure(host, lens, bs, seg, after_call=lambda: None):
    """bench.end_to_end's result; with --each, five one-repetition runs of it."""
    if not each:
        return bench.end_to_end(host, lens, bs, seg, reps=5), 6
    runs = []
    for _ in range(5):
        runs.append(bench.end_to_end(host, lens, bs, seg, reps=1))
        after_call()
    r = dict(sorted(runs, key=lambda x: x["ms"])[2])
    r["runs_gib_s"] = [x["value"] for x in runs]
    return r, 10


for w in names:
    bs, cls, gen, seg, desc = bench.WORKLOADS[w]
    nblk = bench.DEFAULT_BLOCKS[w]
    U = min(nblk * bs, bench.TOTAL_BYTES.get(w, nblk * bs))
    lens = np.full(nblk, bs, dtype=np.int64)
    lens[-1] = U - (nblk - 1) * bs
    extra = {}
    if registered:
        import lz4e_amd
        arena = lz4e_amd.HostArena(2 * nblk * bs + 8192)
        host = arena.alloc(nblk * bs, 4096)
        host[:] = 0
        host[:U] = bench.make_data(gen, U, bench.CORPUS_SEED)
        with arena:
            c0 = lz4e_amd.zero_copy_requests()
            bench.np = _ArenaNumpy(arena)
            used = arena.used

            def reuse_output():
                arena.used = used

            try:
                r, calls = measure(host, lens, bs, seg, reuse_output)
            finally:
                bench.np = np
            extra = {"registered": True,
                     "zero_copy_requests_per_call": (lz4e_amd.zero_copy_requests() - c0) // calls}
    else:
        host = np.zeros(nblk * bs, np.uint8)
        host[:U] = bench.make_data(gen, U, bench.CORPUS_SEED)
        r, _ = measure(host, lens, bs, seg)
    pb = pinned_bytes()
    if pb is not None:
        extra["pinned_host_bytes"] = pb
    print(json.dumps({"workload": w, "lib": os.environ.get("LZ4E_LIB", ""), **r, **extra}), flush=True)
