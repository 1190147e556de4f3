"""Diagnostic: compress time of several builds of the library in ONE process.

    python3 tools/ctime_ab.py name=lib.so [name=lib.so ...] [--workloads a,b,...]

Every library is loaded with ctypes and called through lz4e_compress_batch_dev
on the same device buffers.  Per workload and library: three rounds, each the
median (and fastest-slowest) of 9 launches after 2 warm-ups, HIP events around
the call with a synchronize after every launch; the libraries alternate inside
a round.  Every return value, frame and post-state of the first round is
compared with the first library's (frames_equal).
Workloads: silesia64k, silesia64k-u32 (the same data as byU32), text256k, fio4k.
"""
import ctypes
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lz4-sgori_amd"))
from lz4e_amd import corpus  # noqa: E402

P, U32 = ctypes.c_void_p, ctypes.c_uint32
WORKLOADS = {
    "silesia64k": lambda: (corpus.silesia_proxy(3234 * 65536, 0x5157), 65536, 1),
    "silesia64k-u32": lambda: (corpus.silesia_proxy(3234 * 65536, 0x5157), 65536, 3),
    "text256k": lambda: (corpus.text_proxy(3815 * 262144, 7), 262144, 3),
    "fio4k": lambda: (corpus.fio_pattern(262144 * 4096), 4096, 1),
}


def load(path):
    L = ctypes.CDLL(os.path.abspath(path))
    L.lz4e_compress_batch_dev.argtypes = [P] * 9 + [U32, U32, P]
    L.lz4e_compress_batch_dev.restype = ctypes.c_int
    return L


def run(name, libs):
    data, bs, cls = WORKLOADS[name]()
    dev = torch.device("cuda")
    n = data.size // bs
    cap = bs + bs // 255 + 16
    slot = (cap + 79) // 16 * 16
    offs = torch.arange(n, dtype=torch.int64, device=dev) * bs
    lens = torch.full((n,), bs, dtype=torch.int32, device=dev)
    tt = torch.full((n,), cls, dtype=torch.uint8, device=dev)
    doffs = torch.arange(n, dtype=torch.int64, device=dev) * slot
    caps = torch.full((n,), cap, dtype=torch.int32, device=dev)
    src = torch.from_numpy(data).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    first = None
    for rnd in range(3):
        for tag, L in libs:
            dst = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
            ret = torch.zeros(n, dtype=torch.int32, device=dev)
            aux = torch.zeros(2 * n, dtype=torch.int32, device=dev)
            ts = []
            for i in range(11):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = L.lz4e_compress_batch_dev(src.data_ptr(), offs.data_ptr(), lens.data_ptr(), tt.data_ptr(),
                                              dst.data_ptr(), doffs.data_ptr(), caps.data_ptr(), ret.data_ptr(),
                                              aux.data_ptr(), n, bs, stream)
                e1.record()
                torch.cuda.synchronize()
                assert r == 0, (tag, r)
                if i >= 2:
                    ts.append(e0.elapsed_time(e1))
            extra = ""
            if rnd == 0:
                # bytes of every slot up to its frame's end
                keep = torch.arange(slot, device=dev)[None, :] < ret[:, None]
                got = (ret.clone(), aux.clone(), torch.where(keep, dst.view(n, slot), 0))
                if first is None:
                    first = got
                    extra = f"  frames {n}, bytes {int(ret.sum())}"
                else:
                    extra = f"  frames_equal={all(torch.equal(a, b) for a, b in zip(first, got))}"
            print(f"{name:15s} {tag:10s} round {rnd}: compress {np.median(ts):8.4f} ms "
                  f"({min(ts):.4f}-{max(ts):.4f}){extra}", flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    wl = "silesia64k,silesia64k-u32,text256k,fio4k"
    if "--workloads" in sys.argv:
        wl = sys.argv[sys.argv.index("--workloads") + 1]
        args.remove(wl)
    libs = [(a.split("=", 1)[0], load(a.split("=", 1)[1])) for a in args]
    for w in wl.split(","):
        run(w, libs)
