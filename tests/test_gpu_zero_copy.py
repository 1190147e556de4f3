"""lz4e_chunk_write_batch on registered host memory (the zero-copy path).

A request whose source segments, `data` and `frame` all lie inside one live
registration each (lz4e_register_host_memory) is served by the device itself:
sg_gather_kernel reads the segments out of the caller's pages,
sg_deliver_kernel writes `data` and `frame` there (csrc/lz4e_sg.hip).  Its
results must be those of the staged path, byte for byte, and nothing outside
its buffers may be touched: every data and frame buffer here sits between two
64-byte guards inside the arena.  lz4e_debug_chunk_zero_copy_requests counts
the requests that took the path, so each test also pins WHICH path ran.
"""
import ctypes
import os

import numpy as np
import pytest

import oracle_ref
from lz4e_amd import BYU16, BYU32, corpus, make_sg

pytestmark = pytest.mark.gpu

ARENA = 16 << 20
GUARD = 64
STAT_FIELDS = ("reqs_total", "reqs_failed", "vec_count", "data_in_bytes", "frame_bytes")


def _stats_tuple(st):
    return tuple(getattr(st, f) for f in STAT_FIELDS)


def _expect(gpu, srcs, payloads, frame_caps=None):
    """Per request (status, comp_size, data, frame) from the oracle, and the five stats."""
    exp, st = [], [0, 0, 0, 0, 0]
    for i, (s, blk) in enumerate(zip(srcs, payloads)):
        tt = gpu.table_type(s) if len(blk) >= 13 else BYU16
        if tt == 0:  # more than BIO_MAX_VECS segments
            exp.append((-gpu.EIO, 0, None, None))
            continue
        er, ef, _, _ = oracle_ref.compress(blk, tt)
        cap = None if frame_caps is None else frame_caps[i]
        if cap is not None and cap < er:
            exp.append((-gpu.ENOSPC, er, None, None))
            continue
        exp.append((0, er, blk, ef))
        st[0] += 1
        st[2] += 1 if len(blk) else 0
        st[3] += len(blk)
        st[4] += er
    return exp, tuple(st)


def _run(gpu, srcs, arena, frame_caps=None):
    """One guarded call with frames; returns (results, stats tuple, guard report, counter delta)."""
    stats = gpu.ChunkStats()
    c0 = gpu.zero_copy_requests()
    good, res, rep = gpu.chunk_write_batch(srcs, want_frames=True, stats=stats, arena=arena,
                                           frame_caps=frame_caps, guard=GUARD)
    assert good == sum(1 for r in res if r[0] == 0)
    return res, _stats_tuple(stats), rep, gpu.zero_copy_requests() - c0


def _layout_requests(gpu, arena):
    rng = np.random.default_rng(404)
    data = corpus.silesia_proxy(1 << 20, 41).tobytes()
    srcs, payloads = [], []
    sizes = [0, 1, 12, 13, 100, 4096, 4096, 8192, 65536, 65536, 30001, 131072]
    for i, n in enumerate(sizes):
        s = int(rng.integers(0, len(data) - n))
        blk = data[s:s + n]
        seg = [4096, 512, 1000][i % 3]
        done = int(rng.integers(1, 64)) if i % 4 == 3 else 0
        segs = [min(seg, n + done - k) for k in range(0, n + done, seg)] or [16]
        offs = [int(rng.integers(0, 4096)) for _ in segs]
        offs[0] = 4095 if i % 2 else offs[0]
        offs[-1] = 4095 if i % 3 == 0 else offs[-1]
        srcs.append(make_sg(blk, segs, offsets=offs, start_done=done, shuffle_seed=i, arena=arena))
        payloads.append(blk)
    for n, seg in ((200, 1), (3000, 17)):  # 1-byte segments (byU32: more than 16), 17-byte segments
        blk = data[5000:5000 + n]
        segs = [min(seg, n - k) for k in range(0, n, seg)]
        offs = [int(rng.integers(0, 4096)) for _ in segs]
        offs[3] = 4095
        srcs.append(make_sg(blk, segs, offsets=offs, shuffle_seed=n, arena=arena))
        payloads.append(blk)
    blk = data[:257 * 16]  # 257 segments: rejected before either path
    srcs.append(make_sg(blk, [16] * 257, arena=arena))
    payloads.append(blk)
    return srcs, payloads


def test_zero_copy_layouts(gpu):
    arena = gpu.HostArena(ARENA)
    srcs, payloads = _layout_requests(gpu, arena)
    exp, exp_stats = _expect(gpu, srcs, payloads)
    accepted = sum(1 for e in exp if e[0] == 0)
    assert accepted == len(srcs) - 1 and exp[-1][0] == -gpu.EIO
    staged = _run(gpu, srcs, arena)  # the arena is not registered yet: today's path
    with arena:
        direct = _run(gpu, srcs, arena)
    for name, (res, st, rep, delta), want_delta in (("staged", staged, 0), ("zero-copy", direct, accepted)):
        assert res == exp, name
        assert st == exp_stats, name
        assert rep.intact and not rep.bad, (name, rep.bad)
        assert rep.untouched[-1], name  # the rejected request: nothing written
        assert delta == want_delta, name
    assert staged[0] == direct[0] and staged[1] == direct[1]


def test_zero_copy_frame_capacity(gpu):
    arena = gpu.HostArena(1 << 20)
    data = corpus.silesia_proxy(3 * 20000, 7).tobytes()
    payloads = [data[i * 20000:i * 20000 + 20000 - 7 * i] for i in range(3)] * 2
    srcs = [make_sg(b, [4096] * 5, offsets=[i * 3] * 5, arena=arena) for i, b in enumerate(payloads)]
    sizes = [oracle_ref.compress(b, BYU16)[0] for b in payloads]
    caps = [sizes[0], sizes[1] - 1, 0, sizes[3] + 1, sizes[4], 0]
    exp, exp_stats = _expect(gpu, srcs, payloads, caps)
    assert [e[0] for e in exp] == [0, -gpu.ENOSPC, -gpu.ENOSPC, 0, 0, -gpu.ENOSPC]
    staged = _run(gpu, srcs, arena, caps)
    with arena:
        direct = _run(gpu, srcs, arena, caps)
    for name, (res, st, rep, delta), want_delta in (("staged", staged, 0), ("zero-copy", direct, 6)):
        assert res == exp, name  # -ENOSPC still reports comp_size
        assert st == exp_stats, name
        assert rep.intact, (name, rep.bad)
        # neither frame nor data of a request whose frame does not fit is written
        assert [rep.untouched[i] for i in (1, 2, 5)] == [True] * 3, name
        assert not any(rep.untouched[i] for i in (0, 3, 4)), name
        assert delta == want_delta, name


def test_zero_copy_mixed_call(gpu):
    bs = 16384
    arena = gpu.HostArena(4 << 20)
    data = corpus.silesia_proxy(17 * bs, 99).tobytes()
    payloads = [data[i * bs:(i + 1) * bs] for i in range(17)]
    srcs, where = [], []
    for i, b in enumerate(payloads[:16]):
        a = arena if i % 2 == 0 else None
        srcs.append(make_sg(b, [4096] * 4, arena=a))
        where.append(a)
    # sources and frame registered, only `data` in ordinary memory: staged
    srcs.append(make_sg(payloads[16], [4096] * 4, arena=arena))
    where.append((None, arena))
    exp, exp_stats = _expect(gpu, srcs, payloads)
    with arena:
        res, st, rep, delta = _run(gpu, srcs, where)
    assert res == exp and st == exp_stats
    assert rep.intact, rep.bad
    assert delta == 8


@pytest.fixture(scope="module")
def cycling(gpu):
    """64 x 64 KiB Silesia-proxy blocks as 16 x 4096 B and 16 blocks as 128 x
    512 B at random in-page offsets (byU32), their sources in one arena, and
    the oracle's results; a second arena takes the data and frame buffers."""
    bs = 65536
    rng = np.random.default_rng(17)
    src_arena, out_arena = gpu.HostArena(ARENA), gpu.HostArena(ARENA)
    data = corpus.silesia_proxy(80 * bs, 0x5157).tobytes()
    payloads = [data[i * bs:(i + 1) * bs] for i in range(80)]
    srcs = [make_sg(b, [4096] * 16, arena=src_arena) for b in payloads[:64]]
    for b in payloads[64:]:
        offs = [int(rng.integers(0, 4096 - 512 + 1)) for _ in range(128)]
        srcs.append(make_sg(b, [512] * 128, offsets=offs, shuffle_seed=5, arena=src_arena))
    assert gpu.table_type(srcs[0]) == BYU16 and gpu.table_type(srcs[64]) == BYU32
    exp, exp_stats = _expect(gpu, srcs, payloads)
    return src_arena, out_arena, srcs, payloads, exp, exp_stats


def test_zero_copy_slot_cycling(gpu, cycling):
    src_arena, out_arena, srcs, payloads, exp, exp_stats = cycling
    L = gpu.lib()
    L.lz4e_debug_chunk_sub_bytes.argtypes = [ctypes.c_uint64]
    out_arena.reset()
    with src_arena, out_arena:
        L.lz4e_debug_chunk_sub_bytes(512 << 10)  # ten sub-batches over the four slots
        try:
            res, st, rep, delta = _run(gpu, srcs, out_arena)
        finally:
            L.lz4e_debug_chunk_sub_bytes(0)
    assert res == exp and st == exp_stats
    assert rep.intact, rep.bad
    assert delta == 80


def test_zero_copy_injected_failure(gpu, cycling):
    src_arena, out_arena, srcs, payloads, exp, exp_stats = cycling
    srcs = srcs[:64]
    L = gpu.lib()
    L.lz4e_debug_chunk_sub_bytes.argtypes = [ctypes.c_uint64]
    L.lz4e_debug_chunk_fault_after.argtypes = [ctypes.c_int]
    n = len(srcs)
    stats = gpu.ChunkStats()
    with src_arena, out_arena:
        L.lz4e_debug_chunk_sub_bytes(512 << 10)
        L.lz4e_debug_chunk_fault_after(1)
        try:
            out_arena.reset()
            with pytest.raises(gpu.GpuUnavailable, match="injected"):
                gpu.chunk_write_batch(srcs, want_frames=True, stats=stats, arena=out_arena)
            # once more through the C ABI itself, to see every request's status
            out_arena.reset()
            reqs = (gpu.ChunkRequest * n)()
            bufs = []
            for i, s in enumerate(srcs):
                d = out_arena.alloc(65536 + 64)[64:]
                f = out_arena.alloc(gpu.compress_bound(65536) + 64)[64:]
                bufs.append((d, f))
                reqs[i].src = s.bvecs
                reqs[i].srcIter = ctypes.pointer(s.it)
                reqs[i].data = d.ctypes.data
                reqs[i].frame = f.ctypes.data
                reqs[i].frame_cap = gpu.compress_bound(65536)
                reqs[i].status = 0
            r = L.lz4e_chunk_write_batch(reqs, n, ctypes.byref(stats))
            err = gpu.last_error()
        finally:
            L.lz4e_debug_chunk_fault_after(-1)
            L.lz4e_debug_chunk_sub_bytes(0)
        assert r == -1 and "injected" in err
        out_arena.reset()
        assert all(reqs[i].status == -gpu.EIO and reqs[i].comp_size == 0 for i in range(n))
        assert _stats_tuple(stats) == (0, 0, 0, 0, 0)
        # the next zero-copy call is unaffected by what the failed ones left in flight
        res, st, rep, delta = _run(gpu, srcs[:5], out_arena)
    assert res == exp[:5] and rep.intact
    assert st[0] == 5 and st[3] == 5 * 65536
    assert delta == 5


def test_zero_copy_lifetime(gpu):
    arena = gpu.HostArena(2 << 20)
    data = corpus.silesia_proxy(5 * 10000, 3).tobytes()
    payloads = [data[i * 10000:(i + 1) * 10000 - i] for i in range(5)]
    srcs = [make_sg(b, [1000] * 10, offsets=[97 * k for k in range(10)], arena=arena) for b in payloads]
    exp, exp_stats = _expect(gpu, srcs, payloads)
    page = gpu.PAGE_SIZE

    def call(want_delta):
        used = arena.used
        res, st, rep, delta = _run(gpu, srcs, arena)
        arena.used = used  # the same buffers every time
        assert res == exp and st == exp_stats and rep.intact
        assert delta == want_delta

    with arena:
        call(5)
        # a range overlapping the live registration, and a pointer that is not its base
        assert gpu.register_host_memory(arena.base + page, page) == -22
        assert gpu.register_host_memory(arena.base - page, 2 * page) == -22
        assert gpu.unregister_host_memory(arena.base + page) == -2
        call(5)
        os.environ["LZ4E_CHUNK_ZERO_COPY"] = "0"  # read per call
        try:
            call(0)
        finally:
            del os.environ["LZ4E_CHUNK_ZERO_COPY"]
        call(5)
    call(0)  # unregistered: staged again, same results
    assert gpu.unregister_host_memory(arena.base) == -2
    with arena:  # the same pages again
        call(5)
    call(0)
