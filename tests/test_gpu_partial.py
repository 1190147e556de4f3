"""Partial decoding on the GPU against tests/partial_model.py.

Every batch runs guarded (tests/gpu_batch.py): output slot i is exactly
target[i] bytes, at least 64 bytes from the next, in a tensor pre-filled with
a position-dependent pattern, and every byte outside the slots must survive.
The model's value must come back for every block -- errors included -- and
its bytes for every block with a value >= 0."""
import ctypes
import threading

import numpy as np
import pytest

import frame_synth
import gpu_batch
import oracle_ref
import pack_model
import partial_model
from gpu_batch import DEC_AUTO, DEC_PIPE, DEC_SMALL, DEC_WAVE

pytestmark = pytest.mark.gpu

MODES = [DEC_WAVE, DEC_SMALL, DEC_PIPE, DEC_AUTO]
MODE_IDS = [gpu_batch.DEC_NAMES[m] for m in MODES]


def partial_batch(amd, frames, targets, mode=DEC_AUTO, src_skew=None, dst_skew=None, max_cap=None):
    """lz4e_decompress_partial_batch_dev (forced mode: the diagnostic entry)
    on a guarded batch -> (ret[], outputs[])."""
    import torch
    n = len(frames)
    flen = np.array([len(f) for f in frames], dtype=np.int64)
    offs, total = gpu_batch._place(flen, gpu_batch._per_block(src_skew, n))
    host = gpu_batch.pattern(total)
    for i, f in enumerate(frames):
        host[offs[i]:offs[i] + flen[i]] = np.frombuffer(bytes(f), dtype=np.uint8)
    targets = np.asarray(targets, dtype=np.int64)
    doffs, dtotal = gpu_batch._place(targets, gpu_batch._per_block(dst_skew, n), gap=gpu_batch.GAP)
    image = gpu_batch.pattern(dtotal)
    src = torch.from_numpy(host).to(torch.device("cuda"))
    dst = gpu_batch._dev(image, np.uint8)
    ret = torch.full((n,), -7777, dtype=torch.int32, device=dst.device)
    dev = gpu_batch._dev
    amd.decompress_partial_batch_dev(src, dev(offs, np.int64), dev(flen, np.int32), dst, dev(doffs, np.int64),
                                     dev(targets, np.int32), ret,
                                     max_cap=int(targets.max()) if max_cap is None else max_cap,
                                     mode=None if mode == DEC_AUTO else mode)
    torch.cuda.synchronize()
    r = ret.cpu().numpy()
    d = dst.cpu().numpy()
    gpu_batch.check_guards(d, image, doffs, targets, f"partial[{gpu_batch.DEC_NAMES[mode]}]")
    assert torch.equal(src.cpu(), torch.from_numpy(host)), "partial: the source tensor changed"
    return r, [d[doffs[i]:doffs[i] + max(r[i], 0)].tobytes() for i in range(n)]


_model_cache = {}


def _model(frame, k):
    key = (frame, k)
    if key not in _model_cache:
        _model_cache[key] = partial_model.decode(frame, k, True)
    return _model_cache[key]


def _check(amd, work, mode, skews=False):
    """work: [(label, frame, target)]."""
    n = len(work)
    ss = [(7 * i + 3) % 16 for i in range(n)] if skews else None
    ds = [(5 * i + 1) % 16 for i in range(n)] if skews else None
    r, outs = partial_batch(amd, [w[1] for w in work], [w[2] for w in work], mode, ss, ds)
    bad = []
    for i, (label, frame, k) in enumerate(work):
        want = _model(frame, k)
        if r[i] != want[0] or (want[0] >= 0 and outs[i] != want[1]):
            bad.append((label, k, int(r[i]), want[0]))
    assert not bad, (gpu_batch.DEC_NAMES[mode], len(bad), bad[:8])


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_text600_at_every_target(gpu, mode):
    name, data, frame = partial_model.oracle_blocks()[0]
    assert len(data) == 600
    _check(gpu, [(name, frame, k) for k in range(0, 641)], mode)
    # the model's values on this frame are the prefix property itself
    assert all(_model(frame, k) == (min(k, 600), data[:k]) for k in range(1, 641))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_hand_built_frames(gpu, mode):
    work = []
    for name, (frame, full) in partial_model.hand_frames().items():
        work += [(name, frame, k) for k in partial_model.sampled_targets(len(full))]
        if name.startswith("match529"):
            work += [(name, frame, k) for k in (83, 84, 85, 147, 148, 149, 300)]
    for f in (b"\x00", b"\x10a", b"\xf0\x05" + b"a" * 14, b"\x50abc", b"\x10a\x05\x00zzzz",
              b"\x1fa\x01\x00\xff\x00\x00"):
        work += [("error-site", f, k) for k in (0, 1, 2, 3, 4, 10, 20, 64)]
    _check(gpu, work, mode, skews=True)


_work_cache = {}


def _profile_work(profile, large):
    """Every case of the profile at the sampled targets (partial_model.sampled_targets:
    every k from 0 to n + 19 for n <= 400, else k < 40, |k - n| < 20 and 60 seeded values)."""
    if (profile, large) not in _work_cache:
        _work_cache[profile, large] = [(c.label, c.frame, k)
                                       for ci, c in enumerate(frame_synth.cases(profile, large=large))
                                       for k in partial_model.sampled_targets(c.cap, ci)]
    return _work_cache[profile, large]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("profile", [p for p in frame_synth.PROFILES if p != "dict"])
def test_synthesized_profiles(gpu, profile, mode):
    _check(gpu, _profile_work(profile, False), mode, skews=True)


@pytest.mark.parametrize("mode", [DEC_WAVE, DEC_PIPE, DEC_AUTO], ids=["wave", "pipe", "auto"])
@pytest.mark.parametrize("profile", frame_synth.SIZED)
def test_synthesized_profiles_large(gpu, profile, mode):
    _check(gpu, _profile_work(profile, True), mode, skews=True)


_big = {}


def _big_text(n):
    if n not in _big:
        data = pack_model.text_block(n, 11)
        r, frame, _, _ = oracle_ref.compress(data, 3)
        assert r > 0
        _big[n] = (data, frame)
    return _big[n]


@pytest.mark.parametrize("mode", [DEC_WAVE, DEC_PIPE, DEC_AUTO], ids=["wave", "pipe", "auto"])
@pytest.mark.parametrize("n", [65536, 262144])
def test_large_text_blocks(gpu, n, mode):
    data, frame = _big_text(n)
    ks = [1, 4096, 65535, n - 1, n, n + 7]
    r, outs = partial_batch(gpu, [frame] * len(ks), ks, mode, [3] * len(ks), [9] * len(ks))
    for k, ri, o in zip(ks, r, outs):
        assert ri == min(k, n) and o == data[:min(k, n)], (k, int(ri))


def test_single_call_and_host_batch(gpu):
    name, data, frame = partial_model.oracle_blocks()[0]
    for k in (0, 1, 100, 599, 600, 700):
        assert gpu.decompress_safe_partial(frame, k) == _model(frame, k), k
    # targetOutputSize > dstCapacity: the capacity is the target, and is respected
    L = gpu.lib()
    buf = ctypes.create_string_buffer(b"\xAA" * 160, 160)
    src = ctypes.create_string_buffer(frame, len(frame))
    assert L.LZ4E_decompress_safe_partial(src, buf, len(frame), 600, 100) == 100
    assert buf.raw[:100] == data[:100] and buf.raw[100:] == b"\xAA" * 60
    assert L.LZ4E_decompress_safe_partial(src, buf, len(frame), -1, 100) == -1
    assert L.LZ4E_decompress_safe_partial(src, buf, len(frame), 50, -1) == -1
    # a frame the full decoder rejects and the partial one accepts
    f4, full4 = partial_model.hand_frames()["last4"]
    assert gpu.decompress_safe(f4, 296)[0] == -18
    assert gpu.decompress_safe_partial(f4, 296) == (296, full4)
    # the host batch, errors included
    frames = [frame, f4, b"\x50abc", b"\x10a\x05\x00zzzz", frame, b"\x00"]
    ks = [333, 290, 10, 20, 0, 0]
    got = gpu.decompress_partial_batch(frames, ks)
    want = [_model(f, k) for f, k in zip(frames, ks)]
    assert [r for r, _ in want] == [333, 290, -2, -5, -1, 0]
    # (a failed block's bytes are not part of the contract)
    assert got == [(r, b if r >= 0 else b"") for r, b in want]


def test_many_small_blocks_do_not_take_the_group_decoder(gpu):
    """16 384 blocks of 4 KiB: a full launch of this shape takes the group
    decoder, which has no partial form.  It would end each of these frames
    with an error (a full decode into 1 000 bytes fails at the first sequence
    that does not fit); the partial launch must return the target."""
    import torch
    name, data, frame = partial_model.oracle_blocks()[1]
    assert len(data) == 4096
    assert oracle_ref.decompress(frame, 1000)[0] < 0
    n, k, stride = 16384, 1000, 1088
    dev = torch.device("cuda")
    src = torch.from_numpy(np.frombuffer(frame + bytes(16), dtype=np.uint8).copy()).to(dev)
    image = gpu_batch.device_pattern(n * stride + 64, dev)
    dst = image.clone()
    ret = torch.full((n,), -7777, dtype=torch.int32, device=dev)
    z = torch.zeros(n, dtype=torch.int64, device=dev)
    ln = torch.full((n,), len(frame), dtype=torch.int32, device=dev)
    doff = torch.arange(n, dtype=torch.int64, device=dev) * stride
    cap = torch.full((n,), k, dtype=torch.int32, device=dev)
    gpu.decompress_partial_batch_dev(src, z, ln, dst, doff, cap, ret, max_cap=4096)
    torch.cuda.synchronize()
    assert bool((ret == k).all()), ret[ret != k][:8].tolist()
    want = torch.from_numpy(np.frombuffer(data[:k], dtype=np.uint8).copy()).to(dev)
    assert bool((dst[:n * stride].view(n, stride)[:, :k] == want[None, :]).all())
    gpu_batch.check_guards_strided(dst, image, stride, [k] * n, "partial[auto, 16384 blocks]")


def test_concurrent_full_and_partial_single_calls(gpu):
    """Full and partial single calls from 8 threads at once: the coalescer
    never mixes them into one launch, so each gets its own semantics."""
    name, data, frame = partial_model.oracle_blocks()[0]
    f4, full4 = partial_model.hand_frames()["last4"]
    bad = []

    def caller(t):
        for i in range(6):
            k = 37 * t + 11 * i + 1
            if (t + i) % 2:
                if gpu.decompress_safe_partial(frame, k) != (min(k, 600), data[:k]):
                    bad.append(("partial", t, k))
                if gpu.decompress_safe_partial(f4, 296) != (296, full4):
                    bad.append(("partial last4", t))
            else:
                want = oracle_ref.decompress(frame, k)
                if gpu.decompress_safe(frame, k)[0] != want[0]:
                    bad.append(("full", t, k))
                if gpu.decompress_safe(f4, 296)[0] != -18:
                    bad.append(("full last4", t))

    ts = [threading.Thread(target=caller, args=(t,)) for t in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts)
    assert not bad, bad[:8]
