"""Range reads from the packed frame store on the GPU
(lz4e_unpack_range_batch_dev) against a numpy model.

One store for the module: 40 blocks of 64 KiB compressed and packed on the
device -- text, incompressible blocks (stored raw), an empty block and blocks
whose compress was refused (stored raw) -- checked against
tests/pack_model.py's image first.  A request's expected value and bytes come
from the entry's data: for a frame entry the partial decode with target
lo + len (tests/partial_model.py; on these valid frames that is the block's
prefix, which the module checks once per distinct frame), for a raw entry the
stored bytes.  Every destination slot is exactly the bytes the request must
get, inside a pattern-filled tensor: anything else written is a failure."""
import numpy as np
import pytest

import gpu_batch
import oracle_ref
import pack_model
import partial_model
from lz4e_amd import BYU16

pytestmark = pytest.mark.gpu

BS = 65536
N = 40
RANDOM, EMPTY, REFUSED = (3, 17), (9,), (5, 22)


class Store:
    pass


@pytest.fixture(scope="module")
def store(gpu):
    texts = [pack_model.text_block(BS, 40 + s) for s in range(4)]
    blocks = []
    for i in range(N):
        if i in RANDOM:
            blocks.append(pack_model.random_block(BS, i))
        elif i in EMPTY:
            blocks.append(b"")
        else:
            blocks.append(texts[i % 4])
    lens = np.array([len(b) for b in blocks], dtype=np.int64)
    limited = np.isin(np.arange(N), REFUSED)
    caps = np.where(limited, lens - 1, lens + lens // 255 + 16)
    # a refused compress: a capacity below what the block needs
    caps[list(REFUSED)] = 100
    tts = [BYU16] * N
    k = np.arange(N)
    st = pack_model.DevStore(gpu, blocks, src_skew=k % 16).compress(tts, caps, dst_skew=k * 5 % 16)
    rets, frames = pack_model.oracle_frames(blocks, tts, caps)
    assert np.array_equal(st.ret.cpu().numpy(), rets)
    image, *want = pack_model.pack_expected(blocks, frames, rets, 512)
    got = st.pack(512, image.size, skew=5)
    pack_model.check_index(got, want, "pack")
    st.packed.check(image, "pack")
    s = Store()
    s.st, s.blocks, s.image = st, blocks, image
    s.pk_off, s.pk_len, s.pk_kind = want
    assert all(s.pk_kind[i] == pack_model.RAW for i in RANDOM + EMPTY + REFUSED)
    assert sum(s.pk_kind == pack_model.FRAME) == N - 5
    # the model on each distinct frame: a target past the end gives the block
    for i in (0, 1, 2, 7):
        f = image[s.pk_off[i]:s.pk_off[i] + s.pk_len[i]].tobytes()
        assert s.pk_kind[i] == pack_model.FRAME
        assert partial_model.decode(f, BS + 5, True) == (BS, blocks[i])
        assert partial_model.decode(f, 4097, True) == (4097, blocks[i][:4097])
    return s


def model(s, reqs, image=None, pk_len=None, pk_kind=None, decode_frames=False):
    """reqs: [(sel, lo, len)] -> [(ret, bytes)]."""
    image = s.image if image is None else image
    pk_len = s.pk_len if pk_len is None else pk_len
    pk_kind = s.pk_kind if pk_kind is None else pk_kind
    out = []
    for e, lo, ln in reqs:
        if not (0 <= e < N) or lo < 0 or ln < 0 or pk_kind[e] not in (pack_model.FRAME, pack_model.RAW) or pk_len[e] < 0:
            out.append((-1, b""))
        elif ln == 0:
            out.append((0, b""))
        else:
            body = image[int(s.pk_off[e]):int(s.pk_off[e]) + int(pk_len[e])].tobytes()
            if pk_kind[e] == pack_model.RAW:
                d, data = min(len(body), lo + ln), body
            elif decode_frames:
                d, data = partial_model.decode(body, lo + ln, True)
            else:  # a valid frame: the prefix (checked in the fixture)
                d, data = min(len(s.blocks[e]), lo + ln), s.blocks[e]
            out.append((d, b"") if d < 0 else (max(0, d - lo), data[lo:d]))
    return out


def range_read(gpu, s, reqs, want, null_sel=False, packed=None, pk_len=None, pk_kind=None, graph=False):
    """One guarded lz4e_unpack_range_batch_dev; asserts ret and bytes."""
    import torch
    m = len(reqs)
    sizes = np.array([max(r, 0) for r, _ in want], dtype=np.int64)
    doffs, total = gpu_batch._place(sizes, [(7 * j + 2) % 16 for j in range(m)], gap=gpu_batch.GAP)
    img = gpu_batch.pattern(total)
    dst = gpu_batch._dev(img, np.uint8)
    ret = torch.full((m,), -7777, dtype=torch.int32, device=dst.device)
    dev = gpu_batch._dev
    sel = None if null_sel else dev(np.array([e & 0xFFFFFFFF for e, _, _ in reqs], np.uint32).view(np.int32), np.int32)
    lo = dev([q[1] for q in reqs], np.int32)
    ln = dev([q[2] for q in reqs], np.int32)
    max_end = max([q[1] + q[2] for q in reqs if q[1] >= 0 and q[2] >= 0] + [0])
    st = s.st
    args = (st.packed.view if packed is None else packed, st.pk_off, st.pk_len if pk_len is None else pk_len,
            st.pk_kind if pk_kind is None else pk_kind, sel, lo, ln, dst, dev(doffs, np.int64), ret, max_end)
    before = st.packed.host()
    if graph:
        gpu.unpack_range_batch_dev(*args)  # warm-up outside the capture
        torch.cuda.synchronize()
        dst.copy_(torch.from_numpy(img).to(dst.device))
        ret.fill_(-7777)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gpu.unpack_range_batch_dev(*args)
        torch.cuda.synchronize()
        assert bool((ret == -7777).all()), "the capture itself ran the kernels"
        g.replay()
    else:
        gpu.unpack_range_batch_dev(*args)
    torch.cuda.synchronize()
    r = ret.cpu().numpy()
    d = dst.cpu().numpy()
    bad = [(j, reqs[j], int(r[j]), want[j][0]) for j in range(m) if r[j] != want[j][0]]
    assert not bad, (len(bad), bad[:6])
    gpu_batch.check_guards(d, img, doffs, sizes, "range read")
    for j in range(m):
        assert d[doffs[j]:doffs[j] + sizes[j]].tobytes() == want[j][1], (j, reqs[j])
    if packed is None:
        assert np.array_equal(st.packed.host(), before), "range read: the packed image changed"


def _grid(s):
    reqs = []
    for e in range(N):
        n = len(s.blocks[e])
        for lo in (0, 1, 4095, n - 1, n, n + 5):
            for ln in (0, 1, 4096, n):
                reqs.append((e, lo, ln))
    return reqs


def test_every_entry_at_the_grid_of_ranges(gpu, store):
    reqs = _grid(store)
    assert len(reqs) == N * 24
    # permuted: an entry's 24 requests are spread over the batch
    order = np.random.default_rng(5).permutation(len(reqs))
    reqs = [reqs[i] for i in order]
    range_read(gpu, store, reqs, model(store, reqs))


def test_null_sel_and_repeated_sel(gpu, store):
    reqs = [(j, 7 + j, 5000) for j in range(N)]
    range_read(gpu, store, reqs, model(store, reqs), null_sel=True)
    reqs = [(2, 100 * j, 300 + j) for j in range(70)] + [(3, 64 * j + 1, 4096) for j in range(70)]
    range_read(gpu, store, reqs, model(store, reqs))


def test_invalid_requests_and_a_damaged_store(gpu, store):
    import torch
    s = store
    # sel out of range
    reqs = [(N, 0, 16), (0xFFFFFFFF, 0, 16), (0, 0, 16), (N + 7, 5, 0), (1, -3, 16), (1, 3, -16)]
    want = model(s, [(e if e < 2 ** 31 else -1, lo, ln) for e, lo, ln in reqs])
    assert [r for r, _ in want] == [-1, -1, 16, -1, -1, -1]
    range_read(gpu, s, reqs, want)
    # an unknown kind and a negative length in the index
    kind, ln = s.pk_kind.copy(), s.pk_len.copy()
    kind[1], kind[3] = 2, 255
    ln[4], ln[17] = -1, -65536
    reqs = [(e, lo, 64) for e in (0, 1, 3, 4, 17, 6) for lo in (0, 33)]
    want = model(s, reqs, pk_len=ln, pk_kind=kind)
    assert [r for r, _ in want] == [64, 64] + [-1] * 8 + [64, 64]
    range_read(gpu, s, reqs, want, pk_len=gpu_batch._dev(ln, np.int32), pk_kind=gpu_batch._dev(kind, np.uint8))
    # a damaged frame: the error code is the model's (the partial decode of the damaged bytes)
    # (two 0xFF bytes at the first place where the model then fails: an offset before the block's start)
    at = int(s.pk_off[0])
    reqs = [(0, 0, 4096), (0, 10, 20), (0, 60000, 5000), (1, 0, 4096)]
    for p in range(2, 600):
        image = s.image.copy()
        image[at + p:at + p + 2] = 0xFF
        body = image[at:at + int(s.pk_len[0])].tobytes()
        if partial_model.decode(body, 2048, True)[0] < 0:
            break
    else:
        pytest.fail("no damage found that the model rejects")
    want = model(s, reqs, image=image, decode_frames=True)
    assert want[2][0] < 0 and want[3][0] == 4096
    damaged = pack_model.Guarded(image.size, 5, image)
    range_read(gpu, s, reqs, want, packed=damaged.view)
    assert np.array_equal(damaged.host(), damaged.before)


def test_under_graph_capture(gpu, store):
    reqs = [(e, 1000 + e, 4096) for e in range(N)]
    range_read(gpu, store, reqs, model(store, reqs), graph=True)
