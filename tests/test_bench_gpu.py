"""bench.py's measurement legs on a small batch (GPU): the decompress-only
leg of configs[4] and the per-block floor, through the same functions the
bench line uses, on 256 KiB text blocks -- sizes decoded exact, the bytes
equal to the input, the lines well formed."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def text_batch():
    import torch
    import bench
    import lz4e_amd
    if not lz4e_amd.gpu_available():
        pytest.fail("HIP path unavailable: " + lz4e_amd.last_error())
    dev = torch.device("cuda:0")
    bs, nblk = 262144, 48
    lens = np.full(nblk, bs, dtype=np.int64)
    lens[-1] = 182784  # the enwik9 layout's short last block
    host = np.zeros(nblk * bs, np.uint8)
    host[:int(lens.sum())] = bench.make_data("text", int(lens.sum()), 11)
    b = bench.Batch(torch.from_numpy(host).to(dev), lens, bs, lz4e_amd.BYU32, dev)
    b.run(1, False)
    b.check_roundtrip()
    return b, dev


def test_decompress_only_leg(text_batch):
    import torch
    import bench
    b, dev = text_batch
    b.d_out.zero_()
    b.d_dret.zero_()
    out = bench.decompress_only(b, 3, 0, 1, None, dev, "", "text256k")
    assert (b.d_dret.cpu().numpy() == b.lens).all()
    n = int(b.lens.sum())
    assert torch.equal(b.d_out[:n], b.d_src[:n])
    w, s = out["weak"], out["strong"]
    assert out["kernel"] == "decompress" and w["value"] > 0 and w["ms_per_step"] > 0
    assert w["roofline"]["algorithmic_bytes_per_launch"] == n + int(b.rets.astype(np.int64).sum())
    assert 0 < w["roofline"]["frac"] < 1
    # one rank: the strong job is the whole batch
    assert s["blocks_this_rank"] == b.nblk and s["value"] > 0


def test_block_floor_leg(text_batch):
    import bench
    b, _ = text_batch
    f = bench.block_floor(b, top=2, reps=2)
    assert f["floor_ms"] > 0 and f["compress_ms"] > 0 and f["decompress_ms"] > 0
    assert (b.d_dret.cpu().numpy() == b.lens).all()


def _checksums(rows):
    """bench._row_checksums restated on host byte strings."""
    out = np.zeros((len(rows), 2), np.float64)
    for i, r in enumerate(rows):
        x = np.frombuffer(r, np.uint8).astype(np.int64)
        out[i] = x.sum(), (x * (np.arange(x.size) % 65521 + 1)).sum()
    return out


def test_dump_outputs(text_batch, tmp_path):
    """--dump-outputs: every array float32/float64, within the size limit, and
    equal to what the batch's buffers hold after a step."""
    import bench
    b, _ = text_batch
    b.run(1, False)
    written = bench.dump_outputs(b, str(tmp_path))
    got = {n: np.load(tmp_path / (n + ".npy")) for n in written}
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(n + ".npy" for n in written)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    rets = b.d_ret.cpu().numpy()
    dst, out = b.d_dst.cpu().numpy(), b.d_out.cpu().numpy()
    frames = [dst[o:o + r].tobytes() for o, r in zip(b.doffs, rets)]
    blocks = [out[o:o + n].tobytes() for o, n in zip(b.offs, b.lens)]
    assert (got["compress_ret"] == rets).all() and (rets > 0).all()
    assert (got["decompress_ret"] == b.lens).all()
    assert (got["frame_checksums"] == _checksums(frames)).all()
    assert (got["output_checksums"] == _checksums(blocks)).all()
    pick = got["sample_blocks"].astype(np.int64)
    assert 0 < len(pick) <= b.nblk and len(set(pick)) == len(pick)
    assert got["frames_sample"].shape == (len(pick), b.slot)
    assert got["output_sample"].shape == (len(pick), b.bs)
    for row, i in enumerate(pick):
        f, o = got["frames_sample"][row], got["output_sample"][row]
        assert f[:rets[i]].astype(np.uint8).tobytes() == frames[i] and (f[rets[i]:] == -1).all()
        assert o[:b.lens[i]].astype(np.uint8).tobytes() == blocks[i] and (o[b.lens[i]:] == -1).all()
    # the same state dumped again: the same sample, the same arrays
    again = bench.dump_outputs(b, str(tmp_path / "again"))
    assert again == written
    assert all((np.load(tmp_path / "again" / (n + ".npy")) == got[n]).all() for n in written)


def test_plain_run_line_and_dump(tmp_path):
    """A plain `bench.py --gpus 1 --steps N --warmup W` run: N timed steps, the
    headline keys, none of the --full legs; its dumped frame sizes are the
    oracle's for the seeded corpus (so the inputs are the same in every
    process)."""
    import json
    import subprocess

    import bench
    import oracle_ref
    nblk, bs = 48, 65536
    run = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3",
                          "--warmup", "1", "--blocks", str(nblk), "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads([x for x in run.stdout.splitlines() if x.startswith("{")][-1])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1 and res["full"] is False
    assert res["unit"] == "GiB/s" and res["higher_is_better"] is True and res["dtype"] == "u8"
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(nblk * bs / (res["ms_per_step"] / 1e3) / 2**30, rel=1e-2)
    for leg in ("strong", "end_to_end", "single_call", "cpu_baseline", "cpu_baseline_sg", "decompress_only"):
        assert leg not in res
    assert res["parity"] is None and res["ratio_delta_vs_ref"] is None
    host = bench.make_data("silesia", nblk * bs, bench.CORPUS_SEED)
    want, _ = oracle_ref.compress_blocks(host, np.arange(nblk) * bs, [bs] * nblk, [1] * nblk)
    assert (np.load(tmp_path / "compress_ret.npy") == want).all()
    assert (np.load(tmp_path / "decompress_ret.npy") == bs).all()
