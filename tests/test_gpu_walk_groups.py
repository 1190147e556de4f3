"""The parser's chain walk and clash groups on the GPU.

The blocks of tests/walk_group_inputs.py -- period-k data, groups laid on the
lanes of a window, different bytes with one hash, chains of exactly 1..9 links
ended in each way, chains that leave their window at every shift -- as device
batches through compress_batch_dev: the small blocks (13..4 096 bytes) in a
batch whose max_len selects the LDS-image kernel, the same blocks padded to
4 097..8 192 bytes (and the small ones again) in one that selects the
HBM-image kernel's two waves, and both with every second block's capacity one
byte under the bound (inline emit).  byU16 and byU32, the period and group
blocks also as byU64.  Return values, frames and post-states equal the
oracle's byte for byte, and every frame decodes back to its block;
tests/gpu_batch.py checks the guard bytes around every slot.
"""
import pytest

import gpu_batch
import oracle_ref
import parse_synth as ps
import walk_group_inputs as wg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batches():
    """{name: (labelled blocks, the oracle's results unlimited, max_len)}, computed once."""
    small = list(wg.all_small())
    mixed = list(wg.all_hbm()) + small
    out = {}
    for name, labelled, max_len in (("lds", small, 4096), ("hbm", mixed, 8192)):
        assert max(len(b) for _, b, _ in labelled) <= max_len
        out[name] = (labelled, [oracle_ref.compress(b, tt) for _, b, tt in labelled], max_len)
    assert min(len(b) for _, b, _ in wg.all_hbm()) >= 4097
    return out


def _check(gpu, labelled, expected, max_len, caps=None):
    blocks = [b for _, b, _ in labelled]
    r, frames, aux = gpu_batch.compress(gpu, blocks, [tt for _, _, tt in labelled], caps=caps, max_len=max_len,
                                        dst_skew=[(5 * i + 3) % 16 for i in range(len(labelled))])
    for i, (label, _, tt) in enumerate(labelled):
        er, ef, efs, elr = expected[i]
        assert int(r[i]) == er, (label, tt, int(r[i]), er)
        assert frames[i] == ef, (label, tt)
        if er > 0:
            assert (aux[i][0], aux[i][1]) == (efs, elr), (label, tt)
    ok = [i for i in range(len(blocks)) if r[i] > 0]
    dr, outs = gpu_batch.decompress(gpu, [frames[i] for i in ok], [len(blocks[i]) for i in ok])
    for k, i in enumerate(ok):
        assert int(dr[k]) == len(blocks[i]) and outs[k] == blocks[i], (labelled[i][0], labelled[i][2], int(dr[k]))


@pytest.mark.parametrize("which", ["lds", "hbm"])
def test_walk_and_groups_batch(gpu, batches, which):
    _check(gpu, *batches[which])


@pytest.mark.parametrize("phase", [0, 1], ids=["even", "odd"])
@pytest.mark.parametrize("which", ["lds", "hbm"])
def test_walk_and_groups_batch_every_second_block_limited(gpu, batches, which, phase):
    """Every second block one byte under its bound: it emits inline (and, in
    the HBM-image kernel, its flusher wave leaves at once)."""
    labelled, full, max_len = batches[which]
    caps, expected = [], []
    for i, (_, b, tt) in enumerate(labelled):
        limited = i % 2 == phase
        caps.append(ps.bound(len(b)) - (1 if limited else 0))
        expected.append(oracle_ref.compress(b, tt, caps[-1]) if limited else full[i])
    _check(gpu, labelled, expected, max_len, caps=caps)
