"""The planted inputs of tests/parse_synth.py on the GPU: every named match
length, literal run, catch-up, offset, block end and clash group through
lz4e_compress_batch_dev in guarded batches (tests/gpu_batch.py), both launch
forms, at the bound, one byte under it (limited output: the exact walk instead
of the fast chain) and at skewed placements; the capacity-sweep blocks at
every capacity from 0 to the bound.  Value, frame and iterator post-state
equal the oracle's; a refused block leaves every byte outside its slot alone.
"""
import pytest

import gpu_batch
import oracle_ref
import parse_synth as ps
from parse_synth import BYU32

pytestmark = pytest.mark.gpu

_CLS = [pytest.param(tt, id=ps.CLASS_NAME[tt]) for tt in ps.CLASSES]
PLACEMENTS = ["bound", "bound-1", "skewed"]


@pytest.fixture(scope="module")
def expected():
    """(block, class, capacity) -> the oracle's (ret, frame, final_src, last_run), computed once."""
    memo = {}

    def get(block, tt, cap):
        k = (block, tt, cap)
        if k not in memo:
            memo[k] = oracle_ref.compress(block, tt, cap)
        return memo[k]
    return get


def _run(gpu, expected, cs, placement, max_len):
    n = len(cs)
    blocks = [c.block for c in cs]
    bounds = [ps.bound(len(b)) for b in blocks]
    caps = [b - 1 for b in bounds] if placement == "bound-1" else bounds
    skew = placement == "skewed"
    r, frames, aux = gpu_batch.compress(
        gpu, blocks, [c.tt for c in cs], caps=caps, max_len=max_len,
        src_skew=[i % 16 for i in range(n)] if skew else None,
        dst_skew=[(5 * i + 3) % 16 for i in range(n)] if skew else None)
    for i, c in enumerate(cs):
        er, ef, efs, elr = expected(c.block, c.tt, caps[i])
        assert r[i] == er, (c.label, placement, int(r[i]), er)
        assert frames[i] == ef, (c.label, placement)
        if er > 0:  # a refused block's post-state is not part of the contract
            assert (aux[i][0], aux[i][1]) == (efs, elr), (c.label, placement)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("tt", _CLS)
def test_planted_lds_launch(gpu, expected, tt, placement):
    """Every case of at most 4096 bytes, staged in LDS (max_len <= 4096)."""
    cs = [c for c in ps.plain_cases(tt) if len(c.block) <= 4096]
    assert len(cs) > 100
    _run(gpu, expected, cs, placement, max(len(c.block) for c in cs))


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("tt", _CLS)
def test_planted_hbm_launch(gpu, expected, tt, placement):
    """The same cases read from HBM (max_len = 4097), and the longer ones."""
    cs = ps.plain_cases(tt)
    small = [c for c in cs if len(c.block) <= 4096]
    _run(gpu, expected, small, placement, 4097)
    large = [c for c in cs if len(c.block) > 4096]
    assert large
    _run(gpu, expected, large, placement, None)


@pytest.mark.parametrize("launch", ["lds", "hbm"])
def test_planted_every_cut(gpu, launch):
    """The three capacity-sweep blocks at every capacity from 0 to the bound,
    one block per capacity in one batch: the refused capacities are the
    oracle's, accepted frames are the oracle's, and no byte outside a slot
    changes -- a refused slot's guard bytes included (gpu_batch checks every
    gap, and a slot of capacity 0 is all gap)."""
    blocks, tts, caps, want, sizes = [], [], [], [], 0
    for c in ps.capacity_sweep():
        full = oracle_ref.compress(c.block, c.tt)
        sizes += full[0]
        for cap in range(0, ps.bound(len(c.block)) + 1):
            blocks.append(c.block)
            tts.append(c.tt)
            caps.append(cap)
            want.append(oracle_ref.compress(c.block, c.tt, cap)[:2])
            assert want[-1] == ((full[0], full[1]) if cap >= full[0] else (0, b"")), (c.label, cap)
    r, frames, _ = gpu_batch.compress(gpu, blocks, tts, caps=caps, max_len=4096 if launch == "lds" else 4097,
                                      dst_skew=[(3 * i) % 16 for i in range(len(blocks))])
    refused = {(i, caps[i]) for i in range(len(blocks)) if r[i] == 0}
    assert refused == {(i, caps[i]) for i in range(len(blocks)) if want[i][0] == 0}
    assert len(refused) == sizes  # every capacity below a block's frame size, no other
    for i in range(len(blocks)):
        assert (int(r[i]), frames[i]) == want[i], (i, caps[i])


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_planted_dictionary(gpu, placement):
    """The dict family through lz4e_compress_batch_dev_dict."""
    cs = list(ps.cases("dict", BYU32))
    n = len(cs)
    bounds = [ps.bound(len(c.block)) for c in cs]
    caps = [b - 1 for b in bounds] if placement == "bound-1" else bounds
    skew = placement == "skewed"
    r, frames, _ = gpu_batch.compress(
        gpu, [c.block for c in cs], [BYU32] * n, caps=caps, dicts=[c.dic for c in cs],
        src_skew=[(i + 1) % 16 for i in range(n)] if skew else None,
        dst_skew=[(5 * i + 3) % 16 for i in range(n)] if skew else None)
    for i, c in enumerate(cs):
        er, ef = oracle_ref.compress_dict(c.block, c.dic, caps[i])
        assert (int(r[i]), frames[i]) == (er, ef), (c.label, placement)
        assert oracle_ref.decompress_dict(ef, len(c.block), c.dic) == (len(c.block), c.block)
