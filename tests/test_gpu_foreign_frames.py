"""Frames no LZ4E encoder emits (tests/frame_synth.py) through every decoder.

include/lz4e.h promises that frames of any LZ4 compressor decode; every other
GPU test feeds the decoders the reference's greedy parse or random damage to
it.  Each profile's frames go in one batch per decoder mode through the
guarded helper (tests/gpu_batch.py) at rotating source and destination
residues; values and bytes equal the oracle's, which tests/test_frame_synth.py
checks against the synthesizer's own LZ model.
"""
import functools

import numpy as np
import pytest

import frame_synth
import gpu_batch
import oracle_ref
from gpu_batch import DEC_AUTO, DEC_NAMES, DEC_PIPE, DEC_WAVE, FORCED_MODES
from lz4e_amd import make_sg

pytestmark = pytest.mark.gpu

ALL_MODES = FORCED_MODES + [DEC_AUTO]
LARGE_MODES = [DEC_WAVE, DEC_PIPE, DEC_AUTO]
_ids = lambda modes: [DEC_NAMES[m] for m in modes]


@functools.lru_cache(maxsize=None)
def _cases(profile, large):
    cs = frame_synth.cases(profile, large=large)
    want = [oracle_ref.decompress_dict(c.frame, c.cap, c.dic) for c in cs]
    for c, (r, out) in zip(cs, want):
        assert (r >= 0) == c.must_accept or profile == "ends", c.label
        assert c.want_ret is None or r == c.want_ret, c.label
    return cs, want


def _run(gpu, profile, mode, large):
    cs, want = _cases(profile, large)
    i = np.arange(len(cs))
    ss, ds = i % 16, (5 * i + 3) % 16
    dicts = [c.dic for c in cs] if profile == "dict" else None
    r, outs = gpu_batch.decompress(gpu, [c.frame for c in cs], [c.cap for c in cs], mode=mode,
                                   src_skew=ss, dst_skew=ds, dicts=dicts)
    for k, (c, (er, eb)) in enumerate(zip(cs, want)):
        where = (DEC_NAMES[mode], c.label, f"src {ss[k]} dst {ds[k]} mod 16", r[k], er)
        assert r[k] == er, where
        if er >= 0:
            assert outs[k] == eb, where


@pytest.mark.parametrize("mode", ALL_MODES, ids=_ids(ALL_MODES))
@pytest.mark.parametrize("profile", sorted(frame_synth.PROFILES))
def test_synthesized_frames(gpu, profile, mode):
    """Outputs of <= 4608 bytes on every decoder.  The forced LDS form
    (`small`) never takes a block that has a dictionary: `dict-small` decodes
    on the one-wave HBM form, like `dict-wave`."""
    _run(gpu, profile, mode, False)


@pytest.mark.parametrize("mode", LARGE_MODES, ids=_ids(LARGE_MODES))
@pytest.mark.parametrize("profile", ["boundary", "chains", "far", "dict"])
def test_synthesized_frames_large(gpu, profile, mode):
    """Outputs of about 20000 and 65536 bytes: sources many batches back, on
    the one-wave and pipelined decoders."""
    _run(gpu, profile, mode, True)


def test_synthesized_frames_single_calls(gpu):
    """A dozen of them through LZ4E_decompress_safe and
    lz4e_decompress_safe_sg."""
    picked = []
    for profile in ("boundary", "chains", "far", "ends", "invalid"):
        cs, want = _cases(profile, False)
        step = max(1, len(cs) // 3)
        picked += list(zip(cs, want))[::step][:3]
    assert len(picked) >= 12
    for c, (er, eb) in picked:
        ret, out = gpu.decompress_safe(c.frame, c.cap)
        assert ret == er, (c.label, ret, er)
        if er >= 0:
            assert out[:er] == eb, c.label
        d = make_sg(b"", [512] * (-(-c.cap // 512) or 1), capacity=c.cap, shuffle_seed=5)
        assert gpu.decompress_safe_sg(c.frame, d) == er, c.label
        if er >= 0:
            assert d.read_prefix(er) == eb, c.label
