"""The planted inputs of tests/parse_synth.py against the oracle (CPU).

The oracle's frame is the proof that a plan was planted right: every named
value of every ladder must show in the frame the oracle emits for its case
(literal length, match length, offset), in the trace of the parse (catch-up
length and what stopped it, refused candidates) or in the iterator post-state
of the exit into last_literals.  The trace is parse_synth's own restatement
of the parse; it counts only because its frame equals the oracle's.
"""
import numpy as np
import pytest

import oracle_ref
import parse_synth as ps
from parse_synth import BYU16, BYU32


def _oracle(c, cap=None):
    """-> (ret, frame, aux or None)"""
    if c.dic:
        r, f = oracle_ref.compress_dict(c.block, c.dic, cap)
        return r, f, None
    r, f, fs, lr = oracle_ref.compress(c.block, c.tt, cap)
    return r, f, (fs, lr)


def _all_cases():
    out = [(f, tt, c) for tt in ps.CLASSES for f in sorted(ps.PLAIN_FAMILIES) for c in ps.cases(f, tt)]
    return out + [("dict", BYU32, c) for c in ps.cases("dict", BYU32)]


def check_case(c, frame, aux):
    """The case's checks against a frame (the oracle's) -> the (ladder, value)
    pairs it showed."""
    t = ps.trace(c.block, c.tt, c.dic)
    assert t.frame == frame, f"{c.label}: the trace's frame is not the oracle's"
    if aux is not None:
        assert (t.final_src, t.last_run) == aux, c.label
    seqs, last = ps.parse_frame(frame)
    assert seqs == t.seqs and last == t.last_run, c.label
    by_start = {s[0]: e for s, e in zip(t.seqs, t.events)}
    shown = set()
    for ladder, value, kind, data in c.checks:
        where = f"{c.label}: {ladder} {value}"
        if kind == "seq":
            assert tuple(data) in seqs, f"{where}: sequence {data} not in the frame: {seqs[:8]}"
            name = {"mlen": 3, "lit": 1, "offset": 2, "clash_len": 3, "clash_spacing": 2}
            for k, i in name.items():
                if ladder == k or (k == "mlen" and ladder.startswith("mlen")):
                    assert data[i] == value, where
            if ladder == "mlen_rematch":
                assert data[1] == 0 and by_start[data[0]][0] == "rematch", where
            if ladder == "mlen_search":
                assert 1 <= data[1] <= 14 and by_start[data[0]][0] == "search", where
        elif kind == "event":
            start, probe, cu, stop = data
            ev = by_start.get(start)
            assert ev is not None, f"{where}: no sequence starts at {start}"
            assert ev[0] == "search" and ev[1] == probe and ev[3] == cu, f"{where}: {ev}"
            assert stop in ev[4].split("+"), f"{where}: stopped by {ev[4]}"
            if ladder.startswith("catch_up"):
                assert cu == value
        elif kind == "refuse":
            assert tuple(data) in t.refused, f"{where}: {t.refused[:6]}"
            assert all(not (s[0] <= data[0] < s[0] + s[3]) for s in seqs), where
        elif kind == "exit":
            k, probes, fs, lr = data
            assert (t.exit, t.probes, t.final_src, t.last_run) == (k, probes, fs, lr), \
                f"{where}: {(t.exit, t.probes, t.final_src, t.last_run)}"
            if aux is not None:
                assert aux == (fs, lr), where
        elif kind == "len":
            assert len(c.block) == data == value
        elif kind == "nomatch":
            P, _ = data
            w = ps.hash_width(c.tt)
            assert all(not (s[0] <= P + w - 1 and P < s[0] + s[3]) for s in seqs), f"{where}: a match at {P}"
        else:
            raise AssertionError(kind)
        shown.add((ladder, value))
    return shown


@pytest.fixture(scope="module")
def shown():
    """(class, ladder, value) triples shown by the oracle's frames, all cases."""
    got = set()
    for fam, tt, c in _all_cases():
        r, f, aux = _oracle(c)
        assert r == len(f) > 0, c.label
        if c.dic:
            assert oracle_ref.decompress_dict(f, len(c.block), c.dic) == (len(c.block), c.block), c.label
        else:
            assert oracle_ref.decompress(f, len(c.block)) == (len(c.block), c.block), c.label
        got |= {(tt, l, v) for l, v in check_case(c, f, aux)}
    return got


def test_oracle_round_trip_and_plans(shown):
    """Every case decodes back through the oracle and shows what it planned."""
    assert shown


@pytest.mark.parametrize("tt", ps.CLASSES, ids=[ps.CLASS_NAME[t] for t in ps.CLASSES])
def test_every_ladder_value_is_shown(shown, tt):
    missing = [(l, v) for l, vals in ps.LADDERS[tt].items() for v in vals if (tt, l, v) not in shown]
    assert not missing, missing


def test_ladders_drop_only_what_cannot_be_forced():
    """The issue's ladders, minus what parse_synth._ladders gives a reason for."""
    for tt in ps.CLASSES:
        L = ps.LADDERS[tt]
        assert set(ps.MATCH_LENGTHS) - set(L["mlen_search"]) == ({4} if tt == BYU32 else set())
        assert L["lit"] == ps.LITERAL_RUNS and L["block_len"] == list(range(13, 31))
        assert set(ps.OFFSETS) - set(L["offset"]) == ({65534, 65535} if tt == BYU16 else set())
        for stop in ("byte", "anchor", "zero"):
            assert L["catch_up_" + stop] == ps.CATCH_UPS[stop == "anchor":]
    assert set(ps.MATCH_LENGTHS) - set(ps.LADDERS[BYU16]["mlen_at_limit"]) == {4, 5}


def test_blocks_stay_small():
    big = [(c.label, len(c.block)) for _, _, c in _all_cases() if len(c.block) > 4200]
    assert all(l == "offset-far" for l, _ in big), big


@pytest.mark.parametrize("tt", ps.CLASSES, ids=[ps.CLASS_NAME[t] for t in ps.CLASSES])
def test_collision_groups_are_the_oracles(tt):
    """The members of a group hash alike and differ in bytes, and the oracle
    agrees: with one member replaced by bytes of another hash, the evicted
    copy is found again -- the parse changes."""
    (c,) = [c for c in ps.cases("clashes", tt) if c.groups]
    w = ps.hash_width(tt)
    base = [s[1:] for s in ps.parse_frame(_oracle(c)[1])[0]]
    assert len(c.groups) >= 7
    for pos, rp, repl in c.groups:
        mem = [c.block[p:p + w] for p in pos]
        assert len(set(mem)) == len(mem), "members differ in bytes"
        assert len({ps.hash_value(m, tt) for m in mem}) == 1, "members share a hash"
        assert ps.hash_value(repl, tt) != ps.hash_value(mem[0], tt)
        blk = bytearray(c.block)
        blk[rp:rp + w] = repl
        other = [s[1:] for s in ps.parse_frame(oracle_ref.compress(bytes(blk), tt)[1])[0]]
        assert len(other) == len(base) + 1, (pos, len(base), len(other))


def test_hashes_restate_the_oracles_on_random_blocks():
    """trace() == the oracle on blocks it was not built for."""
    rng = np.random.default_rng(99)
    for i in range(30):
        n = int(rng.integers(0, 3000))
        a = int(rng.choice([2, 4, 16, 256]))
        blk = rng.integers(0, a, n, dtype=np.uint8).tobytes()
        for tt in ps.CLASSES:
            r, f, fs, lr = oracle_ref.compress(blk, tt)
            t = ps.trace(blk, tt)
            assert (t.ret, t.frame, t.final_src, t.last_run) == (r, f, fs, lr), (i, tt)
    dic = rng.integers(0, 4, 5000, dtype=np.uint8).tobytes()
    blk = rng.integers(0, 4, 3000, dtype=np.uint8).tobytes()
    assert ps.trace(blk, BYU32, dic).frame == oracle_ref.compress_dict(blk, dic)[1]


def test_limited_output_cut_points():
    """The capacity-sweep blocks at every capacity from 0 to the bound: the
    oracle accepts exactly the capacities from the frame's size on, and the
    refusals come from at least 10 distinct points of the parse (the check
    that refuses: each sequence's literal check, its match check, the last
    literals)."""
    for c in ps.capacity_sweep():
        n = len(c.block)
        assert 300 <= n <= 700, (c.label, n)
        full = oracle_ref.compress(c.block, c.tt)
        for cap in range(0, ps.bound(n) + 1):
            r, f, _, _ = oracle_ref.compress(c.block, c.tt, cap)
            assert (r, f) == ((full[0], full[1]) if cap >= full[0] else (0, b"")), (c.label, cap)
    # where each refusal happens: the limited parse's checks, restated
    total = set()
    for c in ps.capacity_sweep():
        seqs, last = ps.parse_frame(oracle_ref.compress(c.block, c.tt)[1])
        full = oracle_ref.compress(c.block, c.tt)[0]
        cuts = set()
        for cap in range(0, full):
            op = 0
            where = None
            for i, (_, L, _, m) in enumerate(seqs):
                op += 1
                if op + L + 8 + L // 255 > cap:
                    where = (i, "literals")
                    break
                op += (L - 15) // 255 + 1 if L >= 15 else 0
                op += L + 2
                mc = m - 4
                if op + 6 + (mc >> 8) > cap:
                    where = (i, "match")
                    break
                op += (mc - 15) // 255 + 1 if mc >= 15 else 0
            if where is None:
                assert op + last + 1 + (last + 240) // 255 > cap, (c.label, cap)
                where = (len(seqs), "last")
            cuts.add(where)
        assert len(cuts) >= (10 if len(seqs) >= 10 else 2 * len(seqs)), (c.label, sorted(cuts))
        total |= {(c.label,) + w for w in cuts}
    assert len(total) >= 10
