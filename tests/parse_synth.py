"""Planted inputs for the compressor -- TEST INFRASTRUCTURE ONLY.

frame_synth.py builds frames from a grammar so that every decoder rule is
named and forced; this module does the same for the encoder's parse.  A block
is built from a plan -- literal runs and copies of earlier bytes with a guard
byte on each side -- so that the greedy parse of oracle/lz4e_core.inc emits
exactly the planned (literals, offset, match length) sequence at a planned
position.  The plan respects the search's lattice: only probed positions are
in the table (the first 66 positions of a search, then every second, third ...
position; of a match only its end - 2 and its end), so a copy's source lies
where the table has it, and a position is taken out of the table again with an
"evictor": other bytes with the same hash at a later probed position.

  * parse_frame(frame)        frame -> [(match start, L, offset, mlen)], last literals
  * hash_at / hash_value      the three table hashes (oracle/lz4e_core.inc)
  * trace(block, tt, dic)     lz4e_core.inc restated in Python; besides the
                              frame it records, per sequence, the probe that
                              hit and the catch-up, the refused candidates and
                              the exit into last_literals
  * FAMILIES / cases(name)    the planted cases; LADDERS the values each
                              family must show per table class

Each case carries checks (ladder, value, kind, data) that the oracle's frame
and the trace must satisfy (tests/test_parse_synth.py); the oracle's frame is
the proof that a plan was planted right.  Seeded and deterministic.
"""
import collections
import functools

import numpy as np

BYU16, BYU32, BYU64 = 1, 3, 7
CLASSES = (BYU16, BYU32, BYU64)
CLASS_NAME = {BYU16: "byU16", BYU32: "byU32", BYU64: "byU64"}
MAX_DISTANCE = 65535
MFLIMIT, LASTLITERALS, MINLENGTH = 12, 5, 13
_M32, _M64 = (1 << 32) - 1, (1 << 64) - 1


def bound(n):
    return n + n // 255 + 16


# ---------------------------------------------------------------------------
# hashes (oracle/lz4e_oracle.c o_hash4 / o_hash5, HASHAT)
# ---------------------------------------------------------------------------

def hash_log(tt):
    return 11 if tt == BYU64 else 12 if tt == BYU32 else 13


def hash_width(tt):
    """Bytes of the input a table index depends on."""
    return 5 if tt == BYU32 else 4


def hash_value(b, tt):
    """Table index of the position whose first bytes are b (>= hash_width)."""
    if tt == BYU32:
        v = int.from_bytes(bytes(b[:5]), "little")
        return (((v << 24) & _M64) * 889523592379 & _M64) >> (64 - 12)
    v = int.from_bytes(bytes(b[:4]), "little")
    return ((v * 2654435761) & _M32) >> (32 - hash_log(tt))


def hash_at(buf, p, tt):
    return hash_value(buf[p:p + 8], tt)


@functools.lru_cache(maxsize=None)
def _evictors(tt):
    """slot -> a few distinct byte strings (hash_width long) with that hash,
    found by brute force over seeded random values."""
    rng = np.random.default_rng(977 + tt)
    w = hash_width(tt)
    raw = rng.integers(0, 256, (600000 if tt != BYU64 else 200000, w), dtype=np.uint8)
    v = np.zeros(len(raw), dtype=np.uint64)
    for i in range(w):
        v |= raw[:, i].astype(np.uint64) << np.uint64(8 * i)
    if tt == BYU32:
        h = ((v << np.uint64(24)) * np.uint64(889523592379)) >> np.uint64(52)
    else:
        h = ((v * np.uint64(2654435761)) & np.uint64(_M32)) >> np.uint64(32 - hash_log(tt))
    out = collections.defaultdict(list)
    for i, s in enumerate(h.tolist()):
        if len(out[s]) < 4:
            out[s].append(raw[i].tobytes())
    return out


def colliders(b, tt, k=1):
    """k byte strings that differ from b[:hash_width] and hash like it."""
    w = hash_width(tt)
    got = [x for x in _evictors(tt)[hash_value(b, tt)] if x != bytes(b[:w])][:k]
    assert len(got) == k, "no collider found"
    return got


def non_collider(b, tt, salt=0):
    w = hash_width(tt)
    x = bytearray(b[:w])
    for d in range(1, 256):
        x[0] = (b[0] + d + salt) & 0xFF
        if hash_value(x, tt) != hash_value(b, tt):
            return bytes(x)
    raise AssertionError


# ---------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------

def parse_frame(frame):
    """-> ([(start, L, offset, mlen)], last_literals): start is the block
    position at which the match begins."""
    f = bytes(frame)
    i, pos, seqs = 0, 0, []
    while True:
        tok = f[i]
        i += 1
        L = tok >> 4
        if L == 15:
            while True:
                x = f[i]
                i += 1
                L += x
                if x != 255:
                    break
        i += L
        pos += L
        if i == len(f):
            assert tok & 15 == 0
            return seqs, L
        off = f[i] | (f[i + 1] << 8)
        i += 2
        m = tok & 15
        if m == 15:
            while True:
                x = f[i]
                i += 1
                m += x
                if x != 255:
                    break
        m += 4
        seqs.append((pos, L, off, m))
        pos += m


def probe_lattice(s, limit):
    """Positions a search starting at s probes while it misses, up to limit."""
    q, step, nb = s, 1, 64
    while q <= limit:
        yield q
        q += step
        step = nb >> 6
        nb += 1


Trace = collections.namedtuple("Trace", "ret frame final_src last_run seqs events refused exit probes")
# events[i] for seqs[i]: (kind 'search'|'rematch', probe position, probe number, catch-up, stop)
# stop: what ended the catch-up: 'byte', 'anchor', 'zero' (joined by + when several hold)
# exit: 'match_end' | 'search_start' | 'search_stop' | 'short'; probes: probes of the last search that ran


def trace(block, tt, dic=b""):
    """oracle/lz4e_core.inc in Python (unlimited output), positions relative
    to the block."""
    dic = bytes(dic)[-65536:]
    s = dic + bytes(block)
    start, n = len(dic), len(block)
    out = bytearray()
    anchor = ip = start
    seqs, events, refused = [], [], []
    exit_kind, probes = "short", 0
    table = {}
    H = lambda p: hash_at(s, p, tt)
    if n >= MINLENGTH:
        mflimit, matchlimit = start + n - MFLIMIT, start + n - LASTLITERALS
        p = 0
        while start and p + 8 <= start:
            table[H(p)] = p
            p += 3
        table[H(start)] = start
        ip = start + 1
        while True:
            q, step, nb, pn = ip, 1, 64, 0
            found = False
            while True:
                if q + step > mflimit:
                    exit_kind, probes = ("search_stop" if pn else "search_start"), pn
                    break
                ip = q
                h = H(q)
                cand = table.get(h, 0)
                table[h] = ip
                q += step
                step = nb >> 6
                nb += 1
                pn += 1
                if s[cand:cand + 4] == s[ip:ip + 4]:
                    if tt == BYU16 or cand + MAX_DISTANCE >= ip:
                        found = True
                        break
                    refused.append((ip - start, ip - cand))
            if not found:
                break
            hit, cu = ip, 0
            while ip > anchor and cand > 0 and s[ip - 1] == s[cand - 1]:
                ip -= 1
                cand -= 1
                cu += 1
            stop = [k for k, c in (("anchor", ip == anchor), ("zero", cand == 0)) if c]
            if ip > anchor and cand > 0:
                stop.append("byte")
            kind, L = "search", ip - anchor
            tok = len(out)
            out.append(0)
            token = min(L, 15) << 4
            if L >= 15:
                r = L - 15
                out += b"\xff" * (r // 255) + bytes([r % 255])
            out += s[anchor:ip]
            while True:
                mstart = ip
                out += bytes([(ip - cand) & 255, (ip - cand) >> 8])
                ip += 4
                cand += 4
                mc = 0
                while ip + mc < matchlimit and s[ip + mc] == s[cand + mc]:
                    mc += 1
                ip += mc
                if mc >= 15:
                    r = mc - 15
                    out += b"\xff" * (r // 255) + bytes([r % 255])
                out[tok] = token + min(mc, 15)
                seqs.append((mstart - start, L, mstart - (cand - 4), mc + 4))
                events.append((kind, hit - start, pn - 1, cu, "+".join(stop)) if kind == "search"
                              else ("rematch", mstart - start, 0, 0, ""))
                anchor = ip
                if ip > mflimit:
                    break
                table[H(ip - 2)] = ip - 2
                h = H(ip)
                cand = table.get(h, 0)
                table[h] = ip
                if cand + MAX_DISTANCE >= ip and s[cand:cand + 4] == s[ip:ip + 4]:
                    kind, L, token = "rematch", 0, 0
                    tok = len(out)
                    out.append(0)
                    continue
                break
            if ip > mflimit:
                exit_kind, probes = "match_end", 0
                break
            ip += 1
    R = start + n - anchor
    if R >= 15:
        r = R - 15
        out += b"\xf0" + b"\xff" * (r // 255) + bytes([r % 255])
    else:
        out.append(R << 4)
    out += s[anchor:]
    return Trace(len(out), bytes(out), ip - start, R, seqs, events, refused, exit_kind, probes)


# ---------------------------------------------------------------------------
# the builder
# ---------------------------------------------------------------------------

Case = collections.namedtuple("Case", "label block tt dic checks groups")
# checks: [(ladder, value, kind, data)]:
#   kind 'seq'    data (start, L, offset, mlen): that sequence is in the oracle's frame
#   kind 'event'  data (start, probe, catch-up, stop): the sequence starting there was hit at `probe`
#   kind 'refuse' data (position, distance): the candidate at that distance was refused there
#   kind 'exit'   data (exit kind, probes, final_src, last_run)
#   kind 'len'    data n: the block's length
# groups: collision groups [(positions, replace position, replacement bytes)]


class _B:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.b = bytearray()
        self.L = 0          # literals since the last match
        self.cont = None    # the byte that would prolong the last match

    def lit(self, n=None, data=None):
        r = bytearray(self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()) if data is None else bytearray(data)
        if r and self.cont is not None:
            if r[0] == self.cont:
                assert data is None
                r[0] ^= 0x55
            self.cont = None
        self.b += r
        self.L += len(r)
        return len(self.b) - len(r)

    def match(self, src, m, guard_back=True):
        """Copy m bytes from position src; -> (start, L, offset, m) as planned."""
        P = len(self.b)
        assert 0 <= src < P
        if guard_back and src > 0 and self.L > 0 and self.b[P - 1] == self.b[src - 1]:
            self.b[P - 1] ^= 0x2A
        for i in range(m):
            self.b.append(self.b[src + i])
        self.cont = self.b[src + m]
        plan = (P, self.L, P - src, m)
        self.L = 0
        return plan

    def tail(self, n=MFLIMIT + 1):
        self.lit(n)
        return bytes(self.b)


def _case(label, b, tt, checks, dic=b"", groups=()):
    return Case(label, bytes(b), tt, bytes(dic), list(checks), list(groups))


# ---------------------------------------------------------------------------
# ladders: what every family must show, per table class
# ---------------------------------------------------------------------------

MATCH_LENGTHS = [4, 5, 18, 19, 20, 31, 32, 33, 35, 36, 272, 273, 274, 275, 283, 284, 285, 528, 529, 530, 536, 537,
                 2000]
LITERAL_RUNS = [0, 1, 14, 15, 16, 60, 63, 64, 65, 269, 270, 271, 524, 525, 526, 1023, 1024, 1025, 2047, 2048, 2049,
                2100]
CATCH_UPS = [0, 1, 3, 4, 5, 63, 64, 65, 130]
OFFSETS = [1, 2, 3, 4, 5, 8, 62, 63, 64, 65, 66, 4096, 65534, 65535]
BLOCK_LENGTHS = list(range(13, 31))
END_PROBES = list(range(0, 71)) + list(range(100, 171))
CLASH_SPACINGS = [1, 2, 3, 7, 16, 31, 32, 33, 62, 63]
CLASH_LENGTHS = [4, 5, 8, 16, 31, 32, 33, 40]


def _ladders(tt):
    u32 = tt == BYU32
    # byU32 hashes 5 bytes: a probe finds a 4-byte match only by a hash collision
    ml = [m for m in MATCH_LENGTHS if not (u32 and m == 4)]
    # a match starts at most at mflimit - 1 (search) or mflimit (rematch): one that ends at
    # matchlimit, or a byte short of it, is at least 7 bytes long
    ml_end = [m for m in MATCH_LENGTHS if m >= 18]
    d = {
        "mlen_search": ml, "mlen_rematch": ml,
        "lit": LITERAL_RUNS,
        "offset": [o for o in OFFSETS if o <= 4096 or tt != BYU16],  # a byU16 block has at most 65536 bytes
        "block_len": BLOCK_LENGTHS,
        "end_probes": END_PROBES if tt == BYU16 else END_PROBES[:71],
        "exit": ["match_end", "search_start", "search_stop"],
        "clash_spacing": CLASH_SPACINGS,
        "clash_len": [m for m in CLASH_LENGTHS if not (u32 and m == 4)],
        "clash_group": ["pair", "triple", "split"],
    }
    for stop in ("byte", "anchor", "zero"):
        d["catch_up_" + stop] = CATCH_UPS
    # a hit at the anchor itself is the rematch (mlen_rematch), not a search with a catch-up of 0
    d["catch_up_anchor"] = CATCH_UPS[1:]
    if tt != BYU64:  # the end rules do not depend on the table; byU64 leaves them to the other two
        d["mlen_at_limit"] = ml_end
        d["mlen_short"] = ml_end
    if tt != BYU16:  # byU16 has no distance check (its blocks are shorter than the window)
        d["far"] = [65536, 65537]
    if u32:
        d["dict"] = ["inside", "crossing", "start", "anchor", "65535", "65536"]
    return d


LADDERS = {tt: _ladders(tt) for tt in CLASSES}


# ---------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------

def _split(values, budget=3400):
    """Groups of values whose sum stays under a block's byte budget."""
    groups, cur, tot = [], [], 0
    for v in values:
        if cur and tot + v + 20 > budget:
            groups.append(cur)
            cur, tot = [], 0
        cur.append(v)
        tot += v + 20
    if cur:
        groups.append(cur)
    return groups


def match_lengths(tt):
    out = []
    L = LADDERS[tt]
    # search hits: k literals, then the k-periodic continuation of the run that starts at the anchor
    for gi, grp in enumerate(_split(L["mlen_search"])):
        b, checks = _B(1000 + gi), []
        b.lit(20)
        b.match(1, 8)
        for i, m in enumerate(grp):
            k = 1 + (i * 5 + gi) % 14
            if m == 4 and k < 2:
                k = 2
            U = b.lit(k)
            checks.append(("mlen_search", m, "seq", b.match(U, m)))
        out.append(_case(f"mlen-search-{gi}", b.tail(), tt, checks))
    # rematches: a match that starts where the previous one ended, copied from a probed literal
    for gi, grp in enumerate(_split(L["mlen_rematch"])):
        b, checks = _B(1100 + gi), []
        b.lit(20)
        for i, m in enumerate(grp):
            k = 6 + (i * 3 + gi) % 7
            U = b.lit(k)
            b.match(U, 6)
            if b.b[U + 1] == b.cont:
                b.b[U + 1] ^= 0x11
                b.b[U + k + 1] ^= 0x11
            checks.append(("mlen_rematch", m, "seq", b.match(U + 1, m, guard_back=False)))
        out.append(_case(f"mlen-rematch-{gi}", b.tail(), tt, checks))
    # matches cut by matchlimit (the bytes go on being equal) and ending a byte short of it
    for name in ("mlen_at_limit", "mlen_short"):
        for m in L.get(name, []):
            b = _B(1200 + m)
            k = 3 + m % 9
            U = b.lit(k)
            if name == "mlen_at_limit":
                plan = b.match(U, m)
                b.match(len(b.b) - k, LASTLITERALS)
                blk = bytes(b.b)
                lr = LASTLITERALS
            else:
                plan = b.match(U, m)
                blk = b.tail(LASTLITERALS + 1)
                lr = LASTLITERALS + 1
            out.append(_case(f"{name.replace('_', '-')}-{m}", blk, tt,
                             [(name, m, "seq", plan), (name, m, "exit", ("match_end", 0, plan[0] + m, lr))]))
    return out


def literal_runs(tt):
    """[24 literals | 8-byte match | L literals | 13-byte copy of the head |
    tail]: past 66 literals the probe that hits lies inside the copy and the
    catch-up restores its start."""
    def make(L, seed):
        b = _B(seed)
        b.lit(24)
        b.match(1, 8)
        b.lit(L)
        if L == 0 and b.b[10] == b.cont:
            return None
        plan = b.match(10, 13, guard_back=L > 0)
        return _case(f"lit-{L}", b.tail(), tt, [("lit", L, "seq", plan)])
    return [_planted(lambda seed, L=L: make(L, seed), 2000 + L) for L in LADDERS[tt]["lit"]]


def _planted(make, seed):
    """make(seed) for the first seed (seed, seed + 1000, ...) whose trace shows
    every planned sequence: among a thousand random probes one may by chance
    share a hash with a planted position and take it out of the table."""
    for sd in range(seed, seed + 64000, 1000):
        case = make(sd)
        if case is None:
            continue
        t = trace(case.block, case.tt, case.dic)
        if all(k != "seq" or tuple(d) in t.seqs for _, _, k, d in case.checks) and \
                all(k != "event" or (tuple(d[:1]) + t.events[[x[0] for x in t.seqs].index(d[0])][1:4:2] == d[:3]
                                     if d[0] in [x[0] for x in t.seqs] else False) for _, _, k, d in case.checks):
            return case
    raise AssertionError("no seed plants " + case.label)


def catch_up(tt):
    """The copy's first c source positions are taken out of the table by
    evictors, so the probe at its position + c is the first to hit and the
    catch-up walks c bytes back: to a differing byte, to the anchor, or until
    the candidate reaches position 0."""
    out = []
    for stop in ("byte", "anchor", "zero"):
        for c in LADDERS[tt]["catch_up_" + stop]:
            out.append(_planted(lambda seed: _catch_up_case(tt, stop, c, seed), 3000 + c + 7 * len(stop)))
    return out


def _catch_up_case(tt, stop, c, seed):
    lat = set(probe_lattice(1, 400))
    H = 0 if stop == "zero" else next(h for h in range(8, 20) if h + c in lat)
    b = _B(seed)
    b.lit(H)
    S = b.lit(c + 12)
    # a short match resets the search, so that every evictor is probed
    r0 = next(q for q in range(S + c + 1, S + c + 6) if q in lat)
    reset = lambda: (b.lit(2), b.match(r0, 6))
    b.lit(next(k for k in (2, 3, 4) if len(b.b) + k in lat))  # the first reset starts at a probed position
    b.match(r0, 6)
    ev = [colliders(b.b[S + j:S + j + 8], tt)[0] for j in range(c)]
    for i in range(0, c, 10):
        b.lit(1)
        b.lit(data=b"".join(e + bytes([b.rng.integers(0, 256)]) for e in ev[i:i + 10]))
        reset()
    if stop == "anchor":
        if b.b[S] == b.cont:
            return None
    else:
        lat_e = set(x - 1 for x in lat)  # offsets from the search's start
        b.lit(next(x for x in range(1, 8) if x + c - 1 in lat_e))
        if stop == "byte" and S > 0 and b.b[-1] == b.b[S - 1]:
            b.b[-1] ^= 0x2A
    plan = b.match(S, c + 12, guard_back=False)
    P = plan[0]
    return _case(f"catch-up-{stop}-{c}", b.tail(), tt,
                 [("catch_up_" + stop, c, "seq", plan), ("catch_up_" + stop, c, "event", (P, P + c, c, stop))])


def offsets(tt):
    out = []
    L = LADDERS[tt]["offset"]
    b, checks = _B(4000), []
    b.lit(20)
    b.match(1, 8)
    for d in [o for o in L if o <= 8]:
        U = b.lit(d)
        checks.append(("offset", d, "seq", b.match(U, 9)))
    out.append(_case("offset-near", b.tail(), tt, checks))
    # [20-byte zone | filler: one long periodic match | 3 literals | copy from the zone]
    for d in [o for o in L if 8 < o <= 4096]:
        b = _B(4000 + d)
        b.lit(6)
        U = b.lit(20)
        F = b.lit(4)
        b.match(F, d - 22)
        b.lit(3)
        plan = b.match(U + 5, 10)
        assert plan[2] == d
        out.append(_case(f"offset-{d}", b.tail(), tt, [("offset", d, "seq", plan)]))
    if tt != BYU16:
        # four copies at distances 65537, 65536 (refused: the bytes stay literals), 65535 and 65534
        b = _B(4100)
        b.lit(6)
        U = b.lit(64)
        F = b.lit(4)
        P1 = U + 4 + 65537
        b.match(F, P1 - 3 - len(b.b))
        checks = []
        for i, d in enumerate((65537, 65536, 65535, 65534)):
            b.lit(3)
            P = len(b.b)
            if d > MAX_DISTANCE:
                b.lit(data=bytes(b.b[P - d:P - d + 10]))
                checks.append(("far", d, "refuse", (P, d)))
            else:
                plan = b.match(P - d, 10)
                checks.append(("offset", d, "seq", plan))
        out.append(_case("offset-far", b.tail(), tt, checks))
    return out


def block_ends(tt):
    out = []
    for n in LADDERS[tt]["block_len"]:
        rng = np.random.default_rng(5000 + n)
        out.append(_case(f"end-len-{n}-random", rng.integers(0, 256, n, dtype=np.uint8).tobytes(), tt,
                         [("block_len", n, "len", n)]))
        out.append(_case(f"end-len-{n}-run", bytes([n]) * n, tt, [("block_len", n, "len", n)]))
        out.append(_case(f"end-len-{n}-period3", (bytes([1, 2, n]) * n)[:n], tt, [("block_len", n, "len", n)]))
    # [8 literals | 8-byte match | T random bytes]: the search after the match runs p probes and
    # stops at mflimit; p = 0 is the search whose first probe cannot run
    for p in LADDERS[tt]["end_probes"]:
        b = _B(5100 + p)
        U = b.lit(8)
        plan = b.match(U, 8)
        e = plan[0] + 8
        # the rematch at e misses, the search starts at e + 1; probe q runs iff q + step <= mflimit
        lat = list(probe_lattice(e + 1, e + 2000))
        mflimit = lat[p] if p else e
        n = mflimit + MFLIMIT
        blk = b.tail(n - len(b.b))
        ip = lat[p - 1] if p else e + 1
        kind = "search_stop" if p else "search_start"
        out.append(_case(f"end-probes-{p}", blk, tt,
                         [("end_probes", p, "exit", (kind, p, ip, n - e)), ("exit", kind, "exit", (kind, p, ip, n - e))]))
    # a rematch of 40 bytes (past the 32 held in registers) that ends past mflimit
    b = _B(5200)
    U = b.lit(9)
    b.match(U, 6)
    if b.b[U + 1] == b.cont:
        b.b[U + 1] ^= 0x11
        b.b[U + 10] ^= 0x11
    plan = b.match(U + 1, 40, guard_back=False)
    blk = b.tail(7)
    out.append(_case("end-rematch-past-mflimit", blk, tt,
                     [("exit", "match_end", "seq", plan), ("exit", "match_end", "exit", ("match_end", 0, plan[0] + 40, 7))]))
    # a search that misses for 120 probes (the skip-step search by then) and hits a match that
    # runs to matchlimit
    b = _B(5300)
    b.lit(24)
    b.match(1, 8)
    b.lit(120)
    plan = b.match(10, 13)
    b.match(10 + 13, LASTLITERALS)
    out.append(_case("end-late-hit-past-mflimit", bytes(b.b), tt,
                     [("exit", "match_end", "seq", plan),
                      ("exit", "match_end", "exit", ("match_end", 0, plan[0] + 13, LASTLITERALS))]))
    return out


def _collide_case(tt, seed):
    # different bytes with equal hashes: X is put, then evicted by Y; a later copy of X of just
    # hash_width bytes finds nothing (with Y replaced by other bytes it is a match)
    w = hash_width(tt)
    b, checks, groups, copies = _B(seed), [], [], []
    b.lit(10)
    reset = lambda: (b.lit(2), b.match(1, 6))
    for zone in range(3):
        reset()
        for g in range(3):
            kind = ("pair", "triple", "pair")[g] if zone < 2 else "pair"
            X = bytes(b.rng.integers(0, 256, w, dtype=np.uint8).tobytes())
            ys = colliders(X, tt, 2)
            pos = []
            if kind == "triple":
                b.lit(1)
                pos.append(b.lit(data=ys[1]))
                b.lit(1)
            pos.append(b.lit(1) + 1)
            b.lit(data=X)
            b.lit(2)
            pos.append(b.lit(data=ys[0]))
            b.lit(1)
            copies.append((kind, pos[-2], pos))
            groups.append((pos, pos[-1], non_collider(ys[0], tt)))
    # a group split across two windows: the second member's snapshot candidate is the first
    reset()
    X = bytes(b.rng.integers(0, 256, w, dtype=np.uint8).tobytes())
    px = b.lit(1) + 1
    b.lit(data=X)
    b.lit(30)
    reset()
    b.lit(40)
    py = b.lit(data=colliders(X, tt)[0])
    b.lit(1)
    copies.append(("split", px, [px, py]))
    groups.append(([px, py], py, non_collider(colliders(X, tt)[0], tt)))
    for kind, px, pos in copies:
        reset()
        b.lit(3)
        P = b.lit(data=bytes(b.b[px:px + w]))
        b.cont = b.b[px + w]
        b.lit(2)
        checks.append(("clash_group", kind, "nomatch", (P, pos)))
    return _case("clash-collide", b.tail(), tt, checks, groups=groups)


def clashes(tt):
    out = []
    L = LADDERS[tt]
    # equal prefixes at spacing d that diverge after m bytes
    b, checks = _B(6000), []
    b.lit(20)
    b.match(1, 8)
    lens = L["clash_len"]
    for i, d in enumerate(L["clash_spacing"]):
        for j in range(len(lens)):
            m = lens[(i + j) % len(lens)]
            if j >= 3 and i % 3 != j % 3:
                continue
            U = b.lit(d)
            plan = b.match(U, m)
            checks += [("clash_spacing", d, "seq", plan), ("clash_len", m, "seq", plan)]
    out.append(_case("clash-prefix", b.tail(), tt, checks))
    # (the first seed at which no other probe shares a group's hash by chance)
    for seed in range(6100, 70000, 1000):
        c = _collide_case(tt, seed)
        n0 = len(trace(c.block, tt).seqs)
        w = hash_width(tt)
        if all(len(trace(c.block[:rp] + repl + c.block[rp + w:], tt).seqs) == n0 + 1 for _, rp, repl in c.groups):
            break
    out.append(c)
    # dense mixtures of both: tiny alphabets and a few words, windows full of shared hashes.
    # Seed 21 of the two-letter blocks is the one of 60 seeds at which the kernel's clash
    # fixpoint uses up its six passes and hands the window to the exact walk (byU16 and byU64;
    # seeds 29 and 38 stop after five passes); none of 360 seeded mixtures did so for byU32.
    for seed in (21, 29, 38):
        blk = np.random.default_rng(seed).integers(0, 2, 520, dtype=np.uint8).tobytes()
        out.append(_case(f"clash-mix-a2-s{seed}", blk, tt, []))
    for seed in range(3):
        rng = np.random.default_rng(6200 + seed)
        a = 2 + seed % 3
        words = [rng.integers(0, a, int(rng.integers(3, 10)), dtype=np.uint8).tobytes() for _ in range(5)]
        parts = []
        while sum(map(len, parts)) < 500:
            parts.append(words[int(rng.integers(0, 5))] if rng.integers(0, 3) else
                         rng.integers(0, a, int(rng.integers(1, 6)), dtype=np.uint8).tobytes())
        out.append(_case(f"clash-mix-words-a{a}-s{seed}", b"".join(parts)[:520], tt, []))
    return out


def dict_cases(tt=BYU32):
    """Dictionary mode (byU32 only): image positions are [dictionary | block];
    the preload puts every third dictionary position p with p + 8 <= D."""
    assert tt == BYU32
    out = []
    rng = np.random.default_rng(7000)
    D = 4096
    dic = rng.integers(0, 256, D, dtype=np.uint8).tobytes()

    def mk(label, dic, parts, checks):
        b = _B(7001 + len(out))
        for p in parts:
            b.lit(p) if isinstance(p, int) else b.lit(data=p)
        return _case(label, b.tail(), tt, checks, dic=dic)

    # a candidate inside the dictionary (a preloaded position)
    # (a late one: few preload puts follow it that could share its hash)
    out.append(mk("dict-inside", dic, [5, dic[4062:4074]], [("dict", "inside", "seq", (5, 5, D + 5 - 4062, 12))]))
    # a match whose source starts in the dictionary and runs on into the block
    S = D - 13
    assert S % 3 == 0
    b = _B(7100)
    img = bytearray(dic)
    img += b.rng.integers(0, 256, 6, dtype=np.uint8).tobytes()
    for i in range(30):
        img.append(img[S + i])
    blk = bytes(img[D:]) + bytes([img[S + 30] ^ 0x55]) + b.rng.integers(0, 256, 13, dtype=np.uint8).tobytes()
    out.append(_case("dict-crossing", blk, tt, [("dict", "crossing", "seq", (6, 6, D + 6 - S, 30))], dic=dic))
    # catch-up stopped by the dictionary's start: position 0 is evicted by a later preloaded
    # position, positions 1 and 2 are never preloaded, so the probe at 3 hits and walks back to 0
    D = 48  # (a short dictionary: no preload put shares a hash with positions 0 and 3 by chance)
    dic = dic[:D]
    d2 = bytearray(dic)
    d2[30:35] = colliders(d2[0:8], tt)[0]
    d2 = bytes(d2)
    out.append(mk("dict-start", d2, [1, d2[0:16]],
                  [("dict", "start", "seq", (1, 1, D + 1, 16)), ("dict", "start", "event", (1, 4, 3, "zero"))]))
    # catch-up stopped by the anchor: the block opens with the dictionary's bytes 1..
    out.append(mk("dict-anchor", dic, [dic[1:17]],
                  [("dict", "anchor", "seq", (0, 0, D - 1, 16)), ("dict", "anchor", "event", (0, 2, 2, "anchor"))]))
    # distance exactly 65535 into a 64 KiB dictionary, and 65536 refused
    D = 65536
    # (random bytes, then zeros: 21845 preload puts of random bytes would leave no early position in the table)
    big = np.random.default_rng(7200).integers(0, 256, 64, dtype=np.uint8).tobytes() + bytes(D - 64)
    out.append(mk("dict-65535", big, [2, big[3:15], 4, big[18:30]],
                  [("dict", "65535", "seq", (2, 2, 65535, 12)), ("dict", "65536", "refuse", (18, 65536))]))
    return out


def capacity_sweep():
    """Three blocks of 300-700 bytes for the every-capacity sweeps: one long
    match, one long literal run, many short sequences."""
    b = _B(8000)
    U = b.lit(20)
    b.match(U, 400)
    b.lit(30)
    b.match(U + 3, 9)
    long_match = b.tail()
    b = _B(8001)
    b.lit(24)
    b.match(1, 8)
    b.lit(400)
    b.match(10, 13)
    long_lit = b.tail()
    b = _B(8002)
    b.lit(12)
    for i in range(44):
        U = b.lit(2 + i % 5)
        b.match(U, 4 + (i * 3) % 7 + (1 if i % 11 == 0 else 0) * 14)
    short = b.tail()
    return [_case("sweep-long-match", long_match, BYU16, []), _case("sweep-long-literals", long_lit, BYU16, []),
            _case("sweep-short-sequences", short, BYU16, [])]


PLAIN_FAMILIES = {"match_lengths": match_lengths, "literal_runs": literal_runs, "catch_up": catch_up,
                  "offsets": offsets, "block_ends": block_ends, "clashes": clashes}
FAMILIES = sorted(PLAIN_FAMILIES) + ["dict"]


@functools.lru_cache(maxsize=None)
def cases(family, tt=BYU16):
    if family == "dict":
        return tuple(dict_cases(tt))
    return tuple(PLAIN_FAMILIES[family](tt))


def plain_cases(tt):
    return [c for f in sorted(PLAIN_FAMILIES) for c in cases(f, tt)]
