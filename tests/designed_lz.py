"""Designed-sequence corpus (test infrastructure): LZ4, Snappy and LZO inputs whose matches are chosen,
not found, and decoder streams the in-house encoders never write.

Part A (encoders).  The filler is incompressible (prng_bytes) and a match is a planted copy of
earlier filler, buf[D : D + L] = buf[S : S + L].  The three encoders are greedy and skip positions:
the positions a search visits are a closed form of its attempt count until something matches,

  LZ4 r123   step = attempts++ >> 6, attempts restarting at 67 after every match (search from ip + 1),
  Snappy     step = skip++ >> 5 from skip = 32 (search from next_emit + 1),
  LZO1X-1    ip += 1 + ((ip - ii) >> 5) (search from the match end itself; from byte 5 at a block start),

so a planted copy is found at the first *visited* position inside it whose source counterpart is the
table's entry for its bytes.  Each builder below walks that schedule, plants the copies at visited
positions (LZ4: or lets catch-up walk back to the plant's start), puts a differing byte on either
side of every plant, and then replays its own record of table reads and writes over the final bytes:
every find must read its designed source, every other visit must read something that does not
match.  A case is (tag, input, designed sequences, facts); the CPU tests assert that the oracle's
parsed output is exactly the designed list, so the families' coverage claims are claims about the
oracle's output, and the builder's schedule model (attempt index, batch, lane, table slot, tag) stands
in where the output cannot show which path ran.

LZO has no independent encoder or decoder on the test machines: the oracle's lzo1x_1 / lzo1x_decode
are the only ones, so the LZO cases are checked against the builder's model and the oracle alone.

Part B (decoders).  Every stream is valid and is built from an element list; the expected bytes come
from applying the same elements in a few lines of Python, not from any decoder.

Blocks are generated from helpers.prng_bytes, cached per process and read-only; nothing here is
stored in the tree."""
import functools

import numpy as np

from helpers import prng_bytes

LZ4_MAX_IN = 261100           # BlockCompressorStream MAX_INPUT_SIZE of Lz4Codec
SNAPPY_MAX_IN = 218422
LZO_MAX_IN = 245693
LZ4_64K = 65536 + 11          # blocks below this use the byU16 table
LZ4_BATCHES = (8, 16, 32, 64)  # lz4.hip kLzFirstBatch, then doubled up to 64 (64 from then on)
SN_BATCHES = (16, 32, 64)     # snappy.hip sn_fragment: m = 16, then doubled up to 64
DEC_WIN = 8192                # kDecWin / kSnDecWin: the decoders' LDS input window


def _frozen(a):
    a.flags.writeable = False
    return a


def _copy_fwd(buf, dst, src, n):
    """The LZ copy: n bytes from src to dst > src, byte by byte (an overlapping copy repeats)."""
    assert 0 <= src < dst, (src, dst)
    if n <= 0:
        return
    d = dst - src
    buf[dst:dst + n] = buf[src:src + n] if d >= n else np.resize(buf[src:dst].copy(), n)


def _word(buf, p):
    return int.from_bytes(buf[p:p + 4].tobytes(), "little")


def _poke(buf, p, v):
    buf[p:p + 4] = np.frombuffer(int(v).to_bytes(4, "little"), np.uint8)


def batch_of(k, batches):
    """(batch number, lane) of attempt k when batches grow as `batches` and stay at the last size."""
    for b, m in enumerate(batches):
        if k < m:
            return b, k
        k -= m
    return len(batches) + k // batches[-1], k % batches[-1]


class Undesigned(Exception):
    """The replay found the table holding something else than the design needs (an equal table index
    between two filler words): the case is rebuilt over the next seed's filler."""


def designed(build, seed):
    """build(seed) over the first seed (of 16) whose filler has no such accident."""
    for s in range(seed, seed + 16):
        try:
            return build(s)
        except Undesigned:
            continue
    raise Undesigned(f"no seed in [{seed}, {seed + 16}) works")


class _Differ:
    """Guard bytes: buf[pos] made to differ from every value asked for at that position."""

    def _differ(self, pos, value):
        f = self.forbid.setdefault(pos, set())
        f.add(int(value))
        while int(self.buf[pos]) in f:
            self.buf[pos] = (int(self.buf[pos]) + 1) & 0xFF


# =================================================================================================
# Part A: LZ4 (lz4 r123 LZ4_compress, noDict; oracle/hdrf_oracle.c lz4_compress_rules with rules 0)
# =================================================================================================
def lz4_step(k):
    return max(1, (67 + k) >> 6)


def lz4_index(v, u16):
    return ((int(v) * 2654435761) & 0xFFFFFFFF) >> (19 if u16 else 20)


def lz4_tag(v, u16):
    """lz4.hip's 2-bit tag: the two product bits just below the index bits."""
    return (((int(v) * 2654435761) & 0xFFFFFFFF) >> (17 if u16 else 18)) & 3


@functools.lru_cache(None)
def lz4_equal_index_words(u16):
    """(p, q, q2): distinct 4-byte values with equal table index; q has p's tag, q2 another (brute
    force over generated values)."""
    w = prng_bytes(77, 4 << 20).view(np.uint32)
    prod = (w.astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    idx = prod >> np.uint64(19 if u16 else 20)
    tag = (prod >> np.uint64(17 if u16 else 18)) & np.uint64(3)
    same = np.nonzero((idx == idx[0]) & (w != w[0]))[0]
    q = next(int(w[i]) for i in same if tag[i] == tag[0])
    q2 = next(int(w[i]) for i in same if tag[i] != tag[0])
    p = int(w[0])
    assert lz4_index(p, u16) == lz4_index(q, u16) == lz4_index(q2, u16)
    assert lz4_tag(p, u16) == lz4_tag(q, u16) != lz4_tag(q2, u16)
    return p, q, q2


class Lz4Design(_Differ):
    """One LZ4 block under construction.  match() / chain() / decoy() plant copies in parse order;
    finish() replays the table and returns (frozen input, designed sequences, facts).  A sequence is
    (literal length, offset, match length), the last one (literal length, None, 0)."""

    def __init__(self, n, seed):
        self.n = n
        self.buf = prng_bytes(seed, n)
        self.u16 = n < LZ4_64K
        self.mflimit, self.matchlimit = n - 12, n - 5
        self.events = [("ins", 0)] if n >= 13 else []
        self.anchor, self.start = 0, 1
        self.done = n < 13
        self.seqs, self.facts, self.forbid = [], [], {}
        self.prev_cont = None
        self.want_far = []

    def schedule(self):
        """(attempt index, position) of every position the search from self.start examines."""
        pos, k = self.start, 0
        while pos + lz4_step(k) <= self.mflimit:
            yield k, pos
            pos += lz4_step(k)
            k += 1

    def inserted(self):
        return {e[1] for e in self.events}

    def pair(self, dist, lo=0, src_ok=lambda s: True):
        """The first visited position V >= lo of the running search whose V - dist has been put in
        the table by then (so a copy planted there is found at V, `dist` back)."""
        seen = self.inserted()
        for _, p in self.schedule():
            if p >= lo and p - dist in seen and src_ok(p - dist):
                return p
            seen.add(p)
        raise ValueError(f"no visited pair at distance {dist}")

    def poke(self, pos, v):
        _poke(self.buf, pos, v)

    def match(self, lit, src, L, at=None, stop="byte"):
        """The next sequence: `lit` literals, then a match of L bytes whose first byte copies
        buf[src].  It is found at V = `at` (default: the first visited position >= anchor + lit) and
        catch-up walks back V - (anchor + lit) bytes; `stop` says what ends the walk: "byte" (a
        differing byte), "anchor" (lit == 0) or "zero" (the reference reaches byte 0)."""
        assert not self.done
        A = self.anchor + lit
        k, V = next((k, p) for k, p in self.schedule() if p >= (A if at is None else at))
        assert at is None or V == at, f"{at} is not visited"
        back = V - A
        assert 0 <= src < A and A + L <= self.n
        assert stop == {(True, False): "anchor", (False, True): "zero", (True, True): "zero"}.get(
            (lit == 0, src == 0), "byte"), (stop, lit, src)
        if stop == "byte":
            self._differ(A - 1, self.buf[src - 1])
        _copy_fwd(self.buf, A, src, L)
        ml = min(L, self.matchlimit - A)
        assert ml >= 4
        E = A + ml
        if E < self.matchlimit:
            self._differ(E, self.buf[src + ml])
            self.prev_cont = int(self.buf[src + ml])
        for _, p in self.schedule():
            if p >= V:
                break
            self.events.append(("visit", p))
        self.events.append(("find", V, src + back))
        self.seqs.append((lit, A - src, ml))
        self.facts.append(dict(k=k, ip=V, mref=src + back, back=back, lit=lit, ml=ml, off=A - src, chain=False,
                               stop=stop, start=A, fast=(V - self.anchor <= 64 and V >= 64 and src + back >= 64)))
        self._after(E)
        return A

    def _after(self, E):
        self.anchor = E
        if E > self.mflimit:
            self.done = True
        else:
            self.events += [("ins", E - 2), ("visit", E)]
            self.start = E + 1

    def chain(self, src, L):
        """A match that starts where the previous one ended (a token with 0 literals): the test of
        the next position must read src."""
        assert not self.done and self.events[-1] == ("visit", self.anchor)
        A = self.anchor
        self.events.pop()
        if int(self.buf[src]) == self.prev_cont:
            raise Undesigned("the chained match would extend the previous one")
        _copy_fwd(self.buf, A, src, L)
        ml = min(L, self.matchlimit - A)
        E = A + ml
        if E < self.matchlimit:
            self._differ(E, self.buf[src + ml])
            self.prev_cont = int(self.buf[src + ml])
        self.events.append(("find", A, src))
        self.seqs.append((0, A - src, ml))
        self.facts.append(dict(k=None, ip=A, mref=src, back=0, lit=0, ml=ml, off=A - src, chain=True, stop=None,
                               start=A, fast=False))
        self._after(E)

    def decoy(self, dst, src, L):
        """A planted copy that must produce no match: inside the last bytes, or more than 65,535 back
        (then the replay must see the table hand out src at dst, rejected by distance alone)."""
        assert dst >= self.anchor
        if dst - src > 65535:
            self.want_far.append((dst, src))
        self._differ(dst - 1, self.buf[src - 1])
        _copy_fwd(self.buf, dst, src, L)

    def finish(self):
        if not self.done:
            self.events += [("visit", p) for _, p in self.schedule()]
        self.seqs.append((self.n - self.anchor, None, 0))
        buf, tab, far, slots = self.buf, {}, [], {}
        for ev in self.events:
            p = ev[1]
            v = _word(buf, p)
            h = lz4_index(v, self.u16)
            cand = tab.get(h, 0)
            tab[h] = p
            slots[p] = (h, lz4_tag(v, self.u16), cand)
            if ev[0] == "ins":
                continue
            same = _word(buf, cand) == v
            if ev[0] == "find":
                if not (cand == ev[2] and same and p - cand <= 65535):
                    raise Undesigned(f"find at {p}: table holds {cand}, designed {ev[2]}")
            elif same and cand + 65535 < p:
                far.append((p, cand))                 # equal bytes, rejected by distance alone
            elif same:
                raise Undesigned(f"undesigned match at {p} (candidate {cand})")
        if any(w not in far for w in self.want_far):
            raise Undesigned(f"rejected by distance: {far}, designed {self.want_far}")
        return _frozen(buf), self.seqs, dict(finds=self.facts, far=far, slots=slots, u16=self.u16)


def lz4_first_match(d, A=40, src=8, L=30):
    """The opening match most cases start with: found at byte 40, ends at byte 70; the next search
    starts at 71 with attempt 0 and the table holds bytes 0..40, 68 and 70."""
    d.match(A, src, L)
    return d.anchor


def _cases(specs):
    """[(tag, build, seed)] -> [(tag, input, sequences, facts)]"""
    return [(tag,) + designed(build, seed) for tag, build, seed in specs]


LZ4_ML_SHORT = tuple(range(4, 25))
LZ4_ML_RUNS = tuple(15 + 4 + k for k in (254, 255, 256, 509, 510, 511, 764, 765, 1019, 1020, 1021))
LZ4_ML_LONG = 64 * 510 + 19 + 7                    # two strides of the lane loop that writes 255-pairs
# A match cannot be moved against the 256-byte extension windows independently of its length: the
# window pair starts at the found position - 64 on the fast path and at the match start on the general
# path, so the match end lies L + 64 or L bytes into the windows.  Each length is therefore taken on
# both paths, and the window-edge lengths below put the end at {-1, 0, +1, +3, +4} around the first and
# the second window step on either path.
LZ4_ML_WINDOW = tuple(sorted({256 * j + e - f for j in (1, 2) for e in (-1, 0, 1, 3, 4) for f in (0, 64)}))
LZ4_ML_ALL = LZ4_ML_SHORT + LZ4_ML_RUNS + LZ4_ML_WINDOW + (LZ4_ML_LONG,)


@functools.lru_cache(None)
def lz4_match_lengths():
    """Family 1.  Every length once on the fast path (a second match 20 literals after an opening one,
    both positions >= 64, the source at byte 64) and once on the general path (the block's first
    match, reference < 64)."""
    specs = []
    for L in LZ4_ML_ALL:
        def fast(seed, L=L):
            d = Lz4Design(2 * L + 400, seed)
            d.match(L + 100, 8, 30)                # the opening match, behind L + 100 bytes of filler
            d.match(20, 64, L)                     # byte 64: put in the table by the opening search
            assert d.facts[-1]["fast"] and d.facts[-1]["back"] == 0
            return d.finish()

        def general(seed, L=L):
            d = Lz4Design(2 * L + 400, seed)
            d.match(L + 100, 3, L)
            assert not d.facts[-1]["fast"]
            return d.finish()
        specs += [(f"ml={L} fast", fast, 1000 + L), (f"ml={L} general", general, 1000 + L)]
    return _cases(specs)


LZ4_LIT_RUNS = (0, 1, 14, 15, 16, 64, 65, 15 + 254, 15 + 255, 15 + 256, 16334, 16335, 16336, 15 + 255 * 65)
LZ4_WHERE = ("ip<64", "mref<64", "both>=64")


@functools.lru_cache(None)
def lz4_literal_runs():
    """Family 2.  Each run before a match found at ip < 64 (the block's first match: only runs of
    1..62 exist there), with its reference < 64 <= ip, and with both >= 64.  A run of 0 is a chained
    match."""
    specs = []
    for lit in LZ4_LIT_RUNS:
        for where in LZ4_WHERE:
            if where == "ip<64" and not 1 <= lit <= 62:
                continue

            def build(seed, lit=lit, where=where):
                d = Lz4Design(lit + 400, seed)
                if where == "ip<64":
                    d.match(lit, 0, 9, stop="zero")
                else:
                    E = lz4_first_match(d)
                    mref = 39 if where == "mref<64" else E - 2
                    if lit == 0:
                        d.chain(mref, 11)
                    else:
                        V = next(p for _, p in d.schedule() if p >= E + lit)
                        d.match(lit, mref - (V - E - lit), 13 + V - E - lit)
                f = d.facts[-1]
                assert (f["ip"] < 64, f["mref"] < 64 <= f["ip"], f["mref"] >= 64 and f["ip"] >= 64) == \
                    tuple(where == w for w in LZ4_WHERE), (lit, where, f)
                return d.finish()
            specs.append((f"lit={lit} {where}", build, 2000 + lit))
    return _cases(specs)


@functools.lru_cache(None)
def lz4_attempt_index():
    """Family 3.  The first hit after a match at every attempt index 0..140: each lane of the 8, 16,
    32 and 64 batches and of the 64 batch after them, and the step change from 1 to 2 at attempt 61."""
    specs = []
    for k in range(141):
        def build(seed, k=k):
            d = Lz4Design(700, seed)
            E = lz4_first_match(d)
            V = next(p for kk, p in d.schedule() if kk == k)
            d.match(V - E, 68, 7)
            assert d.facts[-1]["k"] == k and d.facts[-1]["back"] == 0
            return d.finish()
        specs.append((f"attempt={k}", build, 3000 + k))
    return _cases(specs)


LZ4_BACK_FAST = (0, 1, 3, 4, 62, 63)
LZ4_BACK_GENERAL = (63, 64, 65, 128, 150)
LZ4_BACK_ZERO = (1, 3, 4, 44)


@functools.lru_cache(None)
def lz4_catch_up():
    """Family 4.  Catch-up walks of a chosen length b.

    Stop at a differing byte or at the anchor: the walked bytes are visited by the search (its step
    is still 1 or 2) but are not found there.  They copy the inside of the opening match, whose own
    positions were never put in the table; the equal words that are in the table belong to the opening
    match's source, which lies 65,535 bytes before it and so more than 65,535 before the walked bytes
    (rejected by distance).  Only the found position's counterpart is a table entry in range: the
    opening match's end - 2, which the encoder inserts.  Fast path (found <= 64 bytes after the anchor,
    both positions >= 64): b in LZ4_BACK_FAST; general path (found more than 64 bytes after the
    anchor): b in LZ4_BACK_GENERAL.  A walk to the anchor is found at anchor + b, which the search
    visits for b <= 62 and for even b above; b == 64 at the anchor is the fast test finding 64 equal
    bytes and handing over to the general loop.  b == 0 at the anchor is the chained match (family 7).

    Stop at byte 0 of the block: the block's first match, found where the search step has grown above
    b so that nothing inside the walk is visited; the reference is byte b itself.  The found position
    is then at most 65,535 + b, where the step is at most 45, so b <= 44 (LZ4_BACK_ZERO): the walks of
    62 and more cannot end at byte 0.  The fast path cannot stop there either: its reference is >= 64
    and its walk <= 63."""
    specs = []
    combos = [(b, "fast") for b in LZ4_BACK_FAST] + [(b, "general") for b in LZ4_BACK_GENERAL] + [(64, "fast")]

    def opening(d, back):
        V1 = d.pair(65535, lo=65700, src_ok=lambda s: s >= 1)
        d.match(V1, V1 - 65535, 90 + back)
        return d.anchor
    for back, path in combos:
        for stop in ("byte", "anchor"):
            probe = Lz4Design(67200, 0)
            E = opening(probe, back)
            vis = {p for _, p in probe.schedule()}
            if stop == "anchor":
                lit = 0
                if back == 0 or E + back not in vis or (path == "fast") != (back <= 64):
                    continue
            else:
                if (back, path) == (64, "fast"):
                    continue
                lit = [t for t in range(1, 200) if E + t + back in vis and (t + back <= 64) == (path == "fast")][0]

            def build(seed, back=back, lit=lit, stop=stop, path=path):
                d = Lz4Design(67200, seed)
                E = opening(d, back)
                d.match(lit, E - 2 - back, back + 9, at=E + lit + back, stop=stop)
                f = d.facts[-1]
                assert f["back"] == back and f["fast"] == (path == "fast"), (back, stop, f)
                return d.finish()
            specs.append((f"back={back} {path} stop={stop}", build, 4000 + 7 * back))
    for back in LZ4_BACK_ZERO:
        probe = Lz4Design(LZ4_MAX_IN, 0)
        prev = 0
        for _, p in probe.schedule():
            if p - prev > back and p > 2 * back + 70:
                break
            prev = p
        V = p

        def build(seed, back=back, V=V):
            d = Lz4Design(V + 300, seed)
            d.match(V - back, 0, back + 9, at=V, stop="zero")
            assert d.facts[-1]["back"] == back and not d.facts[-1]["fast"]
            return d.finish()
        specs.append((f"back={back} general stop=zero", build, 4500 + back))
    return _cases(specs)


LZ4_DIST = (1, 2, 3, 4, 255, 256, 65534, 65535)
LZ4_SEAMS = (65536, 131072, 196608)


@functools.lru_cache(None)
def lz4_distances():
    """Family 5.  Offsets at both ends of the 16-bit range in a byU32 block, the small ones also in a
    byU16 block; a copy planted exactly 65,536 back, which must give no match; and around each 64 KiB
    seam of the position (bits 16-17 of a byU32 table entry) a pair of visited positions 65,536 apart
    with equal bytes: the later one replaces the earlier one in the table slot (equal low 16 bits,
    another seam nibble, no match: too far), and a copy of it planted 20,000 bytes on must be found at
    its distance from the later one."""
    specs = []
    for u16 in (True, False):
        for dist in LZ4_DIST:
            if u16 and dist > 256:
                continue

            def build(seed, dist=dist, u16=u16):
                d = Lz4Design(700 if u16 else max(66000, dist + 800), seed)
                V = d.pair(dist, lo=30, src_ok=lambda s: s >= 1)
                d.match(V, V - dist, 12)
                return d.finish()
            specs.append((f"dist={dist} {'byU16' if u16 else 'byU32'}", build, 5000 + dist))

    def too_far(seed):
        d = Lz4Design(66400, seed)
        V = d.pair(65536, lo=30, src_ok=lambda s: s >= 1)
        d.decoy(V, V - 65536, 12)
        return d.finish()
    specs.append(("dist=65536 no match", too_far, 5900))
    for B in LZ4_SEAMS:
        for side in ("above", "below"):
            vis = [p for _, p in Lz4Design(LZ4_MAX_IN, 0).schedule()]
            vs = set(vis)
            ok = [p for p in vis if p - 65536 in vs]
            P2 = min((p for p in ok if p >= B), default=None) if side == "above" else \
                max((p for p in ok if p < B), default=None)
            if P2 is None:
                continue                           # no position below the first seam has one 65,536 before it
            D = next(p for p in vis if p >= P2 + 20000)

            def build(seed, P2=P2, D=D):
                d = Lz4Design(D + 100, seed)
                d.decoy(P2, P2 - 65536, 8)
                d.match(D, P2, 10, at=D)
                return d.finish()
            specs.append((f"seam={B} {side} P2={P2}", build, 5950 + B // 65536))
    return _cases(specs)


@functools.lru_cache(None)
def lz4_equal_hashes():
    """Family 6.  Two distinct words with equal table index at two attempts of one batch (the 16
    batch of the search after the opening match: attempts 8..23 at bytes 79..94), with equal and with
    different tags, in a byU16 and in a byU32 block:
      none   no match in the batch (a later match closes the case);
      known  the later attempt matches the earlier one of the same batch (equal words);
      undo   an attempt before them matches, so their table writes must not happen: a third word of
             the same index sits in the table from the opening search (byte 20), and the search after
             the short match finds it from a copy at its attempt 0, which reads that slot."""
    specs = []
    for n, tab in ((400, "byU16"), (66000, "byU32")):
        for tags in ("equal", "different"):
            def none(seed, n=n, tags=tags):
                d = Lz4Design(n, seed)
                E = lz4_first_match(d)
                p, q, q2 = lz4_equal_index_words(d.u16)
                d.poke(E + 1 + 10, p)
                d.poke(E + 1 + 15, q if tags == "equal" else q2)
                d.match(40, 39, 9)
                return d.finish()
            specs.append((f"none tags={tags} {tab}", none, 6000))

        def undo(seed, n=n):
            d = Lz4Design(n, seed)
            p, q, q2 = lz4_equal_index_words(d.u16)
            d.poke(20, p)
            lz4_first_match(d)
            d.match(9, 39, 5)                      # attempt 8 (lane 0 of the 16 batch) at byte 79
            d.match(1, 20, 4)                      # byte 85: lane 6 of that batch, then attempt 0
            d.poke(90, q)                          # lanes 11 and 15 of that batch
            d.poke(94, q2)
            return d.finish()
        specs.append((f"undo {tab}", undo, 6100))

        def known(seed, n=n):
            d = Lz4Design(n, seed)
            E = lz4_first_match(d)
            d.match(17, E + 1 + 10, 6)             # attempts 10 and 16 of the 16 batch
            assert d.facts[-1]["mref"] == E + 11 and d.facts[-1]["k"] == 16
            return d.finish()
        specs.append((f"known {tab}", known, 6200))
    return _cases(specs)


@functools.lru_cache(None)
def lz4_chains():
    """Family 7.  A match that starts at the byte where the previous one ended (0 literals): with the
    words at ip - 2 and ip equal (a period of 2: the source is ip - 2 itself) and not; after a first
    match that ends exactly at a 256-byte window start and one byte before it; and a tag-equal false
    candidate at the chain test (same index, same tag, other bytes), which must not chain."""
    specs = []
    for L1 in (30, 255, 256, 257):
        for src in ("ip-2", 39):
            def build(seed, L1=L1, src=src):
                d = Lz4Design(2 * L1 + 500, seed)
                d.match(L1 + 100, 8, L1)
                d.chain(d.anchor - 2 if src == "ip-2" else 39, 11)
                d.match(12, 25, 8)
                return d.finish()
            specs.append((f"chain after ml={L1} src={src}", build, 7000 + L1))

    def false_candidate(seed):
        d = Lz4Design(400, seed)
        p, q, _ = lz4_equal_index_words(d.u16)
        d.poke(20, q)
        E = lz4_first_match(d)
        d.poke(E, p)
        if int(d.buf[E]) == d.prev_cont:
            raise Undesigned("the poked word would extend the opening match")
        d.match(12, 39, 9)
        return d.finish()
    specs.append(("false chain candidate", false_candidate, 7500))
    return _cases(specs)


@functools.lru_cache(None)
def lz4_block_ends():
    """Family 8.  Blocks of 12, 13 and 14 bytes; a match that runs into the last 5 bytes (it stops at
    n - 5); matches ending at mflimit - 1, mflimit, mflimit + 1; copies planted at mflimit - 1 (the
    last position the search examines), at mflimit and inside the last 12 bytes (both stay literals)."""
    specs = [(f"n={n}", lambda seed, n=n: Lz4Design(n, seed).finish(), 8000 + n) for n in (12, 13, 14)]
    n = 200

    def into_tail(seed):
        d = Lz4Design(n, seed)
        d.match(60, 8, n - 60)
        assert d.seqs[-1][2] == n - 5 - 60
        return d.finish()
    specs.append(("match into the last 5 bytes", into_tail, 8100))
    for e in (-1, 0, 1):
        def build(seed, e=e):
            d = Lz4Design(n, seed)
            d.match(60, 8, n - 12 + e - 60)
            return d.finish()
        specs.append((f"match ends at mflimit{e:+d}", build, 8200 + e))
    m = 120                                        # mflimit 108: bytes 71..107 are examined with step 1
    for at in (m - 13, m - 12, m - 10):
        def build(seed, at=at):
            d = Lz4Design(m, seed)
            E = lz4_first_match(d)
            if at == m - 13:
                d.match(at - E, 39, 6)
            else:
                d.decoy(at, 39, 6)
            return d.finish()
        specs.append((f"copy planted at n-{m - at}", build, 8300 + at))
    return _cases(specs)


LZ4_FAMILIES = {"match_lengths": lz4_match_lengths, "literal_runs": lz4_literal_runs,
                "attempt_index": lz4_attempt_index, "catch_up": lz4_catch_up, "distances": lz4_distances,
                "equal_hashes": lz4_equal_hashes, "chains": lz4_chains, "block_ends": lz4_block_ends}


# =================================================================================================
# Part A: Snappy (google/snappy level 1; oracle/hdrf_oracle.c sn_fragment), one 64 KiB fragment each
# =================================================================================================
SN_FRAG = 65536


def sn_table_mask(n):
    ts = 256
    while ts < (1 << 15) and ts < n:
        ts <<= 1
    return ts - 1


def sn_index(v, mask):
    return (((int(v) * 0x1e35a7bd) & 0xFFFFFFFF) >> 17) & mask


@functools.lru_cache(None)
def sn_equal_index_words(mask):
    """Three distinct 4-byte values with equal table index under `mask` (brute force)."""
    w = prng_bytes(78, 4 << 20).view(np.uint32)
    idx = (((w.astype(np.uint64) * np.uint64(0x1e35a7bd)) & np.uint64(0xFFFFFFFF)) >> np.uint64(17)) & np.uint64(mask)
    same = np.nonzero((idx == idx[0]) & (w != w[0]))[0]
    p, q, q2 = int(w[0]), int(w[same[0]]), int(w[same[1]])
    assert len({p, q, q2}) == 3 and sn_index(p, mask) == sn_index(q, mask) == sn_index(q2, mask)
    return p, q, q2


def sn_copy_elements(off, ln):
    """The copy elements of one match: 64-byte pieces while >= 68 remain, a 60-byte piece if more than
    64 remain, then the rest; the 1-byte-offset form for < 12 bytes at an offset < 2048."""
    out = []
    while ln >= 68:
        out.append(("c2", 64, off))
        ln -= 64
    if ln > 64:
        out.append(("c2", 60, off))
        ln -= 60
    out.append(("c1" if ln < 12 and off < 2048 else "c2", ln, off))
    return out


class SnappyDesign(_Differ):
    """One Snappy fragment under construction (Lz4Design's protocol; no catch-up, no distance limit).
    The designed output is the element list [("lit", n, 0) | ("c1" | "c2", length, offset)]."""

    def __init__(self, n, seed):
        assert n <= SN_FRAG
        self.n, self.buf, self.mask, self.lim = n, prng_bytes(seed, n), sn_table_mask(n), n - 15
        self.events, self.elems, self.facts, self.forbid = [], [], [], {}
        self.next_emit, self.done, self.prev_cont = 0, n < 15, None

    def schedule(self):
        pos, skip, k = self.next_emit + 1, 32, 0
        while pos + (skip >> 5) <= self.lim:
            yield k, pos
            pos, skip, k = pos + (skip >> 5), skip + (skip >> 5), k + 1

    def pair(self, dist, lo=0):
        seen = {e[1] for e in self.events}
        for _, p in self.schedule():
            if p >= lo and p - dist in seen:
                return p
            seen.add(p)
        raise ValueError(f"no visited pair at distance {dist}")

    def poke(self, pos, v):
        _poke(self.buf, pos, v)

    def _plant(self, A, src, L):
        _copy_fwd(self.buf, A, src, L)
        ml = min(L, self.n - A)
        E = A + ml
        if E < self.n:
            self._differ(E, self.buf[src + ml])
            self.prev_cont = int(self.buf[src + ml])
        self.elems += sn_copy_elements(A - src, ml)
        self.next_emit = E
        if E >= self.lim:
            self.done = True
        else:
            self.events += [("ins", E - 1), ("visit", E)]
        return ml

    def match(self, lit, src, L):
        assert not self.done and lit >= 1
        A = self.next_emit + lit
        k = next((k for k, p in self.schedule() if p == A), None)
        assert k is not None, f"{A} is not visited"
        self.events += [("visit", p) for _, p in self.schedule() if p < A] + [("find", A, src)]
        self.elems.append(("lit", lit, 0))
        ml = self._plant(A, src, L)
        self.facts.append(dict(k=k, ip=A, src=src, lit=lit, ml=ml, off=A - src))
        return A

    def chain(self, src, L):
        assert not self.done and self.events[-1] == ("visit", self.next_emit)
        A = self.next_emit
        self.events[-1] = ("find", A, src)
        if int(self.buf[src]) == self.prev_cont:
            raise Undesigned("the chained copy would extend the previous one")
        ml = self._plant(A, src, L)
        self.facts.append(dict(k=None, ip=A, src=src, lit=0, ml=ml, off=A - src))

    def finish(self):
        if not self.done:
            self.events += [("visit", p) for _, p in self.schedule()]
        if self.next_emit < self.n:
            self.elems.append(("lit", self.n - self.next_emit, 0))
        buf, tab, slots = self.buf, {}, {}
        for ev in self.events:
            p = ev[1]
            v = _word(buf, p)
            h = sn_index(v, self.mask)
            cand = tab.get(h, 0)
            tab[h] = p
            slots[p] = (h, cand)
            if ev[0] == "ins":
                continue
            same = _word(buf, cand) == v
            if ev[0] == "find":
                if not (cand == ev[2] and same):
                    raise Undesigned(f"find at {p}: table holds {cand}, designed {ev[2]}")
            elif same:
                raise Undesigned(f"undesigned match at {p} (candidate {cand})")
        return _frozen(buf), self.elems, dict(finds=self.facts, slots=slots, mask=self.mask)


def sn_first_match(d):
    """The opening copy most cases start with: found at byte 20 (source 5), ends at byte 28; the next
    search starts at 29 with attempt 0 and the table holds bytes 1..20 and 27, 28."""
    d.match(20, 5, 8)
    return d.next_emit


SN_COPY_LENGTHS = tuple(range(4, 14)) + (59, 60, 61, 63, 64, 65, 66, 67, 68, 69, 71, 72, 127, 128, 131, 132, 133,
                                          64 * 65 + 68)
# the extension compares 256 bytes a step from the match start + 4: the ends on both sides of a step
SN_COPY_WINDOW = (4 + 255, 4 + 256, 4 + 257, 4 + 511, 4 + 512, 4 + 513)
SN_OFFSETS = (1, 2, 3, 4, 255, 256, 2047, 2048, 32767, 32768)
SN_LIT_TAILS = (1, 59, 60, 61, 255, 256, 257)
SN_TINY = (0, 1, 14, 15, 16)
SN_FRAG_SIZES = tuple(sorted({min(SN_FRAG, (1 << k) + e) for k in range(8, 17) for e in (-1, 0, 1)}))


@functools.lru_cache(None)
def sn_copy_lengths():
    """Family 1.  Every copy length at offset 2047 (a short rest takes the 1-byte-offset form) and at
    2048 (it does not); 64 * 65 + 68 is more than 64 pieces of 64: two strides of the lane loop."""
    specs = []
    for L in SN_COPY_LENGTHS + SN_COPY_WINDOW:
        for off in (2047, 2048):
            def build(seed, L=L, off=off):
                d = SnappyDesign(8192 + L, seed)
                V = d.pair(off, lo=off + 1)
                d.match(V, V - off, L)
                return d.finish()
            specs.append((f"len={L} off={off}", build, 11000 + L))
    return _cases(specs)


def sn_approach(d, target):
    """Short copies (4 bytes of bytes 7, 11, 15, ...) at visited positions until the running search
    starts within 33 bytes below `target`: every byte there is then examined (step 1).  A fresh search
    steps by about 1/32 of its distance from its start, so far positions are reached in a few hops."""
    src = 7
    while target - d.next_emit > 33:
        A = [p for _, p in d.schedule() if p <= target - 12][-1]
        d.match(A - d.next_emit, src, 4)
        src += 4


SN_TOP_OFFSETS = tuple(SN_FRAG - 15 - 1 - s for s in (1, 2, 3))


@functools.lru_cache(None)
def sn_offsets():
    """Family 2.  Offsets at the form edges, and the three largest a fragment holds: the last position
    a search examines is n - 15 - 1, and byte 0 is never in the table, so 65,535 - k exists for k >= 16
    (65,519 against byte 1, then bytes 2 and 3)."""
    specs = []
    for off in SN_OFFSETS + SN_TOP_OFFSETS:
        def build(seed, off=off):
            s = off in SN_TOP_OFFSETS and SN_FRAG - 16 - off or 25
            d = SnappyDesign(SN_FRAG if off > 30000 else off + 8192, seed)
            if off < 40:
                d.match(30, 30 - off, 8)
            else:
                sn_approach(d, off + s)
                d.match(off + s - d.next_emit, s, 8)
            assert d.facts[-1]["off"] == off
            return d.finish()
        specs.append((f"off={off}", build, 12000 + off))
    return _cases(specs)


@functools.lru_cache(None)
def sn_literals():
    """Family 3.  Literal length forms.  The literals before a copy take only the lengths the search
    schedule reaches (1..33, 35, 37, ...: family 4); every length is reachable as the fragment's last
    literal, so each length of SN_LIT_TAILS follows a copy that stops that far before the end, 65,536
    is a whole fragment without a match, and fragments of 0, 1, 14, 15 and 16 bytes are literals only
    (below 15 bytes there is no search)."""
    specs = []
    for T in SN_LIT_TAILS:
        def build(seed, T=T):
            d = SnappyDesign(400 + T, seed)
            d.match(20, 5, d.n - T - 20)
            return d.finish()
        specs.append((f"tail={T}", build, 13000 + T))
    for n in SN_TINY + (SN_FRAG,):
        specs.append((f"n={n}", lambda seed, n=n: SnappyDesign(n, seed).finish(), 13500 + n))
    return _cases(specs)


@functools.lru_cache(None)
def sn_attempt_index():
    """Family 4.  The first hit after a copy at every attempt index 0..140 (batches of 16, 32, 64, 64,
    the constant table kSn.off), and equal table indexes inside one batch: none matches; the later
    attempt matches the earlier one; an earlier attempt matches, so the two writes must not happen (a
    third word of that index, in the table from the opening search, is found right after)."""
    probe = SnappyDesign(SN_FRAG, 0)
    sn_first_match(probe)
    pos = [p for _, p in probe.schedule()][:141]
    specs = []
    for k in range(141):
        def build(seed, k=k):
            d = SnappyDesign(pos[140] + 200, seed)
            E = sn_first_match(d)
            d.match(pos[k] - E, 10, 6)
            assert d.facts[-1]["k"] == k
            return d.finish()
        specs.append((f"attempt={k}", build, 14000 + k))

    def none(seed):
        d = SnappyDesign(400, seed)
        p, q, _ = sn_equal_index_words(d.mask)
        E = sn_first_match(d)
        d.poke(E + 1 + 3, p)
        d.poke(E + 1 + 9, q)
        d.match(30, 10, 7)
        return d.finish()

    def known(seed):
        d = SnappyDesign(400, seed)
        E = sn_first_match(d)
        d.match(10, E + 1 + 3, 6)                  # attempts 3 and 9 of the 16 batch
        return d.finish()

    def undo(seed):
        d = SnappyDesign(400, seed)
        p, q, q2 = sn_equal_index_words(d.mask)
        d.poke(10, p)
        sn_first_match(d)                          # ends at 28
        d.match(1, 15, 4)                          # attempt 0 of the 16 batch (bytes 29..44): ends at 33
        d.match(1, 10, 4)                          # byte 34: lane 5 of that batch, then attempt 0
        d.poke(39, q)                              # lanes 10 and 14 of that batch
        d.poke(43, q2)
        return d.finish()
    specs += [("equal index: none", none, 14500), ("equal index: known", known, 14600),
              ("equal index: undo", undo, 14700)]
    return _cases(specs)


@functools.lru_cache(None)
def sn_fragment_sizes():
    """Family 5.  Fragment sizes around every table size (256 .. 32768 entries, chosen from the fragment
    size) up to 65,535 and 65,536, each with two copies; and a two-fragment buffer in which the second
    fragment repeats bytes of the first one's end: they lie across the 65,536 seam and must not be used
    (the second fragment's only copy is of its own bytes)."""
    specs = []
    for n in SN_FRAG_SIZES:
        def build(seed, n=n):
            d = SnappyDesign(n, seed)
            E = sn_first_match(d)
            d.match(12, 10, 9)
            if n > 2000:
                V = d.pair(600, lo=d.next_emit + 700)
                d.match(V - d.next_emit, V - 600, 70)
            return d.finish()
        specs.append((f"n={n}", build, 15000 + n))
    cases = _cases(specs)

    def second(seed):
        a = SnappyDesign(SN_FRAG, seed)
        sn_first_match(a)
        a_buf, a_el, _ = a.finish()
        b = SnappyDesign(300, seed + 100)
        b.buf[40:60] = a_buf[SN_FRAG - 100:SN_FRAG - 80]
        b.match(71, 45, 12)
        b_buf, b_el, facts = b.finish()
        return _frozen(np.concatenate([a_buf, b_buf])), a_el + b_el, facts
    cases.append(("two fragments",) + designed(second, 15900))
    return cases


@functools.lru_cache(None)
def sn_match_ends():
    """Family 6.  Copies ending at n, n - 1, ... n - 4 of the fragment (the masked last word of the
    extension) and at lim - 1, lim, lim + 1 (lim = n - 15, the search limit: at or past it the parse
    stops, one before it the next search has no position left)."""
    specs = []
    n = 300
    for e in (0, 1, 2, 3, 4, 14, 15, 16):
        def build(seed, e=e):
            d = SnappyDesign(n, seed)
            d.match(20, 5, n - e - 20)
            return d.finish()
        specs.append((f"end=n-{e}", build, 16000 + e))
    return _cases(specs)


# =================================================================================================
# Part A: LZO1X-1 (LZO 2.10 lzo1x_1_compress; oracle/hdrf_lzo.c), sub-blocks of 49,152 bytes
# =================================================================================================
LZO_SUB = 49152


def lzo_index(v):
    return (((int(v) * 0x1824429d) & 0xFFFFFFFF) >> 18) & 0x3FFF


def lzo_class(ln, off):
    return "M2" if ln <= 8 and off <= 2048 else "M3" if off <= 16384 else "M4"


class LzoDesign(_Differ):
    """One lzo1x_1_compress call under construction (Lz4Design's protocol; no catch-up).  The designed
    output is lzo_parse's list: ("lit", n, form) and (class, distance, length).  A literal run is
    counted from the end of the last match, across sub-block seams (the encoder carries it)."""

    def __init__(self, n, seed):
        self.n, self.buf = n, np.concatenate([prng_bytes(seed, n), np.zeros(16, np.uint8)])
        self.out, self.facts, self.forbid, self.events = [], [], {}, []
        self.lit_start, self.left, self.base, self.live = 0, n, 0, False
        self._enter()

    def _enter(self):
        """Start the sub-block at self.base, if the encoder compresses it."""
        ll = min(self.left, LZO_SUB)
        t = self.base - self.lit_start
        self.live = self.left > 20 and (t + ll) >> 5 != 0
        if self.live:
            self.ll, self.ii, self.ip_end = ll, self.base, self.base + ll - 20
            self.cur = self.base + (4 - t if t < 4 else 0) + 1
            self.events.append(("reset", self.base))

    def next_sub(self):
        """No more matches in this sub-block: the search runs to its end, the literals are carried."""
        assert self.live
        self.events += [("visit", p) for p in self.schedule()]
        self.base += self.ll
        self.left -= self.ll
        self._enter()

    def schedule(self):
        ip = self.cur
        while ip < self.ip_end:
            yield ip
            ip += 1 + ((ip - self.ii) >> 5)

    def poke(self, pos, v):
        _poke(self.buf, pos, v)

    def approach(self, target):
        """4-byte matches (of bytes base + 7, 11, ...) at visited positions until the search restarts
        within 32 bytes below target, where every byte is examined."""
        src = self.base + 7
        while target - self.ii > 32:
            A = [p for p in self.schedule() if p <= target - 12][-1]
            self.match(A - self.lit_start, src, 4)
            src += 4

    def match(self, t, src, L, open_end=False):
        """t literals (from the last match's end), then a match whose first byte copies buf[src]; with
        open_end the copy runs on and the length is what the encoder's 8-byte extension makes of it."""
        assert self.live
        A = self.lit_start + t
        assert A in set(self.schedule()), f"{A} is not visited"
        assert self.base <= src < A
        self.events += [("visit", p) for p in self.schedule() if p < A] + [("find", A, src)]
        _copy_fwd(self.buf, A, src, L)
        if not open_end:
            self._differ(A + L, self.buf[src + L])
        m = 4                                      # the encoder's extension: 8 bytes a step, stopped at ip_end
        while True:
            x = self.buf[A + m:A + m + 8] != self.buf[src + m:src + m + 8]
            if x.any():
                m += int(np.argmax(x))
                break
            m += 8
            if A + m >= self.ip_end:
                break
        assert open_end or m == L, (m, L)
        if t:
            self.out.append(("lit", t, "trail" if t <= 3 else "run"))
        self.out.append((lzo_class(m, A - src), A - src, m))
        self.facts.append(dict(ip=A, src=src, lit=t, ml=m, off=A - src, end=A + m, ip_end=self.ip_end))
        self.lit_start = self.ii = self.cur = A + m
        return A

    def decoy(self, dst, src, L):
        _copy_fwd(self.buf, dst, src, L)

    def finish(self):
        while self.live:
            self.next_sub()
        t = self.n - self.lit_start
        if t:
            self.out.append(("lit", t, "first" if not self.facts and t <= 238 else "trail" if t <= 3 else "run"))
        buf, tab, base = self.buf, {}, 0
        for ev in self.events:
            p = ev[1]
            if ev[0] == "reset":
                tab, base = {}, p
                continue
            v = _word(buf, p)
            cand = tab.get(lzo_index(v), base)
            tab[lzo_index(v)] = p
            same = _word(buf, cand) == v
            if ev[0] == "find":
                if not (cand == ev[2] and same):
                    raise Undesigned(f"find at {p}: table holds {cand}, designed {ev[2]}")
            elif same:
                raise Undesigned(f"undesigned match at {p} (candidate {cand})")
        return _frozen(buf[:self.n].copy()), self.out, dict(finds=self.facts)


LZO_M3_LENGTHS = (33, 34, 33 + 255, 33 + 256, 33 + 510, 33 + 511)
LZO_M4_LENGTHS = (9, 10, 9 + 255, 9 + 256)
LZO_EDGES = ((8, 2048), (9, 2048), (8, 2049), (9, 2049), (10, 16384), (10, 16385)) + \
    tuple((ln, 3000) for ln in LZO_M3_LENGTHS) + tuple((ln, 20000) for ln in LZO_M4_LENGTHS) + \
    tuple((12, off) for off in (32767, 32768, 32769))
LZO_LIT_RUNS = (0, 1, 2, 3, 4, 18, 19, 18 + 255, 18 + 256, 18 + 510, 18 + 511)


@functools.lru_cache(None)
def lzo_class_edges():
    """Family 1.  (length, distance) on both sides of every class boundary, the M3 and M4 length-run
    edges, and M4 distances on both sides of 32,768 (the instruction's distance bit)."""
    specs = []
    for ln, off in LZO_EDGES:
        def build(seed, ln=ln, off=off):
            d = LzoDesign(off + ln + 600, seed)
            d.approach(off + 25)
            d.match(off + 25 - d.lit_start, 25, ln)
            return d.finish()
        specs.append((f"len={ln} off={off}", build, 21000 + off + ln))
    return _cases(specs)


@functools.lru_cache(None)
def lzo_literal_runs():
    """Family 2.  Literal runs before a match.  After a match the search examines its end and the 32
    bytes behind it, then every 2nd, 3rd, ... byte (the same from the block's start), so a long run
    that is not on that schedule is split over the sub-block seam: the last match of the first
    sub-block ends t - 10 bytes before it and the next is found at byte 10 of the second, where every
    byte is examined again.  Runs of 1..3 ride in the previous match's last instruction: after an M2,
    an M3 and an M4."""
    specs = []
    for t in LZO_LIT_RUNS:
        def build(seed, t=t):
            d = LzoDesign(t + 2600, seed)
            d.match(20, 9, 6)                      # the opening M2: ends at 26
            if d.lit_start + t in set(d.schedule()):
                d.match(t, 13, 10)
            else:                                  # carried across the seam: t - 10 bytes before it, 10 behind
                d = LzoDesign(LZO_SUB + 300, seed)
                E1 = LZO_SUB - (t - 10)
                d.approach(E1 - 8)
                d.match(E1 - 8 - d.lit_start, 25, 8)
                d.next_sub()
                d.match(t, LZO_SUB + 5, 10)
            return d.finish()
        specs.append((f"lit={t}", build, 22000 + t))
    for cls, ln, off in (("M2", 5, 300), ("M3", 20, 3000), ("M4", 20, 17000)):
        for t in (1, 2, 3):
            def build(seed, cls=cls, ln=ln, off=off, t=t):
                d = LzoDesign(off + 700, seed)
                d.approach(off + 25)
                d.match(off + 25 - d.lit_start, 25, ln)
                assert d.out[-1][0] == cls
                d.match(t, 32 + 2 * t, 7)
                return d.finish()
            specs.append((f"lit={t} after {cls}", build, 22500 + t))
    return _cases(specs)


LZO_SMALL = (0, 1, 20, 21, 31, 32, 237, 238, 239)


@functools.lru_cache(None)
def lzo_first_literals():
    """Family 3.  Blocks without a match: 0, 1, 20 (no search), 21 and 31 (the t + ll < 32 guard), 32
    (the search runs), 237 / 238 (the last lengths of the 17 + t first-literal form) and 239 (a literal
    run); and 1,000 incompressible bytes, which LzopCodec stores raw."""
    return _cases([(f"n={n}", lambda seed, n=n: LzoDesign(n, seed).finish(), 23000 + n) for n in LZO_SMALL + (1000,)])


LZO_END_GAPS = (0, 1, 7, 8, 9)


@functools.lru_cache(None)
def lzo_extension_ends():
    """Family 4.  Matches that end at in_len - 20 - {0, 1, 7, 8, 9} (a differing byte there), and copies
    that run on to the block's end from 8 start phases: the extension stops at the first 8-byte step
    at or past in_len - 20 (the `done` path)."""
    specs = []
    n = 600
    for e in LZO_END_GAPS:
        def build(seed, e=e):
            d = LzoDesign(n, seed)
            d.match(20, 9, n - 20 - e - 20)
            assert d.facts[-1]["end"] == n - 20 - e
            return d.finish()
        specs.append((f"end=in_len-20-{e}", build, 24000 + e))
    for a in range(20, 28):
        def build(seed, a=a):
            d = LzoDesign(n, seed)
            d.match(a, 9, n - a, open_end=True)
            return d.finish()
        specs.append((f"open end from {a}", build, 24100 + a))
    return _cases(specs)


@functools.lru_cache(None)
def lzo_seams():
    """Family 5.  The 49,152-byte sub-block seam.  A match can end at most 11 bytes past in_len - 20
    (the extension's last step), so the literals carried into the next sub-block are at least 9: the
    ip += 4 - ti skip for ti < 4 exists only at the block's start (ti = 0, every case here), and
    ti in {1, 3, 4, 5} cannot occur.  Cases: the smallest carry (9) and a long one (no match in the
    first sub-block), each followed by a match in the second sub-block; a copy in the second sub-block
    whose source lies in the first (not used: the dictionary is reset); a last sub-block of 21 bytes
    behind a carry of 9 (t + ll < 32: not compressed) and one of 23 bytes (compressed)."""
    specs = []

    def carry9(d):
        d.approach(LZO_SUB - 21)
        d.match(LZO_SUB - 21 - d.lit_start, 25, 40, open_end=True)       # found at ip_end - 1
        assert d.facts[-1]["end"] == LZO_SUB - 9, d.facts[-1]
        d.next_sub()

    for tail in (21, 23, 400):
        def build(seed, tail=tail):
            d = LzoDesign(LZO_SUB + tail, seed)
            carry9(d)
            assert d.live == (tail != 21)
            if tail == 400:
                d.match(9 + 30, LZO_SUB + 10, 12)
            return d.finish()
        specs.append((f"carry 9, last sub-block {tail}", build, 25000 + tail))

    def long_carry(seed):
        d = LzoDesign(LZO_SUB + 400, seed)
        d.next_sub()
        d.decoy(LZO_SUB + 60, LZO_SUB - 300, 16)                         # source across the seam
        d.match(LZO_SUB + 30, LZO_SUB + 10, 12)
        return d.finish()
    specs.append(("carry a whole sub-block, source across the seam", long_carry, 25500))
    return _cases(specs)


LZO_FAMILIES = {"class_edges": lzo_class_edges, "literal_runs": lzo_literal_runs, "first_literals": lzo_first_literals,
                "extension_ends": lzo_extension_ends, "seams": lzo_seams}

SN_FAMILIES = {"copy_lengths": sn_copy_lengths, "offsets": sn_offsets, "literals": sn_literals,
               "attempt_index": sn_attempt_index, "fragment_sizes": sn_fragment_sizes, "match_ends": sn_match_ends}



# =================================================================================================
# Part B: decoder streams built from element lists
# =================================================================================================
def be32(v):
    return int(v).to_bytes(4, "big")


def frame_groups(blocks):
    """BlockCompressorStream framing, one block per group: [BE32 raw][BE32 clen][block] each.
    blocks: [(block bytes, decoded bytes)] -> (file, decoded file, [(block start, output start)])."""
    f, out, where = bytearray(), [], []
    o = 0
    for blk, raw in blocks:
        f += be32(len(raw)) + be32(len(blk))
        where.append((len(f), o))
        f += blk
        out.append(np.asarray(raw, np.uint8))
        o += len(raw)
    return bytes(f), np.concatenate(out) if out else np.zeros(0, np.uint8), where


def frame_lzop(header, blocks):
    """An lzop file (flags 0): header, [BE32 raw][BE32 stored][block] each, BE32 0.  Every block must be
    smaller than its decoded size (an equal size means "stored raw" to the reader)."""
    f, out, where = bytearray(header), [], []
    o = 0
    for blk, raw in blocks:
        assert len(blk) < len(raw), (len(blk), len(raw))
        f += be32(len(raw)) + be32(len(blk))
        where.append((len(f), o))
        f += blk
        out.append(np.asarray(raw, np.uint8))
        o += len(raw)
    return bytes(f + be32(0)), np.concatenate(out), where


class _Lits:
    """Literal bytes drawn in order from one prng_bytes buffer."""

    def __init__(self, seed, n=1 << 20):
        self.b, self.i = prng_bytes(seed, n), 0

    def take(self, n):
        assert self.i + n <= self.b.size
        self.i += n
        return self.b[self.i - n:self.i]


# ---- LZ4 ----------------------------------------------------------------------------------------
def _lz4_ext(v):
    """The continuation bytes of a length field whose nibble is 15: v = length - 15."""
    return b"\xff" * (v // 255) + bytes([v % 255])


def lz4_stream(seqs, lits):
    """seqs: [(literal length, offset, match length)], the last (literal length, None, 0); literal bytes
    from lits -> (block bytes, decoded bytes)."""
    out = bytearray()
    dec = np.zeros(sum(s[0] + s[2] for s in seqs), np.uint8)
    o = 0
    for lit, off, ml in seqs:
        tok = (min(lit, 15) << 4) | (0 if off is None else min(ml - 4, 15))
        out.append(tok)
        if lit >= 15:
            out += _lz4_ext(lit - 15)
        b = lits.take(lit)
        out += b.tobytes()
        dec[o:o + lit] = b
        o += lit
        if off is None:
            break
        assert 1 <= off <= min(o, 65535) and ml >= 4
        out += bytes([off & 255, off >> 8])
        if ml - 4 >= 15:
            out += _lz4_ext(ml - 4 - 15)
        _copy_fwd(dec, o, o - off, ml)
        o += ml
    assert o == dec.size
    return bytes(out), dec


STRADDLE_LITS = tuple(range(DEC_WIN - 60, DEC_WIN + 25))


@functools.lru_cache(None)
def lz4_straddle_blocks():
    """B1.  A leading literal of every length in [8192 - 60, 8192 + 24], then (a) a 2-byte offset and a
    match-length run of three 255s, or (b) a short match and a token whose literal-length run has three
    255s.  With the literal's own token and 33 length bytes in front, the fields start between 8166
    and 8250: every byte of every field lies on either side of the first refill of the 8 KiB window
    (at byte 8192 when a field begins before it, at the field's first byte otherwise, in every phase
    mod 16, (ip + 1) % 16 == 0 among them).  The last block is one stream longer than three windows,
    built from random element sizes, so later refills depend on where the earlier ones landed."""
    lits = _Lits(9100, 4 << 20)
    blocks = []
    for i, L0 in enumerate(STRADDLE_LITS):
        tail = 12 + i % 16
        blocks.append((f"offset+mlrun L0={L0}",) + lz4_stream(
            [(L0, 7 + i, 19 + 3 * 255 + 9), (tail, None, 0)], lits))
        blocks.append((f"litrun L0={L0}",) + lz4_stream(
            [(L0, 300 + i, 6), (15 + 3 * 255 + 11, 3, 4), (tail + 1, None, 0)], lits))
    r = prng_bytes(9101, 4096).view(np.uint16)
    seqs, o = [], 0
    for j in range(0, 400, 4):
        lit = int(r[j]) % 700 if r[j + 3] % 4 else int(r[j]) % 15
        o += lit
        if o == 0:
            lit = o = 20
        seqs.append((lit, 1 + int(r[j + 1]) % min(o, 65535), 4 + int(r[j + 2]) % (300 if r[j + 3] % 8 else 19)))
        o += seqs[-1][2]
    seqs.append((40, None, 0))
    long = lz4_stream(seqs, lits)
    assert len(long[0]) > 3 * DEC_WIN
    blocks.append(("random elements, more than 3 windows",) + long)
    return blocks


LZ4_DEC_OFFSETS = (1, 2, 3, 4, 63, 64, 65, 65535)
LZ4_DEC_LENGTHS = (4, 18, 19, 19 + 254, 19 + 255, 70000)


@functools.lru_cache(None)
def lz4_element_blocks():
    """B2.  Every offset of LZ4_DEC_OFFSETS with match lengths below, equal to and above it (the
    overlapping branch and its k % off) and with every length of LZ4_DEC_LENGTHS; a block that is one
    literal run of 261,100 bytes.  Sequences are packed into blocks of at most 261,100 decoded bytes."""
    lits = _Lits(9200, 2 << 20)
    want = []
    for off in LZ4_DEC_OFFSETS:
        for ml in sorted({m for m in (off - 1, off, off + 1) if m >= 4} | set(LZ4_DEC_LENGTHS)):
            want.append((off, ml))
    blocks, seqs, size, need = [], [], 0, 0

    def flush():
        nonlocal seqs, size
        if seqs:
            blocks.append((f"elements {len(blocks)}",) + lz4_stream(seqs + [(16, None, 0)], lits) + (tuple(seqs),))
        seqs, size = [], 0
    for off, ml in want:
        lit = max(off - size, 0) + 5
        if size + lit + ml + 16 > LZ4_MAX_IN:
            flush()
            lit = off + 5
        seqs.append((lit, off, ml))
        size += lit + ml
    flush()
    blocks.append(("one literal run",) + lz4_stream([(LZ4_MAX_IN, None, 0)], lits) + ((),))
    return blocks


# ---- Snappy -------------------------------------------------------------------------------------
def _varint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def snappy_stream(elems, lits):
    """elems: ("lit", length, length bytes or None for the shortest form) or ("c1" | "c2" | "c4", length,
    offset) -> (raw snappy buffer, decoded bytes)."""
    body = bytearray()
    dec = np.zeros(sum(e[1] for e in elems), np.uint8)
    o = 0
    for kind, ln, x in elems:
        if kind == "lit":
            nb = x if x is not None else (0 if ln <= 60 else (ln - 1).bit_length() + 7 >> 3)
            if nb == 0:
                body.append((ln - 1) << 2)
            else:
                assert ln - 1 < 1 << (8 * nb)
                body.append((59 + nb) << 2)
                body += (ln - 1).to_bytes(nb, "little")
            b = lits.take(ln)
            body += b.tobytes()
            dec[o:o + ln] = b
        else:
            assert 1 <= x <= o
            if kind == "c1":
                assert 4 <= ln <= 11 and x < 2048
                body += bytes([1 | ((ln - 4) << 2) | ((x >> 8) << 5), x & 255])
            elif kind == "c2":
                assert 1 <= ln <= 64 and x < 65536
                body += bytes([2 | ((ln - 1) << 2)]) + x.to_bytes(2, "little")
            else:
                assert 1 <= ln <= 64
                body += bytes([3 | ((ln - 1) << 2)]) + x.to_bytes(4, "little")
            _copy_fwd(dec, o, o - x, ln)
        o += ln
    return _varint(dec.size) + bytes(body), dec


SN_STRADDLE_KINDS = ("c2", "c4", "lit1", "lit2", "lit3", "lit4")


@functools.lru_cache(None)
def snappy_straddle_blocks():
    """B1.  A leading literal of every length in [8192 - 60, 8192 + 24] (2 varint bytes, its tag and 2
    length bytes in front: the next element starts between 8137 and 8221), then a copy with a 2-byte
    or a 4-byte offset, or a literal whose length field has 1, 2, 3 or 4 bytes (the 3- and 4-byte
    forms, and here all four, carry small values: legal, and nothing in the project emits them).  The
    last block is a stream longer than three windows built from random element sizes."""
    lits = _Lits(9300, 8 << 20)
    blocks = []
    for i, L0 in enumerate(STRADDLE_LITS):
        for kind in SN_STRADDLE_KINDS:
            x = {"c2": ("c2", 10 + i % 50, 300 + i), "c4": ("c4", 10 + i % 50, 301 + i)}.get(kind) or \
                ("lit", 5 + i % 7, int(kind[3]))
            blocks.append((f"{kind} L0={L0}",) + snappy_stream([("lit", L0, None), x, ("lit", 3 + i % 16, None)], lits))
    r = prng_bytes(9301, 8192).view(np.uint16)
    elems, o = [("lit", 70, None)], 70
    for j in range(0, 4000, 4):
        t = int(r[j]) % 8
        if t < 3:
            e = ("lit", 1 + int(r[j + 1]) % (400 if t else 60), None if r[j + 2] % 4 else 1 + int(r[j + 2]) % 4)
            if e[2] is not None and e[1] - 1 >= 1 << (8 * e[2]):
                e = ("lit", e[1], None)
        elif t == 3:
            e = ("c1", 4 + int(r[j + 1]) % 8, 1 + int(r[j + 2]) % min(o, 2047))
        else:
            e = ("c2" if t < 6 else "c4", 1 + int(r[j + 1]) % 64, 1 + int(r[j + 2]) % min(o, 65535))
        elems.append(e)
        o += e[1]
    long = snappy_stream(elems, lits)
    assert len(long[0]) > 3 * DEC_WIN and long[1].size <= SNAPPY_MAX_IN
    blocks.append(("random elements, more than 3 windows",) + long)
    return blocks


@functools.lru_cache(None)
def snappy_element_blocks():
    """B3.  All three copy forms: c1 lengths 4..11, c2 and c4 lengths 1..64, each at offsets {1, 2, 3,
    len - 1, len, len + 1, 2047, 2048, 65535, 65536, 200000} as far as the form holds them (c1 < 2048,
    c2 < 65536; a c4 copy may reach back further than a fragment).  Two blocks: the second starts with
    200,000 literal bytes and holds the c4 copies at 65,535 and beyond."""
    lits = _Lits(9400, 1 << 20)
    near, far = [("lit", 66000, None)], [("lit", 200000, None)]
    for kind, lens, top in (("c1", range(4, 12), 2047), ("c2", range(1, 65), 65535), ("c4", range(1, 65), 1 << 31)):
        for ln in lens:
            for off in sorted({1, 2, 3, ln - 1, ln, ln + 1, 2047, 2048, 65535, 65536, 200000}):
                if 1 <= off <= top:
                    (far if off > 65535 or (kind == "c4" and off == 65535) else near).extend(
                        [(kind, ln, off), ("lit", 1 + (ln + off) % 3, None)])
    out = [("copies near",) + snappy_stream(near, lits) + (tuple(near),),
           ("copies far",) + snappy_stream(far, lits) + (tuple(far),)]
    assert all(b[2].size <= SNAPPY_MAX_IN for b in out)
    return out


# ---- LZO1X ----------------------------------------------------------------------------------------
def _lzo_run(v):
    """The bytes of a zero-nibble length run carrying v >= 1: (v - 1) // 255 zero bytes, then the rest."""
    nz = (v - 1) // 255
    return b"\0" * nz + bytes([v - 255 * nz])


class LzoStream:
    """An LZO1X stream written instruction by instruction; the decoded bytes are kept beside it.
    lit(n): at the stream's start the 17 + n form when first=True; 1..3 literals after a match ride in
    that match's last instruction byte pair (its low 2 bits); otherwise a literal run of >= 4.
    match(kind, dist, len): M1 is the 2-byte match after 1..3 trailing literals (distance <= 1024) or the
    3-byte match after a literal run of >= 4 (distance 2049..3072); M2 / M3 / M4 as in LZO1X."""

    def __init__(self, lits, cap=LZO_MAX_IN):
        self.out, self.dec, self.o = bytearray(), np.zeros(cap, np.uint8), 0
        self.lits, self.state, self.patch = lits, "start", None
        self.log = []

    def lit(self, n, first=False):
        b = self.lits.take(n)
        if first:
            assert self.state == "start" and 1 <= n <= 238
            self.out.append(17 + n)
            self.state = "run" if n >= 4 else "trail"
        elif n <= 3:
            assert self.state == "match" and n >= 1
            self.out[self.patch] |= n
            self.state = "trail"
        else:
            assert self.state in ("start", "match")
            self.out += bytes([n - 3]) if n <= 18 else b"\0" + _lzo_run(n - 18)
            self.state = "run"
        self.out += b.tobytes()
        self.dec[self.o:self.o + n] = b
        self.o += n
        self.log.append(("lit", n, "first" if first else self.state))

    def match(self, kind, dist, ln):
        assert 1 <= dist <= self.o, (dist, self.o)
        if kind == "M1":
            if self.state == "trail":
                assert ln == 2 and dist <= 1024
                d = dist - 1
            else:
                assert self.state == "run" and ln == 3 and 2049 <= dist <= 3072
                d = dist - 2049
            self.patch = len(self.out)
            self.out += bytes([(d & 3) << 2, d >> 2])
        elif kind == "M2":
            assert self.state != "start" and 3 <= ln <= 8 and dist <= 2048
            d = dist - 1
            self.patch = len(self.out)
            self.out += bytes([((ln - 1) << 5) | ((d & 7) << 2), d >> 3])
        else:
            if kind == "M3":
                assert ln >= 3 and dist <= 16384
                d, base, lim = dist - 1, 32, 33
            else:
                assert kind == "M4" and ln >= 3 and 16385 <= dist <= 49151
                d = dist - 16384
                base, lim = 16 | ((d >> 11) & 8), 9
                d &= 0x3FFF
            self.out += bytes([base | (ln - 2)]) if ln <= lim else bytes([base]) + _lzo_run(ln - lim)
            self.patch = len(self.out)
            self.out += bytes([(d << 2) & 255, d >> 6])
        _copy_fwd(self.dec, self.o, self.o - dist, ln)
        self.o += ln
        self.state = "match"
        self.log.append((kind, dist, ln))

    def end(self):
        self.out += b"\x11\0\0"
        return bytes(self.out), self.dec[:self.o].copy(), tuple(self.log)


@functools.lru_cache(None)
def lzo_element_blocks():
    """B4.  M1 3-byte matches after a literal run of >= 4 (distances 2049 and 3072), M1 2-byte matches
    after 1..3 trailing literals (distances 1 and 1024), M2 / M3 / M4 at their distance and length
    edges, overlapping matches at distances 1..3, length runs with 0, 1 and 3 zero bytes, and blocks
    that start with the 17 + t form for t in {1, 3, 4, 238}.  Every block ends with a long M3 match so
    that it is smaller than what it decodes to."""
    blocks = []
    for t in (1, 3, 4, 238):
        s = LzoStream(_Lits(9500 + t))
        s.lit(t, first=True)
        if t < 4:
            s.match("M2", t, 3)                    # after 17 + t with t < 4 comes a match instruction
            s.lit(50)
        s.match("M3", 1 if t == 1 else 3, 700)     # overlapping, length run with 2 zero bytes
        s.lit(2)
        s.match("M1", 1, 2)
        blocks.append((f"first literal 17+{t}",) + s.end())
    s = LzoStream(_Lits(9600))
    s.lit(4000)
    for dist in (2049, 3072):                      # M1, 3 bytes, after a literal run of >= 4
        s.match("M1", dist, 3)
        s.lit(4 + dist % 5)
    for dist in (1, 1024):                         # M1, 2 bytes, after 1..3 trailing literals
        for trail in (1, 2, 3):
            s.match("M2", 9, 4)
            s.lit(trail)
            s.match("M1", dist, 2)
    for ln, dist in ((3, 1), (8, 2048), (8, 1), (3, 2048), (5, 7), (5, 8), (5, 9)):
        s.match("M2", dist, ln)
        s.lit(1 + ln % 3)
    for ln in (3, 9) + LZO_M3_LENGTHS + (33 + 100, 33 + 255 + 100, 33 + 3 * 255 + 100):
        for dist in (2049, 16384):
            s.match("M3", dist if dist <= s.o else 2049, ln)
            s.lit(ln % 4 if ln % 4 else 7)
    for dist in (1, 2, 3):                         # overlapping: dist < len
        for ln in (3, 8):
            s.match("M2", dist, ln)
        for ln in (33, 200, 65):
            s.match("M3", dist, ln)
            s.lit(20)
    for n in (4, 18, 19, 18 + 255, 18 + 256, 18 + 510, 18 + 511):   # literal-run length forms
        s.match("M2", 5, 4)
        s.lit(n)
    s.match("M3", 3, 3000)
    blocks.append(("M1 M2 M3",) + s.end())
    s = LzoStream(_Lits(9700))
    s.lit(50000)
    for ln in (3,) + LZO_M4_LENGTHS + (9 + 100, 9 + 255 + 100, 9 + 3 * 255 + 100):
        for dist in (16385, 32767, 32768, 32769, 49151):
            s.match("M4", dist, ln)
            s.lit(1 + (ln + dist) % 3)
    s.match("M3", 16384, 60000)
    s.lit(5)
    blocks.append(("M4",) + s.end())
    for tag, blk, raw, _ in blocks:
        assert len(blk) < raw.size <= LZO_MAX_IN, tag
    return blocks


def lzo_parse(c):
    """Walk an LZO1X stream -> [("lit", n, form) | (class, distance, length)], the end marker left out;
    form is "first" (17 + n), "trail" (1..3 after a match) or "run"."""
    c = bytes(c)
    out, i = [], 0

    def run(t, add):
        nonlocal i
        if t:
            return t
        while c[i] == 0:
            t += 255
            i += 1
        t += add + c[i]
        i += 1
        return t
    state = "top"
    if c[0] > 17:
        t = c[0] - 17
        i = 1
        out.append(("lit", t, "first"))
        i += t
        state = "trail" if t < 4 else "run"
    while True:
        t = c[i]
        i += 1
        if t < 16 and state == "top":
            t = run(t, 15) + 3
            out.append(("lit", t, "run"))
            i += t
            state = "run"
            continue
        if t >= 64:
            out.append(("M2", 1 + ((t >> 2) & 7) + (c[i] << 3), (t >> 5) + 1))
            i += 1
        elif t >= 32:
            ln = run(t & 31, 31) + 2
            out.append(("M3", 1 + (c[i] >> 2) + (c[i + 1] << 6), ln))
            i += 2
        elif t >= 16:
            ln = run(t & 7, 7) + 2
            d = ((t & 8) << 11) + (c[i] >> 2) + (c[i + 1] << 6)
            i += 2
            if d == 0:
                assert ln == 3 and i == len(c)
                return out
            out.append(("M4", d + 16384, ln))
        elif state == "run":
            out.append(("M1", 2049 + (t >> 2) + (c[i] << 2), 3))
            i += 1
        else:
            out.append(("M1", 1 + (t >> 2) + (c[i] << 2), 2))
            i += 1
        t = c[i - 2] & 3
        state = "top"
        if t:
            out.append(("lit", t, "trail"))
            i += t
            state = "trail"
